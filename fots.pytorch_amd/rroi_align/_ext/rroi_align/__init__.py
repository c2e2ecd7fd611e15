"""rroi_align._ext.rroi_align -- ctypes binding of librroi_align_hip.so.

Stands where the reference's cffi extension stood (``rroi_align/build.py:7-37``
built ``_ext.rroi_align`` from ``src/rroi_align_cuda.c``): it exports the same
two tensor-taking functions, ``rroi_align_forward_cuda`` and
``rroi_align_backward_cuda`` (``src/rroi_align_cuda.h:1-7``), plus the native
entry points the autograd Function uses.

The shared library is mandatory: importing this module without it raises.
"""
from __future__ import annotations

import collections
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librroi_align_hip.so")

LAYOUT_NCHW, LAYOUT_NHWC = 0, 1
PATH_AUTO, PATH_DIRECT, PATH_TILED, PATH_TILED_ATOMIC, PATH_TILED_LISTS, PATH_TILED_INKERNEL = 0, 1, 2, 3, 4, 5
PATH_TILED_BUCKETS = 6  # backward only: the gather over pixel lists built in one pass (buckets + overflow chains)
PATH_FUSED = 7  # forward only: one launch for few ROIs, the tiled gather reading the NCHW map itself (no workspace)
# the gather formulations of the backward (they also read / write channels-last tensors in place), and every path
GATHER_PATHS = (PATH_TILED, PATH_TILED_LISTS, PATH_TILED_BUCKETS, PATH_TILED_INKERNEL)
BACKWARD_PATHS = (PATH_AUTO, PATH_DIRECT, PATH_TILED_ATOMIC) + GATHER_PATHS
STAGE_PROLOGUE, STAGE_GATHER, STAGE_ALL = 1, 2, 3
# every value `path` may take in forward() (the parity tests run them all)
FORWARD_PATHS = (PATH_AUTO, PATH_DIRECT, PATH_TILED, PATH_FUSED)

# the plan query (include/rroi_align_hip.h section 2): callers, plan families, gather kernels, backward destinations
CALLER_NATIVE, CALLER_LAUNCHER, CALLER_LAUNCHER_CON_IDX = 0, 1, 2
PLAN_NONE = 0
PLAN_FWD_DIRECT_K2P, PLAN_FWD_DIRECT_THREAD, PLAN_FWD_FUSED_STRIDED, PLAN_FWD_FUSED_SHIFT, PLAN_FWD_TWO_LAUNCH = 1, 2, 3, 4, 5
PLAN_BWD_DIRECT, PLAN_BWD_ATOMIC, PLAN_BWD_INKERNEL, PLAN_BWD_LISTS, PLAN_BWD_BUCKETS, PLAN_BWD_LITERAL = 11, 12, 13, 14, 15, 16
PLAN_BWD_ORDERED = 17  # the deterministic backward (PATH_DETERMINISTIC): sorted exact lists, in-order fp64 gather
PLAN_KERNEL_STRIDED, PLAN_KERNEL_CHANNELS_LAST, PLAN_KERNEL_SHIFT, PLAN_KERNEL_STRIDED_MERGE, PLAN_KERNEL_SHIFT_LINES = 0, 1, 2, 3, 4
PLAN_DST_NONE, PLAN_DST_CHUNK_MAJOR, PLAN_DST_NCHW, PLAN_DST_NCHW_ADD, PLAN_DST_NHWC = 0, 1, 2, 3, 4

# element types of the features / crops (forward) and grad_output / gradient (backward), 0.10.0: the `dtype` argument of
# the typed entry points.  rois are float32 in every case.
DTYPE_FP32, DTYPE_BF16, DTYPE_FP16 = 0, 1, 2
_DTYPES = {torch.float32: DTYPE_FP32, torch.bfloat16: DTYPE_BF16, torch.float16: DTYPE_FP16}

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C fots.pytorch_amd/csrc` "
        "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
        "rroi_align has no CPU or PyTorch fallback.")

# torch must be imported first so that libamdhip64.so.7 resolves to the runtime
# torch already loaded (same SONAME) and streams/pointers are interchangeable.
_lib = ctypes.CDLL(LIB_PATH)

_vp, _f, _i, _sz = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_size_t

_lib.rroi_align_hip_version.restype = ctypes.c_char_p
_lib.rroi_align_forward_workspace_bytes.restype = _sz
_lib.rroi_align_forward_workspace_bytes.argtypes = [_i] * 6
_lib.rroi_align_backward_workspace_bytes.restype = _sz
_lib.rroi_align_backward_workspace_bytes.argtypes = [_i] * 7
_lib.rroi_align_forward_hip.restype = _i
_lib.rroi_align_forward_hip.argtypes = [_vp, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp]
_lib.rroi_align_forward_layout_hip.restype = _i
_lib.rroi_align_forward_layout_hip.argtypes = [_vp, _i, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp]
_lib.rroi_align_forward_stages_hip.restype = _i
_lib.rroi_align_forward_stages_hip.argtypes = [_vp, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _i, _vp]
_lib.rroi_align_backward_hip.restype = _i
_lib.rroi_align_backward_hip.argtypes = [_vp, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp]
_lib.rroi_align_backward_layout_hip.restype = _i
_lib.rroi_align_backward_layout_hip.argtypes = [_vp, _i, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp]
_lib.rroi_align_bin_centres_hip.restype = _i
_lib.rroi_align_bin_centres_hip.argtypes = [_f, _i, _i, _i, _i, _i, _vp, _vp, _vp]
_lib.rroi_align_quads_to_rois_hip.restype = _i
_lib.rroi_align_quads_to_rois_hip.argtypes = [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]
_lib.rroi_align_gt_quads_to_rois_hip.restype = _i
_lib.rroi_align_gt_quads_to_rois_hip.argtypes = [_vp, _vp, _vp, _i, _vp, _vp, _vp]
_lib.rroi_rbox_decode_hip.restype = _i
_lib.rroi_rbox_decode_hip.argtypes = [_vp, _vp, _vp, _i, _i, _f, _vp, _i, _vp, _vp]
_lib.rroi_nms_merge_host.restype = _i
_lib.rroi_nms_merge_host.argtypes = [_vp, _i, _i, _i, _f, _f, _vp, _i]
_lib.rroi_ctc_greedy_decode_hip.restype = _i
_lib.rroi_ctc_greedy_decode_hip.argtypes = [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]
_lib.rroi_align_sincos_probe_hip.restype = _i
_lib.rroi_align_sincos_probe_hip.argtypes = [_vp, _i, _vp, _vp]
_lib.rroi_align_write_probe_hip.restype = _i
_lib.rroi_align_write_probe_hip.argtypes = [_vp, _sz, _vp]
_lib.rroi_align_bin_centres_trig_hip.restype = _i
_lib.rroi_align_bin_centres_trig_hip.argtypes = [_f, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp]
_lib.rroi_nms_record_format.restype = _i
_lib.rroi_nms_record_format.argtypes = []
_lib.RROIAlignForwardLaucher.restype = _i
_lib.RROIAlignForwardLaucher.argtypes = [_vp, _f, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]
_lib.RROIAlignBackwardLaucher.restype = _i
_lib.RROIAlignBackwardLaucher.argtypes = [_vp, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]
_lib.rroi_align_release_launcher_scratch.restype = _i
_lib.rroi_align_release_launcher_scratch.argtypes = []
_lib.rroi_align_launcher_scratch_stats.restype = _i
_lib.rroi_align_launcher_scratch_stats.argtypes = [_vp, _vp, _vp, _vp]


class _Plan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("family", "kernel", "groups", "ntiles", "grid_x", "grid_y", "zero_copy", "con_idx", "nk",
                                  "kshift", "raw_bsum", "gy", "dest", "accumulate", "vec4")]


_lib.rroi_align_forward_plan.restype = _i
_lib.rroi_align_forward_plan.argtypes = [_i] * 11 + [ctypes.POINTER(_Plan)]
_lib.rroi_align_backward_plan.restype = _i
_lib.rroi_align_backward_plan.argtypes = [_i] * 11 + [ctypes.POINTER(_Plan)]
_lib.rroi_align_forward_plan_typed.restype = _i
_lib.rroi_align_forward_plan_typed.argtypes = [_i] * 12 + [ctypes.POINTER(_Plan)]
_lib.rroi_align_backward_plan_typed.restype = _i
_lib.rroi_align_backward_plan_typed.argtypes = [_i] * 12 + [ctypes.POINTER(_Plan)]
_lib.rroi_align_forward_typed_hip.restype = _i
_lib.rroi_align_forward_typed_hip.argtypes = [_vp, _i, _i, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp]
_lib.rroi_align_backward_typed_hip.restype = _i
_lib.rroi_align_backward_typed_hip.argtypes = [_vp, _i, _i, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp]
# the callers' kernels on bfloat16 / float16 data (after 0.10.0, same version string: found by symbol)
_lib.rroi_rbox_decode_typed_hip.restype = _i
_lib.rroi_rbox_decode_typed_hip.argtypes = [_i, _vp, _vp, _vp, _i, _i, _f, _vp, _i, _vp, _vp]
_lib.rroi_ctc_greedy_decode_typed_hip.restype = _i
_lib.rroi_ctc_greedy_decode_typed_hip.argtypes = [_i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]

# the bucketed calls (header section 2b; after 0.10.0, same version string: found by symbol)
_ll = ctypes.c_longlong
_lib.rroi_align_forward_bucketed_workspace_bytes.restype = _sz
_lib.rroi_align_forward_bucketed_workspace_bytes.argtypes = [_i] * 5
_lib.rroi_align_backward_bucketed_workspace_bytes.restype = _sz
_lib.rroi_align_backward_bucketed_workspace_bytes.argtypes = [_i] * 7
_lib.rroi_align_forward_bucketed_hip.restype = _i
_lib.rroi_align_forward_bucketed_hip.argtypes = [_vp, _i, _f, _i, _i, _i, _i, _i, _i, _i, _ll, _i, _i, _vp, _vp, _vp, _sz, _i, _vp]
_lib.rroi_align_backward_bucketed_hip.restype = _i
_lib.rroi_align_backward_bucketed_hip.argtypes = [_vp, _i, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp]
_lib.rroi_align_forward_bucketed_plan.restype = _i
_lib.rroi_align_forward_bucketed_plan.argtypes = [_i] * 8 + [_ll] + [_i] * 3 + [ctypes.POINTER(_Plan)]
_lib.rroi_align_backward_bucketed_plan.restype = _i
_lib.rroi_align_backward_bucketed_plan.argtypes = [_i] * 10 + [ctypes.POINTER(_Plan)]
PLAN_KERNEL_STRIDED_RAGGED = 5
# the network's depthwise 3x3 convolution (header section 5; after 0.10.0, same version string: found by symbol)
_lib.rroi_depthwise3x3_forward_hip.restype = _i
_lib.rroi_depthwise3x3_forward_hip.argtypes = [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]
# the network's InstanceNorm2d with its activation (header section 6; after 0.10.0, same version string: found by symbol)
_d = ctypes.c_double


class _InormPlan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("form", "launches", "segments", "segment_elems", "grid_x", "block", "vector_elems", "reserved")]


_lib.rroi_instancenorm_forward_hip.restype = _i
_lib.rroi_instancenorm_forward_hip.argtypes = [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _f, _vp, _sz, _vp]
_lib.rroi_instancenorm_workspace_bytes.restype = _sz
_lib.rroi_instancenorm_workspace_bytes.argtypes = [_i] * 4
_lib.rroi_instancenorm_plan.restype = _i
_lib.rroi_instancenorm_plan.argtypes = [_i] * 5 + [ctypes.POINTER(_InormPlan)]
INORM_PLANE, INORM_SPLIT = 1, 2
# ... with the residual add or the stem's mirror fused in (header section 6b; found by symbol likewise)
_lib.rroi_instancenorm_fused_forward_hip.restype = _i
_lib.rroi_instancenorm_fused_forward_hip.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _d, _f, _vp, _sz, _vp]
# the network's detection heads and attention gate (header section 7; after 0.10.0, same version string: found by symbol)


class _HeadsPlan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("vector_elems", "channel_splits", "tiles", "grid_x", "block", "lds_bytes", "channel_block",
                                  "reserved")]


_lib.rroi_heads_forward_hip.restype = _i
_lib.rroi_heads_forward_hip.argtypes = [_i] + [_vp] * 10 + [_i] * 4 + [_d, _vp]
_lib.rroi_gate_forward_hip.restype = _i
_lib.rroi_gate_forward_hip.argtypes = [_i] + [_vp] * 4 + [_i] * 4 + [_vp]
_lib.rroi_heads_plan.restype = _i
_lib.rroi_heads_plan.argtypes = [_i] * 6 + [ctypes.POINTER(_HeadsPlan)]
# the gated merge of the network's feature merge (header section 8; after 0.10.0, same version string: found by symbol)


class _MergePlan(ctypes.Structure):
    _fields_ = ([(n, _i) for n in ("vector_elems", "channel_groups", "tiles", "grid_x", "block", "channel_block", "resize_a",
                                   "resize_gate")]
                + [(n, _d) for n in ("a_scale_y", "a_scale_x", "gate_scale_y", "gate_scale_x")])


_lib.rroi_merge_forward_hip.restype = _i
_lib.rroi_merge_forward_hip.argtypes = [_i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp]
_lib.rroi_merge_plan.restype = _i
_lib.rroi_merge_plan.argtypes = [_i] * 10 + [ctypes.POINTER(_MergePlan)]
# the network's dense 3x3 convolution on the matrix cores (header section 9; after 0.10.0, same version string: found by symbol)


class _ConvPlan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("tile_m", "tile_h", "tile_w", "k_chunk", "k_chunks", "m_tiles", "y_tiles", "x_tiles",
                                  "grid_x", "block", "lds_bytes", "out_h", "out_w", "reserved")]


_lib.rroi_conv3x3_forward_hip.restype = _i
_lib.rroi_conv3x3_forward_hip.argtypes = [_i, _vp, _vp, _vp] + [_i] * 6 + [_f, _vp]
_lib.rroi_conv3x3_plan.restype = _i
_lib.rroi_conv3x3_plan.argtypes = [_i] * 7 + [ctypes.POINTER(_ConvPlan)]
# the network's 1x1 convolution with a folded BatchNorm (header section 11; after 0.10.0, same version string: found by symbol)


class _Conv1x1Plan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("tile_m", "tile_p", "k_chunk", "k_chunks", "m_tiles", "p_tiles", "grid_x", "block",
                                  "lds_bytes", "out_h", "out_w", "reserved")]


_lib.rroi_conv1x1_forward_hip.restype = _i
_lib.rroi_conv1x1_forward_hip.argtypes = [_i, _vp, _vp, _vp] + [_i] * 6 + [_f] + [_vp] * 4 + [_d, _vp]
_lib.rroi_conv1x1_plan.restype = _i
_lib.rroi_conv1x1_plan.argtypes = [_i] * 7 + [ctypes.POINTER(_Conv1x1Plan)]
# the recogniser's head and its activation + pool (header section 10; after 0.10.0, same version string: found by symbol)


class _OcrHeadPlan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("class_block", "waves", "tile_columns", "tiles", "grid_x", "block", "lds_bytes", "max_classes")]


_lib.rroi_ocr_head_forward_hip.restype = _i
_lib.rroi_ocr_head_forward_hip.argtypes = [_i, _vp, _vp, _vp, _vp] + [_i] * 4 + [_vp]
_lib.rroi_ocr_head_plan.restype = _i
_lib.rroi_ocr_head_plan.argtypes = [_i] * 5 + [ctypes.POINTER(_OcrHeadPlan)]
_lib.rroi_act_maxpool2x1_forward_hip.restype = _i
_lib.rroi_act_maxpool2x1_forward_hip.argtypes = [_i, _vp, _vp] + [_i] * 4 + [_f, _vp]
OCR_HEAD_MAX_CLASSES = 128

EXPORTS = (
    "RROIAlignForwardLaucher", "RROIAlignBackwardLaucher", "rroi_align_forward_hip",
    "rroi_align_backward_hip", "rroi_align_forward_stages_hip", "rroi_align_forward_workspace_bytes",
    "rroi_align_backward_workspace_bytes", "rroi_align_bin_centres_hip",
    "rroi_align_sincos_probe_hip", "rroi_align_quads_to_rois_hip", "rroi_align_hip_version",
    "rroi_ctc_greedy_decode_hip", "rroi_align_backward_layout_hip", "rroi_align_forward_layout_hip",
    "rroi_align_gt_quads_to_rois_hip", "rroi_rbox_decode_hip", "rroi_nms_merge_host",
    "rroi_align_release_launcher_scratch", "rroi_align_bin_centres_trig_hip", "rroi_nms_record_format",
    "rroi_align_write_probe_hip", "rroi_align_launcher_scratch_stats",
    "rroi_align_set_trig_recipe_hip", "rroi_align_get_trig_recipe_hip",   # deprecated shims (refuse TRIG_FP32)
    "rroi_align_forward_plan", "rroi_align_backward_plan",
    "rroi_align_forward_typed_hip", "rroi_align_backward_typed_hip",
    "rroi_align_forward_plan_typed", "rroi_align_backward_plan_typed",
    "rroi_align_launcher_trig_recipe",
    "rroi_rbox_decode_typed_hip", "rroi_ctc_greedy_decode_typed_hip",
    "rroi_align_forward_bucketed_hip", "rroi_align_backward_bucketed_hip",
    "rroi_align_forward_bucketed_plan", "rroi_align_backward_bucketed_plan",
    "rroi_align_forward_bucketed_workspace_bytes", "rroi_align_backward_bucketed_workspace_bytes",
    "rroi_depthwise3x3_forward_hip",
    "rroi_instancenorm_forward_hip", "rroi_instancenorm_workspace_bytes", "rroi_instancenorm_plan",
    "rroi_heads_forward_hip", "rroi_gate_forward_hip", "rroi_heads_plan",
    "rroi_instancenorm_fused_forward_hip",
    "rroi_merge_forward_hip", "rroi_merge_plan",
    "rroi_conv3x3_forward_hip", "rroi_conv3x3_plan",
    "rroi_ocr_head_forward_hip", "rroi_ocr_head_plan", "rroi_act_maxpool2x1_forward_hip",
    "rroi_conv1x1_forward_hip", "rroi_conv1x1_plan",
    "rroi_conv2x3_forward_hip", "rroi_conv2x3_plan", "rroi_up_depthwise3x3_forward_hip",   # bound in remainder.py
    "rroi_preprocess_forward_hip", "rroi_preprocess_plan",   # bound in preprocess.py
    "rroi_ctc_loss_forward_hip", "rroi_ctc_loss_plan", "rroi_ctc_loss_workspace_bytes",   # bound in ctc_loss.py
    "rroi_detection_loss_forward_hip", "rroi_detection_loss_backward_hip", "rroi_detection_loss_plan",
    "rroi_detection_loss_workspace_bytes",   # bound in detection_loss.py
)

# What a call launches (rroi_align_forward_plan / rroi_align_backward_plan); the fields of rroi_align_plan.
Plan = collections.namedtuple("Plan", [n for n, _ in _Plan._fields_])


def _plan(fn, args, what):
    p = _Plan()
    if fn(*(int(a) for a in args), ctypes.byref(p)) != 1:
        raise ValueError(f"{what}: the call would refuse these arguments")
    return Plan(*(getattr(p, n) for n in Plan._fields))


def dtype_code(dtype) -> int:
    """DTYPE_* of a torch dtype (float32, bfloat16, float16) or of a DTYPE_* value; TypeError for anything else."""
    if isinstance(dtype, torch.dtype):
        if dtype not in _DTYPES:
            raise TypeError(f"rroi_align takes float32, bfloat16 or float16 tensors, got {dtype}")
        return _DTYPES[dtype]
    return int(dtype)


def forward_plan(batch_size, channels, height, width, num_rois, pooled_height, pooled_width,
                 feature_layout=LAYOUT_NCHW, top_layout=LAYOUT_NCHW, path=PATH_AUTO, caller=CALLER_NATIVE,
                 trig=0, dtype=DTYPE_FP32) -> Plan:
    """The plan a forward call with these arguments runs (host only, no GPU needed); ValueError where the call
    would refuse them.  dtype: of the features and crops (a torch dtype or DTYPE_*; the default is the fp32 query)."""
    args = (dtype_code(dtype), feature_layout, top_layout, batch_size, num_rois, height, width, channels, pooled_height,
            pooled_width, _path_word(path, trig), caller)
    return _plan(_lib.rroi_align_forward_plan_typed, args, "rroi_align_forward_plan_typed")


def backward_plan(batch_size, channels, height, width, num_rois, pooled_height, pooled_width,
                  top_diff_layout=LAYOUT_NCHW, bottom_diff_layout=LAYOUT_NCHW, path=PATH_AUTO, caller=CALLER_NATIVE,
                  trig=0, dtype=DTYPE_FP32, deterministic=False) -> Plan:
    """The plan a backward call with these arguments runs (host only, no GPU needed); ValueError where the call
    would refuse them.  dtype: of grad_output and the gradient (a torch dtype or DTYPE_*; the default is the fp32
    query).  deterministic: the query of a call with PATH_DETERMINISTIC (backward(deterministic=True))."""
    args = (dtype_code(dtype), top_diff_layout, bottom_diff_layout, batch_size, num_rois, height, width, channels,
            pooled_height, pooled_width, _path_word(path, trig, deterministic), caller)
    return _plan(_lib.rroi_align_backward_plan_typed, args, "rroi_align_backward_plan_typed")


def version() -> str:
    return _lib.rroi_align_hip_version().decode()


# The one library-dependent step of the arithmetic (rroi_align_kernel.cu:73-74): TRIG_DOUBLE (default; the oracle's
# recipe, (float)cos((double)angle)) or TRIG_FP32 (the device library's cosf / sinf -- what the reference's own sources
# evaluate when built for this GPU; bit-exact against that build in every bin).  PER CALL since round 5: the `trig=`
# keyword of forward() / backward() / bin_centres() sets the RROI_PATH_TRIG_FP32 bit of the call's `path`; a kernel
# argument, so two streams may run different recipes at once and either is capturable into a graph.
TRIG_DOUBLE, TRIG_FP32 = 0, 1
PATH_TRIG_FP32 = 0x100
# The deterministic backward: backward(deterministic=True) sets this bit of `path` and runs the ORDERED plan
# -- every gradient element summed in double in the oracle's order and rounded once, the same bits on every run.  With
# PATH_AUTO only.  A backward flag: the forward is deterministic as it is, and its entry points refuse the bit.
PATH_DETERMINISTIC = 0x200


def _path_word(path: int, trig: int, deterministic: bool = False) -> int:
    if trig not in (TRIG_DOUBLE, TRIG_FP32):
        raise ValueError(f"trig must be TRIG_DOUBLE (0) or TRIG_FP32 (1), got {trig!r}")
    return int(path) | (PATH_TRIG_FP32 if trig == TRIG_FP32 else 0) | (PATH_DETERMINISTIC if deterministic else 0)


def _check(status: int, what: str) -> None:
    if status == 1:
        return
    if status == 0:
        raise ValueError(f"{what}: invalid argument (shape/layout/workspace)")
    raise RuntimeError(f"{what}: HIP error {-status}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# Scratch for the tiled paths, one buffer per (device, stream), grown on demand and reused: calls on
# one stream are ordered, so the next call may overwrite what the previous one left (the contents
# are dead after a call); another stream gets its own buffer.  Saves the allocator round trip per call.
# What is kept is bounded: a request above _SCRATCH_KEEP_BYTES (the backward of a 4096-ROI problem asks
# for 2.4 GB) is served by a plain allocation that goes back to torch's caching allocator with the call,
# at most _SCRATCH_MAX_STREAMS buffers are kept (least recently used first out; a buffer whose stream
# has been destroyed ages out this way), and the table is guarded by a lock.
_SCRATCH_KEEP_BYTES = 512 << 20
_SCRATCH_MAX_STREAMS = 8
_scratch = collections.OrderedDict()
_scratch_lock = threading.Lock()


def _workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    if nbytes > _SCRATCH_KEEP_BYTES or torch.cuda.is_current_stream_capturing():
        # too large to pin, or a graph owns its memory: nothing of it is cached
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    with _scratch_lock:
        buf = _scratch.get(key)
        if buf is not None and buf.numel() >= nbytes:
            _scratch.move_to_end(key)
            return buf
        buf = None
        _scratch.pop(key, None)           # release the smaller buffer before asking for the larger one
        while len(_scratch) >= _SCRATCH_MAX_STREAMS:
            _scratch.popitem(last=False)
        buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        _scratch[key] = buf
        return buf


def release_workspaces() -> None:
    """Drop the cached scratch buffers -- the Python surface's and the library's own (the per-stream
    scratch of the reference-ABI launchers); all of them are re-created on demand."""
    with _scratch_lock:
        _scratch.clear()
    _check(_lib.rroi_align_release_launcher_scratch(), "rroi_align_release_launcher_scratch")


def launcher_scratch_stats() -> dict:
    """State of the library's scratch table for the reference-ABI launchers (see the header)."""
    u, p, c, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_ulonglong()
    _lib.rroi_align_launcher_scratch_stats(ctypes.byref(u), ctypes.byref(p), ctypes.byref(c), ctypes.byref(t))
    return {"in_use": u.value, "pinned": p.value, "capacity": c.value, "transient_calls": t.value}


def _require_cuda_f32(t: torch.Tensor, name: str, dtypes=(torch.float32,)) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on {t.device}: rroi_align runs on the GPU only (the reference's CPU "
            "branch, functions/rroi_align.py:22-25, is dead code and is not reproduced)")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, got {t.dtype}")


_IO_DTYPES = (torch.float32, torch.bfloat16, torch.float16)   # features / crops, grad_output / gradient


def _require_features_rois(features: torch.Tensor, rois: torch.Tensor) -> int:
    """What forward() and forward_bucketed() ask of their tensors; returns the DTYPE_* of the features."""
    _require_cuda_f32(features, "features", _IO_DTYPES)
    _require_cuda_f32(rois, "rois")
    if features.dim() != 4:
        raise ValueError(f"features must be (B,C,H,W), got {tuple(features.shape)}")
    if rois.dim() != 2 or rois.size(1) != 6:
        raise ValueError(f"rois must be (R,6) [batch,cx,cy,h,w,angle_deg], got {tuple(rois.shape)}")
    if rois.device != features.device:
        raise ValueError("features and rois must be on the same device")
    return _DTYPES[features.dtype]


# --------------------------------------------------------------------------- native path
def forward(features: torch.Tensor, rois: torch.Tensor, pooled_height: int, pooled_width: int,
            spatial_scale: float, path: int = PATH_AUTO, channels_last_out: bool = False,
            trig: int = TRIG_DOUBLE) -> torch.Tensor:
    """(B,C,H,W) x (R,6) -> (R,C,PH,PW).  NCHW-contiguous or channels_last features.
    channels_last_out: return the crops in channels_last storage (same values) for a recognition
    head that runs in channels_last; needs C % 4 == 0 and the tiled path.
    trig: TRIG_DOUBLE / TRIG_FP32, for this call (pass the same to backward()).
    features: float32, bfloat16 or float16 -- the crops have the same dtype (a 16-bit call computes in fp32 and rounds
    each crop element once: bit for bit the fp32 call on the widened map, rounded; channels_last 16-bit features are
    made contiguous first, PATH_FUSED is fp32 only).  rois: float32."""
    word = _path_word(path, trig)
    code = _require_features_rois(features, rois)
    B, C, H, W = features.shape
    R = rois.size(0)
    ph, pw = int(pooled_height), int(pooled_width)
    if ph <= 0 or pw <= 0:
        raise ValueError("pooled_height and pooled_width must be positive")
    if features.is_contiguous():
        layout = LAYOUT_NCHW
    elif (features.is_contiguous(memory_format=torch.channels_last) and C % 4 == 0 and path not in (PATH_DIRECT, PATH_FUSED)
          and code == DTYPE_FP32):
        layout = LAYOUT_NHWC  # consumed in place: a pixel's channels are already contiguous
    else:
        features, layout = features.contiguous(), LAYOUT_NCHW
    rois = rois.contiguous()
    if channels_last_out and (C % 4 != 0 or path in (PATH_DIRECT, PATH_FUSED)):
        raise ValueError("channels_last_out needs C % 4 == 0 and the tiled path")
    with torch.cuda.device_of(features):
        out = torch.empty((R, C, ph, pw), dtype=features.dtype, device=features.device,
                          memory_format=torch.channels_last if channels_last_out else torch.contiguous_format)
        if R == 0 or out.numel() == 0:
            return out
        nbytes = 0 if path in (PATH_DIRECT, PATH_FUSED) else _lib.rroi_align_forward_workspace_bytes(B, C, H, W, R, layout)
        ws = _workspace(features.device, nbytes)
        top_layout = LAYOUT_NHWC if channels_last_out else LAYOUT_NCHW
        st = _lib.rroi_align_forward_typed_hip(features.data_ptr(), code, layout, top_layout, float(spatial_scale),
                                               B, R, H, W, C, ph, pw, rois.data_ptr(), out.data_ptr(),
                                               ws.data_ptr(), nbytes, word, _stream())
    _check(st, "rroi_align_forward_typed_hip")
    return out


def backward(grad_output: torch.Tensor, rois: torch.Tensor, feature_size, spatial_scale: float,
             path: int = PATH_AUTO, channels_last_grad: bool = False, trig: int = TRIG_DOUBLE,
             deterministic: bool = False) -> torch.Tensor:
    """(R,C,PH,PW) -> grad w.r.t. features (B,C,H,W): NCHW contiguous, or (channels_last_grad, for a
    channels_last backbone; needs C % 4 == 0 and the tiled path) in channels_last storage.
    trig: the recipe the forward of these crops ran with.
    grad_output: float32, bfloat16 or float16 -- the gradient has the same dtype (a 16-bit call sums every gradient
    element in fp32 and rounds it once; a channels_last 16-bit grad_output is made contiguous first; PATH_DIRECT and
    PATH_TILED_ATOMIC are fp32 only).  rois: float32.
    deterministic: run the ORDERED plan (PATH_DETERMINISTIC, with path=PATH_AUTO only): the same bits on every run, equal
    to the oracle's double-precision sum in statement order rounded once (16-bit: that fp32 gradient rounded)."""
    word = _path_word(path, trig, deterministic)
    _require_cuda_f32(grad_output, "grad_output", _IO_DTYPES)
    _require_cuda_f32(rois, "rois")
    code = _DTYPES[grad_output.dtype]
    B, C, H, W = (int(v) for v in feature_size)
    if grad_output.dim() != 4 or grad_output.size(1) != C or grad_output.size(0) != rois.size(0):
        raise ValueError("grad_output must be (R,C,PH,PW) matching rois and the feature size")
    R, _, ph, pw = grad_output.shape
    # channels_last storage (R, PH, PW, C) -- what autograd hands over when the recognition head
    # runs in channels_last -- is consumed in place by the gather path: no .contiguous() copy of
    # the 256 MiB, no relayout pass
    layout = LAYOUT_NCHW
    if (not grad_output.is_contiguous() and grad_output.is_contiguous(memory_format=torch.channels_last)
            and C % 4 == 0 and path in (PATH_AUTO,) + GATHER_PATHS and R > 0 and code == DTYPE_FP32):
        layout = LAYOUT_NHWC
    else:
        grad_output = grad_output.contiguous()
    rois = rois.contiguous()
    cl_grad = bool(channels_last_grad) and C % 4 == 0 and path in (PATH_AUTO,) + GATHER_PATHS and R > 0
    with torch.cuda.device_of(grad_output):
        grad_in = torch.empty((B, C, H, W), dtype=grad_output.dtype, device=grad_output.device,
                              memory_format=torch.channels_last if cl_grad else torch.contiguous_format)
        if grad_in.numel() == 0:
            return grad_in
        nbytes = 0 if path == PATH_DIRECT else _lib.rroi_align_backward_workspace_bytes(B, C, H, W, R, ph, pw)
        ws = _workspace(grad_output.device, nbytes)
        bottom_layout = LAYOUT_NHWC if cl_grad else LAYOUT_NCHW
        st = _lib.rroi_align_backward_typed_hip(grad_output.data_ptr(), code, layout, bottom_layout,
                                                float(spatial_scale), B, R, H, W, C, ph, pw, rois.data_ptr(),
                                                grad_in.data_ptr(), ws.data_ptr(), nbytes, word, _stream())
    _check(st, "rroi_align_backward_typed_hip")
    return grad_in


# --------------------------------------------------------------------------- bucketed calls (header section 2b)
def bucket_layout(widths):
    """Pure host: the ROIs 0 .. R-1 split by pooled width -> [(width, [roi indices])], widths ascending, the ROI order
    kept inside a bucket (a stable split: the index lists together are a permutation of range(R))."""
    groups = {}
    for i, w in enumerate(widths):
        w = int(w)
        if w < 1:
            raise ValueError(f"pooled widths must be >= 1, got {w} for ROI {i}")
        groups.setdefault(w, []).append(i)
    return [(w, groups[w]) for w in sorted(groups)]


def crop_table(addresses, widths, device) -> torch.Tensor:
    """The device table of a bucketed call from host lists: (R, 2) int64 = rroi_align_crop rows {address, width | 0}."""
    rows = [[int(a), int(w) & 0xffffffff] for a, w in zip(addresses, widths)]
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).to(device)


def _pow2_divisor(values, cap=4096) -> int:
    """The largest power of two (<= cap) that divides every value."""
    a = cap
    for v in values:
        v = int(v)
        if v:
            a = min(a, v & -v)
    return a


class _BucketTables(object):
    """What a width list needs on the device, built once and cached: the buckets' index tensors and the tables' constant
    parts -- a call then costs one tiny add per distinct base address, with the address as a kernel argument (no upload,
    so the call can be captured into a graph)."""

    def __init__(self, widths, channels, pooled_height, itemsize, device):
        self.widths = tuple(int(w) for w in widths)
        self.buckets = bucket_layout(self.widths)
        R = len(self.widths)
        self.max_width = max(self.widths) if R else 0
        self.sum_widths = sum(self.widths)
        g = 0
        for w in self.widths:
            g = _gcd(g, w)
        self.width_multiple = max(g, 1)
        self.offsets, at = [], 0            # element offset of every bucket in the forward's one buffer, 256-byte aligned
        fwd = [[0, 0] for _ in range(R)]    # [byte offset in that buffer, width]
        bwd = [[0, 0] for _ in range(R)]    # [byte offset in the bucket's own tensor, width]
        in_bucket, width_of = [], []
        per = 256 // itemsize
        for w, idx in self.buckets:
            crop = channels * pooled_height * w
            self.offsets.append(at)
            hot, wd = [[0, 0] for _ in range(R)], [[0, 0] for _ in range(R)]
            for j, i in enumerate(idx):
                fwd[i] = [(at + j * crop) * itemsize, w]
                bwd[i] = [j * crop * itemsize, w]
                hot[i] = [1, 0]
                wd[i] = [0, w]
            in_bucket.append(hot)
            width_of.append(wd)
            at = (at + len(idx) * crop + per - 1) // per * per
        self.total = at
        # what divides every crop's offset from a bucket's base: with the bases' own alignment, the crops' alignment
        self.offset_alignment = _pow2_divisor([r[0] for r in fwd] + [r[0] for r in bwd])

        def up(rows):
            return torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).to(device)
        self.idx = [torch.tensor(idx, dtype=torch.int64).to(device) for _, idx in self.buckets]
        self.fwd_rel, self.bwd_rel = up(fwd), up(bwd)
        self.addr_col = up([[1, 0]] * R)
        self.in_bucket = [up(h) for h in in_bucket]
        self.width_of = [up(w) for w in width_of]


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


_tables = collections.OrderedDict()
_TABLES_MAX = 32


def _bucket_tables(widths, channels, pooled_height, itemsize, device) -> _BucketTables:
    key = (device.index, tuple(int(w) for w in widths), int(channels), int(pooled_height), int(itemsize))
    with _scratch_lock:
        t = _tables.get(key)
        if t is not None:
            _tables.move_to_end(key)
            return t
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("bucketed rroi_align: run this width list once outside the capture (its tables are uploaded "
                           "on first use)")
    t = _BucketTables(key[1], channels, pooled_height, itemsize, device)
    with _scratch_lock:
        _tables[key] = t
        while len(_tables) > _TABLES_MAX:
            _tables.popitem(last=False)
    return t


def _bucketed_stats(widths):
    widths = [int(w) for w in widths]
    g = 0
    for w in widths:
        g = _gcd(g, w)
    return len(widths), (max(widths) if widths else 1), sum(widths), max(g, 1)


def forward_bucketed_plan(batch_size, channels, height, width, pooled_height, widths, path=PATH_AUTO, trig=0,
                          dtype=DTYPE_FP32, crop_alignment=256) -> Plan:
    """The plan a bucketed forward of these pooled widths runs (host only); ValueError where the call would refuse."""
    R, mx, sm, g = _bucketed_stats(widths)
    return _plan(_lib.rroi_align_forward_bucketed_plan,
                 (dtype_code(dtype), batch_size, R, height, width, channels, pooled_height, mx, sm, g, crop_alignment,
                  _path_word(path, trig)), "rroi_align_forward_bucketed_plan")


def backward_bucketed_plan(batch_size, channels, height, width, pooled_height, widths, path=PATH_AUTO, trig=0,
                           dtype=DTYPE_FP32, bottom_diff_layout=LAYOUT_NCHW, deterministic=False) -> Plan:
    """The plan a bucketed backward of these pooled widths runs (host only); ValueError where the call would refuse."""
    R, mx, _, _ = _bucketed_stats(widths)
    return _plan(_lib.rroi_align_backward_bucketed_plan,
                 (dtype_code(dtype), bottom_diff_layout, batch_size, R, height, width, channels, pooled_height, mx,
                  _path_word(path, trig, deterministic)), "rroi_align_backward_bucketed_plan")


def forward_bucketed(features: torch.Tensor, rois: torch.Tensor, pooled_height: int, widths, spatial_scale: float,
                     path: int = PATH_AUTO, trig: int = TRIG_DOUBLE):
    """RoIRotate with one pooled width PER ROI, in one launch chain: (B,C,H,W) x (R,6) x R host ints ->
    [(index LongTensor (R_b,), crops (R_b, C, PH, W_b))] in ascending width, ROI order kept inside a bucket.  Crop j of a
    bucket is bit for bit forward(features, rois[index], PH, W_b)[j]: nothing wider is written and nothing is sliced or
    copied afterwards.  The buckets are views of ONE allocation (each starts on a 256-byte boundary).
    features: float32, bfloat16 or float16, made NCHW-contiguous; rois float32; path: PATH_AUTO / PATH_DIRECT / PATH_TILED."""
    word = _path_word(path, trig)
    code = _require_features_rois(features, rois)
    B, C, H, W = features.shape
    R, ph = rois.size(0), int(pooled_height)
    if len(widths) != R:
        raise ValueError(f"widths must have one entry per ROI: {len(widths)} for {R}")
    if ph <= 0:
        raise ValueError("pooled_height must be positive")
    if R == 0:
        return []
    features, rois = features.contiguous(), rois.contiguous()
    with torch.cuda.device_of(features):
        t = _bucket_tables(widths, C, ph, features.element_size(), features.device)
        buf = torch.empty((t.total,), dtype=features.dtype, device=features.device)
        out = [(t.idx[b], buf[off:off + len(idx) * C * ph * w].view(len(idx), C, ph, w))
               for b, ((w, idx), off) in enumerate(zip(t.buckets, t.offsets))]
        if buf.numel() == 0:
            return out
        table = torch.add(t.fwd_rel, t.addr_col, alpha=buf.data_ptr())
        align = min(_pow2_divisor([buf.data_ptr()]), t.offset_alignment)
        nbytes = 0 if path == PATH_DIRECT else _lib.rroi_align_forward_bucketed_workspace_bytes(B, C, H, W, R)
        ws = _workspace(features.device, nbytes)
        st = _lib.rroi_align_forward_bucketed_hip(features.data_ptr(), code, float(spatial_scale), B, R, H, W, C, ph,
                                                  t.max_width, t.sum_widths, t.width_multiple, align, rois.data_ptr(),
                                                  table.data_ptr(), ws.data_ptr(), nbytes, word, _stream())
    _check(st, "rroi_align_forward_bucketed_hip")
    return out


def backward_bucketed(grads, rois: torch.Tensor, feature_size, pooled_height: int, widths, spatial_scale: float,
                      path: int = PATH_AUTO, channels_last_grad: bool = False, trig: int = TRIG_DOUBLE,
                      deterministic: bool = False) -> torch.Tensor:
    """The counterpart: `grads` = one (R_b, C, PH, W_b) tensor (or None: that bucket contributes nothing) per bucket of
    bucket_layout(widths), in its order -> grad w.r.t. the features (B,C,H,W), NCHW or (channels_last_grad) channels_last.
    Every gradient tensor is consumed where it is (a non-contiguous one is made contiguous, bucket by bucket): no
    concatenation, no padding to the widest width.  path: PATH_AUTO, PATH_TILED_LISTS or PATH_TILED_BUCKETS;
    deterministic: the ORDERED plan (with PATH_AUTO) -- the bits of the dense deterministic backward on zero-padded crops."""
    word = _path_word(path, trig, deterministic)
    _require_cuda_f32(rois, "rois")
    B, C, H, W = (int(v) for v in feature_size)
    R, ph = rois.size(0), int(pooled_height)
    if len(widths) != R:
        raise ValueError(f"widths must have one entry per ROI: {len(widths)} for {R}")
    layout = bucket_layout(widths)
    grads = list(grads)
    if len(grads) != len(layout):
        raise ValueError(f"one gradient (or None) per bucket: {len(grads)} for {len(layout)} buckets")
    given = [g for g in grads if g is not None]
    dtype = given[0].dtype if given else torch.float32
    for g, (w, idx) in zip(grads, layout):
        if g is None:
            continue
        _require_cuda_f32(g, "grads[...]", _IO_DTYPES)
        if g.dtype != dtype or g.device != rois.device or tuple(g.shape) != (len(idx), C, ph, w):
            raise ValueError(f"the gradient of the width-{w} bucket must be {(len(idx), C, ph, w)} {dtype} on {rois.device}, "
                             f"got {tuple(g.shape)} {g.dtype} on {g.device}")
    rois = rois.contiguous()
    cl_grad = bool(channels_last_grad) and C % 4 == 0 and R > 0
    with torch.cuda.device_of(rois):
        grad_in = torch.empty((B, C, H, W), dtype=dtype, device=rois.device,
                              memory_format=torch.channels_last if cl_grad else torch.contiguous_format)
        if grad_in.numel() == 0:
            return grad_in
        if not given:
            return grad_in.zero_()
        code = _DTYPES[dtype]
        t = _bucket_tables(widths, C, ph, given[0].element_size(), rois.device)
        keep = []   # (the contiguous copies live until the launches are enqueued on this stream)
        table = t.bwd_rel
        for b, g in enumerate(grads):
            if g is None:
                table = torch.sub(table, t.width_of[b])          # width 0: the rows are skipped
            else:
                g = g.contiguous()
                keep.append(g)
                table = torch.add(table, t.in_bucket[b], alpha=g.data_ptr())
        nbytes = _lib.rroi_align_backward_bucketed_workspace_bytes(B, C, H, W, R, ph, t.max_width)
        ws = _workspace(rois.device, nbytes)
        st = _lib.rroi_align_backward_bucketed_hip(table.data_ptr(), code, LAYOUT_NHWC if cl_grad else LAYOUT_NCHW,
                                                   float(spatial_scale), B, R, H, W, C, ph, t.max_width, rois.data_ptr(),
                                                   grad_in.data_ptr(), ws.data_ptr(), nbytes, word, _stream())
    _check(st, "rroi_align_backward_bucketed_hip")
    return grad_in


# --------------------------------------------------------------------------- depthwise 3x3 (header section 5)
def depthwise3x3(x: torch.Tensor, weight: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """(N,C,H,W) x (C,1,3,3) -> (N,C,Ho,Wo): depthwise 3x3 convolution, padding 1, no bias, stride 1 or 2.
    float32, bfloat16 or float16, x and weight alike; x is made NCHW-contiguous.  Every output is the double sum of its
    nine widened products in (ky, kx) order, rounded to fp32 once and then to the tensors' type: the same bits on every
    run.  Forward only (no autograd).  ValueError for mismatched shapes or dtypes, RuntimeError for CPU tensors."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor):
        raise TypeError("x and weight must be torch.Tensors")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,C,H,W), got {tuple(x.shape)}")
    N, C, H, W = x.shape
    if tuple(weight.shape) != (C, 1, 3, 3):
        raise ValueError(f"weight must be {(C, 1, 3, 3)} for x {tuple(x.shape)}, got {tuple(weight.shape)}")
    if weight.dtype != x.dtype:
        raise ValueError(f"x and weight must have one dtype, got {x.dtype} and {weight.dtype}")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2, got {stride!r}")
    _require_cuda_f32(x, "x", _IO_DTYPES)
    _require_cuda_f32(weight, "weight", _IO_DTYPES)
    if weight.device != x.device:
        raise ValueError("x and weight must be on the same device")
    if C < 1 or H < 1 or W < 1:
        raise ValueError(f"x must have at least one channel, row and column, got {tuple(x.shape)}")
    return _depthwise3x3_run(x.contiguous(), weight, int(stride))


def _depthwise3x3_run(x: torch.Tensor, weight: torch.Tensor, stride: int) -> torch.Tensor:
    """The call itself, for arguments already checked (depthwise3x3 above; fots_e2e.native after native_ok): x is a
    contiguous CUDA (N,C,H,W) tensor, weight (C,1,3,3) of its dtype and device, stride 1 or 2.  Kept lean: a network pass
    makes 22 of these calls and the one-image leg of the pipeline is bound by host time."""
    N, C, H, W = x.shape
    weight = weight.contiguous()
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _depthwise3x3_run(x, weight, stride)
    out = torch.empty((N, C, (H - 1) // stride + 1, (W - 1) // stride + 1), dtype=x.dtype, device=x.device)
    if N == 0:
        return out
    st = _lib.rroi_depthwise3x3_forward_hip(_DTYPES[x.dtype], x.data_ptr(), weight.data_ptr(), out.data_ptr(), N, C, H, W,
                                            stride, _stream())
    if st != 1:
        _check(st, "rroi_depthwise3x3_forward_hip")
    return out


# --------------------------------------------------------------------------- InstanceNorm2d (header section 6)
InstanceNormPlan = collections.namedtuple("InstanceNormPlan", [n for n, _ in _InormPlan._fields_[:-1]])


def instance_norm_plan(batch_size, channels, height, width, dtype=DTYPE_FP32) -> InstanceNormPlan:
    """What `instance_norm` launches for a tensor of this shape (host only, no GPU needed: 256 CUs are assumed without
    one): the form (INORM_PLANE / INORM_SPLIT), its launches, segments per plane, elements per segment, the grid.
    ValueError where the call would refuse the arguments."""
    p = _InormPlan()
    if _lib.rroi_instancenorm_plan(dtype_code(dtype), int(batch_size), int(channels), int(height), int(width),
                                   ctypes.byref(p)) != 1:
        raise ValueError("rroi_instancenorm_plan: the call would refuse these arguments")
    return InstanceNormPlan(*(getattr(p, n) for n in InstanceNormPlan._fields))


def instance_norm_workspace_bytes(batch_size, channels, height, width) -> int:
    """Bytes of workspace `rroi_instancenorm_forward_hip` needs for this shape: 0 in the plane form."""
    return int(_lib.rroi_instancenorm_workspace_bytes(int(batch_size), int(channels), int(height), int(width)))


def instance_norm(x: torch.Tensor, weight=None, bias=None, eps: float = 1e-5, negative_slope: float = 1.0) -> torch.Tensor:
    """InstanceNorm2d of (N,C,H,W) `x` over each (n, c) plane (biased variance, instance statistics), then
    `v < 0 ? v * negative_slope : v` (1.0: no activation, 0.0: ReLU) -- DESIGN 5.11.  float32, bfloat16 or float16;
    weight and bias are (C,) of x's dtype, or both None.  x is made NCHW-contiguous.  Statistics in double, shifted by the
    plane's first element; one rounding to fp32 and one to the tensor's type; the same bits on every run.  Forward only (no
    autograd).  ValueError for mismatched shapes or dtypes, RuntimeError for CPU tensors."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,C,H,W), got {tuple(x.shape)}")
    if (weight is None) != (bias is None):
        raise ValueError("weight and bias come together, or neither")
    C = x.size(1)
    for name, p in (("weight", weight), ("bias", bias)):
        if p is None:
            continue
        if not isinstance(p, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if tuple(p.shape) != (C,):
            raise ValueError(f"{name} must be {(C,)} for x {tuple(x.shape)}, got {tuple(p.shape)}")
        if p.dtype != x.dtype:
            raise ValueError(f"x and {name} must have one dtype, got {x.dtype} and {p.dtype}")
    _require_cuda_f32(x, "x", _IO_DTYPES)
    for name, p in (("weight", weight), ("bias", bias)):
        if p is not None:
            _require_cuda_f32(p, name, _IO_DTYPES)
            if p.device != x.device:
                raise ValueError(f"x and {name} must be on the same device")
    if C < 1 or x.size(2) < 1 or x.size(3) < 1:
        raise ValueError(f"x must have at least one channel, row and column, got {tuple(x.shape)}")
    if weight is not None:
        weight, bias = weight.contiguous(), bias.contiguous()
    return _instance_norm_run(x.contiguous(), weight, bias, float(eps), float(negative_slope))


def _instance_norm_run(x: torch.Tensor, weight, bias, eps: float, negative_slope: float) -> torch.Tensor:
    """The call itself, for arguments already checked (instance_norm above; fots_e2e.native after instancenorm_ok): x is a
    contiguous CUDA (N,C,H,W) tensor, weight and bias contiguous (C,) of its dtype and device or both None.  Kept lean: a
    network pass makes 49 of these calls and the one-image leg of the pipeline is bound by host time."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _instance_norm_run(x, weight, bias, eps, negative_slope)
    out = torch.empty_like(x)
    N, C, H, W = x.shape
    if N == 0:
        return out
    nbytes = _lib.rroi_instancenorm_workspace_bytes(N, C, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    st = _lib.rroi_instancenorm_forward_hip(_DTYPES[x.dtype], x.data_ptr(), None if weight is None else weight.data_ptr(),
                                            None if bias is None else bias.data_ptr(), out.data_ptr(), N, C, H, W, eps,
                                            negative_slope, None if ws is None else ws.data_ptr(), nbytes, _stream())
    if st != 1:
        _check(st, "rroi_instancenorm_forward_hip")
    return out


def instance_norm_fused(x: torch.Tensor, weight=None, bias=None, eps: float = 1e-5, negative_slope: float = 1.0,
                        residual=None, mirror: bool = False) -> torch.Tensor:
    """`instance_norm` with an epilogue fused in -- DESIGN 5.13.
    residual (x's shape, dtype and device):  act(instance_norm(x) + residual), the sum in fp32 and rounded once: the tail
    of a residual block in one call.
    mirror:  the InstanceNorm2d of `torch.cat((x, -x), 1)` with its activation, without the concatenation: (N,2C,H,W) from
    (N,C,H,W); weight and bias are (2C,) or both None.  Not together with a residual.
    With neither, `instance_norm`.  The same exceptions as `instance_norm`; ValueError also for a residual whose shape,
    dtype or device is not x's, for mirror together with a residual, and for a weight that is not (2C,) under mirror."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,C,H,W), got {tuple(x.shape)}")
    if (weight is None) != (bias is None):
        raise ValueError("weight and bias come together, or neither")
    mirror = bool(mirror)
    if mirror and residual is not None:
        raise ValueError("mirror takes no residual")
    features = x.size(1) * (2 if mirror else 1)
    for name, p in (("weight", weight), ("bias", bias)):
        if p is None:
            continue
        if not isinstance(p, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if tuple(p.shape) != (features,):
            raise ValueError(f"{name} must be {(features,)} for x {tuple(x.shape)}{' mirrored' if mirror else ''}, "
                             f"got {tuple(p.shape)}")
        if p.dtype != x.dtype:
            raise ValueError(f"x and {name} must have one dtype, got {x.dtype} and {p.dtype}")
    if residual is not None:
        if not isinstance(residual, torch.Tensor):
            raise TypeError("residual must be a torch.Tensor")
        if residual.shape != x.shape:
            raise ValueError(f"residual must have x's shape {tuple(x.shape)}, got {tuple(residual.shape)}")
        if residual.dtype != x.dtype:
            raise ValueError(f"x and residual must have one dtype, got {x.dtype} and {residual.dtype}")
        if residual.device != x.device:
            raise ValueError("x and residual must be on the same device")
    _require_cuda_f32(x, "x", _IO_DTYPES)
    for name, p in (("weight", weight), ("bias", bias)):
        if p is not None:
            _require_cuda_f32(p, name, _IO_DTYPES)
            if p.device != x.device:
                raise ValueError(f"x and {name} must be on the same device")
    if features < 1 or x.size(2) < 1 or x.size(3) < 1:
        raise ValueError(f"x must have at least one channel, row and column, got {tuple(x.shape)}")
    if mirror and 2 * x.numel() >= 1 << 31:
        raise ValueError(f"the mirrored output of x {tuple(x.shape)} has 2^31 elements or more")
    if weight is not None:
        weight, bias = weight.contiguous(), bias.contiguous()
    if residual is None and not mirror:
        return _instance_norm_run(x.contiguous(), weight, bias, float(eps), float(negative_slope))
    return _instance_norm_fused_run(x.contiguous(), weight, bias, float(eps), float(negative_slope),
                                    None if residual is None else residual.contiguous(), mirror)


def _instance_norm_fused_run(x: torch.Tensor, weight, bias, eps: float, negative_slope: float, residual, mirror: bool) -> torch.Tensor:
    """The call itself, for arguments already checked (instance_norm_fused above; fots_e2e.native after fused_norm_ok): as
    `_instance_norm_run`, with `residual` a contiguous tensor like x or None, and under `mirror` weight and bias (2C,) and
    no residual.  Kept lean for the same reason."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _instance_norm_fused_run(x, weight, bias, eps, negative_slope, residual, mirror)
    N, C, H, W = x.shape
    out = torch.empty((N, 2 * C, H, W), dtype=x.dtype, device=x.device) if mirror else torch.empty_like(x)
    if N == 0:
        return out
    nbytes = _lib.rroi_instancenorm_workspace_bytes(N, C, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    st = _lib.rroi_instancenorm_fused_forward_hip(
        _DTYPES[x.dtype], x.data_ptr(), None if weight is None else weight.data_ptr(), None if bias is None else bias.data_ptr(),
        None if residual is None else residual.data_ptr(), out.data_ptr(), N, C, H, W, 1 if mirror else 0, eps, negative_slope,
        None if ws is None else ws.data_ptr(), nbytes, _stream())
    if st != 1:
        _check(st, "rroi_instancenorm_fused_forward_hip")
    return out


# --------------------------------------------------------------------------- heads and gate (header section 7)
HeadsPlan = collections.namedtuple("HeadsPlan", [n for n, _ in _HeadsPlan._fields_[:-1]])


def heads_plan(batch_size, channels, height, width, outputs=7, dtype=DTYPE_FP32) -> HeadsPlan:
    """What `heads` (outputs=7) or `gate` (outputs=1) launches for a map of this shape (host only, no GPU needed: 256 CUs
    are assumed without one): pixels per lane V, channel splits S, tiles per image, grid, block, LDS bytes, channels per
    wave.  ValueError where the call would refuse the arguments."""
    p = _HeadsPlan()
    if _lib.rroi_heads_plan(dtype_code(dtype), int(outputs), int(batch_size), int(channels), int(height), int(width),
                            ctypes.byref(p)) != 1:
        raise ValueError("rroi_heads_plan: the call would refuse these arguments")
    return HeadsPlan(*(getattr(p, n) for n in HeadsPlan._fields))


def _require_pointwise(x, pairs):
    """The checks `heads` and `gate` share: x (N,C,H,W); every (name, weight, bias, k): weight (k,C) or (k,C,1,1), bias
    (k,) or None, of x's dtype and device.  Returns the contiguous (weight, bias) pairs."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,C,H,W), got {tuple(x.shape)}")
    C = x.size(1)
    for name, w, b, k in pairs:
        if not isinstance(w, torch.Tensor) or not (b is None or isinstance(b, torch.Tensor)):
            raise TypeError(f"{name}: weight must be a torch.Tensor, bias a torch.Tensor or None")
        if tuple(w.shape) not in ((k, C), (k, C, 1, 1)):
            raise ValueError(f"{name}: weight must be {(k, C)} or {(k, C, 1, 1)} for x {tuple(x.shape)}, got {tuple(w.shape)}")
        if b is not None and tuple(b.shape) != (k,):
            raise ValueError(f"{name}: bias must be {(k,)}, got {tuple(b.shape)}")
        for t in (w, b):
            if t is not None and t.dtype != x.dtype:
                raise ValueError(f"{name}: x and the parameters must have one dtype, got {x.dtype} and {t.dtype}")
    _require_cuda_f32(x, "x", _IO_DTYPES)
    out = []
    for name, w, b, k in pairs:
        for t in (w, b):
            if t is not None:
                _require_cuda_f32(t, name, _IO_DTYPES)
                if t.device != x.device:
                    raise ValueError(f"{name}: x and the parameters must be on the same device")
        out.append((w.contiguous(), None if b is None else b.contiguous()))
    if C < 1 or x.size(2) < 1 or x.size(3) < 1:
        raise ValueError(f"x must have at least one channel, row and column, got {tuple(x.shape)}")
    return out


def heads(x: torch.Tensor, w_score, b_score, w_rbox, b_rbox, w_angle, b_angle, rbox_scale: float = 128.0):
    """The three detection heads of (N,C,H,W) `x` in one launch: 1x1 convolutions to 1 / 4 / 2 channels
    (weights (k,C) or (k,C,1,1), biases (k,) or None), sigmoid, then score = s, rbox = rbox_scale * s, angle = (2 s - 1)
    normalised to unit length.  -> (score (N,1,H,W), rbox (N,4,H,W), angle (N,2,H,W)) of x's dtype (float32, bfloat16 or
    float16).  x is made NCHW-contiguous.  Sums and epilogue in double in a fixed order, one rounding to fp32 and one to
    the tensor's type: the same bits on every run.  Forward only (no autograd).  ValueError for mismatched shapes or
    dtypes, RuntimeError for CPU tensors."""
    rbox_scale = float(rbox_scale)
    if rbox_scale != rbox_scale or rbox_scale in (float("inf"), float("-inf")):
        raise ValueError(f"rbox_scale must be finite, got {rbox_scale!r}")
    (ws, bs), (wr, br), (wa, ba) = _require_pointwise(x, (("score", w_score, b_score, 1), ("rbox", w_rbox, b_rbox, 4),
                                                         ("angle", w_angle, b_angle, 2)))
    return _heads_run(x.contiguous(), ws, bs, wr, br, wa, ba, rbox_scale)


def _heads_run(x, w_score, b_score, w_rbox, b_rbox, w_angle, b_angle, rbox_scale: float = 128.0):
    """The call itself, for arguments already checked (heads above; fots_e2e.native after heads_ok): x is a contiguous CUDA
    (N,C,H,W) tensor, the parameters contiguous, of its dtype and device, a bias or None."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _heads_run(x, w_score, b_score, w_rbox, b_rbox, w_angle, b_angle, rbox_scale)
    N, C, H, W = x.shape
    score = torch.empty((N, 1, H, W), dtype=x.dtype, device=x.device)
    rbox = torch.empty((N, 4, H, W), dtype=x.dtype, device=x.device)
    angle = torch.empty((N, 2, H, W), dtype=x.dtype, device=x.device)
    if N == 0:
        return score, rbox, angle
    st = _lib.rroi_heads_forward_hip(_DTYPES[x.dtype], x.data_ptr(), w_score.data_ptr(),
                                     None if b_score is None else b_score.data_ptr(), w_rbox.data_ptr(),
                                     None if b_rbox is None else b_rbox.data_ptr(), w_angle.data_ptr(),
                                     None if b_angle is None else b_angle.data_ptr(), score.data_ptr(), rbox.data_ptr(),
                                     angle.data_ptr(), N, C, H, W, rbox_scale, _stream())
    if st != 1:
        _check(st, "rroi_heads_forward_hip")
    return score, rbox, angle


def gate(x: torch.Tensor, w, b) -> torch.Tensor:
    """sigmoid of a 1x1 convolution of (N,C,H,W) `x` to one channel, in one launch: w (1,C) or (1,C,1,1), b
    (1,) or None -> (N,1,H,W).  The terms of `heads`."""
    ((w, b),) = _require_pointwise(x, (("gate", w, b, 1),))
    return _gate_run(x.contiguous(), w, b)


def _gate_run(x, w, b):
    """The call itself, for arguments already checked (gate above; fots_e2e.native after heads_ok)."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _gate_run(x, w, b)
    N, C, H, W = x.shape
    y = torch.empty((N, 1, H, W), dtype=x.dtype, device=x.device)
    if N == 0:
        return y
    st = _lib.rroi_gate_forward_hip(_DTYPES[x.dtype], x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(),
                                    y.data_ptr(), N, C, H, W, _stream())
    if st != 1:
        _check(st, "rroi_gate_forward_hip")
    return y


# --------------------------------------------------------------------------- gated merge (header section 8)
MergePlan = collections.namedtuple("MergePlan", [n for n, _ in _MergePlan._fields_])


def merge_plan(batch_size, channels, height, width, a_size=None, gate_size=None, dtype=DTYPE_FP32) -> MergePlan:
    """What `gated_merge` launches for an `f` of this shape, an `a` of spatial size `a_size` (None: f's) and a gate of
    `gate_size` (None: no gate) (host only, no GPU needed: 256 CUs are assumed without one): pixels per lane V, channel
    groups K, tiles per image, grid, block, channels per group, whether each source is resized, and the four scales.
    ValueError where the call would refuse the arguments."""
    a_h, a_w = (height, width) if a_size is None else a_size
    g_h, g_w = (1, 1) if gate_size is None else gate_size
    p = _MergePlan()
    if _lib.rroi_merge_plan(dtype_code(dtype), int(batch_size), int(channels), int(height), int(width), int(a_h), int(a_w),
                            int(g_h), int(g_w), 0 if gate_size is None else 1, ctypes.byref(p)) != 1:
        raise ValueError("rroi_merge_plan: the call would refuse these arguments")
    return MergePlan(*(getattr(p, n) for n in MergePlan._fields))


def gated_merge(a: torch.Tensor, f: torch.Tensor, gate=None) -> torch.Tensor:
    """y = A + f * G in one launch: `a` (N,C,a_h,a_w) and the one-channel `gate` (N,1,g_h,g_w) are resized
    to f's (H,W) -- bilinear, align_corners=True, in double -- and a source of f's size is read as it is; gate=None:
    y = A + f.  -> (N,C,H,W) of f's dtype (float32, bfloat16 or float16).  The tensors are made NCHW-contiguous.  Every
    operation rounds once to double in a fixed order, one rounding to fp32 and one to the tensor's type: a float64
    restatement gives the same bits.  Forward only (no autograd).  ValueError for mismatched shapes or dtypes, RuntimeError
    for CPU tensors."""
    for name, t in (("a", a), ("f", f)) + ((("gate", gate),) if gate is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dim() != 4:
            raise ValueError(f"{name} must be 4-D (N,C,H,W), got {tuple(t.shape)}")
        if t.dtype != f.dtype:
            raise ValueError(f"a, f and the gate must have one dtype, got {f.dtype} and {t.dtype} ({name})")
    if a.shape[:2] != f.shape[:2]:
        raise ValueError(f"a and f must agree in batch size and channels, got {tuple(a.shape)} and {tuple(f.shape)}")
    if gate is not None and (gate.size(0) != f.size(0) or gate.size(1) != 1):
        raise ValueError(f"the gate must be (N,1,h,w) with f's batch size, got {tuple(gate.shape)} for f {tuple(f.shape)}")
    for name, t in (("f", f), ("a", a)) + ((("gate", gate),) if gate is not None else ()):
        _require_cuda_f32(t, name, _IO_DTYPES)
        if t.device != f.device:
            raise ValueError(f"{name}: a, f and the gate must be on the same device")
    if f.size(0) > 0 and min(f.shape[1:] + a.shape[2:] + (gate.shape[2:] if gate is not None else ())) < 1:
        raise ValueError("every tensor must have at least one channel, row and column")
    return _gated_merge_run(a.contiguous(), f.contiguous(), None if gate is None else gate.contiguous())


def _gated_merge_run(a, f, gate=None):
    """The call itself, for arguments already checked (gated_merge above; fots_e2e.native after merge_ok): contiguous CUDA
    tensors of one dtype and device, a (N,C,a_h,a_w), f (N,C,H,W), gate (N,1,g_h,g_w) or None."""
    index = f.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _gated_merge_run(a, f, gate)
    N, C, H, W = f.shape
    y = torch.empty((N, C, H, W), dtype=f.dtype, device=f.device)
    if N == 0:
        return y
    g_h, g_w = (1, 1) if gate is None else gate.shape[2:]
    st = _lib.rroi_merge_forward_hip(_DTYPES[f.dtype], a.data_ptr(), a.size(2), a.size(3),
                                     None if gate is None else gate.data_ptr(), g_h, g_w, f.data_ptr(), y.data_ptr(),
                                     N, C, H, W, _stream())
    if st != 1:
        _check(st, "rroi_merge_forward_hip")
    return y


# --------------------------------------------------------------------------- dense 3x3 convolution (header section 9)
Conv3x3Plan = collections.namedtuple("Conv3x3Plan", [n for n, _ in _ConvPlan._fields_[:-1]])
_CONV_DTYPES = (torch.bfloat16, torch.float16)


def conv3x3_plan(batch_size, in_channels, out_channels, height, width, stride=1, dtype=DTYPE_BF16) -> Conv3x3Plan:
    """What `conv3x3` launches for an x of (batch_size, in_channels, height, width) and `out_channels` filters (host only,
    no GPU needed): the tile (output channels, rows, columns), the K chunk and their
    number, tiles per image along each axis, grid, block, LDS bytes and the output's size.  ValueError where the call
    would refuse the arguments (float32 among them)."""
    p = _ConvPlan()
    if _lib.rroi_conv3x3_plan(dtype_code(dtype), int(batch_size), int(in_channels), int(out_channels), int(height), int(width),
                              int(stride), ctypes.byref(p)) != 1:
        raise ValueError("rroi_conv3x3_plan: the call would refuse these arguments")
    return Conv3x3Plan(*(getattr(p, n) for n in Conv3x3Plan._fields))


def conv3x3(x: torch.Tensor, weight: torch.Tensor, stride: int = 1, negative_slope: float = 1.0, out=None) -> torch.Tensor:
    """(N,Cin,H,W) x (Cout,Cin,3,3) -> (N,Cout,Ho,Wo): act(conv2d(x, weight, stride=stride, padding=1)) on the matrix cores
    in one launch.  bfloat16 or float16, x and weight alike, both NCHW-contiguous (a non-contiguous tensor is
    refused, not copied); no bias; stride 1 or 2.  act is a leaky ReLU of `negative_slope`: 1.0 none, 0.0 a ReLU.  fp32
    accumulation in a fixed order (the same bits on every run), one rounding to the tensors' type after the activation.
    out: a contiguous tensor of the result's shape, dtype and device to write into.  Forward only (no autograd).
    ValueError for mismatched shapes, dtypes or layouts, TypeError for float32, RuntimeError for CPU tensors."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor):
        raise TypeError("x and weight must be torch.Tensors")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,Cin,H,W), got {tuple(x.shape)}")
    N, C, H, W = x.shape
    if weight.dim() != 4 or weight.size(1) != C or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f"weight must be (Cout, {C}, 3, 3) for x {tuple(x.shape)}, got {tuple(weight.shape)}")
    if weight.dtype != x.dtype:
        raise ValueError(f"x and weight must have one dtype, got {x.dtype} and {weight.dtype}")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2, got {stride!r}")
    negative_slope = float(negative_slope)
    if negative_slope != negative_slope or negative_slope in (float("inf"), float("-inf")):
        raise ValueError(f"negative_slope must be finite, got {negative_slope!r}")
    _require_cuda_f32(x, "x", _CONV_DTYPES)
    _require_cuda_f32(weight, "weight", _CONV_DTYPES)
    if weight.device != x.device:
        raise ValueError("x and weight must be on the same device")
    if C < 1 or H < 1 or W < 1 or weight.size(0) < 1:
        raise ValueError(f"x and weight must have at least one channel, row and column, got {tuple(x.shape)}, {tuple(weight.shape)}")
    if not x.is_contiguous() or not weight.is_contiguous():
        raise ValueError("x and weight must be NCHW-contiguous")
    if out is not None:
        shape = (N, weight.size(0), (H - 1) // stride + 1, (W - 1) // stride + 1)
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != x.dtype or out.device != x.device
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous {shape} tensor of x's dtype and device")
    return _conv3x3_run(x, weight, int(stride), negative_slope, out)


def _conv3x3_run(x: torch.Tensor, weight: torch.Tensor, stride: int, negative_slope: float = 1.0, out=None) -> torch.Tensor:
    """The call itself, for arguments already checked (conv3x3 above; fots_e2e.native after conv3x3_ok): contiguous CUDA
    tensors of one 16-bit dtype and device, x (N,Cin,H,W), weight (Cout,Cin,3,3), stride 1 or 2."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _conv3x3_run(x, weight, stride, negative_slope, out)
    N, C, H, W = x.shape
    K = weight.size(0)
    if out is None:
        out = torch.empty((N, K, (H - 1) // stride + 1, (W - 1) // stride + 1), dtype=x.dtype, device=x.device)
    if N == 0:
        return out
    st = _lib.rroi_conv3x3_forward_hip(_DTYPES[x.dtype], x.data_ptr(), weight.data_ptr(), out.data_ptr(), N, C, K, H, W,
                                       stride, negative_slope, _stream())
    if st != 1:
        _check(st, "rroi_conv3x3_forward_hip")
    return out


# --------------------------------------------------------------------------- 1x1 convolution, folded BatchNorm (header section 11)
Conv1x1Plan = collections.namedtuple("Conv1x1Plan", [n for n, _ in _Conv1x1Plan._fields_[:-1]])


def conv1x1_plan(batch_size, in_channels, out_channels, height, width, stride=1, dtype=DTYPE_BF16) -> Conv1x1Plan:
    """What `conv1x1` launches for an x of (batch_size, in_channels, height, width) and `out_channels` filters (host only,
    no GPU needed): the tile (output channels, output pixels), the K chunk and their number, tiles per image along each
    axis, grid, block, LDS bytes and the output's size.  ValueError where the call would refuse the arguments (float32
    among them)."""
    p = _Conv1x1Plan()
    if _lib.rroi_conv1x1_plan(dtype_code(dtype), int(batch_size), int(in_channels), int(out_channels), int(height), int(width),
                              int(stride), ctypes.byref(p)) != 1:
        raise ValueError("rroi_conv1x1_plan: the call would refuse these arguments")
    return Conv1x1Plan(*(getattr(p, n) for n in Conv1x1Plan._fields))


def conv1x1(x: torch.Tensor, weight: torch.Tensor, stride: int = 1, negative_slope: float = 1.0, norm=None,
            out=None) -> torch.Tensor:
    """(N,Cin,H,W) x (Cout,Cin,1,1) or (Cout,Cin) -> (N,Cout,Ho,Wo): act(s * conv2d(x, weight, stride=stride) + t) on the
    matrix cores in one launch.  bfloat16 or float16, x and weight alike, both contiguous (a non-contiguous
    tensor is refused, not copied); no bias; stride 1 or 2.  norm: None, or an eval-mode BatchNorm as
    (weight or None, bias or None, running_mean, running_var, eps) -- vectors of Cout elements of x's dtype and device,
    weight and bias both given or both None -- folded in as s = weight / sqrt(var + eps), t = bias - mean * s, computed in
    fp32 inside the launch.  act is a leaky ReLU of `negative_slope`: 1.0 none, 0.0 a ReLU.  fp32 accumulation in a fixed
    order (the same bits on every run), one rounding to the tensors' type after the activation.  out: a contiguous tensor
    of the result's shape, dtype and device to write into.  Forward only (no autograd).
    ValueError for mismatched shapes, dtypes or layouts, TypeError for float32, RuntimeError for CPU tensors."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor):
        raise TypeError("x and weight must be torch.Tensors")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,Cin,H,W), got {tuple(x.shape)}")
    N, C, H, W = x.shape
    if not ((weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1)) or weight.dim() == 2) or weight.size(1) != C:
        raise ValueError(f"weight must be (Cout, {C}, 1, 1) or (Cout, {C}) for x {tuple(x.shape)}, got {tuple(weight.shape)}")
    if weight.dtype != x.dtype:
        raise ValueError(f"x and weight must have one dtype, got {x.dtype} and {weight.dtype}")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2, got {stride!r}")
    negative_slope = float(negative_slope)
    if negative_slope != negative_slope or negative_slope in (float("inf"), float("-inf")):
        raise ValueError(f"negative_slope must be finite, got {negative_slope!r}")
    K = weight.size(0)
    if norm is not None:
        if not isinstance(norm, (tuple, list)) or len(norm) != 5:
            raise ValueError("norm must be (weight or None, bias or None, running_mean, running_var, eps)")
        g, b, mean, var, eps = norm
        if (g is None) != (b is None):
            raise ValueError("norm: weight and bias must both be given or both be None")
        if mean is None or var is None:
            raise ValueError("norm: running_mean and running_var must be given")
        for name, v in (("weight", g), ("bias", b), ("running_mean", mean), ("running_var", var)):
            if v is not None and (not isinstance(v, torch.Tensor) or tuple(v.shape) != (K,) or v.dtype != x.dtype
                                  or v.device != x.device or not v.is_contiguous()):
                raise ValueError(f"norm: {name} must be a contiguous ({K},) tensor of x's dtype and device")
        eps = float(eps)
        if not (0.0 <= eps < float("inf")):
            raise ValueError(f"norm: eps must be finite and not negative, got {eps!r}")
        norm = (g, b, mean, var, eps)
    _require_cuda_f32(x, "x", _CONV_DTYPES)
    _require_cuda_f32(weight, "weight", _CONV_DTYPES)
    if weight.device != x.device:
        raise ValueError("x and weight must be on the same device")
    if C < 1 or H < 1 or W < 1 or K < 1:
        raise ValueError(f"x and weight must have at least one channel, row and column, got {tuple(x.shape)}, {tuple(weight.shape)}")
    if not x.is_contiguous() or not weight.is_contiguous():
        raise ValueError("x and weight must be contiguous")
    if out is not None:
        shape = (N, K, (H - 1) // stride + 1, (W - 1) // stride + 1)
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != x.dtype or out.device != x.device
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous {shape} tensor of x's dtype and device")
    return _conv1x1_run(x, weight, int(stride), negative_slope, norm, out)


def _conv1x1_run(x: torch.Tensor, weight: torch.Tensor, stride: int, negative_slope: float = 1.0, norm=None,
                 out=None) -> torch.Tensor:
    """The call itself, for arguments already checked (conv1x1 above; fots_e2e.native after conv1x1_ok / shortcut_ok):
    contiguous CUDA tensors of one 16-bit dtype and device, x (N,Cin,H,W), weight (Cout,Cin[,1,1]), stride 1 or 2, norm
    None or (weight or None, bias or None, running_mean, running_var, eps)."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _conv1x1_run(x, weight, stride, negative_slope, norm, out)
    N, C, H, W = x.shape
    K = weight.size(0)
    if out is None:
        out = torch.empty((N, K, (H - 1) // stride + 1, (W - 1) // stride + 1), dtype=x.dtype, device=x.device)
    if N == 0:
        return out
    if norm is None:
        g = b = mean = var = None
        eps = 0.0
    else:
        g, b, mean, var, eps = norm
        g, b = (None, None) if g is None else (g.data_ptr(), b.data_ptr())
        mean, var = mean.data_ptr(), var.data_ptr()
    st = _lib.rroi_conv1x1_forward_hip(_DTYPES[x.dtype], x.data_ptr(), weight.data_ptr(), out.data_ptr(), N, C, K, H, W,
                                       stride, negative_slope, g, b, mean, var, eps, _stream())
    if st != 1:
        _check(st, "rroi_conv1x1_forward_hip")
    return out


# --------------------------------------------------------------------------- recogniser head, activation + pool (header section 10)
OcrHeadPlan = collections.namedtuple("OcrHeadPlan", [n for n, _ in _OcrHeadPlan._fields_])


def ocr_head_plan(batch_size, channels, classes, steps, dtype=DTYPE_FP32) -> OcrHeadPlan:
    """What `ocr_head` launches for an x of (batch_size, channels, steps) and `classes` rows of weights (host only, no GPU
    needed): classes per wave, waves per workgroup, columns per tile, tiles per crop, grid, block, LDS bytes and the limit on
    `classes`.  ValueError where the call would refuse the arguments (more classes than the limit among them)."""
    p = _OcrHeadPlan()
    if _lib.rroi_ocr_head_plan(dtype_code(dtype), int(batch_size), int(channels), int(classes), int(steps),
                               ctypes.byref(p)) != 1:
        raise ValueError("rroi_ocr_head_plan: the call would refuse these arguments")
    return OcrHeadPlan(*(getattr(p, n) for n in OcrHeadPlan._fields))


def ocr_head(x: torch.Tensor, weight: torch.Tensor, bias=None, out=None) -> torch.Tensor:
    """(N,C,T) or (N,C,1,T) x, (K,C) or (K,C,1,1) weight, (K,) bias or None -> (N,K,T):
    log_softmax(conv1x1(x) + bias, dim=1) in one launch.  float32, bfloat16 or float16, all tensors alike and
    contiguous (a non-contiguous tensor is refused, not copied); K <= OCR_HEAD_MAX_CLASSES.  Logits, maximum, sum and
    logarithm in double in a fixed order, one rounding to fp32 and one to the tensors' type: the same bits on every run.
    out: a contiguous (N,K,T) tensor of x's dtype and device to write into.  Forward only (no autograd).  ValueError for
    mismatched shapes, dtypes or layouts, RuntimeError for CPU tensors."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor) or not (bias is None or isinstance(bias, torch.Tensor)):
        raise TypeError("x and weight must be torch.Tensors, bias a torch.Tensor or None")
    if x.dim() not in (3, 4) or (x.dim() == 4 and x.size(2) != 1):
        raise ValueError(f"x must be (N,C,T) or (N,C,1,T), got {tuple(x.shape)}")
    N, C, T = x.size(0), x.size(1), x.size(-1)
    K = weight.size(0) if weight.dim() > 0 else 0
    if tuple(weight.shape) not in ((K, C), (K, C, 1, 1)):
        raise ValueError(f"weight must be (K, {C}) or (K, {C}, 1, 1) for x {tuple(x.shape)}, got {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (K,):
        raise ValueError(f"bias must be {(K,)}, got {tuple(bias.shape)}")
    for t in (weight, bias):
        if t is not None and t.dtype != x.dtype:
            raise ValueError(f"x and the parameters must have one dtype, got {x.dtype} and {t.dtype}")
    if not 1 <= K <= OCR_HEAD_MAX_CLASSES:
        raise ValueError(f"the head takes 1 to {OCR_HEAD_MAX_CLASSES} classes, got {K}")
    _require_cuda_f32(x, "x", _IO_DTYPES)
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None:
            _require_cuda_f32(t, name, _IO_DTYPES)
            if t.device != x.device:
                raise ValueError(f"{name}: x and the parameters must be on the same device")
    if C < 1 or T < 1:
        raise ValueError(f"x must have at least one channel and column, got {tuple(x.shape)}")
    if not x.is_contiguous() or not weight.is_contiguous() or not (bias is None or bias.is_contiguous()):
        raise ValueError("x, weight and bias must be contiguous")
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (N, K, T) or out.dtype != x.dtype
                            or out.device != x.device or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {(N, K, T)} tensor of x's dtype and device")
    return _ocr_head_run(x, weight, bias, out)


def _ocr_head_run(x: torch.Tensor, weight: torch.Tensor, bias=None, out=None) -> torch.Tensor:
    """The call itself, for arguments already checked (ocr_head above; fots_e2e.native after ocr_head_ok): contiguous CUDA
    tensors of one dtype and device, x (N,C,T) or (N,C,1,T), weight (K,C) or (K,C,1,1), bias (K,) or None."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _ocr_head_run(x, weight, bias, out)
    N, C, T = x.size(0), x.size(1), x.size(-1)
    K = weight.size(0)
    if out is None:
        out = torch.empty((N, K, T), dtype=x.dtype, device=x.device)
    if N == 0:
        return out
    st = _lib.rroi_ocr_head_forward_hip(_DTYPES[x.dtype], x.data_ptr(), weight.data_ptr(),
                                        None if bias is None else bias.data_ptr(), out.data_ptr(), N, C, K, T, _stream())
    if st != 1:
        _check(st, "rroi_ocr_head_forward_hip")
    return out


def act_maxpool2x1(x: torch.Tensor, negative_slope: float = 1.0) -> torch.Tensor:
    """(N,C,H,W) -> (N,C,H//2,W): `F.max_pool2d(F.leaky_relu(x, negative_slope), (2, 1), stride=(2, 1))` in one launch, bit
    for bit; negative_slope = 1.0 is the plain pool.  float32, bfloat16 or float16, NCHW-contiguous (a
    non-contiguous tensor is refused, not copied), H >= 2; an odd last row is dropped.  Forward only (no autograd).
    ValueError for a wrong shape or layout, RuntimeError for CPU tensors."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,C,H,W), got {tuple(x.shape)}")
    negative_slope = float(negative_slope)
    if negative_slope != negative_slope or negative_slope in (float("inf"), float("-inf")):
        raise ValueError(f"negative_slope must be finite, got {negative_slope!r}")
    if x.size(2) < 2:
        raise ValueError(f"x must have at least two rows, got {tuple(x.shape)}")
    _require_cuda_f32(x, "x", _IO_DTYPES)
    if x.size(1) < 1 or x.size(3) < 1:
        raise ValueError(f"x must have at least one channel and column, got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError("x must be NCHW-contiguous")
    return _act_maxpool2x1_run(x, negative_slope)


def _act_maxpool2x1_run(x: torch.Tensor, negative_slope: float = 1.0) -> torch.Tensor:
    """The call itself, for arguments already checked (act_maxpool2x1 above; fots_e2e.native after act_pool_ok): a contiguous
    CUDA (N,C,H,W) tensor with H >= 2."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _act_maxpool2x1_run(x, negative_slope)
    N, C, H, W = x.shape
    out = torch.empty((N, C, H // 2, W), dtype=x.dtype, device=x.device)
    if N == 0:
        return out
    st = _lib.rroi_act_maxpool2x1_forward_hip(_DTYPES[x.dtype], x.data_ptr(), out.data_ptr(), N, C, H, W, negative_slope,
                                              _stream())
    if st != 1:
        _check(st, "rroi_act_maxpool2x1_forward_hip")
    return out


def bin_centres(rois: torch.Tensor, pooled_height: int, pooled_width: int, spatial_scale: float,
                height: int, width: int, trig: int = TRIG_DOUBLE) -> torch.Tensor:
    """(R,PH,PW,2) sample points (kernel.cu:86-107); zero outside the ROI's pooled width."""
    _require_cuda_f32(rois, "rois")
    rois = rois.contiguous()
    R = rois.size(0)
    with torch.cuda.device_of(rois):
        geom = torch.empty((R, int(pooled_height), int(pooled_width), 2), dtype=torch.float32,
                           device=rois.device)
        st = _lib.rroi_align_bin_centres_trig_hip(float(spatial_scale), R, int(height), int(width),
                                                  int(pooled_height), int(pooled_width),
                                                  rois.data_ptr(), geom.data_ptr(), int(trig), _stream())
    _check(st, "rroi_align_bin_centres_trig_hip")
    return geom


def ctc_greedy_decode(logits: torch.Tensor, lengths=None, return_labels: bool = False):
    """(N, nclass, T) logits -> (decoded (N, T) int32 zero-padded, decoded_len (N,) int32
    [, raw arg-max labels (N, T) int32]), all on the device; one launch for all sequences.
    Replaces `labels_pred.max(1)` + strLabelConverter.decode (tools/ocr_utils.py:183-186).
    logits: float32, bfloat16 or float16 (a head that runs in 16 bits): a 16-bit element is widened exactly where the
    kernel loads it, so the result is that of the float32 call on `logits.float()`, ties and NaN included."""
    _require_cuda_f32(logits, "logits", _IO_DTYPES)
    code = _DTYPES[logits.dtype]
    if logits.dim() != 3:
        raise ValueError("logits must be (N, nclass, T)")
    logits = logits.contiguous()
    N, K, T = logits.shape
    if K == 0:
        raise ValueError("logits must have at least one class")
    with torch.cuda.device_of(logits):
        dev = logits.device
        if lengths is not None:
            lengths = torch.as_tensor(lengths, dtype=torch.int32, device=dev).contiguous()
            if lengths.numel() != N:
                raise ValueError("lengths must have one entry per sequence")
        decoded = torch.empty((N, T), dtype=torch.int32, device=dev)
        dlen = torch.empty((N,), dtype=torch.int32, device=dev)
        labels = torch.empty((N, T), dtype=torch.int32, device=dev) if return_labels else None
        st = _lib.rroi_ctc_greedy_decode_typed_hip(code, logits.data_ptr(), N, K, T,
                                                   lengths.data_ptr() if lengths is not None else None,
                                                   labels.data_ptr() if labels is not None else None,
                                                   decoded.data_ptr(), dlen.data_ptr(), _stream())
    _check(st, "rroi_ctc_greedy_decode_typed_hip")
    return (decoded, dlen, labels) if return_labels else (decoded, dlen)


def quads_to_rois(quads: torch.Tensor, batch_index=None, mode: int = 0, target_h: int = 11):
    """(N, 8) quads -> ((N, 6) rois, (N,) int32 pooled widths), both on the device."""
    _require_cuda_f32(quads, "quads")
    quads = quads.contiguous().view(-1, 8)
    n = quads.size(0)
    if batch_index is not None:
        _require_cuda_f32(batch_index, "batch_index")
        batch_index = batch_index.contiguous().view(-1)
        if batch_index.numel() != n:
            raise ValueError("batch_index must have one entry per quad")
    with torch.cuda.device_of(quads):
        rois = torch.empty((n, 6), dtype=torch.float32, device=quads.device)
        gw = torch.empty((n,), dtype=torch.int32, device=quads.device)
        st = _lib.rroi_align_quads_to_rois_hip(quads.data_ptr(),
                                               batch_index.data_ptr() if batch_index is not None else None,
                                               n, int(mode), int(target_h), rois.data_ptr(), gw.data_ptr(),
                                               _stream())
    _check(st, "rroi_align_quads_to_rois_hip")
    return rois, gw


def gt_quads_to_rois(quads: torch.Tensor, batch_index=None, height_jitter=None):
    """(N, 8) ground-truth quads -> ((N, 6) rois, (1,) max w/h over the fp32 rows), on the device
    (src/ocr_process.py:196-219, :259-263)."""
    _require_cuda_f32(quads, "quads")
    quads = quads.contiguous().view(-1, 8)
    n = quads.size(0)
    aux = []
    for t, name in ((batch_index, "batch_index"), (height_jitter, "height_jitter")):
        if t is not None:
            _require_cuda_f32(t, name)
            t = t.contiguous().view(-1)
            if t.numel() != n:
                raise ValueError(f"{name} must have one entry per quad")
        aux.append(t)
    with torch.cuda.device_of(quads):
        rois = torch.empty((n, 6), dtype=torch.float32, device=quads.device)
        ratio = torch.empty((1,), dtype=torch.float32, device=quads.device)
        st = _lib.rroi_align_gt_quads_to_rois_hip(quads.data_ptr(),
                                                  aux[0].data_ptr() if aux[0] is not None else None,
                                                  aux[1].data_ptr() if aux[1] is not None else None,
                                                  n, rois.data_ptr(), ratio.data_ptr(), _stream())
    _check(st, "rroi_align_gt_quads_to_rois_hip")
    return rois, ratio


def sincos_probe(angle_deg: torch.Tensor) -> torch.Tensor:
    _require_cuda_f32(angle_deg, "angle_deg")
    angle_deg = angle_deg.contiguous().view(-1)
    with torch.cuda.device_of(angle_deg):
        out = torch.empty((angle_deg.numel(), 2), dtype=torch.float32, device=angle_deg.device)
        st = _lib.rroi_align_sincos_probe_hip(angle_deg.data_ptr(), angle_deg.numel(),
                                              out.data_ptr(), _stream())
    _check(st, "rroi_align_sincos_probe_hip")
    return out


# --------------------------------------------------------------------------- reference FFI names
def rroi_align_forward_cuda(pooled_height, pooled_width, spatial_scale, features, rois, output,
                            idx_x, idx_y) -> int:
    """Same name, argument order and return value as the reference's FFI function
    (src/rroi_align_cuda.c:7-44): fills ``output``, ``idx_x``, ``idx_y`` in place;
    returns 0 when ``rois.size(1) != 6`` (:22-26), else 1."""
    for t, name in ((features, "features"), (rois, "rois"), (output, "output"), (idx_x, "idx_x"),
                    (idx_y, "idx_y")):
        _require_cuda_f32(t, name)
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous (the reference reads raw storage)")
    if rois.size(1) != 6:
        return 0
    num_rois = rois.size(0)
    _, C, H, W = features.shape
    with torch.cuda.device_of(features):
        st = _lib.RROIAlignForwardLaucher(features.data_ptr(), float(spatial_scale), num_rois, H, W,
                                          C, int(pooled_height), int(pooled_width),
                                          rois.data_ptr(), output.data_ptr(), idx_x.data_ptr(),
                                          idx_y.data_ptr(), _stream())
    _check(st, "RROIAlignForwardLaucher")
    return 1


def _launcher_trig() -> int:
    """The recipe the reference-ABI launchers run in this process (the library reads RROI_ALIGN_LAUNCHER_TRIG once per
    process: asking it keeps the glue's gradient on the recipe of the launcher forward that made the crops)."""
    return int(_lib.rroi_align_launcher_trig_recipe())


def rroi_align_backward_cuda(pooled_height, pooled_width, spatial_scale, top_grad, rois,
                             bottom_grad, idx_x, idx_y) -> int:
    """Reference FFI signature (src/rroi_align_cuda.c:49-87).  ``bottom_grad`` must be
    zero on entry, as functions/rroi_align.py:35 guarantees in the reference.
    Under torch.use_deterministic_algorithms(True) the gradient is the ORDERED one (backward(deterministic=True),
    from the rois -- the same bin centres the forward stored in idx_x / idx_y), computed into a temporary and added
    to ``bottom_grad`` with one torch add: the same bits on every run.  The C launcher itself
    (RROIAlignBackwardLaucher) has no `path` word and stays the reference's scatter, whose order is not fixed."""
    for t, name in ((top_grad, "top_grad"), (rois, "rois"), (bottom_grad, "bottom_grad"),
                    (idx_x, "idx_x"), (idx_y, "idx_y")):
        _require_cuda_f32(t, name)
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous (the reference reads raw storage)")
    if rois.size(1) != 6:
        return 0
    num_rois = rois.size(0)
    B, C, H, W = bottom_grad.shape
    if torch.are_deterministic_algorithms_enabled():
        g = backward(top_grad, rois, (B, C, H, W), spatial_scale, trig=_launcher_trig(), deterministic=True)
        bottom_grad.add_(g)
        return 1
    with torch.cuda.device_of(top_grad):
        st = _lib.RROIAlignBackwardLaucher(top_grad.data_ptr(), float(spatial_scale), B, num_rois, H,
                                           W, C, int(pooled_height), int(pooled_width),
                                           rois.data_ptr(), bottom_grad.data_ptr(),
                                           idx_x.data_ptr(), idx_y.data_ptr(), _stream())
    _check(st, "RROIAlignBackwardLaucher")
    return 1
