"""rroi_align._ext.rroi_align -- ctypes binding of librroi_align_hip.so.

Stands where the reference's cffi extension stood (``rroi_align/build.py:7-37``
built ``_ext.rroi_align`` from ``src/rroi_align_cuda.c``): it exports the same
two tensor-taking functions, ``rroi_align_forward_cuda`` and
``rroi_align_backward_cuda`` (``src/rroi_align_cuda.h:1-7``), plus the native
entry points the autograd Function uses.

The shared library is mandatory: importing this module without it raises.

This file is the package's surface and holds no logic.  `_core` loads the library and holds what every module shares;
each module imported below binds the functions of one `csrc/rroi_*_host.h` (structs, prototypes, plan query, checked
wrappers, lean `_*_run`), so that importing the package sets every prototype a caller of `_lib` relies on.  `remainder`,
`preprocess`, `ctc_loss` and `detection_loss` are modules of the same kind, loaded on first use: their hot calls are named
`run_*`, because the `_*_run` callables of this namespace are a closed list (the network's ledger test reads it).
"""
from __future__ import annotations

# (collections, ctypes, os, threading and torch have always been attributes of this namespace: callers reach `ctypes`
# through it.  `heads`, `conv3x3` and `conv1x1` name a module and its function: here the name is the function, as before.)
from ._core import (_CONV_DTYPES, _DTYPES, _HERE, _IO_DTYPES, _SCRATCH_KEEP_BYTES, _SCRATCH_MAX_STREAMS,  # noqa: F401
                    DTYPE_BF16, DTYPE_FP16, DTYPE_FP32, LIB_PATH, _check, _d, _f, _i, _lib, _ll, _require_cuda_f32, _scratch,
                    _scratch_lock, _stream, _sz, _vp, _workspace, collections, ctypes, dtype_code, launcher_scratch_stats,
                    os, release_workspaces, threading, torch, version)
from .roi import (BACKWARD_PATHS, CALLER_LAUNCHER, CALLER_LAUNCHER_CON_IDX, CALLER_NATIVE, FORWARD_PATHS,  # noqa: F401
                  GATHER_PATHS, LAYOUT_NCHW, LAYOUT_NHWC, PATH_AUTO, PATH_DETERMINISTIC, PATH_DIRECT, PATH_FUSED, PATH_TILED,
                  PATH_TILED_ATOMIC, PATH_TILED_BUCKETS, PATH_TILED_INKERNEL, PATH_TILED_LISTS, PATH_TRIG_FP32,
                  PLAN_BWD_ATOMIC, PLAN_BWD_BUCKETS, PLAN_BWD_DIRECT, PLAN_BWD_INKERNEL, PLAN_BWD_LISTS, PLAN_BWD_LITERAL,
                  PLAN_BWD_ORDERED, PLAN_DST_CHUNK_MAJOR, PLAN_DST_NCHW, PLAN_DST_NCHW_ADD, PLAN_DST_NHWC, PLAN_DST_NONE,
                  PLAN_FWD_DIRECT_K2P, PLAN_FWD_DIRECT_THREAD, PLAN_FWD_FUSED_SHIFT, PLAN_FWD_FUSED_STRIDED,
                  PLAN_FWD_TWO_LAUNCH, PLAN_KERNEL_CHANNELS_LAST, PLAN_KERNEL_SHIFT, PLAN_KERNEL_SHIFT_LINES,
                  PLAN_KERNEL_STRIDED, PLAN_KERNEL_STRIDED_MERGE, PLAN_KERNEL_STRIDED_RAGGED, PLAN_NONE, STAGE_ALL,
                  STAGE_GATHER, STAGE_PROLOGUE, TRIG_DOUBLE, TRIG_FP32, Plan, _launcher_trig, _path_word, _plan, _Plan,
                  _require_features_rois, backward, backward_plan, bin_centres, forward, forward_plan, gt_quads_to_rois,
                  quads_to_rois, rroi_align_backward_cuda, rroi_align_forward_cuda, sincos_probe)
from .bucketed import (_TABLES_MAX, _bucket_tables, _bucketed_stats, _BucketTables, _gcd, _pow2_divisor,  # noqa: F401
                       _tables, backward_bucketed, backward_bucketed_plan, bucket_layout, crop_table, forward_bucketed,
                       forward_bucketed_plan)
from .callers import ctc_greedy_decode  # noqa: F401
from .depthwise import (DepthwiseBackwardPlan, _depthwise3x3_run, _DwBwdPlan, depthwise3x3, depthwise3x3_backward,  # noqa: F401
                        depthwise3x3_backward_plan, depthwise3x3_backward_workspace_bytes, run_depthwise3x3_backward)
from .instancenorm import (INORM_PLANE, INORM_SPLIT, InstanceNormPlan, _InormPlan, _instance_norm_fused_run,  # noqa: F401
                           _instance_norm_run, instance_norm, instance_norm_backward, instance_norm_backward_plan,
                           instance_norm_backward_workspace_bytes, instance_norm_fused, instance_norm_plan,
                           instance_norm_train, instance_norm_workspace_bytes, run_instance_norm_backward,
                           run_instance_norm_train)
from .heads import (HeadsBackwardPlan, HeadsPlan, _gate_run, _heads_run, _HeadsBwdPlan, _HeadsPlan, _require_pointwise,  # noqa: F401
                    gate, gate_backward, gate_train, heads, heads_backward, heads_backward_plan, heads_backward_workspace_bytes,
                    heads_plan, heads_train, run_gate_backward, run_gate_train, run_heads_backward, run_heads_train)
from .merge import (MergeBackwardPlan, MergePlan, ResizeBackwardPlan, _gated_merge_run, _MergeBwdPlan, _MergePlan,  # noqa: F401
                    _ResizeBwdPlan, gated_merge, gated_merge_backward, merge_backward_plan, merge_backward_workspace_bytes,
                    merge_plan, resize_backward_plan, resize_bilinear, resize_bilinear_backward, resize_footprint,
                    run_gated_merge_backward, run_resize_bilinear, run_resize_bilinear_backward)
from .conv3x3 import Conv3x3Plan, _conv3x3_run, _ConvPlan, conv3x3, conv3x3_plan  # noqa: F401
from .conv1x1 import Conv1x1Plan, _conv1x1_run, _Conv1x1Plan, conv1x1, conv1x1_plan  # noqa: F401
from .recogniser import (OCR_HEAD_MAX_CLASSES, OcrHeadPlan, _act_maxpool2x1_run, _ocr_head_run, _OcrHeadPlan,  # noqa: F401
                         act_maxpool2x1, ocr_head, ocr_head_plan)

# every function include/rroi_align_hip.h declares (tests/test_abi.py holds the two equal)
EXPORTS = (
    "RROIAlignForwardLaucher", "RROIAlignBackwardLaucher", "rroi_align_forward_hip", "rroi_align_backward_hip",
    "rroi_align_forward_stages_hip", "rroi_align_forward_workspace_bytes", "rroi_align_backward_workspace_bytes",
    "rroi_align_bin_centres_hip", "rroi_align_sincos_probe_hip", "rroi_align_quads_to_rois_hip", "rroi_align_hip_version",
    "rroi_ctc_greedy_decode_hip", "rroi_align_backward_layout_hip", "rroi_align_forward_layout_hip",
    "rroi_align_gt_quads_to_rois_hip", "rroi_rbox_decode_hip", "rroi_nms_merge_host", "rroi_align_release_launcher_scratch",
    "rroi_align_bin_centres_trig_hip", "rroi_nms_record_format", "rroi_align_write_probe_hip",
    "rroi_align_launcher_scratch_stats",
    "rroi_align_set_trig_recipe_hip", "rroi_align_get_trig_recipe_hip",   # deprecated shims (refuse TRIG_FP32)
    "rroi_align_forward_plan", "rroi_align_backward_plan", "rroi_align_forward_typed_hip", "rroi_align_backward_typed_hip",
    "rroi_align_forward_plan_typed", "rroi_align_backward_plan_typed", "rroi_align_launcher_trig_recipe",
    "rroi_rbox_decode_typed_hip", "rroi_ctc_greedy_decode_typed_hip",
    "rroi_align_forward_bucketed_hip", "rroi_align_backward_bucketed_hip", "rroi_align_forward_bucketed_plan",
    "rroi_align_backward_bucketed_plan", "rroi_align_forward_bucketed_workspace_bytes",
    "rroi_align_backward_bucketed_workspace_bytes", "rroi_depthwise3x3_forward_hip",
    "rroi_instancenorm_forward_hip", "rroi_instancenorm_workspace_bytes", "rroi_instancenorm_plan",
    "rroi_heads_forward_hip", "rroi_gate_forward_hip", "rroi_heads_plan", "rroi_instancenorm_fused_forward_hip",
    "rroi_merge_forward_hip", "rroi_merge_plan", "rroi_conv3x3_forward_hip", "rroi_conv3x3_plan",
    "rroi_ocr_head_forward_hip", "rroi_ocr_head_plan", "rroi_act_maxpool2x1_forward_hip",
    "rroi_conv1x1_forward_hip", "rroi_conv1x1_plan",
    "rroi_conv2x3_forward_hip", "rroi_conv2x3_plan", "rroi_up_depthwise3x3_forward_hip",   # bound in remainder.py
    "rroi_preprocess_forward_hip", "rroi_preprocess_plan",   # bound in preprocess.py
    "rroi_ctc_loss_forward_hip", "rroi_ctc_loss_plan", "rroi_ctc_loss_workspace_bytes",   # bound in ctc_loss.py
    "rroi_detection_loss_forward_hip", "rroi_detection_loss_backward_hip", "rroi_detection_loss_plan",
    "rroi_detection_loss_workspace_bytes",   # bound in detection_loss.py
    "rroi_instancenorm_forward_train_hip", "rroi_instancenorm_backward_hip", "rroi_instancenorm_backward_workspace_bytes",
    "rroi_instancenorm_backward_plan",   # bound in instancenorm.py
    "rroi_depthwise3x3_backward_hip", "rroi_depthwise3x3_backward_workspace_bytes", "rroi_depthwise3x3_backward_plan",
    "rroi_resize_forward_hip", "rroi_resize_backward_hip", "rroi_resize_footprint", "rroi_resize_backward_plan",
    "rroi_merge_backward_hip", "rroi_merge_backward_workspace_bytes", "rroi_merge_backward_plan",   # bound in merge.py
    "rroi_heads_forward_train_hip", "rroi_gate_forward_train_hip", "rroi_heads_backward_hip", "rroi_gate_backward_hip",
    "rroi_heads_backward_workspace_bytes", "rroi_heads_backward_plan",   # bound in heads.py
)
