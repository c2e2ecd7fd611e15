"""rroi_align._ext.rroi_align.roi -- the binding of RoIRotate itself (header sections 1 to 3 and the hooks at the header's
end; `csrc/rroi_host_plan.h`, `rroi_host_launch.h`): the forward, the backward and their plan queries, the ROI builders,
the probes, and -- at the end -- the two tensor-taking functions of the reference's FFI, by their names."""
import collections
import ctypes

import torch

from ._core import (_DTYPES, _IO_DTYPES, DTYPE_FP32, _bind, _check, _f, _i, _lib, _plan_query, _require_cuda_f32, _stream, _sz, _vp,
                    _workspace, dtype_code)

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
PLAN_KERNEL_STRIDED_RAGGED = 5  # the bucketed forward's gather (header section 2b)
PLAN_DST_NONE, PLAN_DST_CHUNK_MAJOR, PLAN_DST_NCHW, PLAN_DST_NCHW_ADD, PLAN_DST_NHWC = 0, 1, 2, 3, 4

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


class _Plan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("family", "kernel", "groups", "ntiles", "grid_x", "grid_y", "zero_copy", "con_idx", "nk",
                                  "kshift", "raw_bsum", "gy", "dest", "accumulate", "vec4")]


# What a call launches (rroi_align_forward_plan / rroi_align_backward_plan); the fields of rroi_align_plan.
Plan = collections.namedtuple("Plan", [n for n, _ in _Plan._fields_])

_bind("rroi_align_forward_workspace_bytes", [_i] * 6, _sz)
_bind("rroi_align_backward_workspace_bytes", [_i] * 7, _sz)
_bind("rroi_align_forward_hip", [_vp, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp])
_bind("rroi_align_forward_layout_hip", [_vp, _i, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp])
_bind("rroi_align_forward_stages_hip", [_vp, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _i, _vp])
_bind("rroi_align_backward_hip", [_vp, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp])
_bind("rroi_align_backward_layout_hip", [_vp, _i, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp])
_bind("rroi_align_forward_typed_hip", [_vp, _i, _i, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp])
_bind("rroi_align_backward_typed_hip", [_vp, _i, _i, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp])
_bind("rroi_align_forward_plan", [_i] * 11 + [ctypes.POINTER(_Plan)])
_bind("rroi_align_backward_plan", [_i] * 11 + [ctypes.POINTER(_Plan)])
_bind("rroi_align_forward_plan_typed", [_i] * 12 + [ctypes.POINTER(_Plan)])
_bind("rroi_align_backward_plan_typed", [_i] * 12 + [ctypes.POINTER(_Plan)])
_bind("rroi_align_bin_centres_hip", [_f, _i, _i, _i, _i, _i, _vp, _vp, _vp])
_bind("rroi_align_bin_centres_trig_hip", [_f, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp])
_bind("rroi_align_quads_to_rois_hip", [_vp, _vp, _i, _i, _i, _vp, _vp, _vp])
_bind("rroi_align_gt_quads_to_rois_hip", [_vp, _vp, _vp, _i, _vp, _vp, _vp])
_bind("rroi_align_sincos_probe_hip", [_vp, _i, _vp, _vp])
# the write probe of the benchmarks (a measurement hook at the header's end): called through `_lib`, it has no wrapper
_bind("rroi_align_write_probe_hip", [_vp, _sz, _vp])
_bind("RROIAlignForwardLaucher", [_vp, _f, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp])
_bind("RROIAlignBackwardLaucher", [_vp, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp])


def _plan(fn, args, what):
    return _plan_query(fn, _Plan, Plan, what, args)


def _path_word(path: int, trig: int, deterministic: bool = False) -> int:
    if trig not in (TRIG_DOUBLE, TRIG_FP32):
        raise ValueError(f"trig must be TRIG_DOUBLE (0) or TRIG_FP32 (1), got {trig!r}")
    return int(path) | (PATH_TRIG_FP32 if trig == TRIG_FP32 else 0) | (PATH_DETERMINISTIC if deterministic else 0)


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
