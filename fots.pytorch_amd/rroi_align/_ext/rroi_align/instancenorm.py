"""rroi_align._ext.rroi_align.instancenorm -- the binding of the network's InstanceNorm2d with its activation (header
section 6), of the same with the residual add or the stem's mirror fused in (section 6b) and of
its training forward and backward (section 6c); `csrc/rroi_instancenorm_host.h`,
`csrc/rroi_instancenorm_backward_host.h`."""
import collections
import ctypes

import torch

from ._core import (_DTYPES, _IO_DTYPES, DTYPE_FP32, _bind, _check, _d, _f, _i, _lib, _plan_query, _require_cuda_f32, _stream, _sz, _vp,
                    dtype_code)


class _InormPlan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("form", "launches", "segments", "segment_elems", "grid_x", "block", "vector_elems", "reserved")]


_bind("rroi_instancenorm_forward_hip", [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _f, _vp, _sz, _vp])
_bind("rroi_instancenorm_workspace_bytes", [_i] * 4, _sz)
_bind("rroi_instancenorm_plan", [_i] * 5 + [ctypes.POINTER(_InormPlan)])
_bind("rroi_instancenorm_fused_forward_hip", [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _d, _f, _vp, _sz, _vp])
_bind("rroi_instancenorm_forward_train_hip", [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _f, _vp, _sz, _vp])
_bind("rroi_instancenorm_backward_hip", [_i] + [_vp] * 8 + [_i, _i, _i, _i, _d, _f, _vp, _sz, _vp])
_bind("rroi_instancenorm_backward_workspace_bytes", [_i] * 4, _sz)
_bind("rroi_instancenorm_backward_plan", [_i] * 5 + [ctypes.POINTER(_InormPlan)])
INORM_PLANE, INORM_SPLIT = 1, 2

InstanceNormPlan = collections.namedtuple("InstanceNormPlan", [n for n, _ in _InormPlan._fields_[:-1]])


def instance_norm_plan(batch_size, channels, height, width, dtype=DTYPE_FP32) -> InstanceNormPlan:
    """What `instance_norm` launches for a tensor of this shape (host only, no GPU needed: 256 CUs are assumed without
    one): the form (INORM_PLANE / INORM_SPLIT), its launches, segments per plane, elements per segment, the grid.
    ValueError where the call would refuse the arguments."""
    return _plan_query(_lib.rroi_instancenorm_plan, _InormPlan, InstanceNormPlan, "rroi_instancenorm_plan",
                       (dtype_code(dtype), batch_size, channels, height, width))


def instance_norm_workspace_bytes(batch_size, channels, height, width) -> int:
    """Bytes of workspace `rroi_instancenorm_forward_hip` needs for this shape: 0 in the plane form."""
    return int(_lib.rroi_instancenorm_workspace_bytes(int(batch_size), int(channels), int(height), int(width)))


def instance_norm(x: torch.Tensor, weight=None, bias=None, eps: float = 1e-5, negative_slope: float = 1.0) -> torch.Tensor:
    """InstanceNorm2d of (N,C,H,W) `x` over each (n, c) plane (biased variance, instance statistics), then
    `v < 0 ? v * negative_slope : v` (1.0: no activation, 0.0: ReLU) -- DESIGN 5.11.  float32, bfloat16 or float16;
    weight and bias are (C,) of x's dtype, or both None.  x is made NCHW-contiguous.  Statistics in double, shifted by the
    plane's first element; one rounding to fp32 and one to the tensor's type; the same bits on every run.  Forward only (no
    autograd).  ValueError for mismatched shapes or dtypes, RuntimeError for CPU tensors."""
    return instance_norm_fused(x, weight, bias, eps, negative_slope)      # its checks, in its order, and the plain call


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


def _check_norm_shapes(x, weight, bias, mirror=False) -> int:
    """The first checks of every norm call: tensors, x 4-D, weight and bias together and (features,) of x's dtype, where
    features is x's channel count (twice it under `mirror`); -> features."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,C,H,W), got {tuple(x.shape)}")
    if (weight is None) != (bias is None):
        raise ValueError("weight and bias come together, or neither")
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
    return features


def _check_norm_devices(x, weight, bias, features):
    """... and the last: all on one GPU, float32 / bfloat16 / float16, x with at least one channel, row and column;
    -> (weight, bias) contiguous."""
    _require_cuda_f32(x, "x", _IO_DTYPES)
    for name, p in (("weight", weight), ("bias", bias)):
        if p is not None:
            _require_cuda_f32(p, name, _IO_DTYPES)
            if p.device != x.device:
                raise ValueError(f"x and {name} must be on the same device")
    if features < 1 or x.size(2) < 1 or x.size(3) < 1:
        raise ValueError(f"x must have at least one channel, row and column, got {tuple(x.shape)}")
    if weight is not None:
        weight, bias = weight.contiguous(), bias.contiguous()
    return weight, bias


def _check_norm_args(x, weight, bias):
    """The checks of `instance_norm` on x and its parameters, in its order; -> (weight, bias) contiguous."""
    return _check_norm_devices(x, weight, bias, _check_norm_shapes(x, weight, bias))


def instance_norm_fused(x: torch.Tensor, weight=None, bias=None, eps: float = 1e-5, negative_slope: float = 1.0,
                        residual=None, mirror: bool = False) -> torch.Tensor:
    """`instance_norm` with an epilogue fused in -- DESIGN 5.13.
    residual (x's shape, dtype and device):  act(instance_norm(x) + residual), the sum in fp32 and rounded once: the tail
    of a residual block in one call.
    mirror:  the InstanceNorm2d of `torch.cat((x, -x), 1)` with its activation, without the concatenation: (N,2C,H,W) from
    (N,C,H,W); weight and bias are (2C,) or both None.  Not together with a residual.
    With neither, `instance_norm`.  The same exceptions as `instance_norm`; ValueError also for a residual whose shape,
    dtype or device is not x's, for mirror together with a residual, and for a weight that is not (2C,) under mirror."""
    mirror = bool(mirror)
    features = _check_norm_shapes(x, weight, bias, mirror)
    if mirror and residual is not None:
        raise ValueError("mirror takes no residual")
    if residual is not None:
        if not isinstance(residual, torch.Tensor):
            raise TypeError("residual must be a torch.Tensor")
        if residual.shape != x.shape:
            raise ValueError(f"residual must have x's shape {tuple(x.shape)}, got {tuple(residual.shape)}")
        if residual.dtype != x.dtype:
            raise ValueError(f"x and residual must have one dtype, got {x.dtype} and {residual.dtype}")
        if residual.device != x.device:
            raise ValueError("x and residual must be on the same device")
    weight, bias = _check_norm_devices(x, weight, bias, features)
    if mirror and 2 * x.numel() >= 1 << 31:
        raise ValueError(f"the mirrored output of x {tuple(x.shape)} has 2^31 elements or more")
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


# --------------------------------------------------------------------------- training: forward with statistics, backward
def instance_norm_backward_plan(batch_size, channels, height, width, dtype=DTYPE_FP32) -> InstanceNormPlan:
    """What `instance_norm_backward` launches for a tensor of this shape (host only, no GPU needed: 256 CUs are assumed
    without one): as `instance_norm_plan`, by the backward's own rule.  `launches` counts the parameter-gradient kernel,
    which a call without parameter gradients leaves out.  ValueError where the call would refuse the arguments."""
    return _plan_query(_lib.rroi_instancenorm_backward_plan, _InormPlan, InstanceNormPlan, "rroi_instancenorm_backward_plan",
                       (dtype_code(dtype), batch_size, channels, height, width))


def instance_norm_backward_workspace_bytes(batch_size, channels, height, width) -> int:
    """Bytes of workspace `rroi_instancenorm_backward_hip` needs for this shape (one pair of doubles per plane, and the
    split form's partials); 0 for a shape the call would refuse."""
    return int(_lib.rroi_instancenorm_backward_workspace_bytes(int(batch_size), int(channels), int(height), int(width)))


def instance_norm_train(x: torch.Tensor, weight=None, bias=None, eps: float = 1e-5, negative_slope: float = 1.0):
    """`instance_norm` for training -- DESIGN 5.24: -> (y, stats).  y has the bits `instance_norm` gives; stats is
    (N, C, 2) float64, every plane's {mean, var} as the forward formed them, which `instance_norm_backward` takes.  The
    same arguments and exceptions as `instance_norm`.  No autograd here: `rroi_align.norm.instance_norm` has it."""
    weight, bias = _check_norm_args(x, weight, bias)
    return run_instance_norm_train(x.contiguous(), weight, bias, float(eps), float(negative_slope))


def run_instance_norm_train(x: torch.Tensor, weight, bias, eps: float, negative_slope: float):
    """The call itself, for arguments already checked (as `_instance_norm_run`); -> (y, stats)."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_instance_norm_train(x, weight, bias, eps, negative_slope)
    out = torch.empty_like(x)
    N, C, H, W = x.shape
    stats = torch.empty((N, C, 2), dtype=torch.float64, device=x.device)
    if N == 0:
        return out, stats
    nbytes = _lib.rroi_instancenorm_workspace_bytes(N, C, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    st = _lib.rroi_instancenorm_forward_train_hip(
        _DTYPES[x.dtype], x.data_ptr(), None if weight is None else weight.data_ptr(), None if bias is None else bias.data_ptr(),
        out.data_ptr(), stats.data_ptr(), N, C, H, W, eps, negative_slope, None if ws is None else ws.data_ptr(), nbytes,
        _stream())
    if st != 1:
        _check(st, "rroi_instancenorm_forward_train_hip")
    return out, stats


def instance_norm_backward(dy: torch.Tensor, x: torch.Tensor, stats: torch.Tensor, weight=None, bias=None, eps: float = 1e-5,
                           negative_slope: float = 1.0, need_dx: bool = True, need_param_grads: bool = True):
    """The backward of `instance_norm_train` -- DESIGN 5.24: -> (dx, dweight, dbias), each None where it was not asked
    for (`need_param_grads` without a weight asks for nothing).  dy has x's shape, dtype and device; stats is what
    `instance_norm_train` returned for this x.  Everything in double, sums in a fixed order: the same bits on every run.
    ValueError for mismatched shapes, dtypes or devices, a stats that is not (N, C, 2) float64, and a call that asks for
    no gradient at all; TypeError / RuntimeError as `instance_norm`."""
    for name, t in (("dy", dy), ("x", x), ("stats", stats)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,C,H,W), got {tuple(x.shape)}")
    if dy.shape != x.shape:
        raise ValueError(f"dy must have x's shape {tuple(x.shape)}, got {tuple(dy.shape)}")
    if dy.dtype != x.dtype:
        raise ValueError(f"x and dy must have one dtype, got {x.dtype} and {dy.dtype}")
    if tuple(stats.shape) != (x.size(0), x.size(1), 2) or stats.dtype != torch.float64:
        raise ValueError(f"stats must be {(x.size(0), x.size(1), 2)} float64, got {tuple(stats.shape)} of {stats.dtype}")
    weight, bias = _check_norm_args(x, weight, bias)
    if dy.device != x.device or stats.device != x.device:
        raise ValueError("x, dy and stats must be on the same device")
    need_dx, need_params = bool(need_dx), bool(need_param_grads) and weight is not None
    if not need_dx and not need_params:
        raise ValueError("no gradient is asked for")
    return run_instance_norm_backward(dy.contiguous(), x.contiguous(), stats.contiguous(), weight, bias, float(eps),
                                      float(negative_slope), need_dx, need_params)


def run_instance_norm_backward(dy, x, stats, weight, bias, eps: float, negative_slope: float, need_dx: bool, need_params: bool):
    """The call itself, for arguments already checked: dy and x contiguous CUDA (N,C,H,W) tensors of one dtype, stats
    contiguous (N,C,2) float64, weight and bias contiguous (C,) or both None (then need_params is False)."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_instance_norm_backward(dy, x, stats, weight, bias, eps, negative_slope, need_dx, need_params)
    N, C, H, W = x.shape
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(weight) if need_params else None
    db = torch.empty_like(weight) if need_params else None
    if N == 0:
        if need_params:
            dw.zero_()
            db.zero_()
        return dx, dw, db
    nbytes = _lib.rroi_instancenorm_backward_workspace_bytes(N, C, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    st = _lib.rroi_instancenorm_backward_hip(
        _DTYPES[x.dtype], dy.data_ptr(), x.data_ptr(), stats.data_ptr(), None if weight is None else weight.data_ptr(),
        None if bias is None else bias.data_ptr(), None if dx is None else dx.data_ptr(), None if dw is None else dw.data_ptr(),
        None if db is None else db.data_ptr(), N, C, H, W, eps, negative_slope, ws.data_ptr(), nbytes, _stream())
    if st != 1:
        _check(st, "rroi_instancenorm_backward_hip")
    return dx, dw, db
