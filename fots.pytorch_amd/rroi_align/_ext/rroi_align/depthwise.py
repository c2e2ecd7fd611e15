"""rroi_align._ext.rroi_align.depthwise -- the binding of the network's depthwise 3x3 convolution (header section 5,
DESIGN 5.10; `csrc/rroi_depthwise_host.h`) and of its backward (section 5b, DESIGN 5.25;
`csrc/rroi_depthwise_backward_host.h`)."""
import collections
import ctypes

import torch

from ._core import (_DTYPES, _IO_DTYPES, DTYPE_FP32, _bind, _check, _i, _lib, _plan_query, _require_cuda_f32,
                    _require_depthwise_device, _require_depthwise_shapes, _stream, _sz, _vp, _workspace, dtype_code)


class _DwBwdPlan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("dx_band", "dx_cols", "dx_grid_x", "dw_band", "segments", "dw_grid_x", "launches", "block")]


_bind("rroi_depthwise3x3_forward_hip", [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp])
_bind("rroi_depthwise3x3_backward_hip", [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp])
_bind("rroi_depthwise3x3_backward_workspace_bytes", [_i] * 5, _sz)
_bind("rroi_depthwise3x3_backward_plan", [_i] * 6 + [ctypes.POINTER(_DwBwdPlan)])

DepthwiseBackwardPlan = collections.namedtuple("DepthwiseBackwardPlan", [n for n, _ in _DwBwdPlan._fields_])


def depthwise3x3(x: torch.Tensor, weight: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """(N,C,H,W) x (C,1,3,3) -> (N,C,Ho,Wo): depthwise 3x3 convolution, padding 1, no bias, stride 1 or 2.
    float32, bfloat16 or float16, x and weight alike; x is made NCHW-contiguous.  Every output is the double sum of its
    nine widened products in (ky, kx) order, rounded to fp32 once and then to the tensors' type: the same bits on every
    run.  Forward only (no autograd).  ValueError for mismatched shapes or dtypes, RuntimeError for CPU tensors."""
    _require_depthwise_shapes(x, weight, "x", "(N,C,H,W)")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2, got {stride!r}")
    _require_depthwise_device(x, weight, "x")
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


# --------------------------------------------------------------------------- backward (header section 5b)
def depthwise3x3_backward_plan(batch_size, channels, height, width, stride=1, dtype=DTYPE_FP32) -> DepthwiseBackwardPlan:
    """What `depthwise3x3_backward` launches for an x of this shape (host only, no GPU needed): the dx launch's rows and
    columns per thread and its grid, the partials launch's rows per thread, its workgroups per plane (`segments`) and its
    grid, the launches of a call that wants both gradients.  ValueError where the call would refuse the arguments."""
    return _plan_query(_lib.rroi_depthwise3x3_backward_plan, _DwBwdPlan, DepthwiseBackwardPlan, "rroi_depthwise3x3_backward_plan",
                       (dtype_code(dtype), batch_size, channels, height, width, stride))


def depthwise3x3_backward_workspace_bytes(batch_size, channels, height, width, stride=1) -> int:
    """Bytes of workspace `rroi_depthwise3x3_backward_hip` needs for dweight at this shape (nine doubles per workgroup of
    the partials launch); 0 for a shape the call would refuse."""
    return int(_lib.rroi_depthwise3x3_backward_workspace_bytes(int(batch_size), int(channels), int(height), int(width), int(stride)))


def depthwise3x3_backward(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, stride: int = 1, need_dx: bool = True,
                          need_dweight: bool = True):
    """The backward of `depthwise3x3` -- DESIGN 5.25: -> (dx, dweight), each None where it was not asked for.  dy is
    (N,C,Ho,Wo) of x's dtype and device.  dx is bit-exact: every element the double sum of its (at most nine) widened
    products, dy visited in row-major order, rounded to fp32 once and then to the tensors' type.  dweight is summed in
    double in a fixed order without atomics and rounded once: the same bits on every run.  dy and x are made
    NCHW-contiguous.  ValueError for mismatched shapes, dtypes or devices and for a call that asks for no gradient,
    TypeError / RuntimeError as `depthwise3x3`."""
    _require_depthwise_shapes(x, weight, "x", "(N,C,H,W)")
    if not isinstance(dy, torch.Tensor):
        raise TypeError("dy must be a torch.Tensor")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2, got {stride!r}")
    N, C, H, W = x.shape
    want = (N, C, (H - 1) // stride + 1, (W - 1) // stride + 1)
    if tuple(dy.shape) != want:
        raise ValueError(f"dy must be {want} for x {tuple(x.shape)} at stride {stride}, got {tuple(dy.shape)}")
    if dy.dtype != x.dtype:
        raise ValueError(f"x and dy must have one dtype, got {x.dtype} and {dy.dtype}")
    _require_depthwise_device(x, weight, "x")
    _require_cuda_f32(dy, "dy", _IO_DTYPES)
    if dy.device != x.device:
        raise ValueError("x and dy must be on the same device")
    need_dx, need_dweight = bool(need_dx), bool(need_dweight)
    if not need_dx and not need_dweight:
        raise ValueError("no gradient is asked for")
    return run_depthwise3x3_backward(dy.contiguous(), x.contiguous(), weight.contiguous(), int(stride), need_dx, need_dweight)


def run_depthwise3x3_backward(dy, x, weight, stride: int, need_dx: bool, need_dweight: bool):
    """The call itself, for arguments already checked (depthwise3x3_backward above; rroi_align.conv): dy, x and weight
    contiguous CUDA tensors of one dtype and device, (N,C,Ho,Wo), (N,C,H,W) and (C,1,3,3), stride 1 or 2, at least one of
    the two flags.  The workspace comes from the per-stream scratch (`_core._workspace`).  Kept lean: a training step of the
    network makes 22 of these calls."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_depthwise3x3_backward(dy, x, weight, stride, need_dx, need_dweight)
    N, C, H, W = x.shape
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(weight) if need_dweight else None
    if N == 0:
        if need_dweight:
            dw.zero_()
        return dx, dw
    ws, nbytes = None, 0
    if need_dweight:
        nbytes = _lib.rroi_depthwise3x3_backward_workspace_bytes(N, C, H, W, stride)
        ws = _workspace(x.device, nbytes)
    st = _lib.rroi_depthwise3x3_backward_hip(_DTYPES[x.dtype], dy.data_ptr(), x.data_ptr(), weight.data_ptr(),
                                             None if dx is None else dx.data_ptr(), None if dw is None else dw.data_ptr(), N, C,
                                             H, W, stride, None if ws is None else ws.data_ptr(), nbytes, _stream())
    if st != 1:
        _check(st, "rroi_depthwise3x3_backward_hip")
    return dx, dw
