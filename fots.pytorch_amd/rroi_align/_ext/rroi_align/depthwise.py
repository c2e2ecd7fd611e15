"""rroi_align._ext.rroi_align.depthwise -- the binding of the network's depthwise 3x3 convolution (header section 5,
DESIGN 5.10; `csrc/rroi_depthwise_host.h`)."""
import torch

from ._core import (_DTYPES, _bind, _check, _i, _lib, _require_depthwise_device, _require_depthwise_shapes, _stream, _vp)

_bind("rroi_depthwise3x3_forward_hip", [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp])


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
