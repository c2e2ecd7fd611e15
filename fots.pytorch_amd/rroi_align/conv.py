"""rroi_align.conv -- the network's depthwise 3x3 convolution as a differentiable function: the native
forward of DESIGN 5.10 and a native backward for its input and its weight.

What it adds to `F.conv2d(x, w, None, stride, 1, 1, C)`: one launch forward, one launch for the input gradient with the
forward's arithmetic (bit-exact against a recipe, as the forward is), and a DETERMINISTIC weight gradient -- every sum in
double, in a fixed order, no atomic -- so it runs under `torch.use_deterministic_algorithms(True)` and gives the same bits
on every run.  Padding 1, no bias, stride 1 or 2; no double backward.  GPU only, as the rest of the package."""
import torch
from torch.autograd.function import once_differentiable

from ._ext.rroi_align._core import _require_depthwise_device, _require_depthwise_shapes
from ._ext.rroi_align.depthwise import _depthwise3x3_run, run_depthwise3x3_backward


class _Depthwise3x3(torch.autograd.Function):
    """x and weight checked, x contiguous (`depthwise3x3` below; fots_e2e.native_train after its predicate)."""

    @staticmethod
    def forward(ctx, x, weight, stride):
        weight = weight.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        return _depthwise3x3_run(x, weight, stride)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not need_dx and not need_dw:
            return None, None, None
        dx, dw = run_depthwise3x3_backward(dy.contiguous(), x, weight, ctx.stride, need_dx, need_dw)
        return dx, dw, None


def depthwise3x3(x: torch.Tensor, weight: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """(N,C,H,W) x (C,1,3,3) -> (N,C,Ho,Wo): depthwise 3x3 convolution, padding 1, no bias, stride 1 or 2, differentiable
    in x and weight.  float32, bfloat16 or float16, x and weight alike; x is made NCHW-contiguous.  The output has the bits
    of `rroi_align._ext.rroi_align.depthwise3x3`, which this is where no gradient is needed.  The same exceptions."""
    _require_depthwise_shapes(x, weight, "x", "(N,C,H,W)")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2, got {stride!r}")
    _require_depthwise_device(x, weight, "x")
    x, stride = x.contiguous(), int(stride)
    if not (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)):
        return _depthwise3x3_run(x, weight, stride)
    return _Depthwise3x3.apply(x, weight, stride)
