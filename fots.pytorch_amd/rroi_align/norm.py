"""rroi_align.norm -- the network's InstanceNorm2d with its activation as a differentiable function: the
native forward of DESIGN 5.11 with every plane's statistics kept, and a native backward that uses them.

What it adds to `F.leaky_relu(F.instance_norm(x, ...))`: one launch forward whatever the dtype (the stock 16-bit path
runs a statistics and a transform kernel with casts around them), the activation's gradient taken from the forward's own
sign decisions without a saved mask, and a DETERMINISTIC backward -- every sum in double, in a fixed order, no atomic --
so it runs under `torch.use_deterministic_algorithms(True)` and gives the same bits on every run.  Instance statistics
only; no double backward.  GPU only, as the rest of the package."""
import torch
from torch.autograd.function import once_differentiable

from ._ext.rroi_align.instancenorm import (_check_norm_args, _instance_norm_run, run_instance_norm_backward,
                                           run_instance_norm_train)


class _InstanceNorm(torch.autograd.Function):
    """x, weight and bias checked and contiguous (`instance_norm` below; fots_e2e.native_train after its predicate)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, negative_slope):
        y, stats = run_instance_norm_train(x, weight, bias, eps, negative_slope)
        ctx.save_for_backward(x, stats, weight, bias)
        ctx.eps, ctx.negative_slope = eps, negative_slope
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, stats, weight, bias = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[0]
        need_params = weight is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        if not need_dx and not need_params:
            return None, None, None, None, None
        dx, dw, db = run_instance_norm_backward(dy.contiguous(), x, stats, weight, bias, ctx.eps, ctx.negative_slope, need_dx,
                                                need_params)
        return (dx, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None, None, None)


def instance_norm(x: torch.Tensor, weight=None, bias=None, eps: float = 1e-5, negative_slope: float = 1.0) -> torch.Tensor:
    """InstanceNorm2d of (N,C,H,W) `x` over each (n, c) plane (biased variance, instance statistics), then
    `v < 0 ? v * negative_slope : v` (1.0: no activation, 0.0: ReLU), differentiable in x, weight and bias.  float32,
    bfloat16 or float16; weight and bias are (C,) of x's dtype, or both None.  The output has the bits of
    `rroi_align._ext.rroi_align.instance_norm`, which this is where no gradient is needed.  The same exceptions."""
    weight, bias = _check_norm_args(x, weight, bias)
    x = x.contiguous()
    eps, negative_slope = float(eps), float(negative_slope)
    if not (torch.is_grad_enabled() and (x.requires_grad or (weight is not None and (weight.requires_grad or bias.requires_grad)))):
        return _instance_norm_run(x, weight, bias, eps, negative_slope)
    return _InstanceNorm.apply(x, weight, bias, eps, negative_slope)
