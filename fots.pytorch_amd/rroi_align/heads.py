"""rroi_align.heads -- the network's detection heads and attention gate as differentiable functions: the
native forward of DESIGN 5.12 and a native backward for the map, the weights and the biases.

What it adds to the stock chain (three 1x1 convolutions, three sigmoids, the scalings and the angle's normalisation, some
fourteen launches forward and twice that back): one launch forward that also leaves the pre-activation sums in double,
and a backward of two launches that reads the map once, writes its gradient once and sums the seven weight rows in double
in a fixed order without atomics -- the same bits on every run.  No double backward.  GPU only, as the rest of the
package."""
import torch
from torch.autograd.function import once_differentiable

from ._ext.rroi_align._core import _finite
from ._ext.rroi_align.heads import (_gate_run, _heads_run, _require_pointwise, run_gate_backward, run_gate_train,
                                    run_heads_backward, run_heads_train)


def _needs_grad(tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _like(grad, param):
    """A weight's gradient in the shape of the parameter ((k, C) or (k, C, 1, 1)); None stays None."""
    return None if grad is None or param is None else grad.view_as(param)


class _DetectionHeads(torch.autograd.Function):
    """Arguments checked, x and the parameters contiguous (`detection_heads` below; fots_e2e.native_train_heads after its
    predicate)."""

    @staticmethod
    def forward(ctx, x, w_score, b_score, w_rbox, b_rbox, w_angle, b_angle, rbox_scale):
        ctx.set_materialize_grads(False)
        score, rbox, angle, z = run_heads_train(x, w_score, b_score, w_rbox, b_rbox, w_angle, b_angle, rbox_scale)
        ctx.save_for_backward(x, z, w_score, w_rbox, w_angle)
        ctx.rbox_scale = rbox_scale
        ctx.has_bias = (b_score is not None, b_rbox is not None, b_angle is not None)
        return score, rbox, angle

    @staticmethod
    @once_differentiable
    def backward(ctx, dscore, drbox, dangle):
        need = ctx.needs_input_grad
        need_dx, need_dw = need[0], need[1] or need[3] or need[5]
        need_db = any(n and h for n, h in zip((need[2], need[4], need[6]), ctx.has_bias))
        if (dscore is None and drbox is None and dangle is None) or not (need_dx or need_dw or need_db):
            return (None,) * 8
        x, z, ws, wr, wa = ctx.saved_tensors
        g = [None if t is None else t.contiguous() for t in (dscore, drbox, dangle)]
        dx, dw, db = run_heads_backward(*g, x, z, ws, wr, wa, ctx.rbox_scale, need_dx, need_dw, need_db)
        pick = lambda t, n: t if n else None  # noqa: E731
        return (dx, pick(_like(dw[0], ws), need[1]), pick(db[0], need[2] and ctx.has_bias[0]),
                pick(_like(dw[1], wr), need[3]), pick(db[1], need[4] and ctx.has_bias[1]),
                pick(_like(dw[2], wa), need[5]), pick(db[2], need[6] and ctx.has_bias[2]), None)


class _AttentionGate(torch.autograd.Function):
    """Arguments checked, x and the parameters contiguous (`attention_gate` below; fots_e2e.native_train_heads)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.set_materialize_grads(False)
        y, z = run_gate_train(x, w, b)
        ctx.save_for_backward(x, z, w)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        need_dx, need_dw, need_db = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
        if dy is None or not (need_dx or need_dw or need_db):
            return None, None, None
        x, z, w = ctx.saved_tensors
        dx, dw, db = run_gate_backward(dy.contiguous(), x, z, w, need_dx, need_dw, need_db)
        return dx, _like(dw, w), db


def detection_heads(x: torch.Tensor, w_score, b_score, w_rbox, b_rbox, w_angle, b_angle, rbox_scale: float = 128.0):
    """The three detection heads of (N,C,H,W) `x`, differentiable in x, the weights and the biases: 1x1 convolutions to
    1 / 4 / 2 channels (weights (k,C) or (k,C,1,1), biases (k,) or None), sigmoid, then score = s, rbox = rbox_scale * s,
    angle = (2 s - 1) normalised to unit length.  -> (score, rbox, angle) of x's dtype (float32, bfloat16 or float16).
    The outputs have the bits of `rroi_align._ext.rroi_align.heads`, which this is where no gradient is needed.  The same
    exceptions."""
    rbox_scale = _finite(rbox_scale, "rbox_scale")
    params = _require_pointwise(x, (("score", w_score, b_score, 1), ("rbox", w_rbox, b_rbox, 4), ("angle", w_angle, b_angle, 2)))
    flat = [t for pair in params for t in pair]
    x = x.contiguous()
    if not _needs_grad([x] + flat):
        return _heads_run(x, *flat, rbox_scale)
    return _DetectionHeads.apply(x, *flat, rbox_scale)


def attention_gate(x: torch.Tensor, w, b) -> torch.Tensor:
    """sigmoid of a 1x1 convolution of (N,C,H,W) `x` to one channel, differentiable in x, w and b: w (1,C) or (1,C,1,1), b
    (1,) or None -> (N,1,H,W).  The terms of `detection_heads`."""
    ((w, b),) = _require_pointwise(x, (("gate", w, b, 1),))
    x = x.contiguous()
    if not _needs_grad((x, w, b)):
        return _gate_run(x, w, b)
    return _AttentionGate.apply(x, w, b)
