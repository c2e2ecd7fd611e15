"""rroi_align.merge -- the network's gated merge and its bilinear resize as differentiable functions: the
native forward of DESIGN 5.14 and native backwards for `a`, `f` and the gate.

What it adds to `up(a) + f * up(gate)` with `up = F.interpolate(..., mode="bilinear", align_corners=True)`: the stock
backward of that resize scatters with atomics, so it raises under `torch.use_deterministic_algorithms(True)` and gives
different bits from run to run without it.  Here every gradient is a gather or an element-wise product: `df` is bit-exact
against a recipe, `da` and `dgate` are double sums in an order the shape alone fixes, rounded once -- the same bits on
every run and device.  NCHW, align_corners=True only; no double backward.  GPU only, as the rest of the package."""
import torch
from torch.autograd.function import once_differentiable

from ._ext.rroi_align._core import _require_map, _size2
from ._ext.rroi_align.merge import (_gated_merge_run, run_gated_merge_backward, run_resize_bilinear,
                                    run_resize_bilinear_backward)


class _BilinearResize(torch.autograd.Function):
    """x checked and contiguous (`bilinear_resize` below; fots_e2e.native_train after its predicate)."""

    @staticmethod
    def forward(ctx, x, H, W):
        ctx.in_size = tuple(x.shape[2:])
        return run_resize_bilinear(x, H, W)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return run_resize_bilinear_backward(dy.contiguous(), *ctx.in_size), None, None


class _GatedMerge(torch.autograd.Function):
    """a, f and the gate checked and contiguous (`gated_merge` below; fots_e2e.native_train after its predicate)."""

    @staticmethod
    def forward(ctx, a, f, gate):
        ctx.a_size = tuple(a.shape[2:])
        ctx.save_for_backward(f, gate)
        return _gated_merge_run(a, f, gate)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        f, gate = ctx.saved_tensors
        need_da, need_df, need_dg = ctx.needs_input_grad
        need_dg = need_dg and gate is not None
        if not (need_da or need_df or need_dg):
            return None, None, None
        dy = dy.contiguous()
        da = df = dg = None
        if need_da:
            da = dy if ctx.a_size == tuple(f.shape[2:]) else run_resize_bilinear_backward(dy, *ctx.a_size)
        if gate is None:
            df = dy if need_df else None
        elif need_df or need_dg:
            df, dg = run_gated_merge_backward(dy, f, gate, need_df, need_dg)
        return da, df, dg


def bilinear_resize(x: torch.Tensor, size) -> torch.Tensor:
    """(N,C,h,w) -> (N,C,*size): bilinear, align_corners=True, differentiable in x.  float32, bfloat16 or float16; x is made
    NCHW-contiguous.  The output has the bits of `rroi_align._ext.rroi_align.resize_bilinear`, which this is where no
    gradient is needed.  The same exceptions."""
    _require_map(x, "x")
    H, W = _size2(size, "size")
    x = x.contiguous()
    if not (torch.is_grad_enabled() and x.requires_grad):
        return run_resize_bilinear(x, H, W)
    return _BilinearResize.apply(x, H, W)


def gated_merge(a: torch.Tensor, f: torch.Tensor, gate=None) -> torch.Tensor:
    """y = up(a) + f * up(gate) (gate=None: up(a) + f), differentiable in a, f and the gate.  a (N,C,a_h,a_w), f (N,C,H,W),
    gate (N,1,g_h,g_w), one dtype and device; the tensors are made NCHW-contiguous.  The output has the bits of
    `rroi_align._ext.rroi_align.gated_merge`, which this is where no gradient is needed.  The same exceptions."""
    _require_map(f, "f")
    _require_map(a, "a", f, "f")
    if a.shape[:2] != f.shape[:2]:
        raise ValueError(f"a and f must agree in batch size and channels, got {tuple(a.shape)} and {tuple(f.shape)}")
    if gate is not None:
        _require_map(gate, "gate", f, "f")
        if gate.size(0) != f.size(0) or gate.size(1) != 1:
            raise ValueError(f"the gate must be (N,1,h,w) with f's batch size, got {tuple(gate.shape)} for f {tuple(f.shape)}")
    a, f = a.contiguous(), f.contiguous()
    gate = None if gate is None else gate.contiguous()
    if not (torch.is_grad_enabled() and (a.requires_grad or f.requires_grad or (gate is not None and gate.requires_grad))):
        return _gated_merge_run(a, f, gate)
    return _GatedMerge.apply(a, f, gate)
