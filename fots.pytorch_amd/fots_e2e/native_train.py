"""fots_e2e.native_train -- the first operator of FOTSNet that stays on the package's own kernels when a gradient is needed.

Every switch of `fots_e2e.native` is inference only: a call that needs a gradient takes the stock path.  The most frequent
operator of the network, InstanceNorm2d (49 calls per pass, instance statistics in training as in the reference), has a
native backward, and `use_trainable_instancenorm(net)` -- called after `native.use_native_instancenorm` --
switches every `NativeInstanceNorm2d` to `TrainableInstanceNorm2d`, which runs `rroi_align.norm`'s autograd function
where a gradient is needed and `trainable_norm_ok` holds, and is its parent class everywhere else.  The same terms as
the other switches: opt-in, only classes change, each call asks a pure predicate.  In training mode the native blocks of
`native.use_native_blocks` run their stock forward, which calls the norm modules one by one, so all 49 are reached.

The residual and mirror epilogues of DESIGN 5.13, running statistics, channels-last inputs and a double backward keep the
stock path when a gradient is needed.

It lives in a module of its own for the reason `native_remainder` does: the `_*_slower` hooks of `fots_e2e.native` are a
closed list that the network tests read."""
import torch
import torch.nn as nn

from . import native as _nat

_NORM = []


def _norm():
    """`rroi_align.norm`, loaded on first use: asking the predicate needs neither the library nor a GPU."""
    if not _NORM:
        from rroi_align import norm
        _NORM.append(norm)
    return _NORM[0]


def _needs_grad(m, x) -> bool:
    if not (isinstance(x, torch.Tensor) and torch.is_grad_enabled()):
        return False
    return x.requires_grad or any(p is not None and p.requires_grad for p in (m._parameters.get("weight"), m._parameters.get("bias")))


def trainable_norm_ok(m, x) -> bool:
    """True where `m(x)` may run the native forward and backward when a gradient is needed: `native.instancenorm_ok`'s
    conditions other than its gradient clause (asked with gradients off, so that there is one copy of them), and not a
    shape class whose forward + backward measured slower (`_inorm_backward_slower`).  Pure, no GPU needed to ask."""
    with torch.no_grad():
        return _nat.instancenorm_ok(m, x) and not _inorm_backward_slower(x, getattr(m, "fused_slope", None))


def _inorm_backward_slower(x, slope) -> bool:
    """The shape classes in which native forward + backward did not meet the bar against autograd of the stock pair
    (profiles/native_instancenorm_backward.md, microseconds per forward + backward, native / stock minimum, two runs).
    `slope` is the module's `fused_slope`: None where it applies no activation.
      float32, more than 16,384 planes of at most 128 elements -- 49,152 planes of 64 / 96 elements, the head's last norm
        on eight images' crops: 262.4 / 204.7 and 266.4 / 215.7 (with the activation 262.4 / 216.1, 266.4 / 232.1).  It is
        the class `native._inorm_slower` declines for the forward, so `instancenorm_ok` has answered before this is asked.
      bfloat16 / float16 without an activation, at most 128 planes of 32,768 to 131,071 elements -- the one measured row is
        64 planes of 176 x 320 at N = 1: 79.0 / 78.8 and 79.2 / 78.6 in bfloat16, 79.7 / 79.8 and 80.6 / 80.6 in float16:
        both legs stand at the floor of a forward + backward issued from Python, and the native one does not get below it.
        The same shape wins with the activation (79.2 / 92.2) and in float32 (78.7 / 81.8); its neighbours win without it
        (64 planes of 225,280 elements 79.0 / 317.4, 128 planes of 14,080 74.2 / 79.2), and the lines are drawn at the
        split form's first plane size and below the next measured one."""
    return (slope is None and x.dtype in (torch.bfloat16, torch.float16) and x.size(0) * x.size(1) <= 128
            and 32768 <= x.size(2) * x.size(3) < 131072)


class TrainableInstanceNorm2d(_nat.NativeInstanceNorm2d):
    """A `NativeInstanceNorm2d` (same parameters, same `state_dict` keys, `fused_slope` honoured on every path) whose
    forward, where a gradient is needed and `trainable_norm_ok(self, x)` holds, is `rroi_align.norm`'s autograd function:
    native forward, native deterministic backward."""

    def forward(self, x):
        if _needs_grad(self, x) and trainable_norm_ok(self, x):
            p, slope = self._parameters, self.fused_slope
            return _norm()._InstanceNorm.apply(x, p.get("weight"), p.get("bias"), float(self.eps),
                                               1.0 if slope is None else float(slope))
        return super().forward(x)


def use_trainable_instancenorm(net: nn.Module, enable: bool = True) -> int:
    """Switch every `NativeInstanceNorm2d` of `net` to `TrainableInstanceNorm2d` (enable=False: back), so call it after
    `native.use_native_instancenorm` and undo it before undoing that.  Only the class of a module changes: no parameter
    is copied, no key of the state_dict moves, a `fused_slope` stays.  Returns the number of modules switched (52 for
    `FOTSNet()`)."""
    src, dst = (_nat.NativeInstanceNorm2d, TrainableInstanceNorm2d) if enable else (TrainableInstanceNorm2d, _nat.NativeInstanceNorm2d)
    n = 0
    for m in net.modules():
        if type(m) is src:
            m.__class__ = dst
            n += 1
    return n
