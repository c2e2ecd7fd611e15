"""fots_e2e.native_train -- the operators of FOTSNet that stay on the package's own kernels when a gradient is needed:
InstanceNorm2d (below) and the depthwise 3x3 convolution (at the end of the file).

Every switch of `fots_e2e.native` is inference only: a call that needs a gradient takes the stock path.  The most frequent
operator of the network, InstanceNorm2d (49 calls per pass, instance statistics in training as in the reference), has a
native backward, and `use_trainable_instancenorm(net)` -- called after `native.use_native_instancenorm` --
switches every `NativeInstanceNorm2d` to `TrainableInstanceNorm2d`, which runs `rroi_align.norm`'s autograd function
where a gradient is needed and `trainable_norm_ok` holds, and is its parent class everywhere else.  The same terms as
the other switches: opt-in, only classes change, each call asks a pure predicate.  In training mode the native blocks of
`native.use_native_blocks` run their stock forward, which calls the norm modules one by one, so all 49 are reached.

The residual and mirror epilogues of DESIGN 5.13, running statistics, channels-last inputs and a double backward keep the
stock path when a gradient is needed.

The second most frequent operator, the depthwise 3x3 convolution (22 calls per pass), has a native backward as well
(DESIGN 5.25): `use_trainable_depthwise(net)` -- called after `native.use_native_depthwise` -- switches every
`DepthwiseConv3x3` to `TrainableDepthwiseConv3x3`, which runs `rroi_align.conv`'s autograd function where a gradient is
needed and `trainable_depthwise_ok` holds.  With `native_remainder.use_native_upconv` on, a call that needs a gradient
already falls back to the block's modules one by one, so all 22 are reached; the fused resize + depthwise has no backward.
Channels-last inputs and autocast keep the stock path; a double backward needs it too (the function is once
differentiable, and whether a graph of the backward will be wanted is not known when the forward runs): switch back with
`enable=False` for one.

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


# --------------------------------------------------------------------------- depthwise 3x3 convolution, DESIGN 5.25
_CONV = []


def _conv():
    """`rroi_align.conv`, loaded on first use, as `_norm`."""
    if not _CONV:
        from rroi_align import conv
        _CONV.append(conv)
    return _CONV[0]


def trainable_depthwise_ok(m, x) -> bool:
    """True where `m(x)` may run the native forward and backward when a gradient is needed: `native.native_ok`'s conditions
    other than its gradient clause (asked with gradients off, so that there is one copy of them), and not a shape class
    whose forward + backward measured slower (`_dw_backward_slower`).  Pure, no GPU needed to ask."""
    with torch.no_grad():
        return _nat.native_ok(m, x) and not _dw_backward_slower(x, m.stride[0])


def _dw_backward_slower(x, stride) -> bool:
    """The shape classes in which native forward + backward did not meet the bar of DESIGN 5.10 against autograd of the
    stock convolution (profiles/native_depthwise_backward.md, microseconds per forward + backward, native / stock minimum,
    two runs of 36 rows: the network's six shapes at one and eight images in three dtypes).  There is none: no row misses
    in both runs.
      One row misses in the first run and not in the second -- float32, 512 planes of 22 x 40 at N = 1: 180.2 / 125.1
        (rounds from 69.7 to 183.9), then 65.7 / 133.8.  It is not a property of the shape: every small shape stands at
        65-68 native against 126-134 stock, the floor of issuing a forward + backward from Python, and in both runs whole
        rounds of some native leg take one or two such floors longer, on the host clock as between device events (first run
        also float32 1 x 256 x 176 x 320: 132.8 against 1517.0, 1 x 256 x 44 x 80 at stride 2: 128.0 / 132.7, 8 x 512 x 22 x 40:
        131.0 / 248.8; second run bfloat16 8 x 256 x 88 x 160: 139.0 / 1075.1), which loses only where the stock leg is at
        its own floor.  A disturbance of the host's issue time, kept and reported as DESIGN 5.24 did for its like.
    A row that misses in both runs becomes a class here, its thresholds halfway to the next measured row, as
    `_inorm_backward_slower` does."""
    return False


class TrainableDepthwiseConv3x3(_nat.DepthwiseConv3x3):
    """A `DepthwiseConv3x3` (same parameters, same `state_dict` keys) whose forward, where a gradient is needed and
    `trainable_depthwise_ok(self, x)` holds, is `rroi_align.conv`'s autograd function: native forward, native input
    gradient, native deterministic weight gradient."""

    def forward(self, x):
        w = self._parameters["weight"]
        if (isinstance(x, torch.Tensor) and torch.is_grad_enabled() and (x.requires_grad or w.requires_grad)
                and trainable_depthwise_ok(self, x)):
            return _conv()._Depthwise3x3.apply(x, w, self.stride[0])
        return super().forward(x)


def use_trainable_depthwise(net: nn.Module, enable: bool = True) -> int:
    """Switch every `DepthwiseConv3x3` of `net` to `TrainableDepthwiseConv3x3` (enable=False: back), so call it after
    `native.use_native_depthwise` and undo it before undoing that.  Only the class of a module changes: no parameter is
    copied, no key of the state_dict moves.  Returns the number of modules switched (22 for `FOTSNet()`)."""
    src, dst = (_nat.DepthwiseConv3x3, TrainableDepthwiseConv3x3) if enable else (TrainableDepthwiseConv3x3, _nat.DepthwiseConv3x3)
    n = 0
    for m in net.modules():
        if type(m) is src:
            m.__class__ = dst
            n += 1
    return n
