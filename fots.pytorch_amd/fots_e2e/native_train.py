"""fots_e2e.native_train -- the operators of FOTSNet that stay on the package's own kernels when a gradient is needed:
InstanceNorm2d (below), the depthwise 3x3 convolution and the feature merge (at the end of the file).

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

The stretch between them, the feature merge -- six bilinear resizes per pass, whose stock backward scatters with atomics
and raises under `torch.use_deterministic_algorithms(True)` -- has native gradients too:
`use_trainable_merge(net)` -- called after `native.use_native_merge` -- switches the network's class to a subclass whose
`_merge`, in training mode, runs the three merges and the two stand-alone resizes through `rroi_align.merge`'s autograd
functions where a gradient is needed and `trainable_merge_ok` holds.

The order, for all three: a trainable switch extends the class its native switch makes, so it goes on after that switch
and comes off before it.  A native switch undone while its trainable one is still on finds no class of its own, changes
nothing and returns zero counts; the network computes what it did (`fots_e2e._switching`).

It lives in a module of its own for the reason `native_remainder` does: the `_*_slower` hooks of `fots_e2e.native` are a
closed list that the network tests read."""
import torch
import torch.nn as nn

from . import _switching as _sw
from . import native as _nat

# The autograd functions, each module loaded on first use: asking a predicate needs neither the library nor a GPU.
_norm = _sw.lazy_module("rroi_align.norm")
_conv = _sw.lazy_module("rroi_align.conv")
_merge_fn = _sw.lazy_module("rroi_align.merge")


def _any_needs_grad(tensors, params) -> bool:
    """Whether autograd wants a gradient through one of `tensors` or into one of `params` (None: an absent parameter)."""
    return torch.is_grad_enabled() and (any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)
                                        or any(p is not None and p.requires_grad for p in params))


def _needs_grad(m, x) -> bool:
    """Whether `m(x)` needs a gradient: through the tensor x, or into a parameter of m's own."""
    return isinstance(x, torch.Tensor) and _any_needs_grad((x,), m._parameters.values())


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
    """Switch every `NativeInstanceNorm2d` of `net` to `TrainableInstanceNorm2d` (enable=False: back): on after
    `native.use_native_instancenorm`, off before it (the module docstring).  Only the class of a module changes: no
    parameter is copied, no key of the state_dict moves, a `fused_slope` stays.  Returns the number of modules switched (52 for
    `FOTSNet()`)."""
    return _sw.swap_classes(net, ((_nat.NativeInstanceNorm2d, TrainableInstanceNorm2d),), enable)[0]


# --------------------------------------------------------------------------- depthwise 3x3 convolution, DESIGN 5.25
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
        if _needs_grad(self, x) and trainable_depthwise_ok(self, x):
            return _conv()._Depthwise3x3.apply(x, self._parameters["weight"], self.stride[0])
        return super().forward(x)


def use_trainable_depthwise(net: nn.Module, enable: bool = True) -> int:
    """Switch every `DepthwiseConv3x3` of `net` to `TrainableDepthwiseConv3x3` (enable=False: back): on after
    `native.use_native_depthwise`, off before it (the module docstring).  Only the class of a module changes: no
    parameter is copied, no key of the state_dict moves.  Returns the number of modules switched (22 for `FOTSNet()`)."""
    return _sw.swap_classes(net, ((_nat.DepthwiseConv3x3, TrainableDepthwiseConv3x3),), enable)[0]


# --------------------------------------------------------------------------- the feature merge, DESIGN 5.26
_MAX_FOOTPRINT = 4096     # kRsMaxFootprint of csrc/rroi_merge_backward_kernels.h


def _footprint_bound(n_in: int, n_out: int) -> int:
    """rs_max_footprint of csrc/rroi_merge_backward_host.h, mirrored: an upper bound of the output rows that meet in one
    source row; the library refuses a backward above `_MAX_FOOTPRINT`."""
    if n_out == 1:
        return 1
    if n_in == 1:
        return n_out
    return min(n_out, int(2.0 / ((n_in - 1) / (n_out - 1))) + 2)


def _gather_ok(src, like) -> bool:
    return all(_footprint_bound(i, o) <= _MAX_FOOTPRINT for i, o in zip(src.shape[2:], like.shape[2:]))


def trainable_merge_ok(a, f, gate=None, resize_only: bool = False) -> bool:
    """True where `up(a) + f * up(gate)` (resize_only: `up(a)` alone, to f's size) may run the native forward and backward
    when a gradient is needed: `native.merge_ok`'s conditions other than its gradient clause (asked with gradients off, so
    that there is one copy of them), a resize the backward's gather accepts (at most 4096 output rows or columns meeting in
    one source element), and not a shape class whose forward + backward measured slower (`_merge_backward_slower`; not
    asked under `torch.use_deterministic_algorithms(True)`, where the stock backward raises and speed is no reason to
    take it).  Pure, no GPU needed to ask."""
    with torch.no_grad():
        return (_nat.merge_ok(a, f, gate) and _gather_ok(a, f) and (gate is None or _gather_ok(gate, f))
                and (torch.are_deterministic_algorithms_enabled() or not _merge_backward_slower(a, f, gate, resize_only)))


def _merge_backward_slower(a, f, gate, resize_only) -> bool:
    """The shape classes in which native forward + backward did not meet the bar of DESIGN 5.10 against autograd of the
    stock expression in BOTH runs (profiles/native_merge_backward.md, microseconds per forward + backward, native median /
    stock minimum, two runs of 30 rows: the network's three merges and two resizes at 704 x 1280, one and eight images,
    three dtypes).  Both are gated merges at one image, where both legs stand at the floor of issuing a forward + backward
    from Python and the native one, with its four or five launches, does not get below it:
      `a` of f's size, 1.8e6 to 9.0e6 elements in f, any dtype -- the one measured row is the second merge at one image,
        256 x 88 x 160 = 3.6e6: float32 84.5 / 79.6 and 85.2 / 77.1, bfloat16 79.8 / 78.6 and 76.6 / 70.6, float16
        77.8 / 73.5 and 81.2 / 78.3.  Its neighbours win: the third merge at one image (1.44e7 elements: 125.2 / 151.0,
        77.7 / 92.3, 77.7 / 89.4) and itself at eight images (2.9e7: 194.9 / 287.6, 106.3 / 184.9, 107.1 / 177.3).
      float32, `a` resized, 4.5e5 to 4.05e6 elements in f -- the first merge at one image, 256 x 44 x 80 = 9.0e5:
        172.2 / 127.3 and 132.2 / 127.9, rounds from 87 to 304; float16 wins twice (88.0 / 97.2, 87.1 / 96.9), bfloat16
        misses once and is no class (179.1 / 104.6, then 88.0 / 104.2), and at eight images (7.2e6) every dtype wins 7-9 x.
    The upper lines are halfway to the next measured row and the lower ones at half the measured size, as
    `_inorm_backward_slower` draws them; nothing smaller was measured and it stays native.  No stand-alone resize misses.
    Under `torch.use_deterministic_algorithms(True)` the predicate does not ask this hook: the stock backward raises there."""
    if resize_only or gate is None:
        return False
    n = f.numel()
    if a.shape[2:] == f.shape[2:]:
        return 1_800_000 <= n < 9_000_000
    return f.dtype == torch.float32 and 450_000 <= n < 4_050_000


class _TrainableMerge:
    """Mixin in front of a `*Merge*FOTSNet`: in training mode, where a gradient is needed, `_merge` runs the three merges
    through `rroi_align.merge.gated_merge` -- the gate at its source's size from `_train_gate`: `torch.sigmoid(self.conv_attenton(t))`
    under stock autograd -- and the two resizes in front of `upconv1` / `upconv2` through `bilinear_resize`, each where
    `trainable_merge_ok` holds and as `FOTSNet._merge`'s expression where it does not.  Everywhere else it is its parent."""

    def _train_resize(self, t, like):
        if trainable_merge_ok(t, like, None, True):
            return _merge_fn()._BilinearResize.apply(t, like.size(2), like.size(3))
        return self._up(t, like)

    def _train_gate(self, t):
        """The gate at its source's size, under stock autograd (`native_train_heads` overrides it)."""
        return torch.sigmoid(self.conv_attenton(t))

    def _train_merge_one(self, a, f, t):
        g = self._train_gate(t) if self.attention else None
        if trainable_merge_ok(a, f, g):
            return _merge_fn()._GatedMerge.apply(a, f, g)
        A = a if a.shape[2:] == f.shape[2:] else self._up(a, f)
        return A + f if g is None else A + f * self._up(g, f)

    def _merge(self, f1, f2, f3, f4):
        own = (self.conv_attenton, self.upconv1, self.upconv2) if self.attention else (self.upconv1, self.upconv2)
        if not (self.training and _any_needs_grad((f1, f2, f3, f4), (p for m in own for p in m.parameters()))):
            return super()._merge(f1, f2, f3, f4)
        t = self._train_merge_one(f4, f3, f4)
        m2 = self._train_merge_one(self.upconv1(self._train_resize(t, f2)), f2, t)
        m1 = self._train_merge_one(self.upconv2(self._train_resize(m2, f1)), f1, m2)
        return m1, m2


class TrainableMergeFOTSNet(_TrainableMerge, _nat.NativeMergeFOTSNet):
    """A `NativeMergeFOTSNet` (same modules, same `state_dict` keys) whose feature merge stays native in training."""


class TrainableHeadsMergeFOTSNet(_TrainableMerge, _nat.NativeHeadsMergeFOTSNet):
    """A `NativeHeadsMergeFOTSNet` whose feature merge stays native in training."""


class TrainableMergeRecogniserFOTSNet(_TrainableMerge, _nat.NativeMergeRecogniserFOTSNet):
    """A `NativeMergeRecogniserFOTSNet` whose feature merge stays native in training."""


class TrainableHeadsMergeRecogniserFOTSNet(_TrainableMerge, _nat.NativeHeadsMergeRecogniserFOTSNet):
    """A `NativeHeadsMergeRecogniserFOTSNet` whose feature merge stays native in training."""


def use_trainable_merge(net: nn.Module, enable: bool = True) -> bool:
    """Switch a network whose type is exactly one of the four `*Merge*FOTSNet` classes of `fots_e2e.native` to its trainable
    subclass (enable=False: back): on after `native.use_native_merge` -- and after `use_native_heads` /
    `use_native_recogniser`, which look for the exact types they know -- and off before them.  Only the class
    of the network changes: no parameter is copied, no key of the state_dict moves.  A network of any other type is left
    alone.  Returns whether the class was switched."""
    return _sw.toggle_feature(net, _NETS, _TrainableMerge, enable)


# Every trainable class (read off the classes above) and the native class it extends, its second base, by what they have.
_TRAINABLE = [c for c in list(globals().values())
              if isinstance(c, type) and issubclass(c, _TrainableMerge) and c is not _TrainableMerge]
_NETS = _sw.feature_table(_TRAINABLE + [c.__bases__[1] for c in _TRAINABLE], _nat._FEATURES + (_TrainableMerge,))
