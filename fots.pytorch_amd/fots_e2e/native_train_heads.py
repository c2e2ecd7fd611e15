"""fots_e2e.native_train_heads -- the detection heads and the attention gates of FOTSNet on the package's own kernels when
a gradient is needed.

`native.use_native_heads` is inference only: a `_heads` or `_gate` call that needs a gradient takes the stock chain, some
fourteen launches forward and twice that back.  `use_trainable_heads(net)` switches the network's class to a subclass whose
`_heads` (twice per pass) and `_gate` (three times; inside `native_train._TrainableMerge`, `_train_gate`) run
`rroi_align.heads`'s autograd functions where a gradient is needed and `trainable_heads_ok` holds: one launch forward, two
back, every sum in double in a fixed order without atomics.  Between the native merge backward and the native
detection loss, that makes the detection tail of a training step native and deterministic.  The dropout in
front of the 1/4 heads stays stock.

The order: this switch extends the classes every other network switch makes, so it goes on last -- after
`native.use_native_heads`, after `use_native_merge` / `use_native_recogniser`, after `native_train.use_trainable_merge` --
and comes off first.  Out of that order a switch finds no class of its own, changes nothing and returns False
(`fots_e2e._switching`).

It lives in a module of its own with a table of its own: `native._NETS` and `native_train._NETS` are closed lists that the
switching tests read."""
import torch
import torch.nn as nn

from . import _switching as _sw
from . import native as _nat
from . import native_train as _tr

# The autograd functions, loaded on first use: asking the predicate needs neither the library nor a GPU.
_heads_fn = _sw.lazy_module("rroi_align.heads")


def trainable_heads_ok(net, t, gate: bool = False) -> bool:
    """True where `net._heads(t)` (gate=True: the convolution and sigmoid of `net._gate(t, like)`) may run the native
    forward and backward when a gradient is needed: `native.heads_ok`'s conditions other than its gradient clauses (asked
    with gradients off, so that there is one copy of them), and not a shape class whose forward + backward measured slower
    (`_heads_backward_slower`; asked under `torch.use_deterministic_algorithms(True)` as well: the stock chain is
    convolutions and element-wise operators, none of which raises there -- the network's other stock convolutions train
    in that mode in the tests -- so determinism is no reason to take a slower path).  Pure, no GPU needed to ask."""
    with torch.no_grad():
        return _nat.heads_ok(net, t, gate) and not _heads_backward_slower(t, gate)


def _heads_backward_slower(t, gate) -> bool:
    """The shape classes in which native forward + backward did not meet the bar of DESIGN 5.10 against autograd of the
    stock expression in BOTH runs (profiles/native_heads_backward.md, microseconds per forward + backward, native median /
    stock minimum, two runs of 30 rows: the heads on the 1/4 and 1/8 maps of a 704 x 1280 image and the gate on its three
    maps, one and eight images, three dtypes).  There is none: no row misses in both runs.
      Two rows miss in the first run and not in the second -- the gate in float16 at eight images, 256 x 44 x 80:
        183.6 / 126.6 (rounds from 77.4 to 188.2), then 75.8 / 130.3; 256 x 88 x 160: 178.6 / 153.4 (rounds from 120.3),
        then 120.8 / 152.2.  Not a property of the shape: in those rows whole rounds of both legs took 60-110 longer
        (the stock leg's rounds run from 126.6 to 161.2 and from 153.4 to 182.2), a disturbance of the host's issue time,
        kept and reported as DESIGN 5.24 did for its like.
    The narrowest wins are the gate on its largest map at eight images (124.1 / 155.1 in float32, 121.2 / 151.7 in
    bfloat16); the heads win 1.8-5.5 x everywhere.  A row that misses in both runs becomes a class here, its thresholds
    halfway to the next measured row, as `native_train._inorm_backward_slower` draws them."""
    return False


class _TrainableHeads:
    """Mixin in front of a network class that has `NativeHeadsFOTSNet`: `_heads`, `_gate` and -- inside
    `native_train._TrainableMerge` -- `_train_gate` run `rroi_align.heads`'s autograd functions where a gradient is needed
    and `trainable_heads_ok` holds.  Everywhere else it is its parent."""

    def _heads(self, t):
        convs = (self.act, self.rbox, self.angle)
        if _tr._any_needs_grad((t,), (p for m in convs for p in m._parameters.values())) and trainable_heads_ok(self, t):
            return _heads_fn()._DetectionHeads.apply(t, *_nat._wb(self.act), *_nat._wb(self.rbox), *_nat._wb(self.angle), 128.0)
        return super()._heads(t)

    def _native_gate(self, t):
        """The gate at its source's size through the autograd function, or None where that is not to be."""
        if _tr._any_needs_grad((t,), self.conv_attenton._parameters.values()) and trainable_heads_ok(self, t, gate=True):
            return _heads_fn()._AttentionGate.apply(t, *_nat._wb(self.conv_attenton))
        return None

    def _gate(self, t, like):
        g = self._native_gate(t)
        return super()._gate(t, like) if g is None else self._up(g, like)

    def _train_gate(self, t):
        g = self._native_gate(t)
        return super()._train_gate(t) if g is None else g


# One class per network class of `native._NETS` and `native_train._NETS` that has the native heads: derived, not written.
_BASES = [c for c in list(_nat._NETS.values()) + list(_tr._NETS.values()) if issubclass(c, _nat.NativeHeadsFOTSNet)]
_BASES = list(dict.fromkeys(_BASES))
_TRAINABLE = [type("TrainableHeads" + c.__name__, (_TrainableHeads, c),
                   {"__doc__": f"A `{c.__name__}` whose heads and gates stay native in training.", "__module__": __name__})
              for c in _BASES]
globals().update({c.__name__: c for c in _TRAINABLE})
_NETS = _sw.feature_table(_TRAINABLE + _BASES, _nat._FEATURES + (_tr._TrainableMerge, _TrainableHeads))


def use_trainable_heads(net: nn.Module, enable: bool = True) -> bool:
    """Switch a network whose type is exactly one of the six classes with the native heads -- four of `fots_e2e.native`,
    two of `fots_e2e.native_train` -- to its trainable-heads subclass (enable=False: back): on after every other network
    switch, off before them (the module docstring).  Only the class of the network changes: no parameter is copied, no key
    of the state_dict moves.  A network of any other type is left alone.  Returns whether the class was switched."""
    return _sw.toggle_feature(net, _NETS, _TrainableHeads, enable)
