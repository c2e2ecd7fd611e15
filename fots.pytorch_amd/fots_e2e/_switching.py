"""fots_e2e._switching -- what the switches of `native`, `native_remainder`, `native_train` and `native_train_heads`
share: the lazy loader of a library module, the class swap over a network's modules, the absorption of an activation into the module in front of it,
and the table that maps a set of features to the network class that has them.

How the switches compose and undo, said once.  Every switch changes classes only and tests exact types, so the switches
leave each other's classes alone and compose in any order, with two rules: a `use_trainable_*` switch goes on after the
`use_native_*` switch whose class it extends and comes off before it, and `use_trainable_merge` goes on after, and comes
off before, `use_native_heads` / `use_native_recogniser` as well; `native_train_heads.use_trainable_heads` goes on after
all of them and comes off first.  A switch undone out of that order finds no class of its
own, changes nothing and says so in what it returns; the network computes what it did before the call."""
import importlib

import torch.nn as nn


def lazy_module(name):
    """A function of no argument that imports the module `name` on its first call and returns it on every call: asking a
    predicate needs neither the library nor a GPU."""
    loaded = []

    def load():
        if not loaded:
            loaded.append(importlib.import_module(name))
        return loaded[0]
    return load


def swap_classes(net, pairs, enable=True, qualifies=None):
    """Give every module of `net` whose type is exactly the first class of one of the (stock, native) `pairs` the second
    (enable=False: the reverse); with enable, only a module for which `qualifies(module)` holds.  One walk of
    `net.modules()`.  Returns the number of modules switched, one count per pair."""
    counts = [0] * len(pairs)
    for m in net.modules():
        for k, (stock, native) in enumerate(pairs):
            src, dst = (stock, native) if enable else (native, stock)
            if type(m) is src:
                if not enable or qualifies is None or qualifies(m):
                    m.__class__ = dst
                    counts[k] += 1
                break
    return tuple(counts)


def _sequential_pairs(net):
    """Every (module, the module directly behind it) of every `nn.Sequential` of `net`."""
    for seq in net.modules():
        if isinstance(seq, nn.Sequential):
            mods = list(seq._modules.values())
            yield from zip(mods, mods[1:])


def absorb_activations(net, owner, passthrough) -> int:
    """Let every module of `net` whose type is exactly `owner`, and which an `nn.Sequential` follows directly with an
    activation of a type in `passthrough` ({stock activation: its pass-through subclass}), take that activation's slope as
    its `fused_slope`, the activation becoming the pass-through.  A pair is fused only where both modules occur once in
    `net`: a module that is also called from somewhere else keeps its meaning.  Returns the number of pairs fused."""
    uses = {}
    for m in net.modules():
        for child in m._modules.values():
            if child is not None:
                uses[id(child)] = uses.get(id(child), 0) + 1
    n = 0
    for front, act in _sequential_pairs(net):
        if (type(front) is owner and front.fused_slope is None and type(act) in passthrough
                and uses[id(front)] == 1 and uses[id(act)] == 1):
            front.fused_slope = float(getattr(act, "negative_slope", 0.0))
            act.__class__ = passthrough[type(act)]
            n += 1
    return n


def release_activations(net, owner, passthrough) -> int:
    """Undo `absorb_activations`: every pass-through activation directly behind a module whose type is exactly `owner` is
    its stock class again, and that module's `fused_slope` is gone.  An activation behind a module of any other type --
    a further-switched subclass of `owner` above all -- stays a pass-through and the slope stays with that module, so the
    pair keeps applying the activation once.  Returns the number of pairs released."""
    stock = {applied: act for act, applied in passthrough.items()}
    n = 0
    for front, act in _sequential_pairs(net):
        if type(front) is owner and type(act) in stock:
            front.__dict__.pop("fused_slope", None)
            act.__class__ = stock[type(act)]
            n += 1
    return n


def swap_absorbing(net, stock, owner, passthrough, enable=True, fuse_activation=True, qualifies=None):
    """`swap_classes` for the one pair (stock, owner), with `absorb_activations` behind it where `fuse_activation` asks
    for it, and `release_activations` in front of the swap back.  Returns (modules switched, activations switched)."""
    if enable:
        n, = swap_classes(net, ((stock, owner),), True, qualifies)
        return n, absorb_activations(net, owner, passthrough) if fuse_activation else 0
    acts = release_activations(net, owner, passthrough)
    return swap_classes(net, ((stock, owner),), False)[0], acts


def feature_table(classes, features):
    """{the set of `features` a class derives from: that class} over `classes`; two classes with one set are an error."""
    table = {}
    for c in classes:
        key = frozenset(f for f in features if issubclass(c, f))
        if key in table:
            raise TypeError(f"{c.__name__} and {table[key].__name__} have the same features")
        table[key] = c
    return table


def toggle_feature(net, table, feature, enable) -> bool:
    """Give a network whose type is exactly a class of `table` (a `feature_table`) the class of the table that differs
    from it by `feature` alone: with it (enable) or without it.  A network of any other type, or one that already is
    what is asked for, is left alone.  Returns whether the class was switched."""
    have = frozenset(f for f in frozenset().union(*table) if isinstance(net, f))
    if table.get(have) is not type(net) or (feature in have) == bool(enable):
        return False
    want = table.get(have ^ {feature})
    if want is None:
        return False
    net.__class__ = want
    return True
