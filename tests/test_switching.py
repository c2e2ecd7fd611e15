"""CPU: what the switches of fots_e2e.native / native_remainder / native_train share (fots_e2e._switching) -- a switch undone
out of order leaves the network's function alone, the network classes' table is the classes' own, and asking a predicate
loads no library.  No kernel is launched here."""
import itertools
import os
import subprocess
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(want, got):
    flat = lambda o: [o] if isinstance(o, torch.Tensor) else [t for p in o for t in flat(p)]  # noqa: E731
    return all(torch.equal(a, b) for a, b in zip(flat(want), flat(got), strict=True))


def check_undo_under_the_trainable_switch(net, x, norms, acts):
    from fots_e2e.native import use_native_instancenorm
    from fots_e2e.native_train import use_trainable_instancenorm
    stock = [type(m) for m in net.modules()]
    with torch.no_grad():
        want = net(x)
    assert use_native_instancenorm(net) == (norms, acts) and use_trainable_instancenorm(net) == norms
    switched = [type(m) for m in net.modules()]
    assert use_native_instancenorm(net, False) == (0, 0)              # nothing of its own left to restore: says so,
    assert [type(m) for m in net.modules()] == switched              # changes no class,
    with torch.no_grad():
        assert same_bits(want, net(x))                               # and every activation is still applied once
    assert use_trainable_instancenorm(net, False) == norms
    assert use_native_instancenorm(net, False) == (norms, acts)      # the same call, in the documented order
    assert [type(m) for m in net.modules()] == stock
    assert all("fused_slope" not in m.__dict__ for m in net.modules())
    with torch.no_grad():
        assert same_bits(want, net(x))


def test_instancenorm_undone_under_the_trainable_switch_leaves_the_function_alone():
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    g = torch.Generator().manual_seed(11)
    seq = nn.Sequential(nn.Conv2d(3, 4, 1), nn.InstanceNorm2d(4, affine=True), nn.LeakyReLU(0.5)).eval()
    check_undo_under_the_trainable_switch(seq, torch.randn(2, 3, 5, 7, generator=g), 1, 1)
    # 64 x 64 is the smallest input the stock network takes: at 32 x 32 layer4's planes have one element, which
    # nn.InstanceNorm2d refuses
    check_undo_under_the_trainable_switch(deterministic_init(FOTSNet()).eval(), torch.randn(1, 3, 64, 64, generator=g), 52, 20)


def test_conv3x3_and_instancenorm_release_their_own_activations_only():
    from fots_e2e import native as nat
    from fots_e2e.model import FOTSNet
    net = FOTSNet().eval()
    stock = [type(m) for m in net.modules()]
    passthrough = lambda classes: sum(type(m) in classes for m in net.modules())  # noqa: E731
    absorbed, applied = tuple(nat._ABSORBED.values()), tuple(nat._CONV_APPLIED.values())
    switches = {"conv": (nat.use_native_conv3x3, (23, 2)), "norm": (nat.use_native_instancenorm, (52, 20))}
    for first, second in itertools.permutations(switches):
        for name in (first, second):
            assert switches[name][0](net) == switches[name][1]
        assert (passthrough(applied), passthrough(absorbed)) == (2, 20)
        assert switches[first][0](net, False) == switches[first][1]      # undone while the other is on
        assert (passthrough(applied), passthrough(absorbed)) == ((0, 20) if first == "conv" else (2, 0))
        assert switches[second][0](net, False) == switches[second][1]
        assert [type(m) for m in net.modules()] == stock
        assert all("fused_slope" not in m.__dict__ for m in net.modules())


def test_network_class_tables_are_read_off_the_classes():
    from fots_e2e import native as nat
    from fots_e2e import native_train as T
    from fots_e2e.model import FOTSNet
    toggles = {nat.NativeHeadsFOTSNet: nat.use_native_heads, nat._NativeMerge: nat.use_native_merge,
               nat._NativeRecogniser: nat.use_native_recogniser}
    features = lambda c, of: frozenset(f for f in of if issubclass(c, f))  # noqa: E731
    assert set(toggles) == set(nat._FEATURES)
    family = list(nat._NETS.values())
    assert len(family) == len(set(family)) == 8 and FOTSNet in family
    assert {features(c, toggles) for c in family} == {frozenset(s) for k in range(4) for s in itertools.combinations(toggles, k)}
    net = FOTSNet()
    for cls in family:
        for feature, switch in toggles.items():
            net.__class__ = cls
            has = feature in features(cls, toggles)
            assert switch(net, has) is False and type(net) is cls                    # already what is asked for
            assert switch(net, not has) is True
            assert features(type(net), toggles) == features(cls, toggles) ^ {feature} and type(net) in family
            assert switch(net, has) is True and type(net) is cls                     # identity, not equality

    trainable = [c for c in T._NETS.values() if issubclass(c, T._TrainableMerge)]
    assert len(trainable) == len(set(trainable)) == 4 and len(T._NETS) == 8
    assert len({features(c, toggles) for c in trainable}) == 4
    for cls in trainable:
        base = cls.__bases__[1]
        assert cls.__bases__[0] is T._TrainableMerge and base in family and issubclass(base, nat._NativeMerge)
        net.__class__ = base
        assert T.use_trainable_merge(net, False) is False and type(net) is base
        assert T.use_trainable_merge(net) is True and type(net) is cls
        for switch in toggles.values():                                              # the other switches know their own types only
            assert switch(net) is False and switch(net, False) is False and type(net) is cls
        assert T.use_trainable_merge(net) is False
        assert T.use_trainable_merge(net, False) is True and type(net) is base
    for cls in family:                                                               # without the native merge: not its to switch
        if not issubclass(cls, nat._NativeMerge):
            net.__class__ = cls
            assert T.use_trainable_merge(net) is False and type(net) is cls

    class Mine(nat.NativeHeadsMergeFOTSNet):                                         # a subclass of the user's is left alone
        pass
    net.__class__ = Mine
    for switch in list(toggles.values()) + [T.use_trainable_merge]:
        assert switch(net) is False and switch(net, False) is False
    assert type(net) is Mine


ASK_EVERY_PREDICATE = """
import sys, torch, torch.nn as nn
from fots_e2e import native as nat, native_remainder as rm, native_train as T
from fots_e2e.model import FOTSNet
net = FOTSNet().eval()
x, like = torch.zeros(1, 256, 4, 4), torch.zeros(1, 256, 8, 8)
dw, norm = nn.Conv2d(256, 256, 3, padding=1, groups=256, bias=False), nn.InstanceNorm2d(256, affine=True)
with torch.no_grad():
    answers = [nat.native_ok(dw, x), nat.instancenorm_ok(norm, x), nat.fused_norm_ok(norm, x, residual=x),
               nat.fused_norm_ok(net.layer0[1].bn, torch.zeros(1, 16, 4, 4), mirror=True), nat.heads_ok(net, x),
               nat.heads_ok(net, x, gate=True), nat.merge_ok(x, like, torch.zeros(1, 1, 4, 4)), nat.merge_ok(x, like),
               nat.conv3x3_ok(net.conv5, torch.zeros(1, 64, 4, 4)), nat.act_pool_ok(x),
               nat.ocr_head_ok(net, torch.zeros(1, 256, 1, 4)),
               nat.conv1x1_ok(net.feature4, x), nat.shortcut_ok(net.layer2[0].downsample, torch.zeros(1, 64, 4, 4)),
               rm.conv2x3_ok(net.conv10_s, torch.zeros(1, 256, 2, 4)), rm.up_depthwise_ok(net.upconv1, x, like),
               T.trainable_norm_ok(norm, x), T.trainable_depthwise_ok(dw, x), T.trainable_merge_ok(x, like, None, True)]
assert len(answers) == 18 and not any(answers), answers
loaded = sorted(m for m in sys.modules if m == "rroi_align" or m.startswith("rroi_align."))
assert not loaded, loaded
for load, name in ((nat._ext, "rroi_align._ext.rroi_align"), (rm._rem, "rroi_align._ext.rroi_align.remainder"),
                   (T._norm, "rroi_align.norm"), (T._conv, "rroi_align.conv"), (T._merge_fn, "rroi_align.merge")):
    assert load() is sys.modules[name] and load() is load(), name
print("asked")
"""


def test_asking_every_predicate_loads_no_library():
    """In a fresh process: the three modules are imported and every predicate is asked with CPU tensors, and no module of
    rroi_align -- the ctypes binding, the autograd functions -- has been imported; each loader then returns its module."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "fots.pytorch_amd")] + sys.path))
    p = subprocess.run([sys.executable, "-c", ASK_EVERY_PREDICATE], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "asked", p.stderr[-2000:]
