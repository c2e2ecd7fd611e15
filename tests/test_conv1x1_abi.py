"""CPU: the 1x1 convolution's entry points are exported, declared and host-checked; the plan query equals the mirrored rule;
the Python surface refuses CPU tensors, float32 and mismatched arguments; `conv1x1_ok` / `shortcut_ok` /
`use_native_conv1x1` do what fots_e2e.native says, in every order with the other seven switches; the exact-integer fixture
is exact and the two bounds hold for an fp32-accumulating emulation on the CPU.  No kernel is launched here."""
import ctypes
import itertools

import pytest
import torch
import torch.nn as nn

import conv1x1_cases as C
from test_abi import declared_functions
from test_depthwise_abi import fake_cuda

NAMES = ("rroi_conv1x1_forward_hip", "rroi_conv1x1_plan")
BF16, FP16 = 1, 2


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def test_symbols_are_exported_and_declared(ext):
    lib = ctypes.CDLL(ext.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions() and name in ext.EXPORTS and hasattr(lib, name), name
    assert not hasattr(lib, "rroi_conv1x1_forward_forced_hip")   # the measurement build's alone
    assert ext.version() == "rroi_align_hip 0.10.0 gfx950"      # the version string stays


def check_plan(ext, case, dtype):
    N, Cin, Cout, H, W, s = case
    tile_m, k_chunks, grid = C.plan_of(case)
    Ho, Wo = C.out_size(H, W, s)
    p = ext.conv1x1_plan(N, Cin, Cout, H, W, s, dtype=dtype)
    assert (p.tile_m, p.tile_p, p.k_chunk, p.k_chunks, p.grid_x, p.block, p.out_h, p.out_w) == \
        (tile_m, 128, 64, k_chunks, grid, 256, Ho, Wo), case
    assert (p.m_tiles, p.p_tiles) == (-(-Cout // tile_m), -(-(Ho * Wo) // 128)), case
    assert p.grid_x == N * p.m_tiles * p.p_tiles
    # 64 channel rows of 128 + 32 pixels, tile_m rows of 64 + 8 weights, two fp32 per channel row for the folded norm
    assert p.lds_bytes == 64 * 160 * 2 + tile_m * 72 * 2 + tile_m * 8 <= 65536, case
    return tile_m, s


def test_plan_query_equals_the_mirrored_rule_on_the_table_and_the_network(ext):
    seen = set()
    for case in C.CASES:
        for dtype in C.DTYPES:
            seen.add(check_plan(ext, case, dtype))
    assert seen == C.FORMS                                        # every form the table is meant to reach
    for n in (1, 8):
        for shape in C.NETWORK_SHAPES:
            check_plan(ext, (n,) + shape, torch.bfloat16)
            check_plan(ext, (n,) + shape, torch.float16)
    assert C.plan_of((1, 256, 256, 44, 80, 1)) == (32, 4, 8 * 28)
    assert C.plan_of((1, 512, 512, 22, 40, 1)) == (32, 8, 16 * 7)
    assert C.plan_of((1, 64, 256, 176, 320, 1)) == (64, 1, 4 * 440)
    assert C.plan_of((8, 512, 512, 22, 40, 1)) == (64, 8, 8 * 8 * 7)


BAD_DIMS = ((0, 4, 4, 8, 8), (1, 0, 4, 8, 8), (1, 4, 0, 8, 8), (1, 4, 4, 0, 8), (1, 4, 4, 8, 0), (-1, 4, 4, 8, 8), (1, 4, 4, 8, -3))
TOO_LARGE = ((1, 1 << 11, 4, 1 << 10, 1 << 10),          # x
             (1, 4, 1 << 11, 1 << 11, 1 << 11),          # y, at stride 2 as well (x is 2^24)
             (1, 1 << 16, 1 << 15, 1, 1),                # w
             (0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff))


def test_refusals_return_zero_before_any_launch(ext):
    conv, plan = (getattr(ext._lib, n) for n in NAMES)
    P = 0x7f0000000000   # non-null, never dereferenced: every call below is refused on the host
    ok = (1, 4, 4, 8, 8)
    none = (None, None, None, None, 0.0)
    full = (P, P, P, P, 1e-5)
    info = ext._Conv1x1Plan()
    for dtype in (0, 3, -1):                                      # float32, an unknown dtype
        assert conv(dtype, P, P, P, *ok, 1, 1.0, *none, None) == 0
        assert conv(dtype, P, P, P, *ok, 1, 1.0, *full, None) == 0
        assert plan(dtype, *ok, 1, ctypes.byref(info)) == 0
    for dtype in (BF16, FP16):
        assert plan(dtype, *ok, 1, ctypes.byref(info)) == 1 and plan(dtype, *ok, 2, ctypes.byref(info)) == 1
        assert plan(dtype, *ok, 1, None) == 0
        for dims in BAD_DIMS + TOO_LARGE:
            for stride in (1, 2):
                assert conv(dtype, P, P, P, *dims, stride, 1.0, *none, None) == 0, dims
                assert conv(dtype, P, P, P, *dims, stride, 1.0, *full, None) == 0, dims
                assert plan(dtype, *dims, stride, ctypes.byref(info)) == 0, dims
        for stride in (0, 3, -1, 4):
            assert conv(dtype, P, P, P, *ok, stride, 1.0, *none, None) == 0
            assert plan(dtype, *ok, stride, ctypes.byref(info)) == 0
        for slope in (float("nan"), float("inf"), float("-inf")):
            assert conv(dtype, P, P, P, *ok, 1, slope, *none, None) == 0
            assert conv(dtype, P, P, P, *ok, 1, slope, *full, None) == 0
        for eps in (float("nan"), float("inf"), float("-inf"), -1e-5):
            assert conv(dtype, P, P, P, *ok, 1, 1.0, P, P, P, P, eps, None) == 0
            assert conv(dtype, P, P, P, *ok, 1, 1.0, None, None, P, P, eps, None) == 0
        assert conv(dtype, P, P, P, *ok, 1, 1.0, P, None, P, P, 1e-5, None) == 0      # weight without bias
        assert conv(dtype, P, P, P, *ok, 1, 1.0, None, P, P, P, 1e-5, None) == 0      # bias without weight
        assert conv(dtype, P, P, P, *ok, 2, 1.0, P, P, None, P, 1e-5, None) == 0      # var without mean
        assert conv(dtype, P, P, P, *ok, 2, 1.0, P, P, P, None, 1e-5, None) == 0      # mean without var
        assert conv(dtype, P, P, P, *ok, 1, 1.0, None, None, None, P, 1e-5, None) == 0
        assert conv(dtype, P, P, P, *ok, 1, 1.0, None, None, P, None, 1e-5, None) == 0
        assert conv(dtype, P, P, P, *ok, 1, 1.0, P, P, None, None, 1e-5, None) == 0   # an affine pair without statistics
        assert conv(dtype, None, P, P, *ok, 1, 1.0, *none, None) == 0
        assert conv(dtype, P, None, P, *ok, 2, 0.0, *full, None) == 0
        assert conv(dtype, P, P, None, *ok, 1, 0.01, *none, None) == 0
        assert conv(dtype, None, None, None, *ok, 1, 1.0, *full, None) == 0


def test_python_surface_refuses_cpu_tensors_float32_and_mismatches(ext):
    x, w = torch.zeros(2, 3, 8, 8), torch.zeros(5, 3, 1, 1)
    for dtype in C.DTYPES:
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.conv1x1(x.to(dtype), w.to(dtype))
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.conv1x1(x.to(dtype), w.to(dtype).reshape(5, 3), stride=2, negative_slope=0.0)
        v = torch.zeros(5, dtype=dtype)
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.conv1x1(x.to(dtype), w.to(dtype), norm=(v, v, v, v, 1e-5))
    with pytest.raises(TypeError):
        ext.conv1x1(fake_cuda(x), fake_cuda(w))                   # float32 keeps the stock path
    with pytest.raises(ValueError):
        ext.conv1x1_plan(1, 3, 5, 8, 8, 1, dtype=torch.float32)
    h = torch.bfloat16
    v = torch.zeros(5, dtype=h)
    with pytest.raises(ValueError):
        ext.conv1x1(x.to(h), w.half())                            # dtypes differ
    with pytest.raises(ValueError):
        ext.conv1x1(x.to(h), torch.zeros(5, 4, 1, 1, dtype=h))    # channels differ
    with pytest.raises(ValueError):
        ext.conv1x1(x.to(h), torch.zeros(5, 3, 3, 3, dtype=h))    # not 1x1
    with pytest.raises(ValueError):
        ext.conv1x1(x.to(h), torch.zeros(5, 3, 1, dtype=h))       # neither (Cout, Cin, 1, 1) nor (Cout, Cin)
    with pytest.raises(ValueError):
        ext.conv1x1(x.to(h)[0], w.to(h))                          # not 4-D
    with pytest.raises(ValueError):
        ext.conv1x1(x.to(h), w.to(h), stride=3)
    with pytest.raises(ValueError):
        ext.conv1x1(x.to(h), w.to(h), negative_slope=float("nan"))
    with pytest.raises(ValueError):
        ext.conv1x1(x.to(h), w.to(h), norm=(v, None, v, v, 1e-5))                 # affine is all or nothing
    with pytest.raises(ValueError):
        ext.conv1x1(x.to(h), w.to(h), norm=(v, v, None, v, 1e-5))                 # no running mean
    with pytest.raises(ValueError):
        ext.conv1x1(x.to(h), w.to(h), norm=(v, v, v, torch.zeros(4, dtype=h), 1e-5))   # a vector of another length
    with pytest.raises(ValueError):
        ext.conv1x1(x.to(h), w.to(h), norm=(v, v, v, v.half(), 1e-5))             # ... of another dtype
    with pytest.raises(ValueError):
        ext.conv1x1(x.to(h), w.to(h), norm=(v, v, v, v, -1.0))
    with pytest.raises(ValueError):
        ext.conv1x1(x.to(h), w.to(h), norm=(v, v, v, v))
    with pytest.raises(ValueError):
        ext.conv1x1(fake_cuda(torch.zeros(2, 3, 8, 16, dtype=h)[:, :, :, ::2]), fake_cuda(w.to(h)))   # a strided view
    with pytest.raises(ValueError):
        ext.conv1x1(fake_cuda(x.to(h)), fake_cuda(w.to(h)), out=fake_cuda(torch.zeros(2, 5, 8, 9, dtype=h)))


def qualifying(cin=4, cout=6, dtype=torch.bfloat16, **kw):
    args = dict(kernel_size=1, stride=1, padding=0, bias=False)
    args.update(kw)
    return nn.Conv2d(cin, cout, **args).to(dtype)


def z(*shape, dtype=torch.bfloat16):
    return fake_cuda(torch.zeros(*shape, dtype=dtype))


def test_conv1x1_ok_declines_each_disqualifying_property(monkeypatch):
    from fots_e2e import native as nat
    conv1x1_ok = nat.conv1x1_ok
    x = z(2, 4, 8, 8)
    with torch.no_grad():
        assert conv1x1_ok(qualifying(), x) and conv1x1_ok(qualifying(stride=2), x)
        assert conv1x1_ok(qualifying(dtype=torch.float16), z(2, 4, 8, 8, dtype=torch.float16))
        assert conv1x1_ok(qualifying(3, 16), z(1, 3, 5, 7)) and conv1x1_ok(qualifying(1, 1), z(1, 1, 1, 1))
        assert not conv1x1_ok(qualifying(), torch.zeros(2, 4, 8, 8, dtype=torch.bfloat16))           # a CPU tensor
        assert not conv1x1_ok(qualifying(dtype=torch.float32), z(2, 4, 8, 8, dtype=torch.float32))  # float32: stock
        assert not conv1x1_ok(qualifying(), z(2, 4, 8, 8, dtype=torch.float16))                     # not the weight's
        assert not conv1x1_ok(qualifying(), z(4, 8, 8))
        assert not conv1x1_ok(qualifying(), fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)))
        assert not conv1x1_ok(qualifying(), fake_cuda(torch.zeros(2, 4, 8, 16, dtype=torch.bfloat16)[:, :, :, ::2]))
        assert not conv1x1_ok(qualifying(), z(0, 4, 8, 8))
        assert not conv1x1_ok(qualifying(), z(2, 5, 8, 8))                                           # channels differ
        for kw in (dict(kernel_size=3, padding=1), dict(kernel_size=(1, 3), padding=(0, 1)), dict(padding=1),
                   dict(stride=3), dict(stride=(1, 2)), dict(groups=2), dict(bias=True),
                   dict(padding=1, padding_mode="reflect")):
            assert not conv1x1_ok(qualifying(**kw), x), kw
        # 2^31 elements of input, of output (views of one element: nothing that large is allocated)
        one = torch.zeros(1, dtype=torch.bfloat16)
        assert not conv1x1_ok(qualifying(1 << 11, 1), fake_cuda(one.expand(1, 1 << 11, 1 << 10, 1 << 10)))
        big_out = qualifying(1, 1)
        big_out.out_channels = 1 << 12
        xs = fake_cuda(torch.zeros(1, 1, 1 << 10, 1 << 9, dtype=torch.bfloat16))
        assert xs.numel() < (1 << 31) and not conv1x1_ok(big_out, xs)
        with monkeypatch.context() as mp:                          # a shape class that measured slower is declined
            mp.setattr(nat, "_conv1x1_slower", lambda m, t: True)
            assert not conv1x1_ok(qualifying(), x)
    m = qualifying()
    assert m.weight.requires_grad and not conv1x1_ok(m, x)         # a gradient is needed
    with torch.no_grad():
        assert conv1x1_ok(m, x)
    m.weight.requires_grad_(False)
    assert conv1x1_ok(m, x)
    with monkeypatch.context() as mp:
        mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert not conv1x1_ok(m, x)
    xg = fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.bfloat16)).requires_grad_(True)
    assert not conv1x1_ok(m, xg)
    with torch.no_grad():
        assert conv1x1_ok(m, xg)


def shortcut(cin=4, cout=6, dtype=torch.bfloat16, stride=2, **bn):
    return nn.Sequential(qualifying(cin, cout, dtype, stride=stride), nn.BatchNorm2d(cout, **bn).to(dtype)).eval()


def test_shortcut_ok_declines_each_disqualifying_property(monkeypatch):
    from fots_e2e.native import shortcut_ok, use_native_conv1x1
    x = z(2, 4, 8, 8)
    with torch.no_grad():
        assert shortcut_ok(shortcut(), x) and shortcut_ok(shortcut(stride=1), x) and shortcut_ok(shortcut(affine=False), x)
        assert shortcut_ok(shortcut(dtype=torch.float16), z(2, 4, 8, 8, dtype=torch.float16))
        switched = shortcut()
        assert use_native_conv1x1(switched) == (1, 1) and shortcut_ok(switched, x)
        assert not shortcut_ok(shortcut(dtype=torch.float32), z(2, 4, 8, 8, dtype=torch.float32))     # float32: stock
        assert not shortcut_ok(shortcut(), fake_cuda(torch.zeros(2, 4, 8, 16, dtype=torch.bfloat16)[:, :, :, ::2]))
        assert not shortcut_ok(shortcut(), torch.zeros(2, 4, 8, 8, dtype=torch.bfloat16))             # a CPU tensor
        assert not shortcut_ok(shortcut().train(), x)                                                # batch statistics
        assert not shortcut_ok(shortcut(track_running_stats=False), x)                               # no running statistics
        half_norm = shortcut()
        half_norm[1].half()
        assert not shortcut_ok(half_norm, x)                                                         # the norm's dtype
        narrow = nn.Sequential(qualifying(4, 6), nn.BatchNorm2d(5).to(torch.bfloat16)).eval()
        assert not shortcut_ok(narrow, x)
        lopsided = shortcut()
        lopsided[1]._parameters["bias"] = None
        assert not shortcut_ok(lopsided, x)                                                          # affine: all or nothing
        assert not shortcut_ok(nn.Sequential(qualifying(4, 6, kernel_size=3, padding=1),
                                             nn.BatchNorm2d(6).to(torch.bfloat16)).eval(), x)
        assert not shortcut_ok(nn.Sequential(qualifying(4, 6), nn.InstanceNorm2d(6)).eval(), x)
        assert not shortcut_ok(nn.Sequential(qualifying(4, 6), nn.BatchNorm2d(6).to(torch.bfloat16), nn.ReLU()).eval(), x)
        with monkeypatch.context() as mp:
            mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
            assert not shortcut_ok(shortcut(), x)
    m = shortcut()
    assert not shortcut_ok(m, x)                                    # a gradient is needed
    m[0].weight.requires_grad_(False)
    assert not shortcut_ok(m, x)                                    # ... by the norm's parameters still
    for p in m[1].parameters():
        p.requires_grad_(False)
    assert shortcut_ok(m, x)
    assert not shortcut_ok(m, fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.bfloat16)).requires_grad_(True))


def network():
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    return deterministic_init(FOTSNet()).eval()


def test_use_native_conv1x1_switches_29_convolutions_and_3_shortcuts_and_back():
    from fots_e2e.native import NativeShortcut, PointwiseConv1x1, use_native_conv1x1
    net = network()
    keys = list(net.state_dict().keys())
    ptrs = {k: p.data_ptr() for k, p in net.named_parameters()}
    classes = [type(m) for m in net.modules()]
    assert use_native_conv1x1(net) == (29, 3)
    names = sorted(n for n, m in net.named_modules() if type(m) is PointwiseConv1x1)
    assert len(names) == 29 and {"feature1", "feature2", "feature3", "feature4", "upconv1.1", "upconv2.1",
                                 "layer2.0.downsample.0", "layer3.0.downsample.0", "layer4.0.downsample.0"} <= set(names)
    assert sum(n.startswith("layer3.") and "downsample" not in n for n in names) == 12
    assert sum(n.startswith("layer4.") and "downsample" not in n for n in names) == 8
    assert sorted(n for n, m in net.named_modules() if type(m) is NativeShortcut) == [
        "layer2.0.downsample", "layer3.0.downsample", "layer4.0.downsample"]
    for name in ("act", "rbox", "angle", "conv_attenton", "conv11", "conv10_s", "conv5"):      # a bias, or not 1x1: not ours
        assert type(getattr(net, name)) is nn.Conv2d, name
    assert type(net.layer3[0].conv_sep1[0]) is nn.Conv2d and type(net.upconv1) is nn.Sequential
    assert use_native_conv1x1(net) == (0, 0)                                                     # idempotent
    assert list(net.state_dict().keys()) == keys and {k: p.data_ptr() for k, p in net.named_parameters()} == ptrs
    assert use_native_conv1x1(net, False) == (29, 3)
    assert [type(m) for m in net.modules()] == classes
    assert use_native_conv1x1(net, False) == (0, 0)


def switches():
    from fots_e2e import native as nat
    return {"depthwise": (nat.use_native_depthwise, 22), "instancenorm": (nat.use_native_instancenorm, (52, 20)),
            "heads": (nat.use_native_heads, True), "merge": (nat.use_native_merge, True),
            "blocks": (nat.use_native_blocks, (2, 7, 10)), "conv3x3": (nat.use_native_conv3x3, (23, 2)),
            "recogniser": (nat.use_native_recogniser, True), "conv1x1": (nat.use_native_conv1x1, (29, 3))}


def test_all_eight_switches_compose_and_restore_exact_classes_in_every_order():
    """All eight switches on in one order and off in another: every on and every off reports its own full count whatever
    is already switched (exact-type tests: no switch takes or restores another's classes), the keys never move, and the
    classes come back exactly.  The new switch is placed at every position of the `on` order and of the `off` order
    around the fixed order of the other seven (8 x 8 orders), and all 24 x 24 orders of (conv1x1, depthwise, conv3x3,
    instancenorm) -- the module switches, which walk the same modules -- are run with the other four switches off; all
    40,320 x 40,320 orders would take hours."""
    table = switches()
    others = [k for k in table if k != "conv1x1"]
    net = network()
    keys = list(net.state_dict().keys())
    classes = [type(m) for m in net.modules()]
    net_class = type(net)

    def run(on, off):
        for name in on:
            fn, count = table[name]
            assert fn(net) == count, (name, on)
        assert list(net.state_dict().keys()) == keys
        for name in off:
            fn, count = table[name]
            assert fn(net, False) == count, (name, off)
        assert [type(m) for m in net.modules()] == classes and type(net) is net_class, (on, off)

    for i in range(8):
        for j in range(8):
            run(others[:i] + ["conv1x1"] + others[i:], others[:j] + ["conv1x1"] + others[j:])
    module_switches = ("conv1x1", "depthwise", "conv3x3", "instancenorm")
    for on in itertools.permutations(module_switches):
        for off in itertools.permutations(module_switches):
            run(on, off)
    assert all("fused_slope" not in m.__dict__ for m in net.modules())


def test_cpu_forward_of_the_switched_network_keeps_every_bit():
    from fots_e2e import native as nat
    net = network()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 3, 64, 64, generator=g)
    with torch.no_grad():
        want = net(x)
        assert nat.use_native_conv1x1(net) == (29, 3) and nat.use_native_blocks(net) == (2, 7, 10)
        got = net(x)                                               # everything falls back to the stock modules
    for p, q in zip(want, got):
        assert all(torch.equal(a, b) for a, b in zip(p, q))


def test_the_exact_integer_fixture_is_exact_in_fp32_accumulation():
    """x and w in {-1, 0, 1}: an fp32 convolution on the CPU, whatever its order, equals the float64 reference, and the
    result is representable in both 16-bit types."""
    for case in C.CASES:
        for dtype in C.DTYPES:
            x, w, ref = C.exact_problem(case, dtype)
            got = torch.nn.functional.conv2d(x.float(), w.float(), stride=case[5])
            assert torch.equal(got.double(), ref) and torch.equal(got.to(dtype).double(), ref)
            assert float(ref.abs().max()) <= 144.0


def test_both_bounds_hold_for_an_fp32_accumulating_cpu_emulation_on_the_whole_table():
    worst = {}
    for case in C.CASES:
        for dtype in C.DTYPES:
            x, w, ref, A = C.problem(case, dtype)
            for norm in (None, C.norm_of(case, dtype)):
                for slope in C.SLOPES:
                    got = C.emulate_fp32(x, w, case[5], slope, norm, dtype)
                    want, lim = C.bound(ref, A, case[1], dtype, slope, norm)
                    ok, ratio = C.within(got, want, lim)
                    assert ok and ratio <= 1.0, (case, dtype, slope, norm is not None, ratio)
                    key = (dtype, norm is not None)
                    worst[key] = max(worst.get(key, 0.0), ratio)
    print({f"{k[0]} norm={k[1]}": round(v, 4) for k, v in worst.items()})
    assert all(v > 0.25 for v in worst.values())                   # not vacuous: the emulation comes near both bounds
