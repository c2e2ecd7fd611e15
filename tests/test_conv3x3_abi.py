"""CPU: the dense 3x3 convolution's entry points are exported, declared and host-checked; the plan query equals the mirrored
rule; the Python surface refuses CPU tensors, float32 and mismatched arguments; `conv3x3_ok` / `use_native_conv3x3` do what
fots_e2e.native says, in every order with `use_native_instancenorm`; the exact-integer fixture is exact on the CPU.  No
kernel is launched here."""
import ctypes
import itertools

import pytest
import torch
import torch.nn as nn

import conv3x3_cases as C
from test_abi import declared_functions
from test_depthwise_abi import fake_cuda

NAMES = ("rroi_conv3x3_forward_hip", "rroi_conv3x3_plan")
BF16, FP16 = 1, 2


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def test_symbols_are_exported_and_declared(ext):
    lib = ctypes.CDLL(ext.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions() and name in ext.EXPORTS and hasattr(lib, name), name
    assert not hasattr(lib, "rroi_conv3x3_forward_forced_hip")   # the measurement build's alone
    assert ext.version() == "rroi_align_hip 0.10.0 gfx950"      # the version string stays


def check_plan(ext, case, dtype):
    N, Cin, Cout, H, W, s = case
    tile_m, tile_h, k_chunks, grid = C.plan_of(case)
    Ho, Wo = C.out_size(H, W, s)
    p = ext.conv3x3_plan(N, Cin, Cout, H, W, s, dtype=dtype)
    assert (p.tile_m, p.tile_h, p.tile_w, p.k_chunk, p.k_chunks, p.grid_x, p.block, p.out_h, p.out_w) == \
        (tile_m, tile_h, 32, 16, k_chunks, grid, 256, Ho, Wo), case
    assert (p.m_tiles, p.y_tiles, p.x_tiles) == (-(-Cout // tile_m), -(-Ho // tile_h), -(-Wo // 32)), case
    assert p.grid_x == N * p.m_tiles * p.y_tiles * p.x_tiles
    in_h, in_w = (tile_h - 1) * s + 3, 31 * s + 3
    assert p.lds_bytes == (in_h * in_w + 9 * tile_m) * 16 * 2 <= 65536, case
    return tile_m, tile_h, s


def test_plan_query_equals_the_mirrored_rule_on_the_table_and_the_network(ext):
    seen = set()
    for case in C.CASES:
        for dtype in C.DTYPES:
            seen.add(check_plan(ext, case, dtype))
    assert seen == C.FORMS                                        # every form the table is meant to reach
    for n in (1, 8):
        for shape in C.NETWORK_SHAPES:
            check_plan(ext, (n,) + shape, torch.bfloat16)
    for n in (24, 192):
        for shape in C.RECOGNISER_SHAPES:
            check_plan(ext, (n,) + shape, torch.float16)
    assert C.plan_of((1, 64, 64, 352, 640, 1)) == (32, 4, 4, 2 * 88 * 20)
    assert C.plan_of((1, 3, 16, 704, 1280, 1)) == (32, 4, 1, 176 * 40)


BAD_DIMS = ((0, 4, 4, 8, 8), (1, 0, 4, 8, 8), (1, 4, 0, 8, 8), (1, 4, 4, 0, 8), (1, 4, 4, 8, 0), (-1, 4, 4, 8, 8), (1, 4, 4, 8, -3))
TOO_LARGE = ((1, 1 << 11, 4, 1 << 10, 1 << 10),          # x
             (1, 4, 1 << 11, 1 << 11, 1 << 11),          # y, at stride 2 as well (x is 2^24)
             (1, 1 << 14, 1 << 14, 1, 1),                # w: 2^28 * 9
             (0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff))


def test_refusals_return_zero_before_any_launch(ext):
    conv, plan = (getattr(ext._lib, n) for n in NAMES)
    P = 0x7f0000000000   # non-null, never dereferenced: every call below is refused on the host
    ok = (1, 4, 4, 8, 8)
    info = ext._ConvPlan()
    for dtype in (0, 3, -1):                                      # float32, an unknown dtype
        assert conv(dtype, P, P, P, *ok, 1, 1.0, None) == 0
        assert plan(dtype, *ok, 1, ctypes.byref(info)) == 0
    for dtype in (BF16, FP16):
        assert plan(dtype, *ok, 1, ctypes.byref(info)) == 1 and plan(dtype, *ok, 2, ctypes.byref(info)) == 1
        assert plan(dtype, *ok, 1, None) == 0
        for dims in BAD_DIMS + TOO_LARGE:
            for stride in (1, 2):
                assert conv(dtype, P, P, P, *dims, stride, 1.0, None) == 0, dims
                assert plan(dtype, *dims, stride, ctypes.byref(info)) == 0, dims
        for stride in (0, 3, -1, 4):
            assert conv(dtype, P, P, P, *ok, stride, 1.0, None) == 0
            assert plan(dtype, *ok, stride, ctypes.byref(info)) == 0
        for slope in (float("nan"), float("inf"), float("-inf")):
            assert conv(dtype, P, P, P, *ok, 1, slope, None) == 0
        assert conv(dtype, None, P, P, *ok, 1, 1.0, None) == 0
        assert conv(dtype, P, None, P, *ok, 2, 0.0, None) == 0
        assert conv(dtype, P, P, None, *ok, 1, 0.01, None) == 0
        assert conv(dtype, None, None, None, *ok, 1, 1.0, None) == 0


def test_python_surface_refuses_cpu_tensors_float32_and_mismatches(ext):
    x, w = torch.zeros(2, 3, 8, 8), torch.zeros(5, 3, 3, 3)
    for dtype in C.DTYPES:
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.conv3x3(x.to(dtype), w.to(dtype))
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.conv3x3(x.to(dtype), w.to(dtype), stride=2, negative_slope=0.0)
    with pytest.raises(TypeError):
        ext.conv3x3(fake_cuda(x), fake_cuda(w))                   # float32 keeps the stock path
    with pytest.raises(ValueError):
        ext.conv3x3_plan(1, 3, 5, 8, 8, 1, dtype=torch.float32)
    h = torch.bfloat16
    with pytest.raises(ValueError):
        ext.conv3x3(x.to(h), w.half())                            # dtypes differ
    with pytest.raises(ValueError):
        ext.conv3x3(x.to(h), torch.zeros(5, 4, 3, 3, dtype=h))    # channels differ
    with pytest.raises(ValueError):
        ext.conv3x3(x.to(h), torch.zeros(5, 3, 2, 3, dtype=h))    # not 3x3
    with pytest.raises(ValueError):
        ext.conv3x3(x.to(h)[0], w.to(h))                          # not 4-D
    with pytest.raises(ValueError):
        ext.conv3x3(x.to(h), w.to(h), stride=3)
    with pytest.raises(ValueError):
        ext.conv3x3(x.to(h), w.to(h), negative_slope=float("nan"))
    with pytest.raises(ValueError):
        ext.conv3x3(fake_cuda(torch.zeros(2, 3, 8, 16, dtype=h)[:, :, :, ::2]), fake_cuda(w.to(h)))   # a strided view
    with pytest.raises(ValueError):
        ext.conv3x3(fake_cuda(x.to(h)), fake_cuda(w.to(h)), out=fake_cuda(torch.zeros(2, 5, 8, 9, dtype=h)))


def qualifying(cin=4, cout=6, dtype=torch.bfloat16, **kw):
    args = dict(kernel_size=3, stride=1, padding=1, bias=False)
    args.update(kw)
    return nn.Conv2d(cin, cout, **args).to(dtype)


def test_conv3x3_ok_declines_each_disqualifying_property(monkeypatch):
    from fots_e2e.native import conv3x3_ok
    z = lambda *shape, dtype=torch.bfloat16: fake_cuda(torch.zeros(*shape, dtype=dtype))  # noqa: E731
    x = z(2, 4, 8, 8)
    with torch.no_grad():
        assert conv3x3_ok(qualifying(), x) and conv3x3_ok(qualifying(stride=2), x)
        assert conv3x3_ok(qualifying(dtype=torch.float16), z(2, 4, 8, 8, dtype=torch.float16))
        assert conv3x3_ok(qualifying(3, 16), z(1, 3, 5, 7)) and conv3x3_ok(qualifying(1, 1), z(1, 1, 1, 1))
        assert not conv3x3_ok(qualifying(), torch.zeros(2, 4, 8, 8, dtype=torch.bfloat16))           # a CPU tensor
        assert not conv3x3_ok(qualifying(dtype=torch.float32), z(2, 4, 8, 8, dtype=torch.float32))  # float32: stock
        assert not conv3x3_ok(qualifying(), z(2, 4, 8, 8, dtype=torch.float16))                     # not the weight's
        assert not conv3x3_ok(qualifying(), z(4, 8, 8))
        assert not conv3x3_ok(qualifying(), fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)))
        assert not conv3x3_ok(qualifying(), fake_cuda(torch.zeros(2, 4, 8, 16, dtype=torch.bfloat16)[:, :, :, ::2]))
        assert not conv3x3_ok(qualifying(), z(0, 4, 8, 8))
        assert not conv3x3_ok(qualifying(), z(2, 5, 8, 8))                                           # channels differ
        for kw in (dict(kernel_size=5, padding=2), dict(kernel_size=(2, 3), padding=(0, 1)), dict(padding=0),
                   dict(padding=2, dilation=2), dict(stride=3), dict(stride=(1, 2)), dict(groups=2), dict(bias=True),
                   dict(padding_mode="reflect"), dict(kernel_size=1, padding=0)):
            assert not conv3x3_ok(qualifying(**kw), x), kw
        # 2^31 elements of input, of output (views of one element: nothing that large is allocated)
        one = torch.zeros(1, dtype=torch.bfloat16)
        assert not conv3x3_ok(qualifying(1 << 11, 1), fake_cuda(one.expand(1, 1 << 11, 1 << 10, 1 << 10)))
        big_out = qualifying(1, 1)
        big_out.out_channels = 1 << 12
        xs = fake_cuda(torch.zeros(1, 1, 1 << 10, 1 << 9, dtype=torch.bfloat16))
        assert xs.numel() < (1 << 31) and not conv3x3_ok(big_out, xs)
    m = qualifying()
    assert m.weight.requires_grad and not conv3x3_ok(m, x)         # a gradient is needed
    with torch.no_grad():
        assert conv3x3_ok(m, x)
    m.weight.requires_grad_(False)
    assert conv3x3_ok(m, x)
    with monkeypatch.context() as mp:
        mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert not conv3x3_ok(m, x)
    xg = fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.bfloat16)).requires_grad_(True)
    assert not conv3x3_ok(m, xg)
    with torch.no_grad():
        assert conv3x3_ok(m, xg)


def network():
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    return deterministic_init(FOTSNet()).eval()


def test_use_native_conv3x3_switches_23_convolutions_and_2_activations_and_back():
    from fots_e2e.native import ConvAppliedReLU, DenseConv3x3, use_native_conv3x3, use_native_depthwise
    net = network()
    keys = list(net.state_dict().keys())
    ptrs = {k: p.data_ptr() for k, p in net.named_parameters()}
    classes = [type(m) for m in net.modules()]
    assert use_native_conv3x3(net) == (23, 2)
    names = sorted(n for n, m in net.named_modules() if type(m) is DenseConv3x3)
    assert len(names) == 23 and {"conv5", "conv6", "conv7", "conv8", "conv9", "layer0.0", "layer0.2", "layer0_1.0",
                                 "layer0_1.2"} <= set(names)
    assert sum(n.startswith("layer1.") for n in names) == 6 and sum(n.startswith("layer2.") for n in names) == 8
    assert type(net.conv10_s) is nn.Conv2d and type(net.conv11) is nn.Conv2d and type(net.feature1) is nn.Conv2d
    assert type(net.layer3[0].conv_sep1[0]) is nn.Conv2d                                         # depthwise: not ours
    assert [type(m) for m in net.layer0_1] == [DenseConv3x3, ConvAppliedReLU, DenseConv3x3, ConvAppliedReLU]
    assert net.layer0_1[0].fused_slope == 0.0 and net.layer0_1[2].fused_slope == 0.0 and net.conv5.fused_slope is None
    assert use_native_conv3x3(net) == (0, 0)                                                     # idempotent
    assert use_native_depthwise(net) == 22                                                       # the other conv switch
    assert list(net.state_dict().keys()) == keys and {k: p.data_ptr() for k, p in net.named_parameters()} == ptrs
    assert use_native_depthwise(net, False) == 22 and use_native_conv3x3(net, False) == (23, 2)
    assert [type(m) for m in net.modules()] == classes
    assert all("fused_slope" not in m.__dict__ for m in net.modules())
    assert use_native_conv3x3(net, fuse_activation=False) == (23, 0) and type(net.layer0_1[1]) is nn.ReLU
    assert use_native_conv3x3(net, False) == (23, 0)


def activations_applied_once(net):
    """Every (module, following activation) pair of an nn.Sequential applies its activation exactly once on the CPU path:
    either the module carries the slope and the activation is a pass-through, or neither."""
    from fots_e2e import native as nat
    passthrough = (nat.AbsorbedReLU, nat.AbsorbedLeakyReLU, nat.ConvAppliedReLU, nat.ConvAppliedLeakyReLU)
    for seq in net.modules():
        if not isinstance(seq, nn.Sequential):
            continue
        mods = list(seq._modules.values())
        for k, m in enumerate(mods):
            slope = getattr(m, "fused_slope", None)
            nxt = mods[k + 1] if k + 1 < len(mods) else None
            if slope is not None:
                owner = (nat.ConvAppliedReLU, nat.ConvAppliedLeakyReLU) if isinstance(m, nn.Conv2d) else \
                    (nat.AbsorbedReLU, nat.AbsorbedLeakyReLU)
                assert type(nxt) in owner and slope == float(getattr(nxt, "negative_slope", 0.0))
            elif type(nxt) in passthrough:
                raise AssertionError(f"{type(nxt).__name__} behind a module that applies nothing")
        if not any(getattr(m, "fused_slope", None) is not None for m in mods):
            assert not any(type(m) in passthrough for m in mods)


def test_conv_and_instancenorm_switches_compose_in_all_four_orders():
    from fots_e2e.native import use_native_conv3x3, use_native_instancenorm
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    net = network()
    classes = [type(m) for m in net.modules()]
    with torch.no_grad():
        want = net(x)
    on = {"conv": lambda: use_native_conv3x3(net), "norm": lambda: use_native_instancenorm(net)}
    off = {"conv": lambda: use_native_conv3x3(net, False), "norm": lambda: use_native_instancenorm(net, False)}
    for first, second in itertools.permutations(("conv", "norm")):
        for off_first, off_second in itertools.permutations(("conv", "norm")):
            assert on[first]() in ((23, 2), (52, 20)) and on[second]() in ((23, 2), (52, 20))
            activations_applied_once(net)
            assert off[off_first]() in ((23, 2), (52, 20))
            activations_applied_once(net)                          # the other switch's work is untouched
            with torch.no_grad():
                got = net(x)
            for p, q in zip(want, got):
                assert all(torch.equal(a, b) for a, b in zip(p, q)), (first, second, off_first)
            assert off[off_second]() in ((23, 2), (52, 20))
            assert [type(m) for m in net.modules()] == classes
            assert all("fused_slope" not in m.__dict__ for m in net.modules())


def test_cpu_forward_of_the_switched_network_keeps_every_bit():
    from fots_e2e.native import use_native_conv3x3
    net = network()
    g = torch.Generator().manual_seed(3)
    x, crops = torch.randn(1, 3, 64, 64, generator=g), torch.randn(2, 64, 11, 24, generator=g)
    with torch.no_grad():
        want, want_ocr = net(x), net.forward_ocr(crops)
        assert use_native_conv3x3(net) == (23, 2)
        got, got_ocr = net(x), net.forward_ocr(crops)              # everything falls back; the fused ReLUs are applied
        for dtype in C.DTYPES:                                     # ... in 16 bits on the CPU as well
            half = network().to(dtype)
            w16 = half(x.to(dtype))
            use_native_conv3x3(half)
            g16 = half(x.to(dtype))
            assert all(torch.equal(a, b) or (a.isnan() == b.isnan()).all() and torch.equal(a.nan_to_num(), b.nan_to_num())
                       for p, q in zip(w16, g16) for a, b in zip(p, q))
    for p, q in zip(want, got):
        assert all(torch.equal(a, b) for a, b in zip(p, q))
    assert torch.equal(want_ocr, got_ocr)
    assert float(got[3][1].min()) == 0.0                           # focr: layer0_1's ReLU was applied


def test_the_exact_integer_fixture_is_exact_in_fp32_accumulation():
    """x and w in {-1, 0, 1}, at most 28 live input channels per output channel: an fp32 convolution on the CPU, whatever
    its order, equals the float64 reference, and the result is representable in both 16-bit types."""
    for case in C.CASES[:10]:
        for dtype in C.DTYPES:
            x, w, ref = C.exact_problem(case, dtype)
            got = torch.nn.functional.conv2d(x.float(), w.float(), stride=case[5], padding=1)
            assert torch.equal(got.double(), ref) and torch.equal(got.to(dtype).double(), ref)
            assert float(ref.abs().max()) <= 252.0


def test_the_bound_holds_for_an_fp32_accumulating_cpu_convolution():
    for case in C.CASES[:10]:
        for dtype in C.DTYPES:
            x, w, ref, S = C.problem(case, dtype)
            y32 = torch.nn.functional.conv2d(x.float(), w.float(), stride=case[5], padding=1)
            for slope in C.SLOPES:
                got = torch.where(y32 < 0, y32 * slope, y32).to(dtype)
                want, lim = C.bound(ref, S, case[1], dtype, slope)
                ok, ratio = C.within(got, want, lim)
                assert ok and ratio <= 1.0, (case, dtype, slope, ratio)
