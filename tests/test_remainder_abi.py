"""CPU: the entry points of the (2,3) convolution and of the fused resize + depthwise 3x3 are
exported, declared and host-checked; the plan query equals the mirrored rule; the Python surface refuses CPU tensors; both
predicates are false on CPU tensors and decline each disqualifying property; the two switches count, restore and compose
with the eight of fots_e2e.native at every position; the conv2x3 bound and table are consistent under an fp32-accumulating
CPU convolution; the float64 restatement of the fused operator equals the composition of the two references.  No kernel is
launched here."""
import ctypes

import pytest
import torch
import torch.nn as nn

import conv2x3_cases as C
import network_cases as NC
import updw_cases as U
from test_abi import declared_functions
from test_depthwise_abi import fake_cuda

NAMES = ("rroi_conv2x3_forward_hip", "rroi_conv2x3_plan", "rroi_up_depthwise3x3_forward_hip")
FP32, BF16, FP16 = 0, 1, 2
P = 0x7f0000000000   # non-null, never dereferenced: every call it is passed to is refused on the host


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


@pytest.fixture(scope="module")
def rem():
    from rroi_align._ext.rroi_align import remainder
    return remainder


def test_symbols_are_exported_and_declared(ext, rem):
    lib = ctypes.CDLL(ext.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions() and name in ext.EXPORTS and hasattr(lib, name), name
    assert ext.version() == "rroi_align_hip 0.10.0 gfx950"      # the version string stays
    # the package's `_*_run` callables stay the closed list the network's ledger reads
    assert not any(k.startswith("_") and k.endswith("_run") for k in vars(rem))
    assert callable(rem.run_conv2x3) and callable(rem.run_up_depthwise3x3)


# ---------------------------------------------------------------- conv2x3: plan and refusals
def test_conv2x3_plan_query_equals_the_mirrored_rule(rem):
    for case in C.CASES + ((8, 256, 256, 2, 32), (192, 256, 256, 2, 128)):
        N, Cin, Cout, H, W = case
        for dtype in C.DTYPES:
            p = rem.conv2x3_plan(N, Cin, Cout, H, W, dtype=dtype)
            assert (p.k_chunks, p.items, p.grid_x) == C.plan_of(case), case
            assert (p.tile_m, p.tile_w, p.wave_items, p.k_chunk, p.block, p.out_h, p.out_w) == (32, 32, 4, 32, 256, H - 1, W)
            assert (p.m_tiles, p.x_tiles) == (-(-Cout // 32), -(-W // 32))
            assert p.lds_bytes == (4 * 2 * 34 + 6 * 32) * (32 + 8) * 2 <= 65536
    assert C.plan_of((24, 256, 256, 2, 64)) == (8, 48, 12 * 8)
    assert {C.plan_of(c)[1] % 4 for c in C.CASES} >= {0, 1, 2, 3}    # every fill of the last workgroup's four waves


BAD_DIMS = ((0, 4, 4, 8, 8), (1, 0, 4, 8, 8), (1, 4, 0, 8, 8), (1, 4, 4, 1, 8), (1, 4, 4, 0, 8), (1, 4, 4, 8, 0),
            (-1, 4, 4, 8, 8), (1, 4, 4, 8, -3))
TOO_LARGE = ((1, 1 << 11, 4, 1 << 10, 1 << 10),          # x
             (1, 4, 1 << 11, (1 << 10) + 1, 1 << 10),    # y: 2^11 channels of 2^10 x 2^10 (x is a little over 2^22)
             (1, 1 << 14, 1 << 15, 2, 1),                # w: 2^29 * 6
             (0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff))


def test_conv2x3_refusals_return_zero_before_any_launch(ext, rem):
    conv, plan = ext._lib.rroi_conv2x3_forward_hip, ext._lib.rroi_conv2x3_plan
    ok = (1, 4, 4, 8, 8)
    info = rem._Conv2x3Plan()
    for dtype in (FP32, 3, -1):                                   # float32, an unknown dtype
        assert conv(dtype, P, P, P, *ok, 1.0, None) == 0
        assert plan(dtype, *ok, ctypes.byref(info)) == 0
    for dtype in (BF16, FP16):
        assert plan(dtype, *ok, ctypes.byref(info)) == 1 and plan(dtype, 1, 4, 4, 2, 1, ctypes.byref(info)) == 1
        assert plan(dtype, *ok, None) == 0
        for dims in BAD_DIMS + TOO_LARGE:                         # H < 2 among them
            assert conv(dtype, P, P, P, *dims, 1.0, None) == 0, dims
            assert plan(dtype, *dims, ctypes.byref(info)) == 0, dims
        for slope in (float("nan"), float("inf"), float("-inf")):
            assert conv(dtype, P, P, P, *ok, slope, None) == 0
        assert conv(dtype, None, P, P, *ok, 1.0, None) == 0
        assert conv(dtype, P, None, P, *ok, 0.0, None) == 0
        assert conv(dtype, P, P, None, *ok, 0.01, None) == 0
    with pytest.raises(ValueError):
        rem.conv2x3_plan(1, 4, 4, 8, 8, dtype=torch.float32)
    with pytest.raises(ValueError):
        rem.conv2x3_plan(1, 4, 4, 1, 8)


def test_up_depthwise_refusals_return_zero_before_any_launch(ext):
    f = ext._lib.rroi_up_depthwise3x3_forward_hip
    ok = (1, 4, 5, 7, 10, 14)
    for dtype in (3, -1, 7):
        assert f(dtype, P, P, P, *ok, None) == 0
    for dtype in (FP32, BF16, FP16):
        for k in range(6):                                        # each dimension below 1
            for bad in (0, -2):
                dims = list(ok)
                dims[k] = bad
                assert f(dtype, P, P, P, *dims, None) == 0, dims
        assert f(dtype, P, P, P, 1, 1 << 11, 1 << 10, 1 << 10, 4, 4, None) == 0      # 2^31 elements in
        assert f(dtype, P, P, P, 1, 1 << 11, 4, 4, 1 << 10, 1 << 10, None) == 0      # ... out
        assert f(dtype, P, P, P, *([0x7fffffff] * 6), None) == 0
        assert f(dtype, None, P, P, *ok, None) == 0
        assert f(dtype, P, None, P, *ok, None) == 0
        assert f(dtype, P, P, None, *ok, None) == 0


# ---------------------------------------------------------------- the Python surface
def test_python_surface_refuses_cpu_tensors_float32_and_mismatches(rem):
    x, w = torch.zeros(2, 3, 4, 8), torch.zeros(5, 3, 2, 3)
    for dtype in C.DTYPES:
        with pytest.raises(RuntimeError, match="GPU only"):
            rem.conv2x3(x.to(dtype), w.to(dtype))
    with pytest.raises(TypeError):
        rem.conv2x3(fake_cuda(x), fake_cuda(w))                   # float32 keeps the stock path
    h = torch.bfloat16
    with pytest.raises(ValueError):
        rem.conv2x3(x.to(h), w.half())                            # dtypes differ
    with pytest.raises(ValueError):
        rem.conv2x3(x.to(h), torch.zeros(5, 4, 2, 3, dtype=h))    # channels differ
    with pytest.raises(ValueError):
        rem.conv2x3(x.to(h), torch.zeros(5, 3, 3, 3, dtype=h))    # not (2,3)
    with pytest.raises(ValueError):
        rem.conv2x3(fake_cuda(x.to(h)[:, :, :1]), fake_cuda(w.to(h)))   # one row
    with pytest.raises(ValueError):
        rem.conv2x3(x.to(h), w.to(h), negative_slope=float("inf"))
    with pytest.raises(ValueError):
        rem.conv2x3(fake_cuda(torch.zeros(2, 3, 4, 16, dtype=h)[:, :, :, ::2]), fake_cuda(w.to(h)))   # a strided view
    with pytest.raises(ValueError):
        rem.conv2x3(fake_cuda(x.to(h)), fake_cuda(w.to(h)), out=fake_cuda(torch.zeros(2, 5, 4, 8, dtype=h)))
    a, dw = torch.zeros(2, 3, 4, 8), torch.zeros(3, 1, 3, 3)
    for dtype in U.DTYPES:
        with pytest.raises(RuntimeError, match="GPU only"):
            rem.up_depthwise3x3(a.to(dtype), dw.to(dtype), (8, 16))
    with pytest.raises(ValueError):
        rem.up_depthwise3x3(a, dw.half(), (8, 16))
    with pytest.raises(ValueError):
        rem.up_depthwise3x3(a, torch.zeros(4, 1, 3, 3), (8, 16))
    with pytest.raises(ValueError):
        rem.up_depthwise3x3(a, dw, (0, 16))
    with pytest.raises(ValueError):
        rem.up_depthwise3x3(a, dw, 8)
    with pytest.raises(TypeError):
        rem.up_depthwise3x3(fake_cuda(a.double()), fake_cuda(dw.double()), (8, 16))


# ---------------------------------------------------------------- the predicates
def conv10(cin=4, cout=6, dtype=torch.bfloat16, **kw):
    args = dict(kernel_size=(2, 3), stride=1, padding=(0, 1), bias=False)
    args.update(kw)
    return nn.Conv2d(cin, cout, **args).to(dtype)


def test_conv2x3_ok_declines_each_disqualifying_property(monkeypatch):
    from fots_e2e.native_remainder import conv2x3_ok
    z = lambda *shape, dtype=torch.bfloat16: fake_cuda(torch.zeros(*shape, dtype=dtype))  # noqa: E731
    x = z(2, 4, 2, 8)
    with torch.no_grad():
        assert conv2x3_ok(conv10(), x) and conv2x3_ok(conv10(), z(1, 4, 5, 1))
        assert conv2x3_ok(conv10(dtype=torch.float16), z(2, 4, 2, 8, dtype=torch.float16))
        assert not conv2x3_ok(conv10(), torch.zeros(2, 4, 2, 8, dtype=torch.bfloat16))               # a CPU tensor
        assert not conv2x3_ok(conv10(dtype=torch.float32), z(2, 4, 2, 8, dtype=torch.float32))      # float32: stock
        assert not conv2x3_ok(conv10(), z(2, 4, 2, 8, dtype=torch.float16))                         # not the weight's
        assert not conv2x3_ok(conv10(), z(4, 2, 8)) and not conv2x3_ok(conv10(), z(2, 4, 1, 8))     # 3-D; one row
        assert not conv2x3_ok(conv10(), fake_cuda(torch.zeros(2, 4, 2, 16, dtype=torch.bfloat16)[:, :, :, ::2]))
        assert not conv2x3_ok(conv10(), z(0, 4, 2, 8)) and not conv2x3_ok(conv10(), z(2, 5, 2, 8))
        for kw in (dict(kernel_size=3, padding=1), dict(kernel_size=(3, 2), padding=(1, 0)), dict(padding=0),
                   dict(padding=(1, 1)), dict(dilation=(1, 2), padding=(0, 2)), dict(stride=2), dict(groups=2),
                   dict(bias=True), dict(padding_mode="reflect")):
            assert not conv2x3_ok(conv10(**kw), x), kw
        one = torch.zeros(1, dtype=torch.bfloat16)
        assert not conv2x3_ok(conv10(1 << 11, 1), fake_cuda(one.expand(1, 1 << 11, 1 << 10, 1 << 10)))
        big_out = conv10(1, 1)
        big_out.out_channels = 1 << 12
        xs = z(1, 1, (1 << 10) + 1, 1 << 9)
        assert xs.numel() < (1 << 31) and not conv2x3_ok(big_out, xs)      # 2^12 x 2^10 x 2^9 outputs
    m = conv10()
    assert m.weight.requires_grad and not conv2x3_ok(m, x)         # a gradient is needed
    with torch.no_grad():
        assert conv2x3_ok(m, x)
    with monkeypatch.context() as mp, torch.no_grad():
        mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert not conv2x3_ok(m, x)
    with monkeypatch.context() as mp, torch.no_grad():
        import fots_e2e.native_remainder as rm
        mp.setattr(rm, "_conv2x3_slower", lambda m, x: True)
        assert not conv2x3_ok(m, x)


def smooth(ch=4, dtype=torch.float32, **kw):
    args = dict(kernel_size=3, stride=1, padding=1, groups=ch, bias=False)
    args.update(kw)
    return nn.Sequential(nn.Conv2d(ch, ch, **args), nn.Conv2d(ch, ch, 1, bias=False)).to(dtype)


def test_up_depthwise_ok_declines_each_disqualifying_property(monkeypatch):
    import fots_e2e.native_remainder as rm
    z = lambda *shape, dtype=torch.float32: fake_cuda(torch.zeros(*shape, dtype=dtype))  # noqa: E731
    t, like = z(2, 4, 5, 7), z(2, 4, 10, 14)
    with torch.no_grad():
        for dtype in U.DTYPES:
            assert rm.up_depthwise_ok(smooth(dtype=dtype), z(2, 4, 5, 7, dtype=dtype), z(2, 9, 10, 14, dtype=dtype))
        assert rm.up_depthwise_ok(smooth(), t, torch.zeros(1, 1, 3, 3))                  # only like's size is used
        assert not rm.up_depthwise_ok(smooth(), torch.zeros(2, 4, 5, 7), like)           # a CPU tensor
        assert not rm.up_depthwise_ok(smooth(), z(4, 5, 7), like) and not rm.up_depthwise_ok(smooth(), t, z(10, 14))
        assert not rm.up_depthwise_ok(smooth(), z(2, 4, 5, 7, dtype=torch.float64), like)
        assert not rm.up_depthwise_ok(smooth(dtype=torch.float16), t, like)              # the weight's dtype differs
        assert not rm.up_depthwise_ok(smooth(), fake_cuda(torch.zeros(2, 4, 5, 14)[:, :, :, ::2]), like)
        assert not rm.up_depthwise_ok(smooth(), z(2, 5, 5, 7), like)                     # channels differ
        assert not rm.up_depthwise_ok(smooth(), z(0, 4, 5, 7), like)
        for kw in (dict(stride=2), dict(padding=0), dict(bias=True), dict(groups=2), dict(kernel_size=5, padding=2),
                   dict(padding_mode="reflect")):
            assert not rm.up_depthwise_ok(smooth(**kw), t, like), kw
        assert not rm.up_depthwise_ok(nn.Sequential(), t, like)
        one = torch.zeros(1)
        assert not rm.up_depthwise_ok(smooth(1 << 11), fake_cuda(one.expand(1, 1 << 11, 1 << 10, 1 << 10)), like)
        assert not rm.up_depthwise_ok(smooth(), t, fake_cuda(one.expand(1, 1, 1 << 15, 1 << 15)))    # 2^31 elements out
    s = smooth()
    assert not rm.up_depthwise_ok(s, t, like)                      # a gradient is needed
    with monkeypatch.context() as mp, torch.no_grad():
        assert rm.up_depthwise_ok(s, t, like)
        mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert not rm.up_depthwise_ok(s, t, like)
    with monkeypatch.context() as mp, torch.no_grad():
        mp.setattr(rm, "_up_depthwise_slower", lambda *a: True)
        assert not rm.up_depthwise_ok(s, t, like)


def test_both_predicates_are_false_on_the_cpu_so_a_switched_network_keeps_every_bit():
    import fots_e2e.native_remainder as rm
    from fots_e2e import native as nat
    net = NC.network()
    g = torch.Generator().manual_seed(3)
    x, crops = torch.randn(1, 3, 64, 64, generator=g), torch.randn(2, 64, 11, 24, generator=g)
    with torch.no_grad():
        want, want_ocr = net(x), net.forward_ocr(crops)
        assert nat.use_native_merge(net) and rm.use_native_conv2x3(net) == 1 and rm.use_native_upconv(net) == 2
        assert not rm.conv2x3_ok(net.conv10_s, torch.zeros(2, 256, 2, 24))
        assert not rm.up_depthwise_ok(net.upconv1, torch.zeros(1, 256, 4, 4), torch.zeros(1, 256, 8, 8))
        got, got_ocr = net(x), net.forward_ocr(crops)              # forward_resized falls back to the stock expression
    assert all(torch.equal(a, b) for p, q in zip(want, got) for a, b in zip(p, q)) and torch.equal(want_ocr, got_ocr)


# ---------------------------------------------------------------- the switches
def test_the_two_switches_count_restore_and_move_no_key():
    import fots_e2e.native_remainder as rm
    net = NC.network()
    keys = list(net.state_dict().keys())
    ptrs = {k: p.data_ptr() for k, p in net.named_parameters()}
    classes = [type(m) for m in net.modules()]
    assert rm.use_native_conv2x3(net) == 1 and type(net.conv10_s) is rm.DenseConv2x3
    assert rm.use_native_upconv(net) == 2 and type(net.upconv1) is type(net.upconv2) is rm.UpSmooth
    assert [type(m) for m in net.upconv1] == [nn.Conv2d, nn.Conv2d]                      # the halves keep their classes
    assert sum(type(m) is not c for m, c in zip(net.modules(), classes)) == 3
    assert rm.use_native_conv2x3(net) == 0 and rm.use_native_upconv(net) == 0            # idempotent
    assert list(net.state_dict().keys()) == keys and {k: p.data_ptr() for k, p in net.named_parameters()} == ptrs
    assert rm.use_native_upconv(net, False) == 2 and rm.use_native_conv2x3(net, False) == 1
    assert [type(m) for m in net.modules()] == classes
    assert rm.use_native_upconv(net, False) == 0 and rm.use_native_conv2x3(net, False) == 0


def test_the_two_switches_compose_with_the_eight_at_every_position():
    """`all_eight` asserts each of the eight switches' full count: run before, between and after the two new ones, on and
    off, the counts are unchanged -- the new switches change the class of no depthwise, dense 3x3 or 1x1 convolution and
    of no shortcut, and the eight leave the new classes alone."""
    import fots_e2e.native_remainder as rm
    from fots_e2e.model import FOTSNet
    stock_classes = [type(m) for m in NC.network().modules()]
    two = (("conv2x3", rm.use_native_conv2x3, 1), ("upconv", rm.use_native_upconv, 2))
    eight_classes = None
    for position in range(3):                                      # the eight before, between, after the two
        for first, second in (two, two[::-1]):
            net = NC.network()
            steps = [first, second]
            steps.insert(position, None)
            for step in steps:
                if step is None:
                    NC.all_eight(net)
                else:
                    assert step[1](net) == step[2], (position, step[0])
            keys = list(NC.network().state_dict().keys())
            assert list(net.state_dict().keys()) == keys
            assert type(net.conv10_s) is rm.DenseConv2x3 and type(net.upconv1) is type(net.upconv2) is rm.UpSmooth
            assert hasattr(net.upconv1, "forward_resized") and hasattr(type(net), "_smoothed")
            # off, in the same interleaving
            for step in steps:
                if step is None:
                    NC.all_eight(net, NC.ORDER[::-1], enable=False)
                else:
                    assert step[1](net, False) == step[2], (position, step[0])
            assert type(net) is FOTSNet and [type(m) for m in net.modules()] == stock_classes
    # with the two on, the eight still switch exactly what they switch without them
    a, b = NC.all_eight(NC.network()), NC.network()
    rm.use_native_conv2x3(b), rm.use_native_upconv(b)
    NC.all_eight(b)
    eight_classes = [type(m) for m in a.modules()]
    differ = [(x, y) for x, y in zip(eight_classes, (type(m) for m in b.modules())) if x is not y]
    assert sorted(y.__name__ for _, y in differ) == ["DenseConv2x3", "UpSmooth", "UpSmooth"]


# ---------------------------------------------------------------- the bound, the table and the references agree
def test_the_conv2x3_bound_holds_for_an_fp32_accumulating_cpu_convolution():
    worst = 0.0
    for case in C.CASES:
        for dtype in C.DTYPES:
            x, w, ref, S = C.problem(case, dtype)
            y32 = torch.nn.functional.conv2d(x.float(), w.float(), padding=(0, 1))
            assert y32.shape == ref.shape == (case[0], case[2], case[3] - 1, case[4])
            for slope in C.SLOPES:
                got = torch.where(y32 < 0, y32 * slope, y32).to(dtype)
                want, lim = C.bound(ref, S, case[1], dtype, slope)
                ok, ratio = C.within(got, want, lim)
                assert ok and ratio <= 1.0, (case, dtype, slope, ratio)
                worst = max(worst, ratio)
    print(f"worst error / bound of the CPU emulation: {worst:.4f}")


def test_the_exact_integer_fixture_is_exact_in_fp32_accumulation():
    for case in C.CASES:
        for dtype in C.DTYPES:
            x, w, ref = C.exact_problem(case, dtype)
            got = torch.nn.functional.conv2d(x.float(), w.float(), padding=(0, 1))
            assert torch.equal(got.double(), ref) and torch.equal(got.to(dtype).double(), ref)
            assert float(ref.abs().max()) <= 252.0


def test_the_float64_restatement_equals_the_depthwise_oracle_on_the_rounded_resize():
    assert {U.band_of_case(c) for c in U.CASES} == U.BANDS_REACHED
    assert len(U.SMALL) == len(U.CASES) - 2
    for case in U.SMALL:
        for dtype in U.DTYPES:
            a, w, want = U.problem(case, dtype)
            assert want.shape == case[0][:2] + case[1] and want.dtype == dtype
            wrong, nan_ok = U.differing(U.restated(a, w, case[1]), want)
            assert wrong == 0 and nan_ok, (case, dtype, wrong)
