"""CPU: the heads and gate entry points are exported, declared and host-checked; the plan query equals the mirrored rule
and the table names every form; the Python surface refuses CPU tensors and mismatched arguments; `heads_ok` /
`use_native_heads` do what fots_e2e.native says; the stock chain lies inside the stock bound.  No kernel is launched here."""
import ctypes

import pytest
import torch
import torch.nn as nn

import heads_cases as HC
from test_abi import declared_functions
from test_depthwise_abi import fake_cuda

NAMES = ("rroi_heads_forward_hip", "rroi_gate_forward_hip", "rroi_heads_plan")


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def test_symbols_are_exported_and_declared(ext):
    lib = ctypes.CDLL(ext.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions() and name in ext.EXPORTS and hasattr(lib, name), name
    assert ext.version() == "rroi_align_hip 0.10.0 gfx950"      # the version string stays


BAD_DIMS = ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (-1, 4, 8, 8), (1, 4, 8, -3))
TOO_LARGE = ((1, 1 << 11, 1 << 10, 1 << 10), (1 << 16, 1 << 15, 1, 1), (2, 2, 1 << 15, 1 << 14),
             (0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff))


def test_refusals_return_zero_before_any_launch(ext):
    heads, gate, plan = (getattr(ext._lib, n) for n in NAMES)
    P = 0x7f0000000000   # non-null, never dereferenced: every call below is refused on the host
    ok = (1, 4, 8, 8)
    info = ext._HeadsPlan()
    for dtype in (3, -1):                                         # unknown dtype
        assert heads(dtype, *[P] * 10, *ok, 128.0, None) == 0
        assert gate(dtype, *[P] * 4, *ok, None) == 0
        assert plan(dtype, 7, *ok, ctypes.byref(info)) == 0
    for dtype in (0, 1, 2):
        for dims in BAD_DIMS + TOO_LARGE:                         # a dimension below 1, N * C * H * W >= 2^31
            assert heads(dtype, *[P] * 10, *dims, 128.0, None) == 0, dims
            assert gate(dtype, *[P] * 4, *dims, None) == 0, dims
            for outputs in (1, 7):
                assert plan(dtype, outputs, *dims, ctypes.byref(info)) == 0, dims
        for k in (0, 1, 3, 5, 7, 8, 9):                           # a NULL x, weight or output (biases may be NULL)
            args = [P] * 10
            args[k] = None
            assert heads(dtype, *args, *ok, 128.0, None) == 0, k
        for k in (0, 1, 3):
            args = [P] * 4
            args[k] = None
            assert gate(dtype, *args, *ok, None) == 0, k
        for scale in (float("nan"), float("inf"), float("-inf")):
            assert heads(dtype, *[P] * 10, *ok, scale, None) == 0
        for outputs in (0, 2, 4, 6, 8, -1):
            assert plan(dtype, outputs, *ok, ctypes.byref(info)) == 0
        assert plan(dtype, 7, *ok, None) == 0
        assert plan(dtype, 7, *ok, ctypes.byref(info)) == 1 and plan(dtype, 1, *ok, ctypes.byref(info)) == 1


def test_plan_query_equals_the_mirrored_rule_and_the_table_names_every_form(ext):
    seen = set()
    for shape in HC.CASES + ((1, 256, 176, 320), (1, 256, 88, 160), (8, 256, 176, 320), (8, 256, 88, 160)):
        N, C, H, W = shape
        V, S = HC.plan_of(*shape)
        for dtype in HC.DTYPES:
            for outputs in (HC.HEADS, HC.GATE):
                p = ext.heads_plan(*shape, outputs=outputs, dtype=dtype)
                tiles = -(-H * W // (64 * V))
                assert p == ext.HeadsPlan(V, S, tiles, N * tiles, 64 * S, (S - 1) * outputs * V * 64 * 8, -(-C // S)), shape
                assert (S - 1) * p.channel_block < C and p.lds_bytes <= 65536 and p.block <= 1024
        if shape in HC.CASES:
            seen.add((V, S))
    assert seen == set(HC.FORMS)
    assert HC.plan_of(1, 256, 176, 320) == (2, 8) and HC.plan_of(1, 256, 88, 160) == (1, 16)     # the network's maps, one image
    assert HC.plan_of(8, 256, 176, 320) == (2, 2) and HC.plan_of(8, 256, 88, 160) == (2, 8)     # and eight
    for dtype in HC.DTYPES:                                       # at least 10^6 outputs per dtype: heads 7 + gate 1 per pixel
        assert sum(N * H * W * 8 for N, _, H, W in HC.CASES) >= 10 ** 6
    with pytest.raises(ValueError):
        ext.heads_plan(1, 4, 8, 8, outputs=3)


def test_python_surface_refuses_cpu_tensors_and_mismatches(ext):
    x = torch.zeros(2, 3, 8, 8)
    ws, bs, wr, br, wa, ba = (torch.zeros(1, 3), torch.zeros(1), torch.zeros(4, 3, 1, 1), torch.zeros(4), torch.zeros(2, 3),
                              torch.zeros(2))
    for dtype in HC.DTYPES:
        c = lambda t: t.to(dtype)  # noqa: E731
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.heads(c(x), c(ws), c(bs), c(wr), c(br), c(wa), c(ba))
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.heads(c(x), c(ws), None, c(wr), None, c(wa), None)
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.gate(c(x), c(ws), c(bs))
    with pytest.raises(ValueError):
        ext.heads(x, ws.half(), bs, wr, br, wa, ba)                # dtypes differ
    with pytest.raises(ValueError):
        ext.heads(x.bfloat16(), ws, bs, wr, br, wa, ba)
    with pytest.raises(ValueError):
        ext.heads(x, ws, bs.double(), wr, br, wa, ba)
    with pytest.raises(ValueError):
        ext.heads(x, ws, bs, torch.zeros(4, 4), br, wa, ba)        # channels differ
    with pytest.raises(ValueError):
        ext.heads(x, ws, bs, wa, br, wa, ba)                       # rbox with two rows
    with pytest.raises(ValueError):
        ext.heads(x, ws, bs, wr, torch.zeros(3), wa, ba)           # bias length
    with pytest.raises(ValueError):
        ext.heads(x[0], ws, bs, wr, br, wa, ba)                    # not 4-D
    with pytest.raises(ValueError):
        ext.heads(x, ws, bs, wr, br, wa, ba, rbox_scale=float("inf"))
    with pytest.raises(ValueError):
        ext.gate(x, wa, bs)
    with pytest.raises(ValueError):
        ext.gate(x, ws, ba)
    with pytest.raises(ValueError):
        ext.gate(x, ws.half(), bs)


# ---------------------------------------------------------------- heads_ok, use_native_heads
@pytest.fixture(scope="module")
def net():
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    return deterministic_init(FOTSNet()).eval()


def test_heads_ok_declines_each_disqualifying_property(net, monkeypatch):
    from fots_e2e.native import heads_ok
    t = fake_cuda(torch.zeros(1, 256, 4, 6))
    with torch.no_grad():
        for gate in (False, True):
            assert heads_ok(net, t, gate=gate)
            assert not heads_ok(net, torch.zeros(1, 256, 4, 6), gate=gate)                               # a CPU tensor
            assert not heads_ok(net, fake_cuda(torch.zeros(256, 4, 6)), gate=gate)                       # not 4-D
            assert not heads_ok(net, fake_cuda(torch.zeros(1, 256, 4, 6).to(memory_format=torch.channels_last)), gate=gate)
            assert not heads_ok(net, fake_cuda(torch.zeros(1, 256, 4, 12)[:, :, :, ::2]), gate=gate)     # a strided view
            assert not heads_ok(net, fake_cuda(torch.zeros(1, 256, 4, 6, dtype=torch.float64)), gate=gate)
            assert not heads_ok(net, fake_cuda(torch.zeros(1, 256, 4, 6, dtype=torch.bfloat16)), gate=gate)   # not the weights'
            assert not heads_ok(net, fake_cuda(torch.zeros(1, 128, 4, 6)), gate=gate)                    # not the convolutions' channels
            assert not heads_ok(net, fake_cuda(torch.zeros(0, 256, 4, 6)), gate=gate)
            assert not heads_ok(net, fake_cuda(torch.zeros(1).expand(1, 256, 1 << 12, 1 << 11)), gate=gate)   # 2^31 elements
        # the modules: each of the three heads, and the gate's convolution, must be the plain 1x1 convolution
        for name, gate, other in (("act", False, nn.Conv2d(256, 1, 3, padding=1)), ("rbox", False, nn.Conv2d(256, 4, 1, stride=2)),
                                  ("angle", False, nn.Conv2d(256, 3, 1)), ("act", False, nn.Conv2d(256, 2, 1, groups=2)),
                                  ("rbox", False, nn.Conv2d(256, 4, 1).double()), ("angle", False, nn.Identity()),
                                  ("conv_attenton", True, nn.Conv2d(256, 2, 1)),
                                  ("conv_attenton", True, nn.Conv2d(256, 1, 1, dilation=2).bfloat16())):
            with monkeypatch.context() as mp:
                mp.setitem(net._modules, name, other)
                assert not heads_ok(net, t, gate=gate), (name, other)
                assert heads_ok(net, t, gate=not gate)             # the other call does not read this module
            assert heads_ok(net, t, gate=gate)
        with monkeypatch.context() as mp:                          # a convolution without a bias qualifies: NULL is +0.0
            mp.setitem(net._modules, "act", nn.Conv2d(256, 1, 1, bias=False))
            assert heads_ok(net, t)
        with monkeypatch.context() as mp:                          # under autocast the stock chain returns 16 bits: declined
            mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
            assert not heads_ok(net, t) and not heads_ok(net, t, gate=True)
    # a gradient is needed: of a weight (a fresh network's default), of the input
    assert net.act.weight.requires_grad and not heads_ok(net, t) and not heads_ok(net, t, gate=True)
    tg = fake_cuda(torch.zeros(1, 256, 4, 6)).requires_grad_(True)
    with torch.no_grad():
        assert heads_ok(net, tg)
    for p in net.parameters():
        p.requires_grad_(False)
    try:
        assert heads_ok(net, t) and not heads_ok(net, tg) and not heads_ok(net, tg, gate=True)
    finally:
        for p in net.parameters():
            p.requires_grad_(True)
    for dtype in (torch.bfloat16, torch.float16):
        from fots_e2e.model import FOTSNet
        half = FOTSNet().eval().to(dtype)
        with torch.no_grad():
            assert heads_ok(half, fake_cuda(torch.zeros(1, 256, 4, 6, dtype=dtype)))
            assert not heads_ok(half, t)


def test_use_native_heads_switches_the_class_once_and_back(net):
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import (NativeHeadsFOTSNet, use_native_depthwise, use_native_heads, use_native_instancenorm)
    keys = list(net.state_dict().keys())
    ptrs = {k: p.data_ptr() for k, p in net.named_parameters()}
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        before = net(x)
    assert use_native_heads(net) is True and type(net) is NativeHeadsFOTSNet
    assert use_native_heads(net) is False and type(net) is NativeHeadsFOTSNet          # once
    assert list(net.state_dict().keys()) == keys and {k: p.data_ptr() for k, p in net.named_parameters()} == ptrs
    assert isinstance(net, FOTSNet)
    with torch.no_grad():
        cpu = net(x)                                              # CPU tensors: the stock path, the same bits
    for a, b in zip(before, cpu):
        for s, t in zip(a, b):
            assert torch.equal(s, t, ) or bool((s.isnan() == t.isnan()).all() and torch.equal(s.nan_to_num(), t.nan_to_num()))
    # composes with the other two switches, in any order
    assert use_native_depthwise(net) == 22 and use_native_instancenorm(net) == (52, 20)
    assert use_native_heads(net, False) is True and type(net) is FOTSNet
    assert use_native_heads(net, False) is False
    assert use_native_heads(net) is True
    assert use_native_depthwise(net, False) == 22 and use_native_instancenorm(net, False) == (52, 20)
    assert use_native_heads(net, False) is True and type(net) is FOTSNet
    assert list(net.state_dict().keys()) == keys

    class Other(FOTSNet):
        pass
    other = Other()
    assert use_native_heads(other) is False and type(other) is Other                   # another type is left alone
    seq = nn.Sequential(nn.Conv2d(3, 3, 1))
    assert use_native_heads(seq) is False and type(seq) is nn.Sequential


def test_declined_calls_take_the_stock_path(net, monkeypatch):
    """A `requires_grad` input, autocast and a channels-last input: the switched network's `_heads` and `_gate` return
    what the stock methods return, and the kernel's fast paths are never entered."""
    from fots_e2e import native
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import use_native_heads

    class Refuse:
        def __getattr__(self, name):
            raise AssertionError(f"the native {name} was called")
    monkeypatch.setattr(native, "_ext", lambda: Refuse())
    g = torch.Generator().manual_seed(11)
    t = torch.randn(1, 256, 4, 6, generator=g)
    like = torch.zeros(1, 256, 8, 12)
    assert use_native_heads(net)
    try:
        with torch.no_grad():
            with pytest.raises(AssertionError, match="native _heads_run"):
                net._heads(fake_cuda(t))                           # qualifies: the kernel would run
            with pytest.raises(AssertionError, match="native _gate_run"):
                net._gate(fake_cuda(t), like)
            want = FOTSNet._heads(net, t), FOTSNet._gate(net, t, like)
            cl = fake_cuda(t.to(memory_format=torch.channels_last))
            got = net._heads(cl), net._gate(cl, like)
            assert all(torch.allclose(a, b, atol=1e-5, equal_nan=True) for a, b in zip(got[0], want[0]))
            assert torch.allclose(got[1], want[1], atol=1e-6)
            with monkeypatch.context() as mp:
                mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
                got = net._heads(fake_cuda(t)), net._gate(fake_cuda(t), like)
            assert all(torch.equal(a, b) for a, b in zip(got[0], want[0])) and torch.equal(got[1], want[1])
        tg = fake_cuda(t.clone()).requires_grad_(True)
        s, r, a = net._heads(tg)                                   # a gradient is needed: stock, and it flows
        assert s.requires_grad and all(torch.equal(p, q) for p, q in zip((s, r, a), want[0]))
        net._gate(tg, like).sum().backward()
        assert tg.grad is not None and net.conv_attenton.weight.grad is not None
    finally:
        net.zero_grad(set_to_none=True)
        assert use_native_heads(net, False)


# ---------------------------------------------------------------- the yardstick of the stock comparison
class StockChain(nn.Module):
    """The four convolutions `FOTSNet._heads` and `FOTSNet._gate` read, for any channel count."""

    def __init__(self, C, heads, gate, dtype):
        super().__init__()
        self.act, self.rbox, self.angle, self.conv_attenton = (nn.Conv2d(C, k, 1).to(dtype) for k in (1, 4, 2, 1))
        with torch.no_grad():
            for m, w, b in zip((self.act, self.rbox, self.angle), heads[0::2], heads[1::2]):
                m.weight.copy_(w.reshape(m.weight.shape))
                m.bias.copy_(b)
            self.conv_attenton.weight.copy_(gate[0].reshape(1, C, 1, 1))
            self.conv_attenton.bias.copy_(gate[1])


def stock_outputs(x, heads, gate):
    """`FOTSNet._heads` and the convolution + sigmoid of `FOTSNet._gate` with these parameters, on x's device."""
    from fots_e2e.model import FOTSNet
    chain = StockChain(x.size(1), heads, gate, x.dtype).to(x.device)
    with torch.no_grad():
        return FOTSNet._heads(chain, x), (torch.sigmoid(chain.conv_attenton(x)),)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
def test_stock_chain_lies_inside_the_stock_bound(dtype):
    """Over the table, on CPU tensors: every finite element of the stock chain is within heads_cases.stock_bound of the
    float64 reference, and NaNs only where the reference has them or the bound is not finite."""
    worst = 0.0
    for shape in HC.CASES:
        x, hp, gp, (_, Rh), (_, Rg) = HC.problem(shape, dtype)
        try:
            sh, sg = stock_outputs(x, hp, gp)
        except RuntimeError as e:                                  # a dtype torch's CPU kernels do not take
            assert dtype != torch.float32, e
            return
        for outs, R in ((sh, Rh), (sg, Rg)):
            got, lim = HC.cat(outs), HC.stock_bound(R, dtype)
            check = R.out64.isfinite() & lim.isfinite()
            if len(outs) == 3:                                     # a stock NaN: the reference's, or a vanished (a_0, a_1)
                vanish = HC.stock_may_vanish(R, dtype)
                assert bool((got.isnan() <= (R.out64.isnan() | vanish)).all()), shape
                check &= ~(vanish & got.isnan())
            err = (got.double() - R.out64).abs()
            assert bool((err[check] <= lim[check]).all()), (shape, float((err[check] / lim[check]).max()))
            worst = max(worst, float((err[check] / lim[check]).max()))
    print(f"{dtype}: worst stock error / stock bound {worst:.3f}")
