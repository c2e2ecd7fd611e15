"""GPU (MI355X): the native detection heads and attention gate against the float64 reference of
heads_cases.py: the bound and the bit count of the contract over the whole table, special values, misaligned views with
the three outputs inside one guarded buffer, determinism, graph capture, the switched network on the tensors it really
sees, and one inference chain."""
import numpy as np
import pytest
import torch

import heads_cases as HC
from test_gpu_bucketed import NAN_PATTERN

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def cuda(params):
    return tuple(None if p is None else p.cuda() for p in params)


def same_bits(got, want):
    d, nan_ok = HC.differing(got.cpu(), want.cpu())
    return d == 0 and nan_ok


def run_both(ext, x, hp, gp):
    xg = x.cuda()
    return HC.cat(ext.heads(xg, *cuda(hp))), HC.cat((ext.gate(xg, *cuda(gp)),))


# ---------------------------------------------------------------- against the reference: conditions (a) and (b)
@pytest.mark.parametrize("dtype", HC.DTYPES, ids=HC.IDS)
def test_against_the_reference_over_the_whole_table(ext, dtype):
    """Every case, heads and gate: (a) every finite element within heads_cases.native_bound of the float64 value, NaN
    positions equal; (b) over the whole table at most 1 element in 10^4, of at least 10^6, differs in bits from the
    rounded reference."""
    total = differ = 0
    for shape in HC.CASES:
        x, hp, gp, (want_h, Rh), (want_g, Rg) = HC.problem(shape, dtype)
        V, S = HC.plan_of(*shape)
        p = ext.heads_plan(*shape, dtype=dtype)
        assert (p.vector_elems, p.channel_splits) == (V, S)
        got_h, got_g = run_both(ext, x, hp, gp)
        for name, got, want, R in (("heads", got_h, HC.cat(want_h), Rh), ("gate", got_g, HC.cat(want_g), Rg)):
            assert got.shape == want.shape and got.dtype == dtype
            d, nan_ok = HC.differing(got, want)
            ok, worst = HC.within(got, R.out64, HC.native_bound(R, dtype, S))
            print(f"{HC.case_id(shape)} {name} V={V} S={S}: {d} of {got.numel()} differ, worst error / bound {worst:.3f}")
            assert nan_ok, (shape, name)
            assert ok, (shape, name, worst)
            total += got.numel()
            differ += d
    print(f"{dtype}: {differ} of {total} elements differ in bits from the reference")
    assert total >= 10 ** 6 and differ * 10 ** 4 <= total, (differ, total)


def test_empty_batch_returns_without_a_call(ext):
    x, hp, gp = HC.random_problem((1, 4, 3, 3), torch.float32, 1)
    s, r, a = ext.heads(x[:0].cuda(), *cuda(hp))
    assert s.shape == (0, 1, 3, 3) and r.shape == (0, 4, 3, 3) and a.shape == (0, 2, 3, 3)
    assert ext.gate(x[:0].cuda(), *cuda(gp)).shape == (0, 1, 3, 3)


# ---------------------------------------------------------------- special values
@pytest.mark.parametrize("dtype", HC.DTYPES, ids=HC.IDS)
def test_non_finite_columns_poison_their_pixel_and_no_other(ext, dtype):
    """C = 64 on 65 pixels is S = 16 blocks of 4 channels.  A NaN, a +inf and a -inf in the first channel, the last
    channel and channels 3 | 4 (either side of a block boundary) of one pixel each: those pixels equal the reference
    (NaN positions and bits), every other pixel keeps the bits of the clean run.  A zero weight against an inf is NaN."""
    shape = (1, 64, 5, 13)
    assert HC.plan_of(*shape) == (1, 16)
    x, hp, gp = HC.random_problem(shape, dtype, seed=21)
    hp = list(hp)
    hp[2] = hp[2].clone()
    hp[2][0, 9] = 0.0                                             # rbox row 0 ignores channel 9 -- unless it holds an inf
    clean_h, clean_g = run_both(ext, x, hp, gp)
    assert bool(clean_h.isfinite().all())
    flat = x.view(1, 64, 65)
    poisoned = {3: (0, NAN), 10: (63, INF), 20: (3, -INF), 30: (4, NAN), 40: (0, -INF), 50: (63, NAN), 60: (4, INF), 64: (9, INF)}
    for pixel, (c, v) in poisoned.items():
        flat[0, c, pixel] = v
    got_h, got_g = run_both(ext, x, hp, gp)
    (want_h, Rh), (want_g, Rg) = HC.reference(x, hp), HC.reference(x, gp)
    touched = torch.zeros(65, dtype=torch.bool)
    touched[list(poisoned)] = True
    for got, clean, want, R in ((got_h, clean_h, HC.cat(want_h), Rh), (got_g, clean_g, HC.cat(want_g), Rg)):
        got, clean, want = (t.view(t.size(1), 65) for t in (got, clean, want))
        assert same_bits(got[:, ~touched], clean[:, ~touched])
        assert HC.differing(got, want)[1]
        assert HC.within(got.view(R.out64.shape), R.out64, HC.native_bound(R, dtype, 16))[0]
        for pixel, (c, v) in poisoned.items():
            if v != v:
                assert bool(got[:, pixel].isnan().all()), pixel
    rbox0 = got_h.view(7, 65)[1]
    assert bool(rbox0[64].isnan()) and not bool(got_h.view(7, 65)[2:5, 64].isnan().any())    # 0 * inf: that output alone


@pytest.mark.parametrize("dtype", HC.DTYPES, ids=HC.IDS)
def test_saturation_null_biases_and_the_vanishing_angle(ext, dtype):
    """z = +-40, +-100, +-800 through NULL biases: the scores saturate to 0 and 1 without a NaN, a subnormal fp32 score is
    kept.  A pixel whose column is zero has z = 0 everywhere: score 1/2, rbox 64, a_0 = a_1 = 0 -> NaN in both angle
    channels and nowhere else."""
    zs = [40.0, -40.0, 100.0, -100.0, 800.0, -800.0, 0.0, 1.0]
    x = torch.zeros(1, 2, 1, len(zs), dtype=dtype)
    x[0, 0, 0] = torch.tensor(zs)
    ones = lambda k: torch.tensor([[1.0, 0.0]] * k, dtype=dtype)  # noqa: E731
    hp, gp = (ones(1), None, ones(4), None, ones(2), None), (ones(1), None)
    got_h, got_g = run_both(ext, x, hp, gp)
    (want_h, Rh), (want_g, Rg) = HC.reference(x, hp), HC.reference(x, gp)
    want_h, want_g = HC.cat(want_h), HC.cat(want_g)
    assert HC.differing(got_h, want_h)[1] and HC.differing(got_g, want_g)[1]
    assert HC.within(got_h, Rh.out64, HC.native_bound(Rh, dtype, 1))[0] and HC.within(got_g, Rg.out64, HC.native_bound(Rg, dtype, 1))[0]
    g = got_h.view(7, len(zs)).double()
    assert not bool(g[:, [0, 1, 2, 3, 4, 5, 7]].isnan().any())
    assert g[0, 4] == 1.0 and g[0, 5] == 0.0 and g[1, 4] == 128.0 and g[0, 0] == 1.0 and got_g.view(-1)[5] == 0.0
    assert g[0, 6] == 0.5 and g[1, 6] == 64.0 and bool(g[5:7, 6].isnan().all()) and not bool(g[:5, 6].isnan().any())
    if dtype == torch.float32:                                    # sigmoid(-100) = 3.7e-44: subnormal, not flushed
        assert 0.0 < g[0, 3] < 2.0 ** -126 and same_bits(got_h.view(7, -1)[0, 3], want_h.view(7, -1)[0, 3])
        assert 0.0 < float(got_g.view(-1)[3]) < 2.0 ** -126
    else:                                                         # sigmoid(-40) = 4.2e-18: a normal bf16, below fp16's range
        assert (float(g[0, 1]) > 0.0) == (dtype == torch.bfloat16)
        assert same_bits(got_h.view(7, -1)[0, 1], want_h.view(7, -1)[0, 1])
    # fp32 subnormal INPUTS are not flushed either: x = 2^-140, w = 2^120 -> z = 2^-20, s = 1/2 + 2^-22
    if dtype == torch.float32:
        xs = torch.full((1, 1, 1, 3), 2.0 ** -140)
        w = torch.full((1, 1), 2.0 ** 120)
        got = ext.gate(xs.cuda(), w.cuda(), None).cpu()
        assert bool((got > 0.5).all()) and same_bits(got, HC.reference(xs, (w, None))[0][0])


# ---------------------------------------------------------------- addresses and guards
@pytest.mark.parametrize("shape", [(2, 255, 11, 23), (1, 4, 362, 363), (1, 5, 181, 183)], ids=HC.case_id)
@pytest.mark.parametrize("dtype", HC.DTYPES, ids=HC.IDS)
def test_views_and_guards(ext, dtype, shape):
    """x, the weights and the outputs 0 .. 3 elements past a 16-byte boundary, through the raw ABI; the three outputs are
    slices of ONE buffer with guards in front, between and behind.  Every output element is written, no guard byte is."""
    x, hp, gp, (want_h, Rh), (want_g, Rg) = HC.problem(shape, dtype)
    N, C, H, W = shape
    S = HC.plan_of(*shape)[1]
    itype = torch.int32 if dtype == torch.float32 else torch.int16
    n, px = x.numel(), N * H * W
    stream = torch.cuda.current_stream().cuda_stream
    lim_h, lim_g = HC.native_bound(Rh, dtype, S), HC.native_bound(Rg, dtype, S)
    first = None
    for ox, oy in ((0, 0), (1, 1), (2, 2), (3, 3), (1, 0), (0, 3), (2, 1)):
        xb = torch.zeros(n + 8, dtype=dtype, device="cuda")
        xv = xb[ox:ox + n]
        xv.copy_(x.reshape(-1))
        assert xv.data_ptr() == xb.data_ptr() + ox * x.element_size() and xb.data_ptr() % 16 == 0
        pb = torch.zeros(8 * C + 8 + 64, dtype=dtype, device="cuda")          # all parameters in one buffer, shifted by ox
        views, at = [], ox
        for p in tuple(hp) + tuple(gp):
            v = pb[at:at + p.numel()]
            v.copy_(p.reshape(-1))
            views.append(v)
            at += p.numel() + 1
        starts = [64 + oy, 64 + oy + px + 64, 64 + oy + px + 64 + 4 * px + 64 + (oy ^ 1)]
        sizes = [px, 4 * px, 2 * px]
        buf = torch.full((starts[2] + sizes[2] + 64,), NAN_PATTERN[dtype], dtype=itype, device="cuda")
        before = buf.clone()
        outs = [buf[s:s + m].view(dtype) for s, m in zip(starts, sizes)]
        st = ext._lib.rroi_heads_forward_hip(ext.dtype_code(dtype), xv.data_ptr(), *(v.data_ptr() for v in views[:6]),
                                             *(o.data_ptr() for o in outs), N, C, H, W, HC.RBOX_SCALE, stream)
        torch.cuda.synchronize()
        assert st == 1
        inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
        for s, m in zip(starts, sizes):
            inside[s:s + m] = True
        assert torch.equal(buf[~inside], before[~inside]), "a byte outside the outputs was written"
        assert not (buf[inside] == before[inside]).any(), "an output element was left unwritten"
        assert bool((xb[:ox] == 0).all()) and bool((xb[ox + n:] == 0).all()) and torch.equal(xv.cpu(), x.reshape(-1))
        got = torch.cat([o.cpu().view(N, k, H, W) for o, k in zip(outs, (1, 4, 2))], dim=1)
        assert HC.differing(got, HC.cat(want_h))[1] and HC.within(got, Rh.out64, lim_h)[0], (ox, oy)
        first = got if first is None else first
        assert same_bits(got, first), (ox, oy)                   # the order of the sums does not depend on an address
        # the gate, its output in the same guarded buffer
        gbuf = torch.full((64 + oy + px + 64,), NAN_PATTERN[dtype], dtype=itype, device="cuda")
        gbefore = gbuf.clone()
        y = gbuf[64 + oy:64 + oy + px].view(dtype)
        st = ext._lib.rroi_gate_forward_hip(ext.dtype_code(dtype), xv.data_ptr(), views[6].data_ptr(), views[7].data_ptr(),
                                            y.data_ptr(), N, C, H, W, stream)
        torch.cuda.synchronize()
        assert st == 1
        assert torch.equal(gbuf[:64 + oy], gbefore[:64 + oy]) and torch.equal(gbuf[64 + oy + px:], gbefore[64 + oy + px:])
        assert not (gbuf[64 + oy:64 + oy + px] == gbefore[64 + oy:64 + oy + px]).any()
        got = y.cpu().view(N, 1, H, W)
        assert HC.differing(got, HC.cat(want_g))[1] and HC.within(got, Rg.out64, lim_g)[0], (ox, oy)


# ---------------------------------------------------------------- determinism, streams, capture
@pytest.mark.parametrize("shape", [(3, 256, 16, 24), (1, 5, 181, 183)], ids=HC.case_id)
def test_two_calls_and_a_second_stream_give_identical_bits(ext, shape):
    for dtype in (torch.float32, torch.bfloat16):
        x, hp, gp, _, _ = HC.problem(shape, dtype)
        x, hp, gp = x.cuda(), cuda(hp), cuda(gp)
        first = HC.cat(ext.heads(x, *hp) + (ext.gate(x, *gp),))
        second = HC.cat(ext.heads(x, *hp) + (ext.gate(x, *gp),))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            third = ext.heads(x, *hp) + (ext.gate(x, *gp),)
        side.synchronize()
        assert same_bits(first, second) and same_bits(first, HC.cat(third))


@pytest.mark.parametrize("shape", [(3, 256, 16, 24), (1, 5, 181, 183)], ids=HC.case_id)
def test_graph_capture_reproduces_the_eager_bits(ext, shape):
    dtype = torch.bfloat16 if shape[0] == 3 else torch.float32
    x, hp, gp, _, _ = HC.problem(shape, dtype)
    x, hp, gp = x.cuda(), cuda(hp), cuda(gp)
    ext.heads(x, *hp), ext.gate(x, *gp)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):                # one stream, no branches
            outs = ext.heads(x, *hp) + (ext.gate(x, *gp),)
    x.copy_(HC.random_problem(shape, dtype, seed=77)[0])          # x changes in place
    for o in outs:
        o.fill_(NAN)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(HC.cat(outs), HC.cat(ext.heads(x, *hp) + (ext.gate(x, *gp),)))


# ---------------------------------------------------------------- in the network
def params_of(net, names):
    out = []
    for name in names:
        m = getattr(net, name)
        out += [m.weight.detach().cpu(), m.bias.detach().cpu()]
    return tuple(out)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=["fp32", "bf16"])
def test_the_switched_network_runs_the_kernel_on_its_own_tensors(ext, dtype, monkeypatch):
    """FOTSNet on a 64 x 96 image: 2 heads calls and 3 gate calls run the kernel; each native output is within (a) of the
    reference of its own input and within the stock bound of the stock method's output on the same tensor; a
    `requires_grad` input falls back; focr, which depends on neither, keeps its bits."""
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import NativeHeadsFOTSNet, heads_ok, use_native_heads
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet()).eval().cuda().to(dtype)
    image = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(7)).cuda().to(dtype)
    with torch.no_grad():
        stock = net(image)
    assert use_native_heads(net) and type(net) is NativeHeadsFOTSNet
    calls = {"heads": [], "gate": []}
    heads_run, gate_run = ext._heads_run, ext._gate_run

    def record(kind, run):
        def wrapped(t, *a):
            out = run(t, *a)
            calls[kind].append((t.detach(), out if isinstance(out, tuple) else (out,)))
            return out
        return wrapped
    monkeypatch.setattr(ext, "_heads_run", record("heads", heads_run))
    monkeypatch.setattr(ext, "_gate_run", record("gate", gate_run))
    with torch.no_grad():
        native = net(image)
    assert len(calls["heads"]) == 2 and len(calls["gate"]) == 3
    assert sorted(tuple(t.shape) for t, _ in calls["heads"]) == [(1, 256, 8, 12), (1, 256, 16, 24)]
    assert sorted(tuple(t.shape) for t, _ in calls["gate"]) == [(1, 256, 2, 3), (1, 256, 4, 6), (1, 256, 8, 12)]
    assert same_bits(native[3][1], stock[3][1])                   # focr
    for a, b in zip(stock, native):
        assert [s.shape for s in a] == [t.shape for t in b]
    for kind, names in (("heads", ("act", "rbox", "angle")), ("gate", ("conv_attenton",))):
        params = params_of(net, names)
        for t, outs in calls[kind]:
            with torch.no_grad():
                want = FOTSNet._heads(net, t) if kind == "heads" else (torch.sigmoid(net.conv_attenton(t)),)
            _, R = HC.reference(t.cpu(), params)
            got, want = HC.cat(outs), HC.cat(want)
            S = HC.plan_of(*t.shape)[1]
            ok, worst = HC.within(got, R.out64, HC.native_bound(R, dtype, S))
            assert ok and bool((got.isnan() == R.out64.isnan()).all()), (kind, tuple(t.shape), worst)
            lim = HC.stock_bound(R, dtype)
            check = R.out64.isfinite() & lim.isfinite() & ~want.isnan()
            if kind == "heads":
                assert bool((want.isnan() <= (R.out64.isnan() | HC.stock_may_vanish(R, dtype))).all())
            else:
                assert not bool(want.isnan().any())
            err = (got.double() - want.double()).abs()
            print(f"{kind} {tuple(t.shape)}: worst |native - stock| / stock bound {float((err[check] / lim[check]).max()):.3f}")
            assert bool((err[check] <= lim[check]).all()), (kind, tuple(t.shape))
    # a gradient is needed: the stock path
    n_heads, n_gate = len(calls["heads"]), len(calls["gate"])
    t = calls["heads"][0][0].clone().requires_grad_(True)
    assert not heads_ok(net, t) and not heads_ok(net, t, gate=True)
    s, r, a = net._heads(t)
    g = net._gate(t, t)
    assert s.requires_grad and g.requires_grad and (len(calls["heads"]), len(calls["gate"])) == (n_heads, n_gate)
    with torch.no_grad():
        assert heads_ok(net, t.detach())
    assert use_native_heads(net, False) and type(net) is FOTSNet


def test_one_inference_chain_gives_the_same_boxes_and_texts(ext):
    """`infer_image` on a small image with the synthetic detector's maps: the switched network (its gates and heads run
    the kernel inside the pass) returns the boxes and texts of the un-switched one."""
    from e2e_inputs import synthetic_detector_maps
    from fots_e2e.alphabet import ALPHABET
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import use_native_heads
    from fots_e2e.pipeline import infer_image
    from fots_e2e.weights import deterministic_init
    from rroi_align.decode import CTCLabelConverter
    dev = torch.device("cuda", 0)
    net = deterministic_init(FOTSNet(len(ALPHABET) + 1)).eval().to(dev)
    conv = CTCLabelConverter(ALPHABET)
    size = (256, 384)
    torch.manual_seed(4)
    im_data = torch.rand(1, 3, *size, device=dev) * 2 - 1
    maps = tuple(torch.from_numpy(a).to(dev) for a in synthetic_detector_maps(size[0], size[1], 6, seed=7))
    hook = lambda _x: maps  # noqa: E731
    with torch.no_grad():
        boxes0, texts0 = infer_image(net, conv, im_data, detector=hook)
        assert use_native_heads(net)
        boxes1, texts1 = infer_image(net, conv, im_data, detector=hook)
    assert len(boxes0) >= 3, "the synthetic detector maps must yield boxes"
    assert np.array_equal(np.asarray(boxes0), np.asarray(boxes1)) and list(texts0) == list(texts1)
