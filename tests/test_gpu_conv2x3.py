"""GPU (MI355X): the native (2,3) convolution against the float64 reference and the derived bound of
conv2x3_cases.py over the whole table for three slopes, the exact-integer table bit for bit, non-finite inputs, misaligned
views inside a guarded buffer, repeatability, graph capture, and `DenseConv2x3` on the network's own shape.

Worst |y - act(ref)| / bound observed over the table on an MI355X: bf16 0.9927, fp16 0.9839 (profiles/native_remainder.md);
the bound is dominated by the one rounding to the type, which reaches it at the bottom of a binade."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv2x3_cases as C
from test_gpu_bucketed import NAN_PATTERN

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def rem():
    from rroi_align._ext.rroi_align import remainder
    return remainder


def same_bits(got, want):
    got, want = got.cpu(), want.cpu()
    both_nan = got.isnan() & want.isnan()
    return got.shape == want.shape and bool(((C.bits(got) == C.bits(want)) | both_nan).all())


# ---------------------------------------------------------------- against the reference
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_the_whole_table_meets_the_bound_and_the_integer_table_every_bit(rem, dtype):
    worst = 0.0
    for case in C.CASES:
        N, Cin, Cout, H, W = case
        x, w, ref, S = C.problem(case, dtype)
        p = rem.conv2x3_plan(N, Cin, Cout, H, W, dtype=dtype)
        assert (p.k_chunks, p.items, p.grid_x) == C.plan_of(case)
        xg, wg = x.cuda(), w.cuda()
        for slope in C.SLOPES:
            got = rem.conv2x3(xg, wg, slope)
            assert got.shape == ref.shape and got.dtype == dtype and got.is_contiguous()
            got = got.cpu()
            want, lim = C.bound(ref, S, Cin, dtype, slope)
            ok, ratio = C.within(got, want, lim)
            print(f"{C.case_id(case)} slope={slope} items={p.items} grid={p.grid_x}: worst error / bound {ratio:.3f}")
            assert bool(got.isfinite().all()) and ok and ratio <= 1.0, (case, slope, ratio)
            worst = max(worst, ratio)
        xe, we, refe = C.exact_problem(case, dtype)
        for slope in (1.0, 0.0):
            got = rem.conv2x3(xe.cuda(), we.cuda(), slope).cpu()
            want = C.act64(refe, slope).to(dtype)                  # integers of magnitude <= 252: exact in the type
            assert torch.equal(want.double(), C.act64(refe, slope))
            wrong = int((got.double() != want.double()).sum())     # (-0.0 of a ReLU equals 0.0)
            assert wrong == 0, (case, slope, wrong)
    print(f"worst error / bound over the table: {worst:.4f}")


# ---------------------------------------------------------------- special values
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_non_finite_inputs_poison_their_windows_and_no_other(rem, dtype):
    case = (2, 17, 48, 4, 37)
    x, w = C.random_problem(case, dtype, seed=11)
    w = torch.where(w == 0, torch.ones_like(w), w)                 # no zero weight: every window that holds one is poisoned
    clean = rem.conv2x3(x.cuda(), w.cuda(), 0.01).cpu()
    bad = x.clone()
    spots = ((0, 3, 0, 0, NAN), (0, 16, 2, 20, INF), (1, 0, 3, 36, -INF), (1, 9, 1, 32, NAN))
    for n, c, i, j, v in spots:
        bad[n, c, i, j] = v
    got = rem.conv2x3(bad.cuda(), w.cuda(), 0.01).cpu()
    hit = torch.zeros_like(bad, dtype=torch.float32)
    for n, c, i, j, _ in spots:
        hit[n, :, i, j] = 1.0
    poisoned = F.conv2d(hit, torch.ones(48, 17, 2, 3), padding=(0, 1)) > 0
    assert poisoned.any() and not poisoned.all()
    assert torch.equal(~got.isfinite(), poisoned)
    ref = C.act64(C.reference(bad, w)[0], 0.01)
    assert torch.equal(got.isnan(), ref.isnan())
    inf_at = got.isinf()
    assert torch.equal(got[inf_at].double(), ref[inf_at])
    assert torch.equal(C.bits(got)[~poisoned], C.bits(clean)[~poisoned])


# ---------------------------------------------------------------- addresses and guards
@pytest.mark.parametrize("case", [(2, 5, 7, 3, 35), (3, 17, 33, 2, 66)], ids=C.case_id)
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_views_and_guards(rem, dtype, case):
    """x, w and y 0 .. 7 elements past a 16-byte boundary, through the raw ABI; y inside a guarded buffer.  Every output
    element is written, no guard byte is, the inputs are unchanged and the bits do not depend on an address."""
    from rroi_align._ext import rroi_align as ext
    N, Cin, Cout, H, W = case
    x, w = C.random_problem(case, dtype, seed=sum(case))
    n = N * Cout * (H - 1) * W
    stream = torch.cuda.current_stream().cuda_stream
    want = rem.conv2x3(x.cuda(), w.cuda(), 0.01)

    def shifted(t, off):
        buf = torch.zeros(t.numel() + 16, dtype=dtype, device="cuda")
        view = buf[off:off + t.numel()]
        view.copy_(t.reshape(-1))
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + off * t.element_size()
        return buf, view

    for ox, ow, oy in ((0, 0, 0), (1, 1, 1), (3, 2, 5), (7, 5, 2), (4, 3, 7), (2, 7, 6)):
        (xb, xv), (wb, wv) = shifted(x, ox), shifted(w, ow)
        buf = torch.full((64 + oy + n + 64,), NAN_PATTERN[dtype], dtype=torch.int16, device="cuda")
        before = buf.clone()
        y = buf[64 + oy:64 + oy + n].view(dtype)
        st = ext._lib.rroi_conv2x3_forward_hip(ext.dtype_code(dtype), xv.data_ptr(), wv.data_ptr(), y.data_ptr(), N, Cin, Cout,
                                               H, W, 0.01, stream)
        torch.cuda.synchronize()
        assert st == 1
        assert torch.equal(buf[:64 + oy], before[:64 + oy]) and torch.equal(buf[64 + oy + n:], before[64 + oy + n:]), \
            "a byte outside the output was written"
        assert not (buf[64 + oy:64 + oy + n] == before[64 + oy:64 + oy + n]).any(), "an output element was left unwritten"
        assert same_bits(y.view(N, Cout, H - 1, W), want), (ox, ow, oy)
        for (b, v), t, off in (((xb, xv), x, ox), ((wb, wv), w, ow)):   # the inputs are unchanged
            assert bool((b[:off] == 0).all()) and bool((b[off + t.numel():] == 0).all()) and torch.equal(v.cpu(), t.reshape(-1))


def test_an_empty_batch_returns_without_a_launch(rem, monkeypatch):
    x, w = C.random_problem((1, 4, 6, 3, 7), torch.float16, 1)
    monkeypatch.setattr(rem._lib, "rroi_conv2x3_forward_hip", None)       # calling it would raise
    assert rem.conv2x3(x[:0].cuda(), w.cuda()).shape == (0, 6, 2, 7)


# ---------------------------------------------------------------- determinism, capture
DET_CASE = (5, 20, 40, 2, 96)


def test_repeated_calls_give_identical_bits(rem):
    for case in (DET_CASE, C.NETWORK_CASES[0]):
        for dtype in C.DTYPES:
            x, w = (t.cuda() for t in C.problem(case, dtype)[:2])
            first = rem.conv2x3(x, w, 0.01)
            for _ in range(3):
                assert torch.equal(C.bits(first), C.bits(rem.conv2x3(x, w, 0.01)))


def test_graph_capture_reproduces_the_eager_bits(rem):
    case, dtype = DET_CASE, torch.bfloat16
    x, w = (t.cuda() for t in C.problem(case, dtype)[:2])
    rem.conv2x3(x, w, 0.0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):                # one call on one stream: a linear graph
            out = rem.conv2x3(x, w, 0.0)
    x2, w2 = C.random_problem(case, dtype, seed=77)                # the inputs change in place
    x.copy_(x2), w.copy_(w2)
    out.fill_(NAN)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(C.bits(out), C.bits(rem.conv2x3(x, w, 0.0))) and bool(out.isfinite().all())


# ---------------------------------------------------------------- the module
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_the_switched_module_equals_the_call_on_the_networks_shape(rem, dtype, monkeypatch):
    import fots_e2e.native_remainder as rm
    case = C.NETWORK_CASES[0]
    x, w, ref, S = C.problem(case, dtype)
    m = nn.Sequential(nn.Conv2d(256, 256, (2, 3), padding=(0, 1), bias=False)).cuda().to(dtype).eval()
    with torch.no_grad():
        m[0].weight.copy_(w)
    assert rm.use_native_conv2x3(m) == 1 and type(m[0]) is rm.DenseConv2x3
    monkeypatch.setattr(rm, "_conv2x3_slower", lambda m, x: False)
    xg = x.cuda()
    direct = rem.conv2x3(xg, w.cuda())
    calls = []
    run = rem.run_conv2x3
    monkeypatch.setattr(rem, "run_conv2x3", lambda *a: calls.append(1) or run(*a))
    with torch.no_grad():
        y = m(xg)
        assert len(calls) == 1 and torch.equal(C.bits(y), C.bits(direct))
        view = torch.cat((xg, xg), 3)[:, :, :, ::2]                # a strided view: the stock path
        assert not rm.conv2x3_ok(m[0], view) and m(view).shape == y.shape and len(calls) == 1
    want, lim = C.bound(ref, S, 256, dtype, 1.0)
    assert C.within(y.cpu(), want, lim)[0]
    assert not rm.conv2x3_ok(m[0], xg) and m(xg).requires_grad and len(calls) == 1      # a gradient is needed: stock
    assert rm.use_native_conv2x3(m, False) == 1 and type(m[0]) is nn.Conv2d
