"""GPU (MI355X): the native gated merge against the float64 reference of merge_cases.py -- bit for bit over
the whole table -- special values, misaligned views with the output inside a guarded buffer, determinism, graph capture,
the switched network on the tensors it really sees, and one inference chain."""
import numpy as np
import pytest
import torch

import merge_cases as MC
from test_gpu_bucketed import NAN_PATTERN

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def same_bits(got, want):
    d, nan_ok = MC.differing(got.cpu(), want.cpu())
    return d == 0 and nan_ok


def run(ext, a, f, gate=None):
    return ext.gated_merge(a.cuda(), f.cuda(), None if gate is None else gate.cuda()).cpu()


# ---------------------------------------------------------------- against the reference: every bit
@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_against_the_reference_over_the_whole_table(ext, dtype):
    """Every case, with and without the gate: 0 elements differ in bits from the float64 reference rounded once, and the
    NaN positions are equal."""
    for case in MC.CASES:
        a, f, gate, gated, ungated = MC.problem(case, dtype)
        p = ext.merge_plan(*case[0], case[1], case[2], dtype=dtype)
        assert (p.vector_elems, p.channel_groups) == MC.plan_of(case[0], case[1], dtype)
        for g, (want, _) in ((gate, gated), (None, ungated)):
            got = run(ext, a, f, g)
            assert got.shape == want.shape and got.dtype == dtype
            d, nan_ok = MC.differing(got, want)
            print(f"{MC.case_id(case)} gate={g is not None} V={p.vector_elems} K={p.channel_groups}: {d} of {got.numel()} differ")
            assert nan_ok and d == 0, (case, g is not None, d)


def test_empty_batch_returns_without_a_call(ext):
    a, f, gate = MC.random_problem(((1, 4, 6, 6), (3, 3), (3, 3)), torch.float32, 1)
    assert ext.gated_merge(a[:0].cuda(), f[:0].cuda(), gate[:0].cuda()).shape == (0, 4, 6, 6)
    assert ext.gated_merge(a[:0].cuda(), f[:0].cuda()).shape == (0, 4, 6, 6)


# ---------------------------------------------------------------- special values
@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_non_finite_taps_poison_their_pixels_and_no_other(ext, dtype):
    """A NaN, a +inf and a -inf each in one tap of `a`, one tap of the gate and one element of f: exactly the pixels the
    reference poisons are poisoned (NaN positions and bits equal the reference's), every other element keeps the bits of
    the clean run.  (8, 12) -> (15, 23): src = dst / 2, so at every even dst l1 == 0 and the neighbouring tap -- an inf
    among them -- meets a zero weight: NaN, as the stock kernel gives."""
    case = ((2, 5, 15, 23), (8, 12), (8, 12))
    a, f, gate = MC.random_problem(case, dtype, seed=31)
    clean = run(ext, a, f, gate)
    clean_u = run(ext, a, f, None)
    assert bool(clean.isfinite().all()) and bool(clean_u.isfinite().all())
    a[0, 1, 2, 3], a[1, 4, 2, 4], a[0, 3, 7, 11] = NAN, INF, -INF
    gate[0, 0, 5, 6], gate[1, 0, 0, 11], gate[1, 0, 4, 4] = NAN, INF, -INF
    f[0, 0, 14, 22], f[1, 2, 3, 3], f[0, 4, 9, 1] = NAN, INF, -INF
    for g, base in ((gate, clean), (None, clean_u)):
        got = run(ext, a, f, g)
        want, R = MC.reference(a, f, g)
        d, nan_ok = MC.differing(got, want)
        assert nan_ok and d == 0
        touched = ~R.out64.isfinite()
        assert same_bits(got[~touched], base[~touched])
        assert 9 < int(touched.sum()) < got.numel() // 4
        # the weight-zero tap.  Output (4, 6) reads a[.., 2, 3] with weight 1 and a[.., 2, 4] -- the inf -- with weight 0:
        # NaN; output (4, 8) reads the inf with weight 1 and finite neighbours with 0: +inf.  The -inf is a's last row and
        # column: output (14, 22) reads it four times with the weights (1, 0, 0, 0): NaN.
        assert bool(got[1, 4, 4, 6].isnan()) and float(got[1, 4, 4, 8]) == INF and bool(got[0, 3, 14, 22].isnan())
        assert bool(got[0, 1, 4, 6].isnan()) and not bool(got[0, 2, 4, 6].isnan())


def test_subnormal_results_and_gates_outside_the_unit_interval(ext):
    """An fp32 subnormal result is kept (inputs and output); a gate value outside [0, 1] is used as it is."""
    tiny = 2.0 ** -140
    a = torch.full((1, 2, 2, 2), tiny)
    f = torch.full((1, 2, 4, 4), 3 * tiny)
    gate = torch.full((1, 1, 2, 2), 0.5)
    for g in (gate, None):
        got = run(ext, a, f, g)
        want, _ = MC.reference(a, f, g)
        assert same_bits(got, want) and bool((got > 0).all()) and bool((got < 2.0 ** -126).all())
    a, f, gate = MC.random_problem(((1, 3, 9, 9), (9, 9), (5, 5)), torch.float32, 5)
    gate = gate * 7 - 3                                           # in [-3, 4)
    assert same_bits(run(ext, a, f, gate), MC.reference(a, f, gate)[0])
    lo = 2.0 ** -20                                               # float16: a result below its normal range rounds as torch's does
    a, f = torch.full((1, 1, 3, 3), lo).half(), torch.full((1, 1, 3, 3), 3 * lo).half()
    gate = torch.full((1, 1, 2, 2), 0.375).half()
    assert same_bits(run(ext, a, f, gate), MC.reference(a, f, gate)[0])


# ---------------------------------------------------------------- addresses and guards
@pytest.mark.parametrize("case", [((2, 5, 11, 23), (6, 12), (5, 11)), ((1, 3, 45, 47), (45, 47), (23, 24)),
                                  ((1, 9, 33, 63), (17, 32), (17, 32))], ids=MC.case_id)
@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_views_and_guards(ext, dtype, case):
    """a, the gate, f and y 0 .. 3 elements past a 16-byte boundary, through the raw ABI; y inside a guarded buffer.  Every
    output element is written, no guard byte is, the inputs are unchanged and the bits do not depend on an address.
    (45 x 47 = 2115 and 33 x 63 = 2079 pixels: odd planes of more than one tile.)"""
    (N, C, H, W), (ah, aw), (gh, gw) = case
    a, f, gate = MC.random_problem(case, dtype, seed=sum(case[0]))
    want = MC.reference(a, f, gate)[0]
    want_u = MC.reference(a, f, None)[0]
    itype = torch.int32 if dtype == torch.float32 else torch.int16
    stream = torch.cuda.current_stream().cuda_stream
    n = f.numel()

    def shifted(t, off):
        buf = torch.zeros(t.numel() + 8, dtype=dtype, device="cuda")
        view = buf[off:off + t.numel()]
        view.copy_(t.reshape(-1))
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + off * t.element_size()
        return buf, view

    for oa, og, of, oy in ((0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (1, 0, 2, 3), (0, 3, 1, 0), (2, 1, 0, 2)):
        (ab, av), (gb, gv), (fb, fv) = shifted(a, oa), shifted(gate, og), shifted(f, of)
        for g_ptr, expect in ((gv.data_ptr(), want), (None, want_u)):
            buf = torch.full((64 + oy + n + 64,), NAN_PATTERN[dtype], dtype=itype, device="cuda")
            before = buf.clone()
            y = buf[64 + oy:64 + oy + n].view(dtype)
            st = ext._lib.rroi_merge_forward_hip(ext.dtype_code(dtype), av.data_ptr(), ah, aw, g_ptr, gh, gw, fv.data_ptr(),
                                                 y.data_ptr(), N, C, H, W, stream)
            torch.cuda.synchronize()
            assert st == 1
            assert torch.equal(buf[:64 + oy], before[:64 + oy]) and torch.equal(buf[64 + oy + n:], before[64 + oy + n:]), \
                "a byte outside the output was written"
            assert not (buf[64 + oy:64 + oy + n] == before[64 + oy:64 + oy + n]).any(), "an output element was left unwritten"
            assert same_bits(y.view(N, C, H, W), expect), (oa, og, of, oy)
        for (b, v), t, off in (((ab, av), a, oa), ((gb, gv), gate, og), ((fb, fv), f, of)):   # the inputs are unchanged
            assert bool((b[:off] == 0).all()) and bool((b[off + t.numel():] == 0).all()) and torch.equal(v.cpu(), t.reshape(-1))


# ---------------------------------------------------------------- determinism, streams, capture
DET_CASES = [((3, 256, 16, 24), (8, 12), (8, 12)), ((1, 9, 40, 52), (40, 52), (20, 26))]


@pytest.mark.parametrize("case", DET_CASES, ids=MC.case_id)
def test_two_calls_and_a_second_stream_give_identical_bits(ext, case):
    for dtype in (torch.float32, torch.bfloat16):
        a, f, gate = (t.cuda() for t in MC.problem(case, dtype)[:3])
        first, second = ext.gated_merge(a, f, gate), ext.gated_merge(a, f, gate)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            third = ext.gated_merge(a, f, gate)
        side.synchronize()
        assert same_bits(first, second) and same_bits(first, third) and same_bits(first, MC.problem(case, dtype)[3][0])


@pytest.mark.parametrize("case", DET_CASES, ids=MC.case_id)
def test_graph_capture_reproduces_the_eager_bits(ext, case):
    dtype = torch.bfloat16 if case[0][0] == 3 else torch.float32
    a, f, gate = (t.cuda() for t in MC.problem(case, dtype)[:3])
    ext.gated_merge(a, f, gate), ext.gated_merge(a, f)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):                # one stream, no branches
            outs = (ext.gated_merge(a, f, gate), ext.gated_merge(a, f))
    a2, f2, gate2 = MC.random_problem(case, dtype, seed=77)       # the inputs change in place
    a.copy_(a2), f.copy_(f2), gate.copy_(gate2)
    for o in outs:
        o.fill_(NAN)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(outs[0], ext.gated_merge(a, f, gate)) and same_bits(outs[1], ext.gated_merge(a, f))
    assert same_bits(outs[0], MC.reference(a2, f2, gate2)[0])


# ---------------------------------------------------------------- in the network
def record_merges(ext, monkeypatch):
    calls = []
    merge_run = ext._gated_merge_run

    def wrapped(a, f, gate=None):
        out = merge_run(a, f, gate)
        calls.append((a.detach(), f.detach(), None if gate is None else gate.detach(), out))
        return out
    monkeypatch.setattr(ext, "_gated_merge_run", wrapped)
    return calls


@pytest.mark.parametrize("heads", (False, True), ids=("merge", "heads+merge"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=["fp32", "bf16"])
def test_the_switched_network_runs_the_kernel_on_its_own_tensors(ext, dtype, heads, monkeypatch):
    """FOTSNet on a 64 x 96 image: three native merge calls; each output is bit for bit the reference of its own inputs and
    within the stock bound of the stock expression on the same tensors; focr keeps its bits; a `requires_grad` input
    takes the stock path."""
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import (NativeHeadsMergeFOTSNet, NativeMergeFOTSNet, merge_ok, use_native_heads, use_native_merge)
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet()).eval().cuda().to(dtype)
    image = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(7)).cuda().to(dtype)
    with torch.no_grad():
        stock = net(image)
    if heads:
        assert use_native_heads(net)
    assert use_native_merge(net) and type(net) is (NativeHeadsMergeFOTSNet if heads else NativeMergeFOTSNet)
    calls = record_merges(ext, monkeypatch)
    gates = []
    if heads:
        gate_run = ext._gate_run
        monkeypatch.setattr(ext, "_gate_run", lambda *a: gates.append(1) or gate_run(*a))
    with torch.no_grad():
        native = net(image)
    assert len(calls) == 3 and len(gates) == (3 if heads else 0)
    assert [tuple(f.shape) for _, f, _, _ in calls] == [(1, 256, 4, 6), (1, 256, 8, 12), (1, 256, 16, 24)]
    assert [tuple(a.shape[2:]) for a, _, _, _ in calls] == [(2, 3), (8, 12), (16, 24)]
    assert [tuple(g.shape) for _, _, g, _ in calls] == [(1, 1, 2, 3), (1, 1, 4, 6), (1, 1, 8, 12)]
    assert same_bits(native[3][1], stock[3][1])                   # focr
    for p, q in zip(stock, native):
        assert [s.shape for s in p] == [t.shape for t in q]
    for a, f, g, out in calls:
        want, R = MC.reference(a.cpu(), f.cpu(), g.cpu())
        d, nan_ok = MC.differing(out.cpu(), want)
        assert nan_ok and d == 0, (tuple(f.shape), d)
        with torch.no_grad():
            expr = MC.stock(a, f, g).cpu()
        ok, worst = MC.within(expr, out.cpu(), MC.stock_bound(a.cpu(), f.cpu(), g.cpu(), R))
        print(f"{tuple(f.shape)}: worst |stock - native| / stock bound {worst:.3f}")
        assert ok, (tuple(f.shape), worst)
    # a gradient is needed: the stock path
    a, f, g, _ = calls[0]
    fg = f.clone().requires_grad_(True)
    assert not merge_ok(a, fg, g)
    t = net._merge_one(a, fg, a)
    assert t.requires_grad and len(calls) == 3
    assert use_native_merge(net, False) and (not heads or use_native_heads(net, False)) and type(net) is FOTSNet


def test_the_network_without_attention_runs_three_ungated_calls(ext, monkeypatch):
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import use_native_merge
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet(attention=False)).eval().cuda()
    image = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(7)).cuda()
    assert use_native_merge(net)
    calls = record_merges(ext, monkeypatch)
    with torch.no_grad():
        net(image)
    assert len(calls) == 3 and all(g is None for _, _, g, _ in calls)
    for a, f, _, out in calls:
        assert same_bits(out, MC.reference(a.cpu(), f.cpu(), None)[0])


def test_one_inference_chain_gives_the_same_boxes_and_texts(ext):
    """`infer_image` on a small image with the synthetic detector's maps: the switched network (its merges run the kernel
    inside the pass) returns the boxes and texts of the un-switched one."""
    from e2e_inputs import synthetic_detector_maps
    from fots_e2e.alphabet import ALPHABET
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import use_native_merge
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
        assert use_native_merge(net)
        boxes1, texts1 = infer_image(net, conv, im_data, detector=hook)
    assert len(boxes0) >= 3, "the synthetic detector maps must yield boxes"
    assert np.array_equal(np.asarray(boxes0), np.asarray(boxes1)) and list(texts0) == list(texts1)
