"""GPU (MI355X): the fused bilinear resize + depthwise 3x3, all three dtypes over the table of
updw_cases.py: every bit of the float64 reference, every bit of the unfused native chain
`depthwise3x3(gated_merge(a, zeros of the target's size), w)`, misaligned views inside a guarded buffer, repeatability,
graph capture, and where a NaN in the source goes."""
import numpy as np
import pytest
import torch

import updw_cases as U
from test_gpu_bucketed import NAN_PATTERN

pytestmark = pytest.mark.gpu

DTYPE_PARAMS = pytest.mark.parametrize("dtype", U.DTYPES, ids=U.IDS)


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


@pytest.fixture(scope="module")
def rem():
    from rroi_align._ext.rroi_align import remainder
    return remainder


def itype(dtype):
    return torch.int32 if dtype == torch.float32 else torch.int16


# ---------------------------------------------------------------- against the reference and the unfused chain
@DTYPE_PARAMS
def test_the_whole_table_equals_the_reference_and_the_unfused_native_chain_bit_for_bit(ext, rem, dtype):
    assert {U.band_of_case(c) for c in U.CASES} == U.BANDS_REACHED
    for case in U.CASES:
        a, w, want = U.problem(case, dtype)
        ag, wg = a.cuda(), w.cuda()
        got = rem.up_depthwise3x3(ag, wg, case[1])
        assert got.shape == want.shape and got.dtype == dtype and got.is_contiguous()
        wrong, nan_ok = U.differing(got.cpu(), want)
        print(f"{U.case_id(case)} band {U.band_of_case(case)}: {wrong} of {want.numel()} elements differ from the reference")
        assert wrong == 0 and nan_ok and bool(got.isfinite().all()), (case, wrong)
        zeros = torch.zeros(case[0][:2] + case[1], dtype=dtype, device="cuda")
        resized = ext.gated_merge(ag, zeros)                       # A + 0: the rounded resized map, stored
        assert U.differing(resized.cpu(), U.resized(a, case[1])) == (0, True)
        chain = ext.depthwise3x3(resized, wg, 1)
        assert torch.equal(U.bits(got), U.bits(chain)), case


# ---------------------------------------------------------------- addresses and guards
@pytest.mark.parametrize("case", [((2, 3, 3, 4), (5, 7)), ((1, 2, 6, 13), (6, 13)), ((1, 3, 5, 6), (9, 12))], ids=U.case_id)
@DTYPE_PARAMS
def test_views_and_guards(ext, rem, dtype, case):
    """a, w and y 0 .. 7 elements past a 16-byte boundary, through the raw ABI; y inside a guarded buffer.  Every output
    element is written, no guard byte is, the inputs are unchanged and the bits do not depend on an address."""
    (N, C, h, wi), (Ho, Wo) = case
    a, w = U.random_problem(case, dtype, seed=5)
    n = N * C * Ho * Wo
    stream = torch.cuda.current_stream().cuda_stream
    want = U.reference(a, w, case[1])

    def shifted(t, off):
        buf = torch.zeros(t.numel() + 16, dtype=dtype, device="cuda")
        view = buf[off:off + t.numel()]
        view.copy_(t.reshape(-1))
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + off * t.element_size()
        return buf, view

    for oa, ow, oy in ((0, 0, 0), (1, 1, 1), (3, 2, 5), (7, 5, 2), (4, 3, 7), (2, 6, 4), (5, 7, 3), (6, 4, 6)):
        (ab, av), (wb, wv) = shifted(a, oa), shifted(w, ow)
        buf = torch.full((64 + oy + n + 64,), NAN_PATTERN[dtype], dtype=itype(dtype), device="cuda")
        before = buf.clone()
        y = buf[64 + oy:64 + oy + n].view(dtype)
        st = ext._lib.rroi_up_depthwise3x3_forward_hip(ext.dtype_code(dtype), av.data_ptr(), wv.data_ptr(), y.data_ptr(), N, C,
                                                       h, wi, Ho, Wo, stream)
        torch.cuda.synchronize()
        assert st == 1
        assert torch.equal(buf[:64 + oy], before[:64 + oy]) and torch.equal(buf[64 + oy + n:], before[64 + oy + n:]), \
            "a byte outside the output was written"
        assert not (buf[64 + oy:64 + oy + n] == before[64 + oy:64 + oy + n]).any(), "an output element was left unwritten"
        assert U.differing(y.view(N, C, Ho, Wo).cpu(), want) == (0, True), (oa, ow, oy)
        for (b, v), t, off in (((ab, av), a, oa), ((wb, wv), w, ow)):   # the inputs are unchanged
            assert bool((b[:off] == 0).all()) and bool((b[off + t.numel():] == 0).all()) and torch.equal(v.cpu(), t.reshape(-1))


def test_an_empty_batch_returns_without_a_launch(rem, monkeypatch):
    a, w = U.random_problem(((1, 4, 5, 7), (10, 14)), torch.float16, 1)
    monkeypatch.setattr(rem._lib, "rroi_up_depthwise3x3_forward_hip", None)      # calling it would raise
    assert rem.up_depthwise3x3(a[:0].cuda(), w.cuda(), (10, 14)).shape == (0, 4, 10, 14)


# ---------------------------------------------------------------- determinism, capture
DET_CASE = ((2, 3, 9, 5), (19, 13))


@DTYPE_PARAMS
def test_repeated_calls_give_identical_bits(rem, dtype):
    a, w = (t.cuda() for t in U.problem(DET_CASE, dtype)[:2])
    first = rem.up_depthwise3x3(a, w, DET_CASE[1])
    for _ in range(3):
        assert torch.equal(U.bits(first), U.bits(rem.up_depthwise3x3(a, w, DET_CASE[1])))


def test_graph_capture_reproduces_the_eager_bits(rem):
    case, dtype = DET_CASE, torch.bfloat16
    a, w = (t.cuda() for t in U.problem(case, dtype)[:2])
    rem.up_depthwise3x3(a, w, case[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):                # one call on one stream: a linear graph
            out = rem.up_depthwise3x3(a, w, case[1])
    a2, w2 = U.random_problem(case, dtype, seed=77)                # the inputs change in place
    a.copy_(a2), w.copy_(w2)
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert U.differing(out.cpu(), U.reference(a2, w2, case[1])) == (0, True) and bool(out.isfinite().all())


# ---------------------------------------------------------------- special values
@pytest.mark.parametrize("case", [((1, 2, 5, 7), (10, 14)), ((1, 2, 6, 9), (6, 9)), ((1, 2, 7, 9), (4, 5))], ids=U.case_id)
@DTYPE_PARAMS
def test_a_nan_reaches_exactly_the_windows_that_hold_a_value_tapping_it(rem, dtype, case):
    """No tap of the resize and no tap of the convolution is skipped, whatever its weight: a NaN at (i, j) of one plane is
    in every element of U whose blend reads (i, j), and in every output whose 3x3 window holds such an element -- and
    nowhere else, not in the other plane either."""
    a, w = U.random_problem(case, dtype, seed=9)
    w[0, 0, 1, 1] = 0.0                                            # a zero weight poisons as well: 0 * NaN
    clean = rem.up_depthwise3x3(a.cuda(), w.cuda(), case[1]).cpu()
    (_, _, h, wi), _ = case
    for i, j in ((0, 0), (h - 1, wi - 1), (h // 2, wi // 2)):
        bad = a.clone()
        bad[0, 0, i, j] = float("nan")
        got = rem.up_depthwise3x3(bad.cuda(), w.cuda(), case[1]).cpu()
        want = np.zeros(tuple(got.shape), bool)
        want[0, 0] = U.window_of(U.tapped_by(case, i, j))
        assert want.any() and not want[0, 0].all()
        assert np.array_equal(got.isnan().numpy(), want), (i, j)
        assert torch.equal(U.bits(got)[~got.isnan()], U.bits(clean)[~got.isnan()])
        assert U.differing(got, U.reference(bad, w, case[1])) == (0, True)
