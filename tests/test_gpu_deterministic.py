"""GPU (MI355X): the deterministic backward (RROI_PATH_DETERMINISTIC, plan ORDERED).  Its contract is the
oracle's own sum -- every feature-gradient element added in double from +0.0 in statement order (ROI, pooled row,
pooled column, tap) and rounded once -- so every comparison here is exact against oracle.backward_c: the same bits, or
NaN where the oracle has NaN, whatever the layouts, the stream or a graph capture.  16-bit calls: that fp32 gradient of
the widened grad_output, rounded with torch's .to(dtype).  ROIs with a bad batch index give no gradient: the oracle
gets index 0 and a zero grad_output for them."""
import contextlib

import numpy as np
import pytest
import torch

import plan_cases as PC
import workloads as Wk
from test_gpu_fuzz import problem

pytestmark = pytest.mark.gpu

LAYOUTS = ((False, False), (True, False), (False, True), (True, True))   # (channels-last top_diff, channels-last grad)


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


@contextlib.contextmanager
def torch_deterministic(on=True):
    """torch.use_deterministic_algorithms for the block; the process-wide flag is restored whatever happens."""
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before)


def same(got, want):
    """Bit for bit, NaN where the other has NaN (any payload)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got[~gn].view(np.uint32), want[~wn].view(np.uint32)))


def diff(got, want):
    return f"{int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())} of {got.size} differ"


def run(ext, g, rois, shape, s, cl_td=False, cl_bd=False, **kw):
    G = g.contiguous(memory_format=torch.channels_last) if cl_td else g
    out = ext.backward(G, rois, shape, s, channels_last_grad=cl_bd, deterministic=True, **kw)
    if cl_bd and shape[1] % 4 == 0:
        assert out.is_contiguous(memory_format=torch.channels_last)
    return out.float().cpu().numpy()


def oracle_inputs(r, g, B):
    """The oracle's ROIs and grad_output: bad batch indices -> index 0 and no gradient."""
    bi = r[:, 0]
    bad = ~((bi > -1) & (bi < B))   # (int) truncation: -0.5 -> 0 is valid
    r_o, g_o = r.copy(), g.copy()
    r_o[bad, 0] = 0
    g_o[bad] = 0
    return r_o, g_o


def check_plan(ext, B, C, H, W, R, ph, pw, cl_td, cl_bd, dtype=torch.float32):
    plan = ext.backward_plan(B, C, H, W, R, ph, pw, top_diff_layout=int(cl_td), bottom_diff_layout=int(cl_bd),
                             dtype=dtype, deterministic=True)
    assert plan.family == (ext.PLAN_BWD_ORDERED if R > 0 else ext.PLAN_NONE), plan


def sandwich(r, g, big):
    """Inputs whose rounded sums depend on the ORDER of each pixel's list (with N(0, 1) data a double sum of fp32
    products is almost always exact, so any order gives the same fp32 result).  Three blocks of ROIs: copies of `r` with
    grad_output +big, `r` with `g`, copies of `r` with -big.  A pixel's statement-order sum runs up to S = big * sum(w),
    takes the O(1) terms at S's granularity (their low bits are rounded away), and comes back down by exactly S: the
    result is the O(1) part, rounded in a way that any other order -- another ROI order, the reverse one, the lists as
    the fill left them -- does not reproduce."""
    rr = np.concatenate([r, r, r])
    gg = np.concatenate([np.full_like(g, big), g, np.full_like(g, -big)])
    return rr, gg


def assert_order_sensitive(oracle, g, r, shape, s, want, dtype=None):
    """The input tells orders apart: the oracle's sum over the ROIs in reverse order, and in a shuffled order, differ
    from the statement-order sum in many elements."""
    rnd = lambda x: x if dtype is None else torch.from_numpy(x).to(dtype).float().numpy()
    for perm in (np.arange(len(r))[::-1], np.random.default_rng(0).permutation(len(r))):
        other = rnd(oracle.backward_c(np.ascontiguousarray(g[perm]), np.ascontiguousarray(r[perm]), shape, s, threads=8))
        assert (other != want).sum() > 100, "the input does not tell the orders apart"


def list_lengths(oracle, g, r, shape, s):
    """Terms per feature element (>= the element's list length, <= 4 x it: aliased taps share one entry)."""
    return oracle.backward_bound_c(g, r, shape, s, threads=8)[1]


@pytest.mark.parametrize("regime", ["register", "lds", "global"])
def test_order_of_each_list(ext, oracle, regime):
    """Each sort regime on order-sensitive inputs (sandwich()): lists of <= 64 entries (the register rank sort), of
    hundreds (the queued LDS sort) and of more than 4096 (the queued sort in global memory).  Only the statement order
    reproduces the oracle here."""
    if regime == "register":      # the reference's shapes, 3 x 32 ROIs
        f, r0 = Wk.bench_inputs(R=32, C=64, H=120, W=160, img=640, seed=21, batch=2)
        ph, pw, s, big = 11, 96, 0.25, 2.0 ** 40
    elif regime == "lds":         # the overlap generator, 3 x 60 ROIs
        f, r0 = PC.inputs(PC.Case("overlap", "bwd", 2, 36, 64, 64, 60, 16, 9, gen="overlap"), seed=4)
        ph, pw, s, big = 16, 9, PC.SCALE, 2.0 ** 40
    else:                         # 3 x 1400 copies of one ROI whose bins lie about a pixel apart
        f = np.random.default_rng(6).standard_normal((1, 8, 40, 48)).astype(np.float32)
        r0 = np.tile(np.array([[0, 24.25, 20.5, 8.0, 20.0, 17.0]], np.float32), (1400, 1))
        ph, pw, s, big = 8, 20, 1.0, 2.0 ** 26
    g0 = np.random.default_rng(8).standard_normal((len(r0), f.shape[1], ph, pw)).astype(np.float32)
    r, g = sandwich(r0, g0, big)
    want = oracle.backward_c(g, r, f.shape, s, threads=8)
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert_order_sensitive(oracle, g, r, f.shape, s, want)
    n = list_lengths(oracle, g, r, f.shape, s)
    if regime == "register":
        assert (n[(n > 0)] <= 64).mean() > 0.9
    elif regime == "lds":
        assert (n > 4 * 64).sum() > 1000 and n.max() <= 4096
    else:
        assert n.max() > 4 * 4096
    G, Rr = torch.from_numpy(g).cuda(), torch.from_numpy(r).cuda()
    for cl_td, cl_bd in (LAYOUTS if f.shape[1] % 4 == 0 else LAYOUTS[:1]):
        for k in range(2):
            got = run(ext, G, Rr, f.shape, s, cl_td, cl_bd)
            assert same(got, want), f"{regime} layouts {cl_td, cl_bd} call {k}: {diff(got, want)}"


def test_order_bf16(ext, oracle):
    """The same for a bfloat16 grad_output (big = 2^50: bf16 keeps 8 bits, so the lost low bits must lie above its
    ulp), against the rounded oracle."""
    f, r0 = Wk.bench_inputs(R=64, C=64, H=120, W=160, img=640, seed=22, batch=2)
    g0 = torch.randn(64, 64, 11, 96, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16).float().numpy()
    r, g = sandwich(r0, g0, 2.0 ** 50)
    want = torch.from_numpy(oracle.backward_c(g, r, f.shape, 0.25, threads=8)).to(torch.bfloat16).float().numpy()
    assert_order_sensitive(oracle, g, r, f.shape, 0.25, want, torch.bfloat16)
    Gh = torch.from_numpy(g).to(torch.bfloat16).cuda()
    assert torch.equal(Gh.float().cpu(), torch.from_numpy(g))
    for cl_bd in (False, True):
        got = ext.backward(Gh, torch.from_numpy(r).cuda(), f.shape, 0.25, channels_last_grad=cl_bd, deterministic=True)
        got = got.float().cpu().numpy()
        assert same(got, want), f"bf16 cl_bd {cl_bd}: {diff(got, want)}"


@pytest.mark.parametrize("case", [c for c in PC.CASES if c.kind == "bwd" and c.caller == PC.NATIVE],
                         ids=lambda c: c.name)
def test_plan_case(ext, oracle, case):
    """Every native backward case of the coverage table, in its layouts, with the bit: ORDERED, equal to the oracle."""
    f, r = PC.inputs(case)
    B, C, H, W = f.shape
    g = np.random.default_rng(1).standard_normal((case.R, C, case.ph, case.pw)).astype(np.float32)
    r_o, g_o = oracle_inputs(r, g, B)
    want = oracle.backward_c(g_o, r_o, f.shape, PC.SCALE, threads=8)
    cl_td, cl_bd = case.fl == PC.NHWC, case.tl == PC.NHWC
    check_plan(ext, B, C, H, W, case.R, case.ph, case.pw, cl_td and case.ph * case.pw > 1, cl_bd)
    got = run(ext, torch.from_numpy(g).cuda(), torch.from_numpy(r).cuda(), f.shape, PC.SCALE, cl_td, cl_bd)
    assert same(got, want), diff(got, want)


def test_cfg2_all_layouts_three_calls(ext, oracle):
    """configs[2] at full size (1 x 256 x 160 x 160, 512 ROIs, 8 x 64): four layout pairs, three calls each -- twelve
    results, all the oracle's bits."""
    f, r = Wk.bench_inputs()
    g = np.random.default_rng(11).standard_normal((512, 256, 8, 64)).astype(np.float32)
    want = oracle.backward_c(g, r, f.shape, 0.25, threads=oracle.max_threads())
    G, Rr = torch.from_numpy(g).cuda(), torch.from_numpy(r).cuda()
    for cl_td, cl_bd in LAYOUTS:
        check_plan(ext, 1, 256, 160, 160, 512, 8, 64, cl_td, cl_bd)
        for k in range(3):
            got = run(ext, G, Rr, f.shape, 0.25, cl_td, cl_bd)
            assert same(got, want), f"layouts {cl_td, cl_bd} call {k}: {diff(got, want)}"


@pytest.mark.parametrize("R", [32, 512])
def test_reference_training_shapes(ext, oracle, R):
    """The reference's training shapes: C = 64, two 120 x 160 maps, 11 x 96."""
    f, r = Wk.bench_inputs(R=R, C=64, H=120, W=160, img=640, seed=R, batch=2)
    g = np.random.default_rng(R).standard_normal((R, 64, 11, 96)).astype(np.float32)
    want = oracle.backward_c(g, r, f.shape, 0.25, threads=8)
    G, Rr = torch.from_numpy(g).cuda(), torch.from_numpy(r).cuda()
    for cl_td, cl_bd in LAYOUTS:
        got = run(ext, G, Rr, f.shape, 0.25, cl_td, cl_bd)
        assert same(got, want), f"R={R} layouts {cl_td, cl_bd}: {diff(got, want)}"


def test_long_lists(ext, oracle):
    """Lists of hundreds (the overlap generator, R = 1500) and of thousands (4096 copies of one ROI whose bins lie
    about a pixel apart: ~4 pairs per pixel per copy) -- the LDS and the global-memory sorts."""
    case = PC.Case("overlap", "bwd", 2, 36, 64, 64, 1500, 16, 9, gen="overlap")
    f, r = PC.inputs(case, seed=3)
    g = np.random.default_rng(5).standard_normal((1500, 36, 16, 9)).astype(np.float32)
    want = oracle.backward_c(g, r, f.shape, PC.SCALE, threads=8)
    got = run(ext, torch.from_numpy(g).cuda(), torch.from_numpy(r).cuda(), f.shape, PC.SCALE)
    assert same(got, want), "overlap: " + diff(got, want)
    # 4096 copies: an 8 x 20-pixel ROI pooled 8 x 20 at scale 1 on a 1 x 8 x 40 x 48 map
    f = np.random.default_rng(6).standard_normal((1, 8, 40, 48)).astype(np.float32)
    r = np.tile(np.array([[0, 24.25, 20.5, 8.0, 20.0, 17.0]], np.float32), (4096, 1))
    g = np.random.default_rng(7).standard_normal((4096, 8, 8, 20)).astype(np.float32)
    want = oracle.backward_c(g, r, f.shape, 1.0, threads=8)
    assert np.abs(want).max() > 0
    got = run(ext, torch.from_numpy(g).cuda(), torch.from_numpy(r).cuda(), f.shape, 1.0)
    assert same(got, want), "4096 copies: " + diff(got, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_half(ext, oracle, dtype):
    """16-bit grad_output: the fp32 ORDERED gradient of the widened grad_output, rounded with .to(dtype) -- both gradient
    layouts, the reference's shapes and the overlap generator."""
    for f, r, ph, pw, s in ((*Wk.bench_inputs(R=512, C=64, H=120, W=160, img=640, seed=2, batch=2), 11, 96, 0.25),
                            (*PC.inputs(PC.Case("o", "bwd", 2, 36, 64, 64, 600, 16, 9, gen="overlap")), 16, 9, PC.SCALE)):
        B, C, H, W = f.shape
        R = len(r)
        gh = torch.randn(R, C, ph, pw, generator=torch.Generator().manual_seed(R)).to(dtype)
        want32 = oracle.backward_c(gh.float().numpy(), r, f.shape, s, threads=8)
        want = torch.from_numpy(want32).to(dtype).float().numpy()
        for cl_bd in (False, True):
            check_plan(ext, B, C, H, W, R, ph, pw, False, cl_bd, dtype)
            got = ext.backward(gh.cuda(), torch.from_numpy(r).cuda(), f.shape, s, channels_last_grad=cl_bd,
                               deterministic=True)
            assert got.dtype == dtype
            got = got.float().cpu().numpy()
            assert same(got, want), f"{dtype} R={R} cl_bd {cl_bd}: {diff(got, want)}"


def test_seeded_fuzz(ext, oracle):
    """48 trials of test_gpu_fuzz.problem (degenerate and non-finite ROIs, bad batch indices, rounding ties, awkward
    channel and pooled sizes), every layout leg."""
    rng = np.random.default_rng(7)
    fails = []
    for t in range(48):
        f, r, ph, pw, s = problem(rng, t)
        B, C, H, W = f.shape
        R = len(r)
        g = np.random.default_rng(t).standard_normal((R, C, ph, pw)).astype(np.float32)
        r_o, g_o = oracle_inputs(r, g, B)
        want = oracle.backward_c(g_o, r_o, f.shape, s, threads=8)
        G, Rr = torch.from_numpy(g).cuda(), torch.from_numpy(r).cuda()
        for cl_td, cl_bd in (LAYOUTS if C % 4 == 0 else LAYOUTS[:1]):
            got = run(ext, G, Rr, f.shape, s, cl_td, cl_bd)
            if not same(got, want):
                fails.append(f"trial {t}: C={C} {H}x{W} B={B} {ph}x{pw} s={s} R={R} layouts {cl_td, cl_bd}: "
                             + diff(got, want))
    assert not fails, "\n".join(fails)


def test_trig_fp32(ext, oracle):
    """TRIG_FP32: the same bits across calls and layouts; equal to the oracle (which has the double recipe only) on a
    problem whose bin centres the two recipes agree on."""
    for seed in range(40, 60):
        f, r = Wk.bench_inputs(R=64, C=64, H=120, W=160, img=640, seed=seed, batch=2)
        Rr = torch.from_numpy(r).cuda()
        c0 = ext.bin_centres(Rr, 11, 96, 0.25, 120, 160, trig=ext.TRIG_DOUBLE)
        c1 = ext.bin_centres(Rr, 11, 96, 0.25, 120, 160, trig=ext.TRIG_FP32)
        if torch.equal(c0, c1):
            break
    else:
        pytest.fail("no seed in 40..59 whose bin centres agree between the two recipes")
    g = np.random.default_rng(seed).standard_normal((64, 64, 11, 96)).astype(np.float32)
    want = oracle.backward_c(g, r, f.shape, 0.25, threads=8)
    G = torch.from_numpy(g).cuda()
    first = run(ext, G, Rr, f.shape, 0.25, trig=ext.TRIG_FP32)
    assert same(first, want), diff(first, want)
    for cl_td, cl_bd in LAYOUTS:
        for _ in range(2):
            got = run(ext, G, Rr, f.shape, 0.25, cl_td, cl_bd, trig=ext.TRIG_FP32)
            assert same(got, first), f"layouts {cl_td, cl_bd}: {diff(got, first)}"
    # a problem where the recipes do disagree somewhere: still the same bits on every call and layout
    f, r = Wk.bench_inputs(seed=1)
    G = torch.randn(512, 256, 8, 64, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    Rr = torch.from_numpy(r).cuda()
    first = run(ext, G, Rr, f.shape, 0.25, trig=ext.TRIG_FP32)
    for cl_td, cl_bd in LAYOUTS:
        got = run(ext, G, Rr, f.shape, 0.25, cl_td, cl_bd, trig=ext.TRIG_FP32)
        assert same(got, first), f"configs[2] layouts {cl_td, cl_bd}: {diff(got, first)}"


def test_graph_replay_and_two_streams(ext, oracle):
    """Replays of a captured ORDERED backward, and two ORDERED calls on two streams in flight together: bit-exact."""
    f, r0 = Wk.bench_inputs(R=96, C=64, H=64, W=96, img=384, seed=31)
    _, r1 = Wk.bench_inputs(R=96, C=64, H=64, W=96, img=384, seed=32)
    g = np.random.default_rng(3).standard_normal((96, 64, 8, 64)).astype(np.float32)
    want = [oracle.backward_c(g, r, f.shape, 0.25, threads=8) for r in (r0, r1)]
    G, Rr = torch.from_numpy(g).cuda(), [torch.from_numpy(r0).cuda(), torch.from_numpy(r1).cuda()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm the workspace cache on the capture stream
        ext.backward(G, Rr[0], f.shape, 0.25, deterministic=True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ext.backward(G, Rr[0], f.shape, 0.25, deterministic=True)
    for k in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), want[0]), f"replay {k}"
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    grads = []
    for i in range(8):
        with torch.cuda.stream(streams[i % 2]):
            grads.append(ext.backward(G, Rr[i % 2], f.shape, 0.25, deterministic=True,
                                      channels_last_grad=bool(i & 2)))
    for st in streams:
        st.synchronize()
    for i, gi in enumerate(grads):
        assert same(gi.cpu().numpy(), want[i % 2]), f"call {i} on stream {i % 2}"


def test_autograd_follows_torch_flag(ext, oracle, monkeypatch):
    """Under torch.use_deterministic_algorithms(True) the op's backward runs ORDERED (the oracle's bits); an explicit
    deterministic=False overrides the flag; with the flag off nothing changes."""
    from rroi_align.functions.rroi_align import RRoiAlignFunction
    from rroi_align.modules.rroi_align import _RRoiAlign
    f, r = Wk.bench_inputs(R=64, C=64, H=64, W=96, img=384, seed=9)
    want_f = oracle.forward_c(f, r, 8, 64, 0.25, threads=8)
    want = oracle.backward_c((2 * want_f).astype(np.float32), r, f.shape, 0.25, threads=8)
    Rr = torch.from_numpy(r).cuda()
    seen = []
    real = ext.backward

    def spy(*a, **kw):
        seen.append(kw.get("deterministic"))
        return real(*a, **kw)
    monkeypatch.setattr(ext, "backward", spy)

    def grad(deterministic=None, module=True):
        F = torch.from_numpy(f).cuda().requires_grad_(True)
        op = (_RRoiAlign(8, 64, 0.25, deterministic=deterministic) if module
              else RRoiAlignFunction(8, 64, 0.25, deterministic=deterministic))
        (op(F, Rr) ** 2).sum().backward()
        return F.grad.cpu().numpy()

    with torch_deterministic(True):
        got = grad()
        assert seen[-1] is True and same(got, want), diff(got, want)
        got = grad(module=False)
        assert seen[-1] is True and same(got, want)
        grad(deterministic=False)
        assert seen[-1] is False
    with torch_deterministic(False):
        grad()
        assert seen[-1] is False
        got = grad(deterministic=True)
        assert seen[-1] is True and same(got, want)
    # the legacy by-hand backward follows the same rule
    fn = RRoiAlignFunction(8, 64, 0.25)
    F = torch.from_numpy(f).cuda()
    out = fn.forward(F, Rr)
    with torch_deterministic(True):
        gi, _ = fn.backward(2 * out)
        assert seen[-1] is True and same(gi.cpu().numpy(), want)
    gi, _ = fn.backward(2 * out)
    assert seen[-1] is False


def test_reference_glue_under_flag(ext, oracle):
    """rroi_align_backward_cuda (the reference's FFI name, adds into bottom_grad): under the flag, one torch add of the
    ORDERED gradient -- float32(base) + oracle exactly."""
    f, r = Wk.bench_inputs(R=64, C=64, H=64, W=96, img=384, seed=12)
    g = np.random.default_rng(4).standard_normal((64, 64, 8, 64)).astype(np.float32)
    want = oracle.backward_c(g, r, f.shape, 0.25, threads=8)
    base = np.random.default_rng(5).standard_normal(f.shape).astype(np.float32)
    G, Rr = torch.from_numpy(g).cuda(), torch.from_numpy(r).cuda()
    ix = torch.zeros(64, 64, 8, 64, device="cuda")
    iy = torch.zeros_like(ix)
    for _ in range(2):
        bottom = torch.from_numpy(base).cuda()
        with torch_deterministic(True):
            assert ext.rroi_align_backward_cuda(8, 64, 0.25, G, Rr, bottom, ix, iy) == 1
        got = bottom.cpu().numpy()
        assert same(got, base + want), diff(got, base + want)
