"""GPU (MI355X): bfloat16 / float16 features, crops, grad_output and gradients (0.10.0).

The contract: a 16-bit forward widens every map element exactly, runs the fp32 arithmetic unchanged and rounds each crop
element once -- bit for bit the oracle's fp32 crops of the widened map rounded by torch (NaN for NaN), and the fp32 call
on the widened map rounded.  A 16-bit backward sums each gradient element in fp32 and rounds it once: the fp32
per-element bound of workloads.check_backward_elementwise plus one rounding.  Every case of tests/half_cases.py runs in
both dtypes and records its plan; the last test fails if a HALF_REQUIRED key did not run."""
import numpy as np
import pytest
import torch

import half_cases as HC
import plan_cases as PC
import workloads as Wk

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float16)
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}               # unit roundoff of one rounding
TINY = {torch.bfloat16: 2.0 ** -133 / 2, torch.float16: 2.0 ** -24 / 2}   # half the smallest subnormal
RAN = {}   # (dtype, case name) -> plan key


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, want):
    """Every element: the same bits, or both NaN."""
    g, w = got.cpu(), want.cpu()
    assert g.dtype == w.dtype and g.shape == w.shape
    ok = (g.view(torch.int16) == w.view(torch.int16)) | (g.isnan() & w.isnan())
    return int((~ok).sum())


def oracle_rounded(oracle, f_wide, r, ph, pw, scale, dtype):
    return torch.from_numpy(oracle.forward_c(f_wide, r, ph, pw, scale, threads=16)).to(dtype)


def check_half_backward(got, want, S, n, dtype, what):
    """|got - want| <= b + u (|want| + b), b = the fp32 bound of the same element, plus half the smallest subnormal;
    +-inf is accepted where |want| + bound exceeds the float16 range."""
    g = got.float().cpu().numpy().astype(np.float64)
    w = np.asarray(want, np.float64)
    assert (np.isnan(g) == np.isnan(w)).all(), (what, "NaN where the oracle has none, or the reverse")
    inf_w = np.isinf(w)
    assert (g[inf_w] == w[inf_w]).all(), (what, "an infinite element differs")
    fin = np.isfinite(w)
    b = Wk.backward_bound(S, n, np.where(fin, w, 0.0), 0)
    bound = b + U[dtype] * (np.abs(w) + b) + TINY[dtype]
    err = np.abs(g - w)
    over_range = np.isinf(g) & (np.sign(g) == np.sign(w)) & (np.abs(w) + bound >= 65504.0) & (dtype == torch.float16)
    bad = fin & ~(err <= bound) & ~over_range
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements beyond their bound; first {i}: got {g[i]!r} want {w[i]!r} "
                             f"bound {bound[i]:.3e}")
    keep = fin & ~over_range
    return float((err[keep] / bound[keep]).max()) if keep.any() else 0.0


def run_case(ext, oracle, case, dtype):
    f, r = PC.inputs(case)
    Fh = dev(f).to(dtype)
    f_wide = Fh.float().cpu().numpy()
    Rr = dev(r)
    R, C, ph, pw = case.R, case.C, case.ph, case.pw
    if case.kind == "fwd":
        got = ext.forward(Fh, Rr, ph, pw, PC.SCALE, path=case.path, channels_last_out=case.tl == PC.NHWC)
        assert got.dtype == dtype
        assert got.is_contiguous(memory_format=torch.channels_last if case.tl == PC.NHWC else torch.contiguous_format)
        # the fp32 call on the widened map, rounded: every element
        ref = ext.forward(Fh.float(), Rr, ph, pw, PC.SCALE, path=case.path if case.path != PC.FUSED else PC.AUTO).to(dtype)
        assert same_bits(got, ref) == 0, case.name
        del ref
        if case.gen == "beyond":   # hundreds of MB of crops: the oracle on a sample of ROIs
            pick = np.sort(np.random.default_rng(1).choice(R, 48, replace=False))
            want = oracle_rounded(oracle, f_wide, r[pick], ph, pw, PC.SCALE, dtype)
            assert same_bits(got[torch.from_numpy(pick).cuda()], want) == 0, case.name
        else:
            assert same_bits(got, oracle_rounded(oracle, f_wide, r, ph, pw, PC.SCALE, dtype)) == 0, case.name
        return
    gout = torch.from_numpy(np.random.default_rng(7).standard_normal((R, C, ph, pw)).astype(np.float32)).to(dtype)
    g_wide = gout.float().numpy()
    want = oracle.backward_c(g_wide, r, f.shape, PC.SCALE, threads=16)
    S, n = oracle.backward_bound_c(g_wide, r, f.shape, PC.SCALE, threads=16)
    got = ext.backward(gout.cuda(), Rr, f.shape, PC.SCALE, path=case.path, channels_last_grad=case.tl == PC.NHWC)
    assert got.dtype == dtype
    assert got.is_contiguous(memory_format=torch.channels_last if case.tl == PC.NHWC else torch.contiguous_format)
    check_half_backward(got, want, S, n, dtype, f"{case.name} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", HC.HALF_CASES, ids=[c.name for c in HC.HALF_CASES])
def test_case(ext, oracle, case, dtype):
    k = HC.key_of(ext, case, dtype)
    run_case(ext, oracle, case, dtype)
    torch.cuda.synchronize()
    RAN[(dtype, case.name)] = k


def test_cfg1_forward_bf16_full_size_bit_exact(ext, oracle):
    f, r = Wk.bench_inputs()
    Fh = dev(f).to(torch.bfloat16)
    got = ext.forward(Fh, dev(r), 8, 64, 0.25)
    want = oracle_rounded(oracle, Fh.float().cpu().numpy(), r, 8, 64, 0.25, torch.bfloat16)
    assert same_bits(got, want) == 0
    for p in (ext.PATH_TILED, ext.PATH_DIRECT):
        assert torch.equal(ext.forward(Fh, dev(r), 8, 64, 0.25, path=p).view(torch.int16), got.view(torch.int16))


def test_cfg2_backward_bf16_within_bound(ext, oracle):
    f, r = Wk.bench_inputs()
    g = torch.from_numpy(np.random.default_rng(3).standard_normal((512, 256, 8, 64)).astype(np.float32)).to(torch.bfloat16)
    gw = g.float().numpy()
    want = oracle.backward_c(gw, r, f.shape, 0.25, threads=16)
    S, n = oracle.backward_bound_c(gw, r, f.shape, 0.25, threads=16)
    for p in (ext.PATH_AUTO, ext.PATH_TILED_LISTS, ext.PATH_TILED_INKERNEL):
        got = ext.backward(g.cuda(), dev(r), f.shape, 0.25, path=p)
        check_half_backward(got, want, S, n, torch.bfloat16, f"configs[2] path {p}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_non_finite_edge_degenerate_and_channel_counts(ext, oracle, dtype):
    rng = np.random.default_rng(11)
    rois = np.concatenate([Wk.edge_rois(), Wk.degenerate_rois(), Wk.bench_inputs(R=40, C=1)[1]])
    for C in (3, 33, 64):
        f = rng.standard_normal((1, C, 160, 160)).astype(np.float32) * 300.0   # beyond float16 range once summed
        flat = f.reshape(-1)
        idx = rng.choice(flat.size, 200, replace=False)
        flat[idx[:80]] = np.nan
        flat[idx[80:140]] = np.inf
        flat[idx[140:]] = -np.inf
        Fh = dev(f).to(dtype)
        fw = Fh.float().cpu().numpy()
        for trig in (ext.TRIG_DOUBLE, ext.TRIG_FP32):
            for p in (ext.PATH_AUTO, ext.PATH_DIRECT, ext.PATH_TILED):
                got = ext.forward(Fh, dev(rois), 8, 64, 0.25, path=p, trig=trig)
                ref = ext.forward(Fh.float(), dev(rois), 8, 64, 0.25, path=p, trig=trig).to(dtype)
                assert same_bits(got, ref) == 0, (C, trig, p)
                if trig == ext.TRIG_DOUBLE:
                    assert same_bits(got, oracle_rounded(oracle, fw, rois, 8, 64, 0.25, dtype)) == 0, (C, p)
        # backward of the same ROIs (finite gradients), both destinations
        g = torch.from_numpy(rng.standard_normal((len(rois), C, 8, 64)).astype(np.float32)).to(dtype)
        want = oracle.backward_c(g.float().numpy(), rois, f.shape, 0.25, threads=16)
        S, n = oracle.backward_bound_c(g.float().numpy(), rois, f.shape, 0.25, threads=16)
        for p in (ext.PATH_AUTO, ext.PATH_TILED_LISTS, ext.PATH_TILED_INKERNEL, ext.PATH_TILED_BUCKETS):
            got = ext.backward(g.cuda(), dev(rois), f.shape, 0.25, path=p)
            check_half_backward(got, want, S, n, dtype, f"C={C} path {p}")
            if C % 4 == 0:
                got = ext.backward(g.cuda(), dev(rois), f.shape, 0.25, path=p, channels_last_grad=True)
                check_half_backward(got, want, S, n, dtype, f"C={C} path {p} nhwc")


def test_r0_and_negative_zero(ext):
    for dtype in DTYPES:
        F = torch.randn(2, 8, 16, 16, device="cuda").to(dtype)
        R = torch.zeros(0, 6, device="cuda")
        assert ext.forward(F, R, 4, 8, 0.25).shape == (0, 8, 4, 8)
        gin = ext.backward(torch.zeros(0, 8, 4, 8, device="cuda", dtype=dtype), R, F.shape, 0.25)
        assert gin.dtype == dtype and gin.shape == F.shape and not gin.view(torch.int16).any()
        # a map of -0.0: the crops keep the sign bit where the fp32 call does
        Z = torch.full((1, 8, 16, 16), -0.0, device="cuda", dtype=dtype)
        rois = torch.tensor([[0, 30, 30, 10, 40, 20.0]], device="cuda")
        got = ext.forward(Z, rois, 4, 16, 0.25)
        assert torch.equal(got.view(torch.int16), ext.forward(Z.float(), rois, 4, 16, 0.25).to(dtype).view(torch.int16))


def test_autograd_outside_autocast(ext):
    from rroi_align.modules.rroi_align import _RRoiAlign
    from rroi_align.functions.rroi_align import RRoiAlignFunction
    f, r = Wk.bench_inputs(R=24, C=32, H=40, W=60, img=240, seed=77)
    R = dev(r)
    op = _RRoiAlign(8, 32, 0.25)
    for dtype in DTYPES:
        Fh = dev(f).to(dtype).requires_grad_(True)
        out = op(Fh, R)
        assert out.dtype == dtype
        F32 = Fh.detach().float().requires_grad_(True)
        o32 = op(F32, R)
        assert torch.equal(out.view(torch.int16), o32.to(dtype).view(torch.int16))
        g = torch.randn_like(o32).to(dtype)
        out.backward(g)
        o32.backward(g.float())
        assert Fh.grad.dtype == dtype and Fh.grad.shape == Fh.shape
        assert torch.allclose(Fh.grad.float(), F32.grad, rtol=2 * U[dtype], atol=1e-5 * float(F32.grad.abs().max()))
        # the legacy methods follow the features' dtype too
        fn = RRoiAlignFunction(8, 32, 0.25)
        assert fn.forward(Fh.detach(), R).dtype == dtype
        assert fn.backward(g)[0].dtype == dtype
    # a channels_last bf16 backbone: channels_last features and grad_output, channels_last crops
    Fh = dev(f).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    opc = _RRoiAlign(8, 32, 0.25, channels_last_out=True)
    out = opc(Fh, R)
    assert out.dtype == torch.bfloat16 and out.is_contiguous(memory_format=torch.channels_last)
    F32 = Fh.detach().float().requires_grad_(True)
    o32 = _RRoiAlign(8, 32, 0.25)(F32, R)
    assert torch.equal(out.contiguous().view(torch.int16), o32.to(torch.bfloat16).view(torch.int16))
    g = torch.randn_like(o32).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    out.backward(g)
    o32.backward(g.float())
    assert Fh.grad.dtype == torch.bfloat16 and Fh.grad.is_contiguous(memory_format=torch.channels_last)
    assert torch.allclose(Fh.grad.float(), F32.grad, rtol=2 ** -7, atol=1e-5 * float(F32.grad.abs().max()))


def test_graph_capture_and_replay(ext):
    f, r = Wk.bench_inputs(R=128, C=64, H=120, W=160, img=640, seed=5)
    F, R = dev(f).to(torch.bfloat16), dev(r)
    g = torch.randn(128, 64, 8, 64, device="cuda").to(torch.bfloat16)
    want_f = ext.forward(F, R, 8, 64, 0.25)
    want_b = ext.backward(g, R, F.shape, 0.25)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm the workspace cache on the capture stream
        ext.forward(F, R, 8, 64, 0.25)
        ext.backward(g, R, F.shape, 0.25)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_f = ext.forward(F, R, 8, 64, 0.25)
        out_b = ext.backward(g, R, F.shape, 0.25)
    out_f.zero_()
    out_b.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_f.view(torch.int16), want_f.view(torch.int16))
    assert torch.equal(out_b.view(torch.int16), want_b.view(torch.int16))


def test_validation(ext):
    F = torch.zeros(1, 4, 16, 16, device="cuda")
    R = torch.zeros(2, 6, device="cuda")
    with pytest.raises(TypeError):
        ext.forward(F.double(), R, 8, 8, 1.0)
    for dtype in DTYPES:
        with pytest.raises(TypeError):
            ext.forward(F.to(dtype), R.to(dtype), 8, 8, 1.0)
        with pytest.raises(TypeError):
            ext.backward(torch.zeros(2, 4, 8, 8, device="cuda", dtype=dtype), R.double(), F.shape, 1.0)
        with pytest.raises(ValueError):
            ext.forward(F.to(dtype), R, 8, 8, 1.0, path=ext.PATH_FUSED)
        with pytest.raises(ValueError):
            ext.backward(torch.zeros(2, 4, 8, 8, device="cuda", dtype=dtype), R, F.shape, 1.0, path=ext.PATH_DIRECT)
        with pytest.raises(ValueError):
            ext.backward(torch.zeros(2, 4, 8, 8, device="cuda", dtype=dtype), R, F.shape, 1.0,
                         path=ext.PATH_TILED_ATOMIC)


def test_coverage_of_the_plans_that_ran():
    if not RAN:
        pytest.skip("no case of test_case ran in this session (run the whole file): nothing to check coverage over")
    for dtype in DTYPES:
        ran = {k for (dt, _), k in RAN.items() if dt == dtype}
        missing = set(HC.HALF_REQUIRED) - ran
        assert not missing, (dtype, sorted(missing))
