"""GPU (MI355X): every case of the dispatch table (tests/plan_cases.py) -- the plan the library reports for it, the call
itself, and the oracle: the forward bit-exact (NaN for NaN), the backward within the per-element bound of
workloads.check_backward_elementwise.  Then coverage again, over the plans that actually ran."""
import numpy as np
import pytest
import torch

import plan_cases as PC
import workloads as Wk

pytestmark = pytest.mark.gpu

RAN = {}     # case name -> (plan key, max error)


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_forward(ext, oracle, case):
    f, r = PC.inputs(case)
    F, Rr = dev(f), dev(r)
    if case.fl == PC.NHWC:
        F = F.contiguous(memory_format=torch.channels_last)
    R, C, ph, pw = case.R, case.C, case.ph, case.pw
    if case.caller == PC.NATIVE:
        got = ext.forward(F, Rr, ph, pw, PC.SCALE, path=case.path, channels_last_out=case.tl == PC.NHWC)
        assert got.is_contiguous(memory_format=torch.channels_last if case.tl == PC.NHWC else torch.contiguous_format)
        if case.gen == "beyond":   # > 320 MB of crops: the oracle on a sample of ROIs, the rest against the direct path
            direct = ext.forward(F, Rr, ph, pw, PC.SCALE, path=ext.PATH_DIRECT)
            assert torch.equal(got.view(torch.int32), direct.view(torch.int32))
            del direct
            pick = np.sort(np.random.default_rng(1).choice(R, 48, replace=False))
            want = oracle.forward_c(f, r[pick], ph, pw, PC.SCALE, threads=16)
            assert eq(got[torch.from_numpy(pick).cuda()].cpu().numpy(), want)
            return 0.0
        want = oracle.forward_c(f, r, ph, pw, PC.SCALE, threads=16)
        g = got.cpu().numpy()
        assert eq(g, want), f"{case.name}: {int((~((g == want) | (np.isnan(g) & np.isnan(want)))).sum())} elements differ"
        return 0.0
    # the reference-ABI launcher: (B, C, H, W) features of two images, ROIs of both; no batch count in the signature
    assert set(r[:, 0].astype(int)) == set(range(case.B))
    out = torch.full((R, C, ph, pw), 7.0, device="cuda")
    if case.gen == "beyond":   # > 320 MB of crops: the direct path on all of it, the literal oracle on a sample of ROIs
        pick = np.sort(np.random.default_rng(1).choice(R, 48, replace=False))
        want, wx, wy = oracle.forward_literal_c(f, r[pick], ph, pw, PC.SCALE)
        idx = torch.from_numpy(pick).cuda()
        if case.caller == PC.LAUNCHER_CON_IDX:
            ix, iy = torch.full_like(out, 7.0), torch.full_like(out, 7.0)
            assert ext.rroi_align_forward_cuda(ph, pw, PC.SCALE, F, Rr, out, ix, iy) == 1
            assert eq(ix[idx].cpu().numpy(), wx) and eq(iy[idx].cpu().numpy(), wy)
            del ix, iy
        else:
            assert ext._lib.RROIAlignForwardLaucher(F.data_ptr(), PC.SCALE, R, case.H, case.W, C, ph, pw, Rr.data_ptr(),
                                                    out.data_ptr(), None, None, stream()) == 1
        assert out.numel() * 4 > (320 << 20)
        assert eq(out[idx].cpu().numpy(), want)
        direct = ext.forward(F, Rr, ph, pw, PC.SCALE, path=ext.PATH_DIRECT)
        assert torch.equal(out.view(torch.int32), direct.view(torch.int32))
        return 0.0
    want, wx, wy = oracle.forward_literal_c(f, r, ph, pw, PC.SCALE)
    if case.caller == PC.LAUNCHER_CON_IDX:
        ix, iy = torch.full_like(out, 7.0), torch.full_like(out, 7.0)
        assert ext.rroi_align_forward_cuda(ph, pw, PC.SCALE, F, Rr, out, ix, iy) == 1
        assert eq(ix.cpu().numpy(), wx) and eq(iy.cpu().numpy(), wy)
    else:
        assert ext._lib.RROIAlignForwardLaucher(F.data_ptr(), PC.SCALE, R, case.H, case.W, C, ph, pw, Rr.data_ptr(),
                                                out.data_ptr(), None, None, stream()) == 1
    assert eq(out.cpu().numpy(), want)
    return 0.0


def run_backward(ext, oracle, case, plan):
    f, r = PC.inputs(case)
    R, C, ph, pw = case.R, case.C, case.ph, case.pw
    gout = np.random.default_rng(7).standard_normal((R, C, ph, pw)).astype(np.float32)
    want = oracle.backward_c(gout, r, f.shape, PC.SCALE, threads=16)
    S, n = oracle.backward_bound_c(gout, r, f.shape, PC.SCALE, threads=16)
    if case.name == "b_buckets_chains":   # some pixel's list is longer than its bucket: the overflow chains are walked
        longest = int(distinct_bins_per_pixel(oracle, f.shape, r, ph, pw).max())
        assert longest > (1 << plan.kshift), (longest, plan.kshift)
    if case.name == "b_lists_scan2_carry":   # more than 1024 scan blocks, lists on both sides of the second round
        PC.assert_scan2_carries(case, plan, n)
    G, Rr = dev(gout), dev(r)
    if case.caller == PC.NATIVE:
        if case.fl == PC.NHWC:
            G = G.contiguous(memory_format=torch.channels_last)
        got = ext.backward(G, Rr, f.shape, PC.SCALE, path=case.path, channels_last_grad=case.tl == PC.NHWC)
        assert got.is_contiguous(memory_format=torch.channels_last if case.tl == PC.NHWC else torch.contiguous_format)
        got, base = got.cpu().numpy(), 0
    else:   # the launcher ADDS to bottom_diff: a non-zero one; con_idx from the launcher's own forward
        out, ix, iy = (torch.empty((R, C, ph, pw), device="cuda") for _ in range(3))
        assert ext.rroi_align_forward_cuda(ph, pw, PC.SCALE, dev(f), Rr, out, ix, iy) == 1
        base = np.random.default_rng(8).standard_normal(f.shape).astype(np.float32)
        gin = dev(base)
        assert ext.rroi_align_backward_cuda(ph, pw, PC.SCALE, G, Rr, gin, ix, iy) == 1
        got = gin.cpu().numpy()
        want = base.astype(np.float64) + want
    Wk.check_backward(got, want, case.name, require_abs=False)
    Wk.check_backward_elementwise(got, want, S, n, extra=base, what=case.name)
    return float(np.abs(got - want).max())


def distinct_bins_per_pixel(oracle, shape, r, ph, pw):
    """Per (image, y, x): the number of distinct bins with a tap there that passes the backward's border tests
    (kernel.cu:267-274).  A pixel's list holds at least one entry per such bin -- a lower bound of the list length
    that does not depend on whether the library keeps coinciding taps of one bin (integral centres) as one entry or
    several, unlike the oracle's per-element term count n."""
    B, _, H, W = shape
    _, geom = oracle.forward_c(np.zeros((B, 1, H, W), np.float32), r, ph, pw, PC.SCALE, return_geom=True)
    cx, cy = geom[..., 0].reshape(-1).astype(np.float64), geom[..., 1].reshape(-1).astype(np.float64)
    x0, x1, y0, y1 = np.floor(cx), np.ceil(cx), np.floor(cy), np.ceil(cy)   # masked bins: (0, 0), which fails every test
    img = np.repeat(r[:, 0].astype(np.int64), ph * pw)
    bins = np.arange(cx.size)
    taps = []
    for yy, xx, ok in ((y0, x0, (y0 > 0) & (x0 > 0) & (y0 < H - 1) & (x0 < W - 1)),
                       (y0, x1, (y0 > 0) & (x1 < W - 1) & (y0 < H - 1) & (x1 > 0)),
                       (y1, x1, (y1 < H - 1) & (x1 < W - 1) & (y1 > 0) & (x1 > 0)),
                       (y1, x0, (y1 < H - 1) & (x0 > 0) & (y1 > 0) & (x0 < W - 1))):
        px = (img * H + yy.astype(np.int64)) * W + xx.astype(np.int64)
        taps.append(np.stack([bins[ok], px[ok]], 1))
    pairs = np.unique(np.concatenate(taps), axis=0)
    return np.bincount(pairs[:, 1], minlength=B * H * W)


@pytest.mark.parametrize("case", PC.CASES, ids=[c.name for c in PC.CASES])
def test_case(ext, oracle, case):
    plan = PC.plan_of(ext, case)
    k = PC.key(case.kind, plan, case.caller)
    err = run_forward(ext, oracle, case) if case.kind == "fwd" else run_backward(ext, oracle, case, plan)
    torch.cuda.synchronize()
    RAN[case.name] = (k, err)


def test_coverage_of_the_plans_that_ran():
    if not RAN:
        pytest.skip("no case of test_case ran in this session (run the whole file): nothing to check coverage over")
    print("\ncase -> plan -> max |error|")
    for name, (k, err) in RAN.items():
        print(f"  {name:30s} {' '.join(str(v) for v in k[1:]):70s} {err:.3e}")
    ran = {k for k, _ in RAN.values()}
    missing = PC.REQUIRED - ran
    not_run = [c.name for c in PC.CASES if c.name not in RAN]
    assert not missing, f"required plans that no passing case ran: {sorted(missing)} (cases that did not run: {not_run})"
