"""GPU (MI355X): the seeded fuzz of tools/fuzz_gpu.py in the suite -- random problems with degenerate and non-finite
ROIs, bad batch indices, rounding ties, and channel / pooled sizes at awkward residues.  Every forward path (plus NHWC
features and NHWC crops where C % 4 == 0) bit-exact against the oracle; every backward path within the per-element
bound; the reference-ABI launchers too (forward with con_idx, backward adding to a non-zero bottom_diff), on the ROIs
with their bad batch indices replaced -- the launchers trust the index, as the reference does.  The histogram of the
plans that ran must span the direct (K2p), fused and two-launch forwards and every backward family.  The direct
forward's thread-per-bin fallback runs on maps one pixel wide only, which this generator never draws: the coverage
table (tests/plan_cases.py) runs it."""
import collections

import numpy as np
import pytest
import torch

import plan_cases as PC
import workloads as Wk

pytestmark = pytest.mark.gpu

TRIALS = 48
SEED = 7


def problem(rng, t):
    C = int(rng.choice([1, 2, 3, 4, 7, 8, 31, 32, 33, 40, 64, 65, 128, 257, 300]))
    H, W = int(rng.integers(2, 70)), int(rng.integers(2, 100))
    B = int(rng.integers(1, 5))
    ph = int(rng.choice([1, 2, 3, 7, 8, 11, 16]))
    pw = int(rng.integers(1, 100))
    s = float(rng.choice([1.0, 0.5, 0.25, 0.125, 0.3]))
    R = int(rng.integers(1, 60))
    f, r = Wk.bench_inputs(R=R, C=C, H=H, W=W, img=max(4, int(W / s)), seed=5000 + t, batch=B)
    r[:, 2] = rng.uniform(-5, H / s + 5, R)
    r[:, 1] = rng.uniform(-5, W / s + 5, R)
    r[:, 3] = rng.uniform(0.5, 60, R) / (s * 4)
    r[:, 4] = r[:, 3] * rng.uniform(0.1, 20, R)
    kind = rng.integers(0, 12, R)
    r[kind == 0, 5] = rng.choice([0.0, 90.0, -90.0, 180.0, 45.0], int((kind == 0).sum()))
    r[kind == 1, 0] = rng.choice([-1.0, float(B), float(B) + 3.0], int((kind == 1).sum()))  # bad batch index
    r[kind == 2, 3] = 0.0
    r[kind == 3, 4] = 0.0
    r[kind == 4, 1:3] = np.round(r[kind == 4, 1:3] * s) / s  # integer feature-space centres: rounding ties
    if rng.random() < 0.1:
        r[int(rng.integers(0, R)), int(rng.integers(1, 6))] = rng.choice([np.nan, np.inf, -np.inf, 1e30])
    return f, r, ph, pw, s


def test_seeded_fuzz(oracle):
    from rroi_align._ext import rroi_align as ext
    rng = np.random.default_rng(SEED)
    hist = collections.Counter()
    fails = []
    eq = lambda a, b: np.array_equal(a, b, equal_nan=True)
    for t in range(TRIALS):
        f, r, ph, pw, s = problem(rng, t)
        B, C, H, W = f.shape
        R = len(r)
        what = f"trial {t}: C={C} {H}x{W} B={B} {ph}x{pw} s={s} R={R}"
        # an out-of-range batch index is undefined behaviour in the reference (and in the oracle, which follows it);
        # the library defines zeros / no gradient for such ROIs
        bi = r[:, 0]
        badb = ~((bi > -1) & (bi < B))   # (int) truncation: -0.5 -> 0 is valid
        r_o = r.copy()
        r_o[badb, 0] = 0
        want = oracle.forward_c(f, r_o, ph, pw, s, threads=16)
        want[badb] = 0
        F, Rr = torch.from_numpy(f).cuda(), torch.from_numpy(r).cuda()
        legs = [(p, False, False) for p in (ext.PATH_DIRECT, ext.PATH_TILED, ext.PATH_FUSED, ext.PATH_AUTO)]
        if C % 4 == 0:
            legs += [(ext.PATH_AUTO, True, False), (ext.PATH_AUTO, False, True), (ext.PATH_AUTO, True, True)]
        for p, cl_src, cl_out in legs:
            src = F.contiguous(memory_format=torch.channels_last) if cl_src else F
            # the layout the wrapper passes: NCHW where the tensor is contiguous in both formats (H = W = 1)
            fl = int(cl_src and not src.is_contiguous())
            plan = ext.forward_plan(B, C, H, W, R, ph, pw, feature_layout=fl, top_layout=int(cl_out), path=p)
            hist[PC.key("fwd", plan, 0)[1:]] += 1
            got = ext.forward(src, Rr, ph, pw, s, path=p, channels_last_out=cl_out).cpu().numpy()
            if not eq(got, want):
                fails.append(f"FWD {what} path {p} cl_src {cl_src} cl_out {cl_out}")
        gout = np.random.default_rng(t).standard_normal(want.shape).astype(np.float32)
        gout_o = gout.copy()
        gout_o[badb] = 0
        gw = oracle.backward_c(gout_o, r_o, f.shape, s, threads=16)
        S, n = oracle.backward_bound_c(gout_o, r_o, f.shape, s, threads=16)
        G = torch.from_numpy(gout).cuda()
        legs = [(p, False, False) for p in (ext.PATH_DIRECT, ext.PATH_TILED, ext.PATH_TILED_LISTS, ext.PATH_TILED_BUCKETS,
                                            ext.PATH_TILED_INKERNEL, ext.PATH_TILED_ATOMIC, ext.PATH_AUTO)]
        if C % 4 == 0:
            legs += [(p, a, b) for p in (ext.PATH_AUTO, ext.PATH_TILED_LISTS, ext.PATH_TILED_INKERNEL)
                     for a, b in ((True, False), (False, True), (True, True))]
        for p, cl_td, cl_bd in legs:
            Gp = G.contiguous(memory_format=torch.channels_last) if cl_td else G
            td = int(cl_td and not Gp.is_contiguous())   # (PH = PW = 1: the wrapper passes NCHW)
            plan = ext.backward_plan(B, C, H, W, R, ph, pw, top_diff_layout=td, bottom_diff_layout=int(cl_bd), path=p)
            hist[PC.key("bwd", plan, 0)[1:]] += 1
            g = ext.backward(Gp, Rr, f.shape, s, path=p, channels_last_grad=cl_bd).cpu().numpy()
            try:
                Wk.check_backward_elementwise(g, gw, S, n, what=f"{what} path {p}")
            except AssertionError as e:
                fails.append(f"BWD {what} path {p} cl_td {cl_td} cl_bd {cl_bd}: {e}")
        # the reference-ABI launchers on the ROIs with valid batch indices
        Ro = torch.from_numpy(r_o).cuda()
        lw, lx, ly = oracle.forward_literal_c(f, r_o, ph, pw, s)
        out, ix, iy = (torch.full(want.shape, 7.0, device="cuda") for _ in range(3))
        hist[PC.key("fwd", ext.forward_plan(B, C, H, W, R, ph, pw, caller=ext.CALLER_LAUNCHER_CON_IDX), 2)[1:]] += 1
        assert ext.rroi_align_forward_cuda(ph, pw, s, F, Ro, out, ix, iy) == 1
        if not (eq(out.cpu().numpy(), lw) and eq(ix.cpu().numpy(), lx) and eq(iy.cpu().numpy(), ly)):
            fails.append(f"FWD {what} launcher")
        lg = oracle.backward_c(gout, r_o, f.shape, s, threads=16)
        lS, ln = oracle.backward_bound_c(gout, r_o, f.shape, s, threads=16)
        base = np.random.default_rng(100 + t).standard_normal(f.shape).astype(np.float32)
        gin = torch.from_numpy(base).cuda()
        hist[PC.key("bwd", ext.backward_plan(B, C, H, W, R, ph, pw, caller=ext.CALLER_LAUNCHER), 1)[1:]] += 1
        assert ext.rroi_align_backward_cuda(ph, pw, s, G, Ro, gin, ix, iy) == 1
        try:
            Wk.check_backward_elementwise(gin.cpu().numpy(), base.astype(np.float64) + lg, lS, ln, extra=base,
                                          what=f"{what} launcher")
        except AssertionError as e:
            fails.append(f"BWD {what} launcher: {e}")
    print("\nplan histogram:")
    for k, v in sorted(hist.items(), key=lambda kv: -kv[1]):
        print(f"  {v:5d}  {' '.join(str(x) for x in k)}")
    assert not fails, "\n".join(fails[:20])
    fams = {k[1] for k in hist}
    assert {"k2p", "two_launch"} <= fams and fams & {"fused_strided", "fused_shift"}, fams
    assert {"direct", "atomic", "inkernel", "lists", "buckets", "literal"} <= fams, fams
