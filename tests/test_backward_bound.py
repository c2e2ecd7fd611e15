"""CPU: the per-element backward bound (workloads.check_backward_elementwise on oracle.backward_bound_c) -- its data
agree with the oracle's backward, and it catches a bug that the max-relative bar of check_backward lets through."""
import numpy as np
import pytest

import workloads as Wk


def heavy_overlap(seed=77):
    """test_backward_heavy_overlap's first problem, with fewer channels: hundreds of ROIs on the same few pixels."""
    rng = np.random.default_rng(seed)
    R, C, H, W, ph, pw, B = 600, 2, 24, 40, 8, 24, 1
    rois = np.zeros((R, 6), np.float32)
    rois[:, 1] = (W / 2 + rng.uniform(-3, 3, R)) * 4
    rois[:, 2] = (H / 2 + rng.uniform(-3, 3, R)) * 4
    rois[:, 3] = rng.uniform(8, 40, R)
    rois[:, 4] = rois[:, 3] * rng.uniform(1, 4, R)
    rois[:, 5] = rng.uniform(-90, 90, R)
    rois[: R // 3] = rois[0]
    gout = rng.standard_normal((R, C, ph, pw), dtype=np.float32)
    return gout, rois, (B, C, H, W)


def test_bound_data_match_the_oracle(oracle):
    """n = 0 exactly where the oracle's gradient is exactly 0 by construction, |want| <= S, the thread count does not
    matter, and the oracle's own gradient passes its bound with room to spare."""
    gout, rois, shape = heavy_overlap()
    want = oracle.backward_c(gout, rois, shape, 0.25)
    S, n = oracle.backward_bound_c(gout, rois, shape, 0.25, threads=1)
    S4, n4 = oracle.backward_bound_c(gout, rois, shape, 0.25, threads=4)
    assert np.array_equal(S, S4) and np.array_equal(n, n4)
    assert (want[n == 0] == 0).all() and n.max() > 1000
    assert (np.abs(want) <= S * (1 + 2 ** -23)).all()
    assert Wk.check_backward_elementwise(want, want, S, n, what="oracle vs itself") == 0.0
    # an fp32 sum in another order (the library's atomics) stays inside: the oracle's float32 literal backward
    out, ix, iy = oracle.forward_literal_c(np.zeros(shape, np.float32), rois, 8, 24, 0.25)
    lit = oracle.backward_literal_c(gout, rois, ix, iy, shape, 0.25)
    Wk.check_backward_elementwise(lit, want, S, n, what="fp32 literal order")
    # and the accumulating form: the existing value is one more term
    base = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    Wk.check_backward_elementwise((base + lit).astype(np.float32), base.astype(np.float64) + want, S, n, extra=base,
                                  what="accumulate")


def test_bound_catches_one_dropped_term(oracle):
    """Remove ONE term from a pixel whose gradient is ~1e-3 of the largest: check_backward(require_abs=False) -- the
    1e-4 x max|grad| bar of the heavy-overlap tests -- still passes; the per-element bound fails."""
    gout, rois, shape = heavy_overlap()
    want = oracle.backward_c(gout, rois, shape, 0.25)
    S, n = oracle.backward_bound_c(gout, rois, shape, 0.25)
    scale = float(np.abs(want).max())
    _, geom = oracle.forward_c(np.zeros(shape, np.float32), rois, 8, 24, 0.25, return_geom=True)
    cx, cy = geom[..., 0], geom[..., 1]
    half = (cx != np.floor(cx)) & (cy != np.floor(cy))   # all four taps distinct, each of weight 1/4
    for b, c, y, x in np.argwhere((n >= 4) & (np.abs(want) > 5e-4 * scale) & (np.abs(want) < 2e-3 * scale)):
        hit = half & ((np.floor(cx) == x) | (np.ceil(cx) == x)) & ((np.floor(cy) == y) | (np.ceil(cy) == y))
        hit &= (rois[:, 0].astype(int) == b)[:, None, None]
        if not hit.any():
            continue
        r, ph, pw = np.argwhere(hit)[0]
        # that bin's gradient set so that its term on (y, x) is 4e-5 of the scale: several times the element's own bound,
        # 0.4 of the old bar
        g1 = gout.copy()
        g1[r, c, ph, pw] = np.float32(4 * 4e-5 * scale)
        want = oracle.backward_c(g1, rois, shape, 0.25)
        S, n = oracle.backward_bound_c(g1, rois, shape, 0.25)
        g2 = g1.copy()
        g2[r, c, ph, pw] = 0.0
        got = oracle.backward_c(g2, rois, shape, 0.25)
        S2, _ = oracle.backward_bound_c(g2, rois, shape, 0.25)
        if not abs(S[b, c, y, x] - S2[b, c, y, x] - 4e-5 * scale) < 1e-3 * 4e-5 * scale:
            continue                                # the tap fails a border test: not a term of this pixel
        assert (S2 != S).sum() <= 4                 # one term on each of at most four pixels
        d = abs(float(got[b, c, y, x]) - float(want[b, c, y, x]))
        bound = float(Wk.backward_bound(S, n, want)[b, c, y, x])
        print(f"pixel {(b, c, y, x)}: |grad| {abs(want[b, c, y, x]):.3e} = {abs(want[b, c, y, x]) / scale:.1e} of max "
              f"{scale:.3g}, n = {n[b, c, y, x]}, dropped term {d:.3e}, its bound {bound:.3e}")
        assert d > 5 * bound
        Wk.check_backward(got, want, "one term dropped", require_abs=False)   # the old bar: passes
        with pytest.raises(AssertionError, match="beyond their bound"):
            Wk.check_backward_elementwise(got, want, S, n, what="one term dropped")
        return
    pytest.fail("no pixel with a single droppable term")


def test_tiny_maps_get_no_gradient_on_their_border(oracle):
    """The border tests of the backward (kernel.cu:267-274) reject every tap on row 0, row H - 1, column 0 and column
    W - 1: a map with H <= 2 or W <= 2 gets no gradient at all, a 3 x 3 map on pixel (1, 1) only -- what
    test_backward_tiny_maps_every_path (tests/test_gpu_parity.py) holds every backward path to."""
    rng = np.random.default_rng(78)
    some = 0
    for (H, W) in Wk.TINY_MAPS:
        shape = (2, 3, H, W)
        r = Wk.tiny_map_rois(rng, H, W)
        for (ph, pw) in Wk.TINY_POOLED:
            gout = rng.standard_normal((len(r), 3, ph, pw), dtype=np.float32)
            want = oracle.backward_c(gout, r, shape, 1.0)
            _, n = oracle.backward_bound_c(gout, r, shape, 1.0)
            inner = np.zeros(shape, bool)
            inner[:, :, 1:-1, 1:-1] = True
            assert not n[~inner].any() and not want[~inner].any(), (H, W, ph, pw)
            assert (H > 2 and W > 2) or not n.any()
            some += int((n > 0).sum())
    assert some > 0
