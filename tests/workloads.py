"""Seeded synthetic inputs shared by the tests."""
import numpy as np


def bench_inputs(R=512, C=256, H=160, W=160, img=640, seed=0, all_active=False,
                 axis_aligned=False, batch=1):
    """BASELINE.json configs[1..3]: features ~ N(0,1); ROIs in img x img pixels,
    cx,cy ~ U[0,img), h ~ U[16,64), w = h*U[4,8), angle ~ U[-90,90)."""
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((batch, C, H, W), dtype=np.float32)
    cx = rng.uniform(0, img, R)
    cy = rng.uniform(0, img, R)
    h = rng.uniform(16, 64, R)
    ratio = np.full(R, 8.0) if all_active else rng.uniform(4, 8, R)
    w = h * ratio
    ang = np.zeros(R) if axis_aligned else rng.uniform(-90, 90, R)
    bidx = rng.integers(0, batch, R) if batch > 1 else np.zeros(R)
    rois = np.stack([bidx, cx, cy, h, w, ang], 1).astype(np.float32)
    return feats, rois


def cfg1_inputs(seed=0):
    """BASELINE.json configs[0]: 1x3x64x128 map, 4 rotated ROIs, pooled 8x32, scale 1."""
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((1, 3, 64, 128), dtype=np.float32)
    R = 4
    rois = np.stack([np.zeros(R), rng.uniform(0, 128, R), rng.uniform(0, 64, R),
                     rng.uniform(6, 20, R), rng.uniform(20, 80, R), rng.uniform(-90, 90, R)],
                    1).astype(np.float32)
    return feats, rois


def edge_rois(img_w=640, img_h=640):
    """ROIs that stress the reference's corner cases: outside the map on every side,
    straddling each border, 0/+-45/+-90/180 degrees, w/h < 1 and > 8, integer and
    half-integer centres (round() ties), batch index with a fractional part."""
    rows = []
    for ang in (0.0, 45.0, -45.0, 90.0, -90.0, 180.0, 30.0, -135.0):
        rows.append([0, img_w / 2, img_h / 2, 32, 200, ang])
    for cx, cy in ((-40, 100), (img_w + 40, 100), (100, -40), (100, img_h + 40),
                   (2, 2), (img_w - 2, img_h - 2), (0, 0), (img_w, img_h),
                   (-500, -500), (5000, 5000)):
        rows.append([0, cx, cy, 24, 150, 17.0])
    rows += [
        [0, 320, 320, 64, 32, 10],      # w/h < 1
        [0, 320, 320, 8, 200, -20],     # w/h = 25 >> pooled width ratio
        [0, 320, 320, 16, 128, 0],      # exactly w/h = 8
        [0, 320.5, 320.5, 16, 128, 0],  # half-integer centre
        [0, 100, 200, 40, 160, 90],     # ties at 90 degrees
        [0, 128, 256, 32, 256, 0],      # integer grid, scale .25 -> bin edges on integers
        [0.9, 300, 300, 20, 100, 5],    # batch index truncates to 0
        [0, 320, 320, 1, 4, 3],         # tiny
        [0, 320, 320, 600, 2400, 33],   # much larger than the map
    ]
    return np.asarray(rows, np.float32)


def degenerate_rois():
    """h == 0, w == 0, negative h, NaN / inf fields (SURVEY.md section 7 'Degenerate ROIs')."""
    nan, inf = float("nan"), float("inf")
    return np.asarray([
        [0, 320, 320, 0, 100, 10],
        [0, 320, 320, 20, 0, 10],
        [0, 320, 320, 0, 0, 10],
        [0, 320, 320, -20, 100, 10],
        [0, 320, 320, 20, -100, 10],
        [0, 320, 320, 20, 100, nan],
        [0, nan, 320, 20, 100, 10],
        [0, 320, inf, 20, 100, 10],
        [0, 320, 320, inf, 100, 10],
        [0, 320, 320, 20, inf, 10],
        [0, 1e30, 320, 20, 100, 10],
        [0, 320, 320, 1e-30, 1e30, 10],
    ], np.float32)


def tie_rois(img=640):
    """Rounding-tie stress (SURVEY.md 8c fixture 3): with h = 32, w = 256, pooled 8x64 and scale 0.25 the
    affine has unit steps (Sx = Sy = 1), so at 0 / 90 / 180 / -90 degrees and centres on the integer or
    half-integer grid of the map every bin corner is an exact integer or half-integer: round() sits
    on ties in every bin, and one ulp in the affine (e.g. from FMA contraction) flips the sample."""
    rows = []
    for ang in (0.0, 90.0, 180.0, -90.0, 45.0, -45.0, 30.0):
        for cx, cy in ((320, 320), (322, 318), (321, 321), (320.5, 320.5), (323, 320), (200, 440), (50, 50), (600, 30)):
            rows.append([0, cx, cy, 32, 256, ang])
    for h, w in ((16, 128), (64, 512), (24, 192), (40, 200)):
        rows.append([0, 320, 320, h, w, 0.0])
        rows.append([0, 320, 320, h, w, 90.0])
    return np.asarray(rows, np.float32)


# maps with fewer rows or columns than a key tile of the backward (4 x 8 pixels), down to one pixel
TINY_MAPS = ((1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (3, 2), (3, 3), (1, 7), (7, 1), (3, 9), (9, 3), (5, 4), (4, 5))
TINY_POOLED = ((2, 3), (3, 21), (8, 16))


def tiny_map_rois(rng, H, W, R=12, batch=2):
    """ROIs at scale 1 for an H x W map of TINY_MAPS, drawn as test_forward_tiny_maps_every_path draws them: centres from
    one pixel outside the map to one pixel outside, extents larger than the map, any angle of +-90 degrees."""
    return np.stack([rng.integers(0, batch, R), rng.uniform(-1, W + 1, R), rng.uniform(-1, H + 1, R), rng.uniform(0.5, 2 * H + 1, R),
                     rng.uniform(0.5, 3 * W + 1, R), rng.uniform(-90, 90, R)], 1).astype(np.float32)


def check_backward(got, want, what="", require_abs=True, rel=1e-4, abs_bar=1e-4):
    """The backward's bar.  BASELINE configs[2] says "autograd.Function parity <= 1e-4": asserted as a MAX-ABS bound
    wherever the data allow it (`require_abs`: cfg1 ... cfg3, the training shapes, smoke -- gradients of magnitude
    tens, sums of at most a few dozen fp32 terms per pixel, measured error 1e-6 ... 2e-5).  fp32 sums do not
    associate (the reference's own atomicAdds are unordered, kernel.cu:267-274), so the heavy-overlap cases -- lists
    of thousands of pairs on one pixel, gradients of magnitude thousands -- keep the bound RELATIVE to max |grad|
    only, and say so.  Prints both errors; returns (abs_err, rel_err)."""
    import numpy as _np
    g, w = _np.asarray(got, dtype=_np.float64), _np.asarray(want, dtype=_np.float64)
    err = float(_np.abs(g - w).max()) if g.size else 0.0
    scale = max(1.0, float(_np.abs(w).max())) if w.size else 1.0
    print(f"[backward parity] {what}: max-abs {err:.3e}, relative to max|grad| = {scale:.3g}: {err / scale:.3e}")
    assert err <= rel * scale, (what, err, scale)
    if require_abs:
        assert err <= abs_bar, (what, err, "absolute bar", abs_bar, "scale", scale)
    return err, err / scale


U32 = 2.0 ** -24      # unit roundoff of fp32
TINY32 = 2.0 ** -126  # smallest normal fp32


def backward_bound(S, n, want, extra=0):
    """The per-element bound of check_backward_elementwise (float64, the shape of `want`)."""
    import numpy as _np
    S = _np.asarray(S, _np.float64) + _np.abs(_np.asarray(extra, _np.float64))
    n = _np.asarray(n, _np.int64) + (_np.asarray(extra) != 0)
    return 2.0 * (n + 1) * U32 * S + U32 * _np.abs(_np.asarray(want, _np.float64)) + n * TINY32


def check_backward_elementwise(got, want, S, n, extra=0, what=""):
    """A bound for EACH element of a backward, from what that element sums (oracle.backward_bound_c: S = sum |w * g|
    in double, n = the number of terms):

        |got - want| <= 2 (n + 1) u S + u |want| + n 2^-126,   u = 2^-24

    n fp32 additions in ANY order err by at most (n - 1) u S (to first order); FMA contraction instead of a rounded
    product by another u |w g| per term; the oracle's rounding of its double sum by u |want|; a flushed subnormal
    product or partial sum by < 2^-126 each; the doubled first term is the slack for the second-order terms.  `extra`:
    the existing value an accumulating path adds to (one more term and one more rounding).  Also: where nothing lands
    (n = 0) got == want exactly (0, or the existing value), and the NaN / +inf / -inf classes match.  Measured on the
    MI355X over the dispatch table and the seeded fuzz (every backward path): the worst element used 0.26 of its bound.
    Returns the largest error as a fraction of its bound."""
    import numpy as _np
    g, w = _np.asarray(got, _np.float64), _np.asarray(want, _np.float64)
    n0 = _np.asarray(n)
    assert g.shape == w.shape == n0.shape, (what, g.shape, w.shape, n0.shape)
    for cls in (_np.isnan, _np.isposinf, _np.isneginf):
        diff = cls(g) != cls(w)
        assert not diff.any(), (what, cls.__name__, int(diff.sum()), "elements differ in class",
                                _np.argwhere(diff)[:4].tolist())
    empty = n0 == 0
    bad = empty & (g != w) & _np.isfinite(w)
    assert not bad.any(), (what, int(bad.sum()), "elements with no term are not exact", _np.argwhere(bad)[:4].tolist())
    fin = _np.isfinite(w)
    bound = backward_bound(S, n0, w, extra)
    err = _np.abs(g - w)
    over = fin & ~(err <= bound)
    if over.any():
        i = tuple(_np.argwhere(over)[0])
        raise AssertionError(f"{what}: {int(over.sum())} elements beyond their bound; first {i}: got {g[i]!r} want {w[i]!r} "
                             f"err {err[i]:.3e} bound {bound[i]:.3e} (n = {int(n0[i])}, S = {float(_np.asarray(S)[i]):.3e})")
    ratio = float((err[fin] / _np.maximum(bound[fin], 1e-300)).max()) if fin.any() else 0.0
    print(f"[backward bound] {what}: worst element at {ratio:.3f} of its bound, max terms per element {int(n0.max()) if n0.size else 0}")
    return ratio


def sparse_rois(R=520, seed=5):
    """Large, coarsely pooled ROIs for ONE 160 x 160 map at scale 0.25 (a 640 x 640 image): h and w of 520 .. 600 image
    pixels around the middle, any angle.  Pooled 16 x 16 their bins lie 8 .. 9 map pixels apart -- each in a key tile
    (4 rows x 8 columns of pixels) of its own, so a patch of 8 x 8 bins touches dozens of tiles."""
    rng = np.random.default_rng(seed)
    return np.stack([np.zeros(R), rng.uniform(280, 360, R), rng.uniform(280, 360, R), rng.uniform(520, 600, R),
                     rng.uniform(520, 600, R), rng.uniform(-180, 180, R)], 1).astype(np.float32)


def patch_shape(ph, pw):
    """The backward's pair pass walks a ROI's bins in patches of 64, one per wave: (rows, columns, patches per ROI);
    rows = the largest power of two <= min(ph, 8)."""
    pr = 1
    while pr * 2 <= min(ph, 8):
        pr *= 2
    pc = 64 // pr
    return pr, pc, -(-ph // pr) * -(-pw // pc)


def pairs_aggregate(R, ph, pw, cus):
    """Whether the one-pass bucket build reserves its slots per wave through the 16-tile LDS table (more than eight
    patches per CU) or with one atomic per pair."""
    return R * patch_shape(ph, pw)[2] > 8 * cus


def patch_tile_counts(oracle, shape, r, ph, pw, scale):
    """Per patch (ROI-major, then patch row, then patch column): the number of DISTINCT key tiles -- (image, y // 4,
    x // 8) -- its bins touch through taps that pass the backward's border tests (kernel.cu:267-274).  More than 16 and
    the wave's reservation table is full: the pairs of the tiles it has no room for reserve their slot alone."""
    B, _, H, W = shape
    _, geom = oracle.forward_c(np.zeros((B, 1, H, W), np.float32), r, ph, pw, scale, return_geom=True)
    cx, cy = geom[..., 0].reshape(-1).astype(np.float64), geom[..., 1].reshape(-1).astype(np.float64)
    x0, x1, y0, y1 = np.floor(cx), np.ceil(cx), np.floor(cy), np.ceil(cy)   # masked bins: (0, 0), which fails every test
    pr, pc, per_roi = patch_shape(ph, pw)
    npx = -(-pw // pc)
    n, iy, ix = np.unravel_index(np.arange(cx.size), (len(r), ph, pw))
    patch = (n * per_roi + (iy // pr) * npx + ix // pc).astype(np.int64)
    img = np.repeat(r[:, 0].astype(np.int64), ph * pw)
    Ht, Wt = -(-H // 4), -(-W // 8)
    taps = []
    for yy, xx, ok in ((y0, x0, (y0 > 0) & (x0 > 0) & (y0 < H - 1) & (x0 < W - 1)),
                       (y0, x1, (y0 > 0) & (x1 < W - 1) & (y0 < H - 1) & (x1 > 0)),
                       (y1, x1, (y1 < H - 1) & (x1 < W - 1) & (y1 > 0) & (x1 > 0)),
                       (y1, x0, (y1 < H - 1) & (x0 > 0) & (y1 > 0) & (x0 < W - 1))):
        tile = (img * Ht + yy.astype(np.int64) // 4) * Wt + xx.astype(np.int64) // 8
        taps.append(np.stack([patch[ok], tile[ok]], 1))
    pairs = np.unique(np.concatenate(taps), axis=0)
    return np.bincount(pairs[:, 0], minlength=len(r) * per_roi)
