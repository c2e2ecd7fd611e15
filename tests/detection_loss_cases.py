"""Shared by the detection-loss tests: the float64 restatement of the loss and its gradient, written in numpy
from the contract in include/rroi_align_hip.h section 16; the case table; the bound.

The bound is derived, not fitted.  u = 2^-53.  Every quantity below is computed once by the kernel and once by the
restatement, so a difference is bounded by the two errors added.

A sum.  S = sum of n terms t_i, each evaluated with a handful of double operations.  Whatever the order, the accumulation
errs by at most (n - 1) u A, A = sum of |t_i| (to first order); a term itself errs by at most 16 u a_i, a_i its magnitude
below, 16 being more operations than any term has, the transcendental ones counted as four (sin, cos and log are not
correctly rounded: a few ulp).  So  dS <= (n + 16) u A  with A = sum of a_i:
    dice sums   t = (p m)(g m), p m, g m: products of exact values, a_i = |t_i|
    angle sums  t = e^2, e = a - sin th: e errs by u |e| + 4 u (sin's ulps, |sin| <= 1), so t by 2 |e| of that: a_i = e^2 + |e|
    box sums    t = -log((X + 1) / (U + 1)).  X >= 0 and U >= max(A_gt, A_pred) >= (A_gt + A_pred) / 2 > 0 (the builder keeps
                roi_gt >= 0 and the predictions positive), so the one subtraction in U cancels at most half and X + 1, U + 1
                carry a few u of relative error; the logarithm turns that into the same ABSOLUTE error and adds its own
                ulps of |t|: a_i = 1 + |t_i|
Counts are sums of ones: exact.

A quotient.  dice = -(2 I + 1) / D, D = P + G + 1 >= 1:  d dice <= 2 dI / D + |2 I + 1| (dP + dG) / D^2 + 4 u |dice|.
angle = Ss / c + Sc / c:  d angle <= (dSs + dSc) / c + 3 u |angle|.  box likewise.  total = segm + 2 angle + 0.5 box:
d total <= d segm + 2 d angle + 0.5 d box + 3 u (|segm| + 2 |angle| + 0.5 |box|).  Summing two scales adds the two errors
and one rounding.

The outputs.  A term is rounded to float32 once: |got - ref| <= ulp_fp32(ref) + 2 d (one ulp, not half: the two doubles
that are rounded differ by up to 2 d and may fall on either side of a rounding boundary).  A gradient element is rounded to
the output dtype once: the rounding errs by at most half the spacing of the binade its argument lies in, so
|got - ref| <= ulp_out(|ref| + 2 e) / 2 + 2 e, e the error of the double value:
    d/dp   = w (m c1 - g m m c2), c1 = (2 I + 1) / D^2, c2 = 2 / D:  dc1 <= c1 (2 dI / |2 I + 1| + 2 dD / D + 6 u),
             dc2 <= c2 (dD / D + 2 u), dD = dP + dG + 2 u D;  e = |w| (m dc1 + g m m dc2) + 8 u |w| (m c1 + g m m c2)
    d/da   = (2 w / c)(a - sin th):  e = |2 w / c| u (4 |a - sin th| + 4)
    d/dr   = cl (r3 / (U + 1) - min(d3, r3) share (1 / (U + 1) + 1 / (X + 1))) + the right half: sums of products whose
             factors carry a few u each;  e = 16 u (the sum of the products' magnitudes)."""
import numpy as np
import torch

U53 = 2.0 ** -53
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
G_TOTAL = (0.0, 0.0, 0.0, 1.0)


# ---------------------------------------------------------------- the restatement
def resize(plane, h8, w8):
    """(N, H, W) float64 -> (N, h8, w8): bilinear, align_corners = true, section 8's recipe, every operation in double."""
    N, H, W = plane.shape

    def axis(n_in, n_out):
        s = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        src = s * np.arange(n_out, dtype=np.float64)
        i0 = np.minimum(src.astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        l1 = src - i0
        return i0, i1, 1.0 - l1, l1

    y0, y1, ly0, ly1 = axis(H, h8)
    x0, x1, lx0, lx1 = axis(W, w8)
    ly0, ly1 = ly0[None, :, None], ly1[None, :, None]
    lx0, lx1 = lx0[None, None, :], lx1[None, None, :]
    v00, v01 = plane[:, y0][:, :, x0], plane[:, y0][:, :, x1]
    v10, v11 = plane[:, y1][:, :, x0], plane[:, y1][:, :, x1]
    top = lx0 * v00 + lx1 * v01
    bot = lx0 * v10 + lx1 * v11
    return ly0 * top + ly1 * bot


def truth_of_scale(gt, size=None):
    """The ground truth of a scale as float64 planes (g, m, th, d (N, h, w, 4)); size (h8, w8): resized, d halved."""
    g, m, th, d = (np.asarray(v, dtype=np.float64) for v in gt)
    if size is None:
        return g, m, th, d
    d8 = np.stack([resize(d[..., k], *size) * 0.5 for k in range(4)], -1)
    return resize(g, *size), resize(m, *size), resize(th, *size), d8


def _share(gt, pred):
    return np.where(pred < gt, 1.0, np.where(pred == gt, 0.5, 0.0))


def _half(d1, d2, ds, r1, r2, rs):
    x = np.minimum(ds, rs) * (np.minimum(d1, r1) + np.minimum(d2, r2))
    return x, (d1 + d2) * ds + (r1 + r2) * rs - x


def scale64(p, a, r, truth, w):
    """One scale: p (N, h, w), a (N, 2, h, w), r (N, 4, h, w) float64; truth from truth_of_scale; w = (w_segm, w_angle, w_box).
    -> (segm, angle, box), their errors (d segm, d angle, d box), the gradients (gp, ga, gr) and their errors."""
    g, m, th, d = truth
    n = p.size
    mask = g > 0.5

    def dsum(terms, mags):
        return float(terms.sum()), (terms.size + 16) * U53 * float(mags.sum())

    tI, tP, tG = (p * m) * (g * m), p * m, g * m
    (I, dI), (P, dP), (G, dG) = dsum(tI, np.abs(tI)), dsum(tP, np.abs(tP)), dsum(tG, np.abs(tG))
    D = P + G + 1.0
    segm = -((2.0 * I + 1.0) / D)
    d_segm = 2 * dI / D + abs(2 * I + 1) * (dP + dG) / D ** 2 + 4 * U53 * abs(segm)
    c1, c2 = (2.0 * I + 1.0) / (D * D), 2.0 / D
    dD = dP + dG + 2 * U53 * D
    dc1 = c1 * (2 * dI / abs(2 * I + 1) + 2 * dD / D + 6 * U53)
    dc2 = c2 * (dD / D + 2 * U53)
    gp = w[0] * (m * c1 - g * m * m * c2)
    e_gp = abs(w[0]) * (m * dc1 + g * m * m * dc2) + 8 * U53 * abs(w[0]) * (np.abs(m * c1) + np.abs(g * m * m * c2))

    ga, e_ga = np.zeros_like(a), np.zeros_like(a)
    gr, e_gr = np.zeros_like(r), np.zeros_like(r)
    angle = d_angle = box = d_box = 0.0
    c = int(mask.sum())
    if c:
        es, ec = a[:, 0] - np.sin(th), a[:, 1] - np.cos(th)
        (Ss, dSs), (Sc, dSc) = (dsum(e[mask] ** 2, e[mask] ** 2 + np.abs(e[mask])) for e in (es, ec))
        angle = Ss / c + Sc / c
        d_angle = (dSs + dSc) / c + 3 * U53 * angle
        ca = w[1] * 2.0 / c
        for k, e in enumerate((es, ec)):
            ga[:, k] = np.where(mask, ca * e, 0.0)
            e_ga[:, k] = np.where(mask, abs(ca) * U53 * (4 * np.abs(e) + 4), 0.0)
    d1, d2, r1, r2 = d[..., 0], d[..., 1], r[:, 0], r[:, 1]
    m1, m2 = _share(d1, r1), _share(d2, r2)
    ht = np.minimum(d1, r1) + np.minimum(d2, r2)
    for side in (2, 3):
        ds, rs = d[..., side], r[:, side]
        sel = mask & (ds > 0)
        cnt = int(sel.sum())
        if not cnt:
            continue
        x, u = _half(d1, d2, ds, r1, r2, rs)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = -np.log((x + 1.0) / (u + 1.0))
        L, dL = dsum(t[sel], 1.0 + np.abs(t[sel]))
        box += L / cnt
        d_box += dL / cnt + 3 * U53 * abs(L / cnt)
        cf = w[2] / cnt
        iu = 1.0 / (u + 1.0)
        ix = iu + 1.0 / (x + 1.0)
        wd = np.minimum(ds, rs)
        parts = ((0, rs * iu, wd * m1 * ix), (1, rs * iu, wd * m2 * ix), (side, (r1 + r2) * iu, ht * _share(ds, rs) * ix))
        for k, pos, neg in parts:
            gr[:, k] += np.where(sel, cf * (pos - neg), 0.0)
            e_gr[:, k] += np.where(sel, 16 * U53 * abs(cf) * (np.abs(pos) + np.abs(neg)), 0.0)
    return (segm, angle, box), (d_segm, d_angle, d_box), (gp, ga, gr), (e_gp, e_ga, e_gr), n


def ref64(preds4, preds8, gt, g=G_TOTAL):
    """preds4 = (s (N, 1, H, W), a, r) float64 arrays, preds8 likewise or None; gt = (segm_gt, iou_mask, angle_gt, roi_gt).
    g: the gradient arriving at [segm, angle, box, total].  -> dict(terms (4), d_terms (4): the error of each term's double
    value, grads: six (three) float64 arrays in the order s4, a4, r4, s8, a8, r8, e_grads: their errors)."""
    g = [float(np.float32(v)) for v in g]
    w = (g[0] + g[3], g[1] + 2.0 * g[3], g[2] + 0.5 * g[3])
    terms, d_terms, grads, e_grads = np.zeros(3), np.zeros(3), [], []
    for k, preds in enumerate((preds4, preds8)):
        if preds is None:
            continue
        s, a, r = (np.asarray(v, dtype=np.float64) for v in preds)
        truth = truth_of_scale(gt, s.shape[2:] if k else None)
        t, dt, (gp, ga, gr), (ep, ea, er), _ = scale64(s[:, 0], a, r, truth, w)
        terms += t
        d_terms += np.asarray(dt) + U53 * np.abs(terms)
        grads += [gp[:, None], ga, gr]
        e_grads += [ep[:, None], ea, er]
    total = terms[0] + 2.0 * terms[1] + 0.5 * terms[2]
    d_total = d_terms[0] + 2 * d_terms[1] + 0.5 * d_terms[2] + 3 * U53 * (abs(terms[0]) + 2 * abs(terms[1]) + 0.5 * abs(terms[2]))
    return dict(terms=np.append(terms, total), d_terms=np.append(d_terms, d_total), grads=grads, e_grads=e_grads)


# ---------------------------------------------------------------- the bound
def ulp(ref, dtype):
    """One unit in the last place of `dtype` at each |ref| (float64 array): the spacing of the binade |ref| lies in, the
    subnormal spacing below the smallest normal."""
    p, emin = {torch.float32: (24, -126), torch.bfloat16: (8, -126), torch.float16: (11, -14)}[dtype]
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    e = np.floor(np.log2(np.where(ref > 0, ref, 1.0)))
    e = np.where(ref > 0, np.maximum(e, emin), emin)
    return 2.0 ** (e - (p - 1))


def _np(v):
    return v.detach().double().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64)


def terms_ratio(got, ref):
    """max over the four terms of |got - ref| / (ulp_fp32(ref) + 2 d); a NaN or an infinity in `got` is an infinite ratio."""
    got = _np(got)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref["terms"]) / (ulp(ref["terms"], torch.float32) + 2 * ref["d_terms"])).max())


def grads_ratio(got, ref, dtype):
    """max over the gradients and their elements of |got - ref| / (ulp_out(|ref| + 2 e) / 2 + 2 e)."""
    worst = 0.0
    for gt, rf, e in zip(got, ref["grads"], ref["e_grads"]):
        gt = _np(gt)
        if gt.shape != rf.shape or not np.isfinite(gt).all():
            return float("inf")
        worst = max(worst, float((np.abs(gt - rf) / (0.5 * ulp(np.abs(rf) + 2 * e, dtype) + 2 * e)).max()))
    return worst


def f32_tol(ref, n):
    """What a float32 evaluation (the stock restatement) may differ from a float64 value by: every sum over up to n elements
    errs by n 2^-24 relative to its magnitude, a term or a gradient element depends on at most three such sums and sixteen
    further float32 operations (the resize among them), so (3 n + 16) 2^-24 of the magnitude -- of the value itself for a
    term (floor 1: the dice term's `+ 1`), of the tensor's largest element for a gradient (an element is a difference of
    parts that large)."""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    scale = max(1.0, float(ref)) if ref.ndim == 0 else max(float(ref.max()), 2.0 ** -126)
    return (3 * n + 16) * 2.0 ** -24 * scale


def f32_terms_ratio(got, ref_terms, n):
    got = _np(got)
    return max(abs(float(a) - float(b)) / f32_tol(np.float64(b), n) for a, b in zip(got, ref_terms))


def f32_grads_ratio(got, ref_grads, n):
    return max(float((np.abs(_np(a) - b) / f32_tol(b, n)).max()) for a, b in zip(got, ref_grads))


# ---------------------------------------------------------------- the cases
def _blocks(rng, N, H, W, count, low=1):
    """(N, H, W) zeros with `count` random rectangles of ones per image, each at least `low` pixels a side."""
    out = np.zeros((N, H, W), dtype=np.float32)
    for n in range(N):
        for _ in range(count):
            h, w = int(rng.integers(low, max(low + 1, H // 2 + 1))), int(rng.integers(low, max(low + 1, W // 2 + 1)))
            y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            out[n, y:y + h, x:x + w] = 1.0
    return out


def _case(name, N, H, W, H8, W8, seed, multi=True, g=G_TOTAL, kind=""):
    """A case: the float32 ground truth and float32 predictions (rounded per dtype by materialise), as numpy arrays."""
    rng = np.random.default_rng(7000 + seed)
    f32 = np.float32
    segm = _blocks(rng, N, H, W, 2, low=min(2, H, W))
    if kind == "tiny":
        segm[:] = 1.0
    if kind == "empty":
        segm[:] = 0.0
    mask = np.ones((N, H, W), dtype=f32)
    mask[:, : max(H // 4, 0), W // 2:] = 0.0                              # a zeroed region of the training mask
    if kind == "tiny":
        mask[:] = 1.0
    if kind == "fractional":
        segm = segm * rng.choice(np.array([0.25, 0.75, 1.0], dtype=f32), (N, H, W)) + \
            (1 - segm) * rng.choice(np.array([0.0, 0.125], dtype=f32), (N, H, W))
        mask = mask * rng.choice(np.array([0.5, 1.0, 0.75], dtype=f32), (N, H, W))
    angle = (rng.uniform(-0.8, 0.8, (N, H, W)) * (segm > 0)).astype(f32)
    roi = (rng.uniform(0.5, 40.0, (N, H, W, 4)) * (segm > 0)[..., None]).astype(f32)
    if kind not in ("tiny", "no_left", "no_right"):
        roi[..., 2] *= rng.random((N, H, W)) > 0.15                       # pixels on a box's left / right edge: distance 0
        roi[..., 3] *= rng.random((N, H, W)) > 0.15
    if kind == "no_left":
        roi[..., 2] = 0.0
    if kind == "no_right":
        roi[..., 3] = 0.0
    sizes = [(H, W)] + ([(H8, W8)] if multi else [])
    preds = []
    for (h, w) in sizes:
        preds.append((rng.uniform(0.02, 0.98, (N, 1, h, w)).astype(f32), rng.uniform(-1.0, 1.0, (N, 2, h, w)).astype(f32),
                      rng.uniform(0.1, 60.0, (N, 4, h, w)).astype(f32)))
    if kind == "tie":
        # exact ties on the 1/4 scale, at values every dtype holds: top, left and right on a third of the masked pixels each
        for ch, val in ((0, 3.5), (2, 12.0), (3, 0.75)):
            at = (segm > 0.5) & (rng.random((N, H, W)) < 0.34)
            roi[..., ch][at] = val
            preds[0][2][:, ch][at] = val
    return dict(name=name, N=N, H=H, W=W, H8=H8 if multi else 0, W8=W8 if multi else 0, multi=multi, g=tuple(g), kind=kind,
                gt=(segm, mask, angle, roi), preds=preds)


def _conditions(c):
    """What the builder promises, so that the reference side alone stays inside them."""
    segm, mask, angle, roi = c["gt"]
    assert (roi >= 0).all() and segm.dtype == np.float32
    if c["multi"]:
        r8 = resize(segm.astype(np.float64), c["H8"], c["W8"])
        assert (np.abs(r8 - 0.5) > 1e-6).all(), c["name"]                 # no resized segm_gt within 1e-6 of 0.5
    assert (np.abs(segm.astype(np.float64) - 0.5) > 1e-6).all()
    ties = 0
    for dtype in DTYPES:
        for k, (s, a, r) in enumerate(c["preds"]):
            rd = torch.from_numpy(r).to(dtype).double().numpy()
            assert ((rd > 0) & (rd < 128)).all()                          # every logarithm's argument is positive
            d = truth_of_scale(c["gt"], r.shape[2:] if k else None)[3]
            ties += int((rd == np.moveaxis(d, -1, 1)).sum())
    assert (ties > 0) == (c["kind"] == "tie"), (c["name"], ties)          # d_pred == d_gt only where it is meant
    masked = segm > 0.5
    if c["kind"] == "empty":
        assert not masked.any()
    if c["kind"] == "no_left":
        assert masked.any() and (roi[..., 2][masked] <= 0).all() and (roi[..., 3][masked] > 0).any()
    if c["kind"] == "no_right":
        assert masked.any() and (roi[..., 3][masked] <= 0).all() and (roi[..., 2][masked] > 0).any()
    if c["kind"] in ("", "tie", "tiny", "fractional"):
        for k in range(1 + c["multi"]):
            g, _, _, d = truth_of_scale(c["gt"], (c["H8"], c["W8"]) if k else None)
            assert ((g > 0.5) & (d[..., 2] > 0)).any() and ((g > 0.5) & (d[..., 3] > 0)).any(), (c["name"], k)
    return c


# The smallest cases at which each mechanism can fail: sizes that are no multiple of a wave and no halves of each other, the
# out == 1 resize, one workgroup and several with more than one item per thread (the plan's thresholds are 4096 and 16384
# items: `square` has 2560, `multiblock` 23040), every empty selection, a single scale, m^2 against m, exact ties, weights.
CASES = [_conditions(c) for c in (
    _case("odd", 2, 13, 21, 7, 11, 1),
    _case("tiny", 1, 2, 2, 1, 1, 2, kind="tiny"),
    _case("square", 2, 32, 32, 16, 16, 3),
    _case("multiblock", 3, 64, 96, 32, 48, 4),
    _case("empty", 2, 12, 20, 6, 10, 5, kind="empty"),
    _case("no_left", 2, 12, 20, 6, 10, 6, kind="no_left"),
    _case("no_right", 2, 12, 20, 6, 10, 7, kind="no_right"),
    _case("single_scale", 2, 13, 21, 7, 11, 8, multi=False),
    _case("fractional", 2, 12, 20, 6, 10, 9, kind="fractional"),
    _case("tie", 2, 12, 20, 6, 10, 10, kind="tie"),
    _case("weights", 2, 13, 21, 7, 11, 11, g=(0.5, -1.25, 3.0, 0.75)),
)]
CASE = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]
NO_EMPTY_SELECTION = [c["name"] for c in CASES if c["kind"] not in ("empty", "no_left", "no_right")]
GOLDEN = ("odd", "tiny", "single_scale", "fractional", "tie")        # the cases tests/golden/detection_loss.npz holds

_cache = {}


def items(case):
    return case["N"] * (case["H"] * case["W"] + case["H8"] * case["W8"])


def materialise(case, dtype=torch.float32):
    """(preds: per scale a tuple (s, a, r) of CPU tensors rounded to dtype; ref: ref64 on exactly those values with the
    case's g), computed once per (case, dtype) and shared: treat both as read-only."""
    key = (case["name"], dtype)
    if key not in _cache:
        preds = [tuple(torch.from_numpy(v).to(dtype) for v in p) for p in case["preds"]]
        as64 = [tuple(v.double().numpy() for v in p) for p in preds]
        _cache[key] = (preds, ref64(as64[0], as64[1] if case["multi"] else None, case["gt"], case["g"]))
    return _cache[key]


def tensors(case, dtype, device, requires_grad=True):
    """The call's arguments on `device`: ([s4, s8], [a4, a8], [r4, r8]) as fresh leaves, and the four ground-truth tensors."""
    preds = materialise(case, dtype)[0]
    lists = [[p[k].to(device, copy=True).requires_grad_(requires_grad) for p in preds] for k in range(3)]
    return lists, [torch.from_numpy(v).to(device) for v in case["gt"]]
