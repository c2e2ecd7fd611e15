"""Shared by test_heads_backward_abi.py (CPU) and test_gpu_heads_backward.py: the problems of the native backward of the
detection heads and the attention gate, its reference, its bounds and the mirror of the host's plan rule; no
test in here.  The shapes, x, the parameters and the dtypes are those of heads_cases.py, which is imported unchanged; the
output gradients are drawn as instancenorm_backward_cases.random_dy draws them (N(0,1) scaled by 2^(plane % 5 - 2)).

The reference is header section 7b in np.longdouble, from x, w, b and the output gradients (a None gradient is zero):
    z_o = b_o + sum_c w[o][c] x[c],  s_o = 1 / (1 + exp(-z_o)),  g_0 = dscore,  g_{1+j} = scale * drbox_j,
    a_i = 2 s_{5+i} - 1, r = |a|, u_i = a_i / r, g_{5+i} = 2 (dangle_i - u_i (u_0 dangle_0 + u_1 dangle_1)) / r,
    dz_o = g_o s_o (1 - s_o),  dx_c = sum_o w[o][c] dz_o,  dw[o][c] = sum_{n,p} dz_o x[c],  db[o] = sum_{n,p} dz_o.

Beside every result stands `mag`, the sum of the absolute values of its terms, built from a per-pixel magnitude M_o of dz_o:
    o < 5:   M_o = |g_o| s_o (1 - s_o) (1 + mass_o),                       mass_o = |b_o| + sum_c |w[o][c] x[c]|
    angles:  M_{5+i} = s (1 - s) (G_i (1 + mass_{5+i}) + D / r^2 (1 + mass_5 + mass_6)),
             G_i = 2 (|dangle_i| + |u_i| (|u_0 dangle_0| + |u_1 dangle_1|)) / r,   D = |dangle_0| + |dangle_1|
    mag(dx_c) = sum_o |w[o][c]| M_o,   mag(dw[o][c]) = sum_{n,p} M_o |x[c]|,   mag(db[o]) = sum_{n,p} M_o
-- the angle rows carry the 1 / r and 1 / r^2 factors -- and the bound has the form of DESIGN 5.25's:
    |got - ref| <= 2 u |ref| + c mag + 2^-25,    c = 2^-37
u the unit roundoff of the dtype (2 u leaves room for the half-ulp of a result next to a binade's edge), 2^-25 half the
smallest float16 subnormal.  NaN positions must agree.  Nothing is left out.

Where c comes from.  With e = 2^-53, what the kernel's dz_o differs from the reference's by, relative to M_o:
  * the z it reads is the training forward's: |dz_o| <= (C + S + 1) e mass_o (heads_cases.native_bound), S <= 16; s (1 - s)
    has a logarithmic slope of |1 - 2 s| <= 1, so that is (C + 17) e (1 + mass_o) of the term, and some 12 e for the
    exp, the divide and the products behind it;
  * an angle row also sees a = 2 s - 1 move by e_a <= |dz| / 2 + 17 e in each component, and g = 2 (d - u (u . d)) / r moves
    by at most 20 D e_a / r^2 (|dr| <= 2 e_a, |du_i| <= 3 e_a / r, |d (u . d)| <= 3 D e_a / r, |g| <= 4 D / r), which is
    20 (C + 34) e of the D / r^2 term.
  So a term is off by at most 20 (C + 34) e M_o: 10,980 e at the table's largest C = 515.
  * the sums: dx_c is a chain of 7 fused multiply-adds.  A dw or db entry is, by the plan (plan_of below; the kernel's
    comment names the same stages), a chain of V <= 2 in the lane, 6 over the wave's lanes, `tiles per workgroup` in the
    workgroup, ceil(rows / 4) + 3 in the finish: the plan allows tiles per workgroup up to 2^31 / 64 / 1024 = 2^15 (fewer
    than 2^31 pixels, tiles of at least 64, at least 1024 workgroups once there is more than one tile each) and rows up to
    1024, so 2 + 6 + 32768 + 256 + 3 = 33,035 additions, each e of the running sum, which mag bounds.
  10,980 + 33,035 = 44,015 < 2^16, and c = 2^16 e = 2^-37.

z itself is checked the same way against the longdouble z: |got - ref| <= 2 e |ref| + 2^-43 mass, 2^-43 = 2^10 e for the
chain of C + S + 1 <= 532 additions."""
import functools

import numpy as np
import torch

import heads_cases as H
from instancenorm_backward_cases import random_dy

LD = np.longdouble
DTYPES, IDS, UNIT_ROUNDOFF = H.DTYPES, H.IDS, H.UNIT_ROUNDOFF
HEADS, GATE = H.HEADS, H.GATE
C_BOUND = 2.0 ** -37
Z_BOUND = 2.0 ** -43

# The plan rule of csrc/rroi_heads_backward_host.h (plan_heads_backward), mirrored: change both together.
CUS = H.CUS
WAVES, CHUNK, GRID_PER_CU, PASS_BLOCK = 4, 8, 4, 128


def plan_of(N, C, H_, W, cus=CUS):
    """-> dict(V, tiles per image, total tiles, tpw: tiles per workgroup, rows: workgroups = partial rows, cb: channels per
    wave, passes over the tiles)."""
    hw = H_ * W
    tiles = lambda v: -(-hw // (64 * v))  # noqa: E731
    V = 2 if N * tiles(2) >= cus else 1
    total = N * tiles(V)
    tpw = -(-total // (GRID_PER_CU * cus))
    cb = -(-C // (WAVES * CHUNK)) * CHUNK
    return dict(V=V, tiles=tiles(V), total=total, tpw=tpw, rows=-(-total // tpw), cb=cb, passes=-(-cb // PASS_BLOCK))


def workspace_bytes(N, C, H_, W, outputs, cus=CUS):
    return plan_of(N, C, H_, W, cus)["rows"] * outputs * (C + 1) * 8


# heads_cases.CASES has one partial row ((1,1,1,1) ...), two rows with a partial last tile ((1,64,5,13): 65 pixels), C in
# {1, 7, 255, 257} -- a wave's block of 8, 64 or 72 channels of which 1, 7, 63 or 41 exist in the last wave that has any --
# odd H * W in 16 bits and one pixel per image.  Added here:
#   (3,3,181,242)  343 tiles of 128 pixels per image, 1029 in all, two per workgroup, 515 rows: workgroup 171 has the last
#                  tile of image 0 and the first of image 1, and the finish's quarters are of 129, 129, 129 and 128 rows
#   (2,515,3,5)    136 channels per wave: two passes over the tiles (128 + 8 channels), the second of one chunk
EXTRA = ((3, 3, 181, 242), (2, 515, 3, 5))
CASES = tuple(dict.fromkeys(H.CASES + EXTRA))
case_id = H.case_id


def random_grads(shape, dtype, seed):
    """(dscore, drbox, dangle), (dy,) of `dtype` on the CPU for x of `shape`."""
    N, _, H_, W = shape
    g = random_dy((N, 7, H_, W), dtype, seed)
    return (g[:, 0:1].contiguous(), g[:, 1:5].contiguous(), g[:, 5:7].contiguous()), (random_dy((N, 1, H_, W), dtype, seed + 1),)


def _ld(t):
    return t.detach().double().cpu().numpy().astype(LD)


class Reference:
    """z, dx, dw, db of one call as float64 tensors (computed in longdouble), each with its bound: `z` (N,k,H,W), `dx`
    (N,C,H,W), `dw` (k,C), `db` (k), and `z_lim`, `dx_lim`, `dw_lim`, `db_lim`.
    x (N,C,H,W); params (w, b, w, b, ...) as heads_cases.reference takes them; grads: one tensor or None per output group."""

    def __init__(self, x, params, grads, rbox_scale=H.RBOX_SCALE):
        N, C, H_, W = x.shape
        u = UNIT_ROUNDOFF[x.dtype]
        wm, bv = H._stack(params, C)
        k = len(wm)
        widths = (1,) if k == GATE else (1, 4, 2)
        with np.errstate(all="ignore"):
            wm, bv = wm.astype(LD), bv.astype(LD)
            X = _ld(x).reshape(N, C, H_ * W)
            G = np.concatenate([np.zeros((N, n, H_ * W), LD) if g is None else _ld(g).reshape(N, n, H_ * W)
                                for g, n in zip(grads, widths)], axis=1)
            z = np.einsum("oc,ncp->nop", wm, X) + bv[None, :, None]
            mass = np.einsum("oc,ncp->nop", np.abs(wm), np.abs(X)) + np.abs(bv)[None, :, None]
            s = 1 / (1 + np.exp(-z))
            ds = s * (1 - s)
            g = G.copy()
            M = np.abs(G) * ds * (1 + mass)
            if k == HEADS:
                g[:, 1:5] = LD(rbox_scale) * G[:, 1:5]
                M[:, 1:5] = np.abs(g[:, 1:5]) * ds[:, 1:5] * (1 + mass[:, 1:5])
                d = G[:, 5:7]
                a = 2 * s[:, 5:7] - 1
                r = np.sqrt(a[:, 0:1] * a[:, 0:1] + a[:, 1:2] * a[:, 1:2])
                uu = a / r
                p = uu[:, 0:1] * d[:, 0:1] + uu[:, 1:2] * d[:, 1:2]
                g[:, 5:7] = 2 * (d - uu * p) / r
                pa = np.abs(uu[:, 0:1] * d[:, 0:1]) + np.abs(uu[:, 1:2] * d[:, 1:2])
                Gi = 2 * (np.abs(d) + np.abs(uu) * pa) / r
                D = np.abs(d[:, 0:1]) + np.abs(d[:, 1:2])
                both = 1 + mass[:, 5:6] + mass[:, 6:7]
                M[:, 5:7] = ds[:, 5:7] * (Gi * (1 + mass[:, 5:7]) + D / (r * r) * both)
            dz = g * ds
            dx, dx_mag = np.einsum("oc,nop->ncp", wm, dz), np.einsum("oc,nop->ncp", np.abs(wm), M)
            dw, dw_mag = np.einsum("nop,ncp->oc", dz, X), np.einsum("nop,ncp->oc", M, np.abs(X))
            db, db_mag = dz.sum(axis=(0, 2)), M.sum(axis=(0, 2))
            lim = lambda ref, mag: 2 * u * np.abs(ref) + LD(C_BOUND) * mag + LD(2.0 ** -25)  # noqa: E731
            t = lambda v, shape: torch.from_numpy(np.asarray(v, dtype=np.float64)).reshape(shape)  # noqa: E731
            self.z, self.z_lim = t(z, (N, k, H_, W)), t(2 * LD(2.0 ** -53) * np.abs(z) + LD(Z_BOUND) * mass, (N, k, H_, W))
            self.dx, self.dx_lim = t(dx, x.shape), t(lim(dx, dx_mag), x.shape)
            self.dw, self.dw_lim = t(dw, (k, C)), t(lim(dw, dw_mag), (k, C))
            self.db, self.db_lim = t(db, (k,)), t(lim(db, db_mag), (k,))


def overflow_threshold(dtype):
    """The magnitude from which a value rounds to an infinity of `dtype`: its largest finite value and half an ulp."""
    if dtype not in UNIT_ROUNDOFF:                # z is float64: nothing of the table comes near its range
        return float("inf")
    top = float(torch.finfo(dtype).max)
    return top + 2.0 ** np.floor(np.log2(top)) * UNIT_ROUNDOFF[dtype]


def check(got, ref, lim):
    """-> (ok, worst |got - ref| / bound over the finite reference elements); the NaN positions must agree.  A sum of
    131,406 pixels leaves float16's range (dw of the rbox rows of 1x4x362x363): where |ref| + bound reaches the magnitude
    that rounds to an infinity of got's dtype, that infinity, of ref's sign, is within the bound as well."""
    thr = overflow_threshold(got.dtype)
    got = got.detach().cpu().double().reshape(ref.shape)
    nan_ok = bool(torch.equal(got.isnan(), ref.isnan()))
    fin = ref.isfinite()
    if not bool(fin.any()):
        return nan_ok, 0.0
    ratio = (got - ref).abs() / lim
    rounds_to_inf = got.isinf() & (got.sign() == ref.sign()) & (ref.abs() + lim >= thr)
    ratio = torch.where(rounds_to_inf, torch.zeros_like(ratio), ratio)[fin]
    return nan_ok and bool((ratio <= 1).all()), float(ratio.max())


def check_all(R, dx, dw, db):
    """dx (N,C,H,W) or None; dw, db: a tensor, a tuple of the three heads' tensors (concatenated in output order), or None.
    -> (ok, {name: worst ratio})."""
    ok, worst = True, {}
    join = lambda v, k: None if v is None else (torch.cat([t.reshape(-1, k) if k else t.reshape(-1) for t in v])  # noqa: E731
                                                if isinstance(v, (tuple, list)) else v)
    for name, got, ref, lim in (("dx", dx, R.dx, R.dx_lim), ("dw", join(dw, R.dw.size(1)), R.dw, R.dw_lim),
                                ("db", join(db, 0), R.db, R.db_lim)):
        if got is not None:
            good, worst[name] = check(got, ref, lim)
            ok = ok and good
    return ok, worst


@functools.lru_cache(maxsize=None)
def problem(shape, dtype):
    """x, heads parameters, gate parameters, heads gradients, gate gradients of the table's case, computed once and not
    modified."""
    x, hp, gp = H.random_problem(shape, dtype, seed=sum(shape))
    hg, gg = random_grads(shape, dtype, sum(shape))
    return x, hp, gp, hg, gg


@functools.lru_cache(maxsize=None)
def reference(shape, dtype):
    """(heads Reference, gate Reference) of the table's case, computed once and not modified."""
    x, hp, gp, hg, gg = problem(shape, dtype)
    return Reference(x, hp, hg), Reference(x, gp, gg)
