"""Shared by test_heads_abi.py (CPU) and test_gpu_heads.py: the case table of the native detection heads and attention
gate, the float64 reference, and the two bounds of the comparisons.

The reference is numpy: z = w.astype(f64) @ x.astype(f64) + b, s = 1 / (1 + exp(-z)), score = s_0, rbox = scale * s_{1..4},
a = 2 s_{5,6} - 1, angle = a / sqrt(a_0 a_0 + a_1 a_1), all in float64; rounded once by torch (`.to(dtype)`, which goes
through fp32 for the 16-bit types exactly as the kernel's `(T)(float)v` does).
"""
import functools

import numpy as np
import torch

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
IDS = ("fp32", "bf16", "fp16")
UNIT_ROUNDOFF = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SMALLEST_SUBNORMAL = {torch.float32: 2.0 ** -149, torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}
RBOX_SCALE = 128.0
HEADS, GATE = 7, 1

# The plan rule of csrc/rroi_heads_host.h (plan_heads), mirrored: change both together.
CUS = 256                   # MI355X, and what the library assumes where there is no GPU
WAVES_PER_CU, MAX_WAVES = 16, 16
FORMS = tuple((2, s) for s in (1, 2, 4, 8)) + tuple((1, s) for s in (1, 2, 4, 8, 16))   # all the rule can return


def plan_of(N, C, H, W, cus=CUS):
    """(V, S) by the mirrored rule: V pixels per lane, S channel blocks of ceil(C / S) channels."""
    hw = H * W
    tiles = lambda v: N * -(-hw // (64 * v))  # noqa: E731
    V = 2 if 8 * tiles(2) >= 5 * cus else 1
    S = 1
    while S < MAX_WAVES and tiles(V) * S < WAVES_PER_CU * cus:
        S *= 2
    while S * V > MAX_WAVES:
        S //= 2
    while S > 1 and (S - 1) * -(-C // S) >= C:
        S //= 2
    return V, S


# (N, C, H, W).  The small maps cross C in {1, 3, 5, 64, 255, 256, 257} (C < S, blocks that do not divide C, a remainder
# of the 8-channel step) with H * W in {1, 63, 64, 65, 253, 16 * 24, 44 * 80} (less than a tile, a partial last tile, odd
# planes that move a 16-bit plane's alignment from channel to channel) and N in {1, 2, 3}; all of them are V = 1.  The
# large maps reach V = 2 (from 160 tiles of 128 pixels): the rule reads pixel counts, so few channels suffice.
CASES = (
    (1, 1, 1, 1),        # (1, 1)
    (2, 3, 7, 9),        # 63    (1, 2)
    (3, 5, 8, 8),        # 64    (1, 2): blocks of 3 and 2 channels
    (1, 64, 5, 13),      # 65    (1, 16)
    (2, 255, 11, 23),    # 253   (1, 16): blocks of 16, the last of 15
    (3, 256, 16, 24),    # 384   (1, 16): the network's 1/8 map at a 128 x 192 image
    (1, 257, 44, 80),    # 3520  (1, 16): blocks of 17, the last of 2
    (2, 64, 44, 80),     #       (1, 16)
    (3, 257, 7, 9),      # 63, odd plane and odd channel count
    (1, 255, 5, 13),     # 65
    (2, 256, 1, 1),      # one pixel per image
    (1, 7, 11, 23),      # (1, 4): blocks of 2, the last of 1
    (1, 8, 16, 24),      # (1, 8): C < 16, one channel per wave
    (1, 64, 176, 187),   # 32912 pixels, 258 tiles of 128: (2, 8)
    (1, 5, 181, 183),    # 33123 pixels, an odd plane with two pixels per lane: (2, 2) by C
    (1, 257, 80, 257),   # 20560 pixels, 161 tiles: the smallest V = 2, blocks of 33, the last of 26: (2, 8)
    (1, 4, 362, 363),    # 131406 pixels, 1027 tiles: (2, 4)
    (1, 1, 362, 363),    # (2, 1) by C
    (1, 3, 512, 512),    # 2048 tiles: (2, 2)
    (2, 3, 512, 512),    # 4096 tiles: (2, 1)
)


def case_id(shape):
    return "x".join(str(v) for v in shape)


def random_problem(shape, dtype, seed):
    """x = N(0,1); weights N(0,1) * {1, 4} / sqrt(C), the factor alternating over the seven rows (+ the gate's row);
    biases N(0,1); all rounded to `dtype` (the reference sees the rounded values).
    -> x, (w_score, b_score, w_rbox, b_rbox, w_angle, b_angle), (w_gate, b_gate)"""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    factor = torch.tensor([(1.0, 4.0)[(o + seed) % 2] for o in range(8)], dtype=torch.float64)[:, None] / C ** 0.5
    w = torch.randn(8, C, generator=g, dtype=torch.float64) * factor
    b = torch.randn(8, generator=g, dtype=torch.float64)
    w, b = w.to(dtype), b.to(dtype)
    return x.to(dtype), (w[0:1], b[0:1], w[1:5], b[1:5], w[5:7], b[5:7]), (w[7:8], b[7:8])


def _stack(params, C):
    """(k, C) float64 weights and (k,) biases of a parameter list (w, b, w, b, ...); a None bias is +0.0."""
    ws = [p.detach().double().reshape(-1, C).numpy() for p in params[0::2]]
    bs = [np.zeros(len(w)) if b is None else b.detach().double().reshape(-1).numpy() for w, b in zip(ws, params[1::2])]
    return np.concatenate(ws), np.concatenate(bs)


class Ref:
    """The float64 values of one call and what the bounds need: `out64` (N, k, H, W) float64 before any rounding, `mass`
    = |b| + sum |w x| per pre-activation, `s` the sigmoids, and for the heads `a` (2 s - 1) and `r` (its norm)."""


def reference(x, params, rbox_scale=RBOX_SCALE):
    """params: (w_score, b_score, w_rbox, b_rbox, w_angle, b_angle) -> heads; (w, b) -> gate.
    -> (outputs rounded to x's dtype by torch: (score, rbox, angle) or (y,), Ref)."""
    N, C, H, W = x.shape
    wm, bv = _stack(params, C)
    X = x.double().numpy().reshape(N, C, H * W)
    R = Ref()
    with np.errstate(all="ignore"):
        z = wm @ X + bv[None, :, None]
        R.mass = np.abs(wm) @ np.abs(X) + np.abs(bv)[None, :, None]
        s = 1.0 / (1.0 + np.exp(-z))
        R.s, R.C = s, C
        if len(wm) == GATE:
            out = s
        else:
            a = 2.0 * s[:, 5:7] - 1.0
            r = np.sqrt(a[:, 0:1] * a[:, 0:1] + a[:, 1:2] * a[:, 1:2])
            out = np.concatenate([s[:, 0:1], rbox_scale * s[:, 1:5], a / r], axis=1)
            R.a, R.r, R.scale = a, r, rbox_scale
    R.out64 = torch.from_numpy(out.reshape(N, -1, H, W))
    rounded = R.out64.to(x.dtype)
    return ((rounded,) if len(wm) == GATE else (rounded[:, 0:1], rounded[:, 1:5], rounded[:, 5:7])), R


def _shape_like(R, v):
    return torch.from_numpy(np.ascontiguousarray(v)).reshape(R.out64.shape)


def native_bound(R, dtype, S):
    """What condition (a) allows |got - out64| to be, per element (the shape of out64).

    The final rounding: out64 goes to fp32 and (16-bit types) on to T: u_T |v| + 2^-24 |v| for the step through fp32, and
    half the smallest subnormal of T where the value is below T's normal range.
    The double arithmetic in front of it: the products are exact; a sum of C terms in S + 1 partial chains and the bias
    carries |dz| <= (C + S + 1) 2^-53 (|b| + sum |w x|) whatever the order; the sigmoid has slope s (1 - s) and its own
    exp, add and divide (8 * 2^-53 relative covers a 1-ulp exp at |z| <= 745); rbox scales that by rbox_scale;
    a = 2 s - 1 has |da| <= 2 |ds| + 2^-53 and the normalised angle |d angle| <= 2 (|da_0| + |da_1|) / r + 4 * 2^-53."""
    u, eps = UNIT_ROUNDOFF[dtype] + (0.0 if dtype == torch.float32 else 2.0 ** -24), 2.0 ** -53
    with np.errstate(all="ignore"):
        mass = np.where(np.isfinite(R.mass), R.mass, 0.0)         # an inf in the column: z is +-inf or NaN exactly
        ds = R.s * (1 - R.s) * (R.C + S + 1) * eps * mass + 8 * eps * R.s
        if R.s.shape[1] == GATE:
            prop = ds
        else:
            da = 2 * ds[:, 5:7] + eps
            dang = 2 * (da[:, 0:1] + da[:, 1:2]) / R.r + 4 * eps
            prop = np.concatenate([ds[:, 0:1], R.scale * ds[:, 1:5] + eps * R.scale, dang, dang], axis=1)
    return u * R.out64.abs() + SMALLEST_SUBNORMAL[dtype] / 2 + _shape_like(R, prop)


def stock_bound(R, dtype):
    """What |stock - other| may be, per element, where `stock` is the stock chain (`FOTSNet._heads`, or the convolution and
    sigmoid of `_gate`) run in T and `other` is out64 itself or out64 rounded once to T.

    With u = u_T, u32 = 2^-24 and eta = T's smallest subnormal, every stock operation rounding its result to T:
      convolution  accumulated in fp32 or wider in some order, rounded to T:  |dz| <= (C + 2) u32 mass + u |z| <= ((C + 2) u32 + u) mass
      sigmoid      |ds| <= s (1 - s) |dz| + 4 u s        (a few-ulp exp, the add, the divide, the rounding to T)
      score        ds;   rbox = s * scale: |d| <= scale |ds| + u |rbox|
      a = 2 s - 1  the doubling is exact, the subtraction rounds: |da| <= 2 |ds| + u |a| -- ABSOLUTE: a cancels where s is
                   near 1/2, so relative to |a| this is unbounded (3e6 u was seen in fp32), and it reaches the angle as da / r
      r            two squares, an add, a square root: |dr| / r <= (|a_0| |da_0| + |a_1| |da_1|) / r^2 + 3 u + eta / r^2
      angle_i      a_i / r: |d| <= |da_i| / r + |angle_i| |dr| / r + u |angle_i| + eta
    plus `other`'s own rounding, u |v| + eta / 2."""
    u, eta = UNIT_ROUNDOFF[dtype], SMALLEST_SUBNORMAL[dtype]
    with np.errstate(all="ignore"):
        ds = _stock_ds(R, dtype)
        if R.s.shape[1] == GATE:
            err = ds
        else:
            da = 2 * ds[:, 5:7] + u * np.abs(R.a)
            rel_r = (np.abs(R.a[:, 0:1]) * da[:, 0:1] + np.abs(R.a[:, 1:2]) * da[:, 1:2]) / R.r ** 2 + 3 * u + eta / R.r ** 2
            ang = np.abs(R.a) / R.r
            dang = da / R.r + ang * rel_r + u * ang + eta
            err = np.concatenate([ds[:, 0:1], R.scale * ds[:, 1:5] + u * R.scale * R.s[:, 1:5], dang], axis=1)
    return _shape_like(R, err) + u * R.out64.abs() + eta / 2


def _stock_ds(R, dtype):
    u = UNIT_ROUNDOFF[dtype]
    return R.s * (1 - R.s) * ((R.C + 2) * 2.0 ** -24 + u) * R.mass + 4 * u * R.s


def stock_may_vanish(R, dtype):
    """(N, 7, H, W) bool, true in the two angle channels of the pixels where the stock chain's rounded (a_0, a_1) may both
    be exactly 0 -- |a_i| <= |da_i| of stock_bound for both i -- so that its angle may be 0 / 0 = NaN where the float64
    reference is finite: in 16 bits both sigmoids round to 1/2 long before the float64 ones meet it."""
    with np.errstate(all="ignore"):
        da = 2 * _stock_ds(R, dtype)[:, 5:7] + UNIT_ROUNDOFF[dtype] * np.abs(R.a)
        both = np.all(np.abs(R.a) <= da, axis=1, keepdims=True)
    out = np.zeros(R.s.shape, dtype=bool)
    out[:, 5:7] = both
    return torch.from_numpy(out).reshape(R.out64.shape)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def differing(got, want):
    """Elements whose bits differ (NaN for NaN counts as equal), and whether the NaN positions match."""
    both_nan = got.isnan() & want.isnan()
    return int(((bits(got) != bits(want)) & ~both_nan).sum()), bool(torch.equal(got.isnan(), want.isnan()))


def within(got, ref64, lim):
    """|got - ref64| <= lim on every finite element of the reference; -> (ok, worst error / bound)."""
    finite = ref64.isfinite()
    if not bool(finite.any()):
        return True, 0.0
    err = (got.double() - ref64).abs()[finite]
    lim = lim[finite]
    return bool((err <= lim).all()), float((err / lim).max())


def cat(outs):
    """(score, rbox, angle) or (y,) as one (N, k, H, W) tensor, the layout of Ref.out64."""
    return torch.cat([o.cpu() for o in outs], dim=1)


@functools.lru_cache(maxsize=None)
def problem(shape, dtype):
    """The table's problem for (shape, dtype) with both references, computed once per session and not modified:
    -> x, heads parameters, gate parameters, (heads outputs, Ref), (gate outputs, Ref)."""
    x, hp, gp = random_problem(shape, dtype, seed=sum(shape))
    return x, hp, gp, reference(x, hp), reference(x, gp)
