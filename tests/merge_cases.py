"""Shared by test_merge_abi.py (CPU) and test_gpu_merge.py: the case table of the native gated merge, its
float64 reference, the mirrored plan rule and the bound of the comparison with the stock chain.

The reference is numpy in float64, written with separate multiplies and adds in the order of header section 8 (no lerp,
no addcmul, no einsum): per axis s = (in - 1) / (out - 1) (0 where out == 1), src = s * dst, i0 = min(int(src), in - 1),
i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1; value = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
z = A + f * G (no gate: A + f); a source of f's size is read as it is.  z is rounded once by torch (`.to(dtype)`, which goes
through fp32 for the 16-bit types exactly as the kernel's `(T)(float)z` does).  Nothing in it is transcendental or
reduced, so the kernel reproduces it bit for bit: that is the parity bar, derived and not measured.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
IDS = ("fp32", "bf16", "fp16")
UNIT_ROUNDOFF = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SMALLEST_SUBNORMAL = {torch.float32: 2.0 ** -149, torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}

# The plan rule of csrc/rroi_merge_host.h (plan_merge), mirrored: change both together.
CUS = 256                   # MI355X, and what the library assumes where there is no GPU
THREADS, GROUPS_PER_CU, MIN_CHANNELS = 256, 4, 8


def plan_of(shape, a_size, dtype, cus=CUS):
    """(V, K) by the mirrored rule: V pixels per lane, K channel blocks of ceil(C / K) channels."""
    N, C, H, W = shape
    V = 4 if tuple(a_size) == (H, W) else 2                       # (the dtype does not enter the rule today)
    tiles = -(-H * W // (THREADS * V))
    K = 1
    while K < C and N * tiles * K < GROUPS_PER_CU * cus:
        K *= 2
    while K > 1 and C - (K - 1) * -(-C // K) < MIN_CHANNELS:
        K //= 2
    return V, K


# ((N, C, H, W), a's size, the gate's size)
CASES = (
    ((1, 1, 1, 1), (1, 1), (1, 1)),                 # the smallest case
    ((2, 3, 7, 9), (3, 4), (3, 4)),                 # an odd plane
    ((2, 5, 11, 23), (6, 12), (5, 11)),             # the sizes differ, the alignment moves per channel
    ((1, 4, 1, 37), (1, 9), (1, 9)),                # one row
    ((1, 4, 37, 1), (9, 1), (9, 1)),                # one column
    ((3, 256, 16, 24), (8, 12), (8, 12)),           # several channel groups: K = 32, blocks of 8
    ((1, 7, 44, 80), (22, 40), (22, 40)),           # 2x up
    ((2, 6, 4, 5), (9, 7), (9, 7)),                 # downscale on both axes
    ((1, 5, 29, 31), (29, 31), (15, 16)),           # a as it is
    ((1, 3, 176, 320), (88, 160), (88, 160)),       # many tiles
    ((1, 2, 23, 700), (12, 1023), (12, 1023)),      # a long source axis
    # beyond the issue's table: the branches of the rule and the kernel that none of the above reaches
    ((1, 19, 5, 7), (3, 4), (3, 4)),                # K = 2 with unequal blocks (10 and 9 channels), a is resized
    ((2, 21, 9, 13), (9, 13), (9, 13)),             # K = 2 (11 and 10), a and the gate both as they are, an odd plane
    ((1, 64, 6, 10), (6, 10), (3, 5)),              # K = 8 with a as it is: four pixels per lane in several channel groups
    ((1, 9, 40, 52), (40, 52), (20, 26)),           # a as it is, three tiles of 1024 pixels, the last partial
)


def case_id(case):
    return "-".join("x".join(str(v) for v in part) for part in case)


def _axis(n_in, n_out):
    s = 0.0 if n_out == 1 else np.float64(n_in - 1) / np.float64(n_out - 1)
    src = s * np.arange(n_out, dtype=np.float64)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0
    l0 = 1.0 - l1
    return i0, i1, l0, l1


def resize64(v, H, W):
    """(..., h, w) float64 -> ((..., H, W) float64, the largest tap magnitude per output element)."""
    h, w = v.shape[-2:]
    if (h, w) == (H, W):
        return v.copy(), np.abs(v)
    y0, y1, ly0, ly1 = _axis(h, H)
    x0, x1, lx0, lx1 = _axis(w, W)
    v00 = v[..., y0[:, None], x0[None, :]]
    v01 = v[..., y0[:, None], x1[None, :]]
    v10 = v[..., y1[:, None], x0[None, :]]
    v11 = v[..., y1[:, None], x1[None, :]]
    with np.errstate(all="ignore"):
        top = lx0 * v00
        t2 = lx1 * v01
        top = top + t2
        bot = lx0 * v10
        b2 = lx1 * v11
        bot = bot + b2
        r = ly0[:, None] * top
        r2 = ly1[:, None] * bot
        out = r + r2
    M = np.maximum(np.maximum(np.abs(v00), np.abs(v01)), np.maximum(np.abs(v10), np.abs(v11)))
    return out, M


class Ref:
    """`out64` (N, C, H, W) float64 before any rounding; `Ma`, `Mg` the largest tap magnitudes of `a` and of the gate per
    element (|a| where a is read as it is; 1 without a gate); `absf` = |f|."""


def reference(a, f, gate=None):
    """-> (y rounded to f's dtype by torch, Ref)."""
    H, W = f.shape[-2:]
    R = Ref()
    A, R.Ma = resize64(a.double().numpy(), H, W)
    fd = f.double().numpy()
    R.absf = np.abs(fd)
    with np.errstate(all="ignore"):
        if gate is None:
            z = A + fd
            R.Mg = np.ones_like(fd[:, :1])
        else:
            G, R.Mg = resize64(gate.double().numpy(), H, W)
            p = fd * G
            z = A + p
    R.out64 = torch.from_numpy(z)
    return R.out64.to(f.dtype), R


def _E(h, w, u):
    return u + 8 * 2.0 ** -24 + 2.0 ** -22 * (h + w)


def stock_bound(a, f, gate, R):
    """What |stock - rounded reference| may be, per element, where `stock` is the stock chain `up(a) + f * up(gate)` run in
    T = f's dtype with every operation rounding to T.

    With u = u_T, u32 = 2^-24 and eta = T's smallest subnormal, a resized source of size (h, w) carries
        E(h, w) = u + 8 u32 + 2^-22 (h + w)
    relative to its largest tap M: 2^-22 (h + w) for coordinates computed in fp32 (an error of at most 2^-23 (in - 1) per
    axis, times a tap difference of at most 2 M), 8 u32 for the interpolation arithmetic in fp32, u for the resize's
    rounding to T; E = 0 where the source is read as it is.  Then
        lim = (1 + 2^-6) [ Ma (E_a + 2 u) + |f| Mg (E_g + 3 u) ] + 4 eta       (without a gate the second term is 2 u |f|)
    covers the resize's, the product's, the sum's and the reference's own rounding.  An index flip at a near-integer src
    is harmless: bilinear interpolation is continuous."""
    dtype = f.dtype
    u, eta = UNIT_ROUNDOFF[dtype], SMALLEST_SUBNORMAL[dtype]
    ea = 0.0 if a.shape[-2:] == f.shape[-2:] else _E(*a.shape[-2:], u)
    if gate is None:
        lim = (1 + 2.0 ** -6) * (R.Ma * (ea + 2 * u) + R.absf * 2 * u) + 4 * eta
    else:
        eg = 0.0 if gate.shape[-2:] == f.shape[-2:] else _E(*gate.shape[-2:], u)
        lim = (1 + 2.0 ** -6) * (R.Ma * (ea + 2 * u) + R.absf * R.Mg * (eg + 3 * u)) + 4 * eta
    return torch.from_numpy(np.broadcast_to(lim, R.out64.shape).copy())


def stock(a, f, gate=None):
    """The stock chain of `FOTSNet._merge` for one merge, on the tensors' device and in their dtype."""
    up = lambda t: t if t.shape[-2:] == f.shape[-2:] else F.interpolate(  # noqa: E731
        t, size=f.shape[-2:], mode="bilinear", align_corners=True)
    return up(a) + f if gate is None else up(a) + f * up(gate)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def differing(got, want):
    """Elements whose bits differ (NaN for NaN counts as equal), and whether the NaN positions match."""
    both_nan = got.isnan() & want.isnan()
    return int(((bits(got) != bits(want)) & ~both_nan).sum()), bool(torch.equal(got.isnan(), want.isnan()))


def within(got, ref, lim):
    """|got - ref| <= lim on every finite element of the reference; -> (ok, worst error / bound)."""
    finite = ref.isfinite() & lim.isfinite()
    if not bool(finite.any()):
        return True, 0.0
    err = (got.double() - ref.double()).abs()[finite]
    lim = lim[finite]
    return bool((err <= lim).all()), float((err / lim).max())


def random_problem(case, dtype, seed):
    """a, f = N(0, 1), gate = U(0, 1), rounded to `dtype` (the reference sees the rounded values)."""
    (N, C, H, W), (ah, aw), (gh, gw) = case
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(N, C, ah, aw, generator=g).to(dtype)
    f = torch.randn(N, C, H, W, generator=g).to(dtype)
    gate = torch.rand(N, 1, gh, gw, generator=g).to(dtype)
    return a, f, gate


@functools.lru_cache(maxsize=None)
def problem(case, dtype):
    """The table's problem for (case, dtype) with both references, computed once per session and not modified:
    -> a, f, gate, (gated y, Ref), (ungated y, Ref)."""
    a, f, gate = random_problem(case, dtype, seed=sum(case[0]))
    return a, f, gate, reference(a, f, gate), reference(a, f, None)
