"""Shared by test_recogniser_abi.py (CPU) and test_gpu_recogniser.py: the case tables of the native recogniser head and of
the activation + (2,1) max-pool, the mirrored plan rule, the float64 references and the head's error bound.

The head's reference is numpy in float64: z = w @ x + b, m = max_k z, L = m + log(sum_k exp(z_k - m)), out = z - L; rounded
once by torch (`.to(dtype)`, which goes through fp32 for the 16-bit types exactly as the kernel's `(T)(float)v` does).
The pool's reference restates the kernel's rule with torch on the CPU; test_recogniser_abi.py shows that it equals
`F.max_pool2d(F.leaky_relu(x, s), (2, 1), stride=(2, 1))` bit for bit.
"""
import functools
import math

import numpy as np
import torch

from heads_cases import DTYPES, IDS, SMALLEST_SUBNORMAL, UNIT_ROUNDOFF, bits, differing, within  # noqa: F401  (re-exported)

# The plan rule of csrc/rroi_recogniser_host.h (plan_ocr_head), mirrored: change both together.
CLASS_BLOCK, ROW_CLASSES, TILE_COLUMNS, MAX_CLASSES, CHUNK = 32, 8, 16, 128, 32


def head_plan_of(N, C, K, T):
    """(waves S, tiles per crop, grid, LDS bytes) by the mirrored rule."""
    S, tiles = -(-K // CLASS_BLOCK), -(-T // TILE_COLUMNS)
    return S, tiles, N * tiles, 8 * max(64 * S, TILE_COLUMNS * K)


# (N, C, K, T, seed).  C in {1, 5, 255, 256}: fewer channels than a chunk of 32, a remainder of the last chunk, whole chunks (an
# even number: the two load buffers; the views test runs 37 channels, two chunks with a tail, and the poison test 70).  K in {1, 2, 63, 64, 65, 87, 88, 128}: one row of lanes with a tail,
# a last row of 7 / 8 / 1 classes, rows without a class, the network's 87, the limit.  T in {1, 31, 32, 33, 64, 65, 130}:
# less than a tile of 16, whole tiles, a tail of 1, 2 or 15 columns; odd T moves a 16-bit row's alignment from channel to
# channel.  N in {1, 3}.  The four (24, 256, 87, 128) problems -- the network's
# head on 24 crops of the widest bucket -- bring the table above 10^6 outputs.
HEAD_CASES = (
    (1, 1, 1, 1, 1),
    (3, 5, 2, 31, 2),
    (1, 255, 63, 32, 3),
    (1, 256, 64, 33, 4),
    (3, 5, 65, 64, 5),
    (1, 256, 87, 65, 6),
    (1, 255, 88, 130, 7),
    (3, 1, 128, 33, 8),
    (1, 256, 128, 64, 9),
    (3, 256, 87, 130, 10),
    (1, 5, 87, 1, 11),
    (1, 1, 63, 65, 12),
    (3, 255, 2, 130, 13),
    (1, 5, 1, 32, 14),
    (3, 256, 1, 31, 15),
    (1, 255, 64, 1, 16),
    (24, 256, 87, 128, 17),
    (24, 256, 87, 128, 18),
    (24, 256, 87, 128, 19),
    (24, 256, 87, 128, 20),
)
# what the recogniser runs: (C, K) of conv11, T of the pipeline's buckets
NETWORK_HEAD_SHAPES = tuple((n, 256, 87, t) for n in (1, 8, 24, 192) for t in (32, 40, 64, 128))


def case_id(case):
    return "x".join(str(v) for v in case)


def head_problem_of(N, C, K, T, dtype, seed, bias=True):
    """x = N(0,1); w = N(0,1) * {1, 4} / sqrt(C), the factor alternating over the classes; b = N(0,1); all rounded to
    `dtype` (the reference sees the rounded values).  -> x (N, C, 1, T), w (K, C, 1, 1), b (K) or None."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, 1, T, generator=g, dtype=torch.float64)
    factor = torch.tensor([(1.0, 4.0)[(k + seed) % 2] for k in range(K)], dtype=torch.float64)[:, None] / C ** 0.5
    w = torch.randn(K, C, generator=g, dtype=torch.float64) * factor
    b = torch.randn(K, generator=g, dtype=torch.float64)
    return x.to(dtype), w.to(dtype).reshape(K, C, 1, 1), (b.to(dtype) if bias else None)


class HeadRef:
    """The float64 values of one call and what the bound needs: `out64` (N, K, T) before any rounding, `mass` = |b| + sum
    |w x| per logit, `L` the log-sum-exp per column, C and K."""


def head_reference(x, w, b):
    """-> (the output rounded to x's dtype by torch, HeadRef)."""
    N, C, T = x.size(0), x.size(1), x.size(-1)
    K = w.size(0)
    X = x.detach().double().reshape(N, C, T).numpy()
    W = w.detach().double().reshape(K, C).numpy()
    B = np.zeros(K) if b is None else b.detach().double().reshape(K).numpy()
    R = HeadRef()
    with np.errstate(all="ignore"):
        z = W[None] @ X + B[None, :, None]
        R.mass = np.abs(W)[None] @ np.abs(X) + np.abs(B)[None, :, None]
        m = z.max(axis=1, keepdims=True)
        L = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
        out = z - L
    R.L, R.C, R.K = L, C, K
    R.out64 = torch.from_numpy(out)
    return R.out64.to(x.dtype), R


def head_bound(R, dtype):
    """What |got - out64| may be, per element (the shape of out64), with eps = 2^-53, the unit roundoff of double.

    The logits.  The products are exact; z_k is a chain of C + 1 double additions (the bias first), each rounded once:
      |dz_k| <= gamma_{C+1} mass_k <= (C + 2) eps mass_k,   mass_k = |b_k| + sum_c |w_kc x_c|.
    The log-sum-exp.  As a function of the logits it moves by at most max_j |dz_j| (its gradient is a probability vector).
    Its own arithmetic, with s = sum_j e_j >= 1 (the maximum's term is exp(0) = 1):
      d_j = z_j - m       rounds once: the exponent moves by eps |d_j|, e_j by e_j |d_j| eps <= 0.37 eps in absolute terms
      exp                 the device library's double exp is specified to 1 ulp; 2 ulp = 4 eps relative are allowed for
      the K-term sum      (K - 1) eps relative, every term being positive
                          together |ds| / s <= (1.37 K + 4) eps, which is what log s moves by
      log                 likewise 2 ulp = 4 eps relative of log s <= log K <= 4.86: below 20 eps
      L = m + log s       rounds once: eps |L|
    so |dL| <= max_j |dz_j| + (1.37 K + 24) eps + eps |L|, for which (2 K + 32) eps + eps |L| is taken.
    The output.  z_k - L rounds once in double (eps |out|), once to fp32 and (16-bit types) once more to T:
    (u_T + 2^-24) |out|, and half the smallest subnormal of T where the value is below T's normal range."""
    u, eps = UNIT_ROUNDOFF[dtype] + (0.0 if dtype == torch.float32 else 2.0 ** -24), 2.0 ** -53
    with np.errstate(all="ignore"):
        mass = np.where(np.isfinite(R.mass), R.mass, 0.0)          # an inf in the column: its outputs are not finite
        dz = (R.C + 2) * eps * mass
        L = np.where(np.isfinite(R.L), np.abs(R.L), 0.0)
        out = np.abs(R.out64.numpy())
        prop = dz + dz.max(axis=1, keepdims=True) + (2 * R.K + 32) * eps + eps * (L + np.where(np.isfinite(out), out, 0.0))
    return u * R.out64.abs() + SMALLEST_SUBNORMAL[dtype] / 2 + torch.from_numpy(np.ascontiguousarray(prop))


@functools.lru_cache(maxsize=None)
def head_problem(case, dtype):
    """The table's problem for (case, dtype) with its reference, computed once per session and not modified:
    -> x, w, b, the rounded reference, HeadRef."""
    N, C, K, T, seed = case
    x, w, b = head_problem_of(N, C, K, T, dtype, seed)
    return (x, w, b) + head_reference(x, w, b)


# ---------------------------------------------------------------- the pool
SLOPES = (1.0, 0.01, 0.0)
# (N, C, H, W): H in {2, 3, 5, 11} (one output row, an odd last row that is dropped, the network's 11 -> 5 and 5 -> 2);
# W in {1, 7, 32, 33, 40}: less than a vector, whole vectors, a tail, rows whose alignment moves (odd W; 40 * 2 bytes with an
# odd row count).  The last two cases exceed one workgroup of 256 threads in every dtype.
POOL_CASES = (
    (1, 1, 2, 1),
    (1, 3, 3, 7),
    (2, 1, 5, 32),
    (1, 3, 11, 33),
    (2, 3, 11, 40),
    (1, 1, 3, 1),
    (2, 3, 2, 33),
    (1, 3, 5, 40),
    (3, 1, 11, 7),
    (4, 3, 11, 40),
    (2, 64, 5, 33),
)


def pool_problem(case, dtype, seed=0):
    """Normal values salted with +-0, +-1, +-inf and NaN (a quarter of the elements), so that ties -- signed zeros among
    them, more of them after a slope of 0.0 -- and NaNs meet in either row of a pair.  The first columns of the first two
    rows hold every ordered pair of (+0, -0, NaN, 1) where the plane is wide enough."""
    N, C, H, W = case
    g = torch.Generator().manual_seed(1000 + seed + sum(case))
    x = torch.randn(N, C, H, W, generator=g)
    special = torch.tensor([0.0, -0.0, 1.0, -1.0, float("inf"), -float("inf"), float("nan"), -0.5])
    pick = torch.randint(0, 32, (N, C, H, W), generator=g)
    x = torch.where(pick < 8, special[pick.clamp(max=7)], x)
    pairs = [(a, b) for a in (0.0, -0.0, float("nan"), 1.0) for b in (0.0, -0.0, float("nan"), 1.0)]
    for j, (a, b) in enumerate(pairs[:W]):
        x[0, 0, 0, j], x[0, 0, 1, j] = a, b
    return x.to(dtype)


def pool_reference(x, slope):
    """The kernel's rule, restated: the activation in fp32 and rounded once; the lower row's element where it is greater
    or a NaN, the upper row's otherwise."""
    Ho = x.size(2) // 2
    v = x.float()
    act = torch.where(v < 0, v * slope, v).to(x.dtype)
    a, c = act[:, :, 0:2 * Ho:2], act[:, :, 1:2 * Ho:2]
    return torch.where((c.float() > a.float()) | c.isnan(), c, a).contiguous()


def pool_stock(x, slope):
    return torch.nn.functional.max_pool2d(torch.nn.functional.leaky_relu(x, slope), (2, 1), stride=(2, 1))


assert MAX_CLASSES == CLASS_BLOCK * 4 and CLASS_BLOCK == 4 * ROW_CLASSES and math.ceil(87 / CLASS_BLOCK) == 3
