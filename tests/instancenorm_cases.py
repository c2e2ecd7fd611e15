"""Shared by test_instancenorm_abi.py (CPU) and test_gpu_instancenorm.py: the case table of the native InstanceNorm2d
(DESIGN 5.11), its reference, and the bound of the comparison.

The reference is built the way the contract's own check was: mean and biased variance of every (n, c) plane in two
passes in np.longdouble, a = gamma / sqrt(var + eps) and b = beta - mean * a and the map x * a + b in float64, rounded to
fp32 by torch, the activation `v < 0 ? v * slope : v` in fp32, one conversion to the tensor's type by torch.  (A float64
reference that computes s2 / n - mean^2 itself is wrong at the |mean| / std the table reaches.)
"""
import functools

import numpy as np
import torch

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
IDS = ("fp32", "bf16", "fp16")
UNIT_ROUNDOFF = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SLOPES = (1.0, 0.0, 0.01)
EPS = 1e-5

# The form rule of csrc/rroi_instancenorm_host.h (plan_instancenorm), mirrored: change both together.
PLANE, SPLIT = 1, 2
SPLIT_MIN_PLANE = 32768     # elements: a plane below it is never split
SEG_QUANTUM, MIN_SEG, MAX_SEGS, WG_PER_CU = 2048, 8192, 256, 8
CUS = 256                   # MI355X, and what the library assumes where there is no GPU


def plan_of(N, C, H, W, cus=CUS):
    """(form, segments, segment_elems) by the mirrored rule."""
    planes, n = N * C, H * W
    if planes >= cus or n < SPLIT_MIN_PLANE:
        return PLANE, 1, n
    want = min(MAX_SEGS, -(-WG_PER_CU * cus // planes))
    seg = max(MIN_SEG, -(-(-(-n // want)) // SEG_QUANTUM) * SEG_QUANTUM)
    return SPLIT, -(-n // seg), seg


# (N, C, H, W).  Vectors are 4 (fp32) / 8 (16-bit) elements and a workgroup has 256 lanes with 4 vectors in flight each:
# planes of one element, below one vector, around 1024 elements (one fp32 vector per lane), odd planes whose base
# alignment changes from plane to plane, one below / at / one above the split threshold (32767 also runs the unrolled
# loop of the plane form 7 times), a split plane whose last segment is one element, and a split call with N, C > 1.
CASES = (
    (2, 3, 1, 1),
    (2, 3, 7, 9),
    (1, 2, 33, 31),      # 1023
    (1, 2, 32, 32),      # 1024
    (1, 2, 25, 41),      # 1025
    (3, 5, 24, 40),      # 960: layer4's plane at a small input, 15 planes
    (1, 2, 217, 151),    # 32767: the largest plane of the plane form with few planes
    (1, 2, 128, 256),    # 32768: split, 4 whole segments
    (1, 2, 99, 331),     # 32769: split, the fifth segment holds one element
    (2, 2, 128, 257),    # 32896: split, N > 1 and C > 1, odd width
)


def case_id(shape):
    return "x".join(str(v) for v in shape)


def random_problem(shape, dtype, seed):
    """x = N(0,1) * scale + offset per plane, |offset| / scale cycling through 0, 1, 100, 10^4 (scale 2^-3 .. 2^2), and
    gamma, beta; all rounded to `dtype` (the reference sees the rounded values)."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    planes = N * C
    k = torch.arange(planes)
    scale = 2.0 ** ((k % 6).double() - 3)
    ratio = torch.tensor([0.0, 1.0, 100.0, 1e4], dtype=torch.float64)[(k + seed) % 4]
    sign = torch.where((k // 4) % 2 == 0, 1.0, -1.0).double()
    x = torch.randn(planes, H * W, generator=g, dtype=torch.float64) * scale[:, None] + (sign * ratio * scale)[:, None]
    gamma = torch.randn(C, generator=g, dtype=torch.float64) * 0.5 + 1.0
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    return x.view(N, C, H, W).to(dtype), gamma.to(dtype), beta.to(dtype)


def plane_statistics(x):
    """mean, biased variance per plane, two passes in np.longdouble, returned as float64 (N, C, 1, 1)."""
    xl = x.double().numpy().astype(np.longdouble)
    with np.errstate(all="ignore"):
        mean = xl.mean(axis=(2, 3), keepdims=True)
        var = ((xl - mean) ** 2).mean(axis=(2, 3), keepdims=True)
    return mean.astype(np.float64), var.astype(np.float64)


def reference(x, gamma=None, beta=None, eps=EPS, slope=1.0, stats=None):
    """-> (out of x's dtype, ref64 (the float64 value before any rounding, activation applied), a, b (float64,
    (N, C, 1, 1)))."""
    N, C, H, W = x.shape
    mean, var = stats if stats is not None else plane_statistics(x)
    g = np.ones(C) if gamma is None else gamma.double().numpy()
    bt = np.zeros(C) if beta is None else beta.double().numpy()
    with np.errstate(all="ignore"):
        a = g.reshape(1, C, 1, 1) / np.sqrt(var + np.float64(eps))
        b = bt.reshape(1, C, 1, 1) - mean * a
        v64 = x.double().numpy() * a + b
    s32 = np.float32(slope)
    v32 = torch.from_numpy(v64).float()
    v32 = torch.where(v32 < 0, v32 * torch.tensor(s32), v32)
    with np.errstate(all="ignore"):
        ref64 = np.where(v64 < 0, v64 * np.float64(s32), v64)
    return v32.to(x.dtype), torch.from_numpy(ref64), torch.from_numpy(a), torch.from_numpy(b)


def bound(x, a, b):
    """2 u (|x a| + |b|) + 2^-25, u the unit roundoff of x's dtype: what condition (a) allows |got - ref64| to be."""
    return 2 * UNIT_ROUNDOFF[x.dtype] * ((x.double() * a).abs() + b.abs()) + 2.0 ** -25


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def differing(got, want):
    """Elements whose bits differ (NaN for NaN counts as equal), and whether the NaN positions match."""
    both_nan = got.isnan() & want.isnan()
    return int(((bits(got) != bits(want)) & ~both_nan).sum()), bool(torch.equal(got.isnan(), want.isnan()))


def within_bound(got, ref64, x, a, b):
    """Condition (a) on every finite element of the reference; -> (ok, worst |got - ref64| / bound)."""
    finite = ref64.isfinite()
    if not bool(finite.any()):
        return True, 0.0
    err = (got.double() - ref64).abs()[finite]
    lim = bound(x, a, b)[finite]
    return bool((err <= lim).all()), float((err / lim).max())


@functools.lru_cache(maxsize=None)
def problem(shape, dtype, seed=None):
    """The table's problem for (shape, dtype) with its plane statistics, computed once per session and not modified."""
    x, gamma, beta = random_problem(shape, dtype, seed=sum(shape) if seed is None else seed)
    return x, gamma, beta, plane_statistics(x)
