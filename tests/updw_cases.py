"""Shared by test_remainder_abi.py (CPU) and test_gpu_updw.py: the case table of the fused bilinear resize + depthwise 3x3
 and its float64 reference.

The reference is the composition of two references the project already has, not a third restatement:
    U   = resize64(a) of merge_cases.py (header section 8's resize in numpy float64, separate multiplies and adds),
          rounded once to the tensors' type by torch (`.to(dtype)`, through fp32 as the kernel's `(T)(float)value`);
    y   = oracle_depthwise3x3(U, w, 1) of depthwise_cases.py (header section 5's recipe), rounded once likewise.
Nothing in either is transcendental or reduced in an order the kernel may choose, so the kernel reproduces it bit for bit:
that is the parity bar, derived and not measured.  `restated` is the same arithmetic written element by element the way the
header's section 13 states it, for the CPU test that the two agree.
"""
import functools

import numpy as np
import torch

from depthwise_cases import band_of, oracle_depthwise3x3
from merge_cases import _axis, bits, differing, resize64  # noqa: F401  (one definition of each)

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
IDS = ("fp32", "bf16", "fp16")

# ((N, C, h, w), (Ho, Wo)).  A thread owns 4 output columns over a band of 2, 4 or 8 output rows (band_of on the OUTPUT's
# size: the rule of the depthwise kernel).
CASES = (
    ((1, 1, 5, 7), (10, 14)),          # twice the size, one plane
    ((2, 3, 3, 4), (5, 7)),            # a non-integer ratio, six planes
    ((1, 6, 6, 9), (6, 9)),            # equal sizes: the source is read as it is
    ((1, 2, 5, 7), (1, 14)),           # a target of one row (scale 0 along y)
    ((1, 2, 5, 7), (10, 1)),           # a target of one column: Wo = 1
    ((1, 6, 1, 1), (4, 13)),           # a 1x1 source; Wo = 13: three strips and a tail of one, an odd width
    ((1, 1, 2, 2), (3, 3)),            # Wo = 3: a single partial strip
    ((2, 3, 9, 5), (19, 13)),          # Ho = 19 in bands of 2, the alignment changes from row to row
    ((1, 6, 7, 9), (4, 5)),            # a reduction on both axes: source rows are skipped
    ((1, 2, 4, 6), (4, 11)),           # one axis equal, the other resized: both go through the resize
    ((1, 5462, 9, 6), (19, 13)),       # the fewest planes that run bands of 8: Ho = 19 crosses two band borders
    ((1, 3300, 9, 6), (19, 13)),       # bands of 4
)
BANDS_REACHED = {2, 4, 8}
SMALL = tuple(c for c in CASES if c[0][0] * c[0][1] * c[1][0] * c[1][1] <= 4096)   # what a Python loop restates in a moment

# the two resizes of FOTSNet in front of upconv1 / upconv2 on a 704 x 1280 image: (C, h, w, Ho, Wo)
NETWORK_SHAPES = ((256, 44, 80, 88, 160), (256, 88, 160, 176, 320))


def case_id(case):
    return "-".join("x".join(str(v) for v in part) for part in case)


def band_of_case(case):
    (N, C, _, _), (Ho, Wo) = case
    return band_of(N, C, Ho, Wo, 1)


def resized(a, size):
    """U: `a` resized to `size` in float64 and rounded once to a's dtype (a CPU tensor of that dtype)."""
    U, _ = resize64(a.double().numpy(), *size)
    return torch.from_numpy(U).to(a.dtype)


def reference(a, w, size):
    """-> y of a's dtype: the depthwise oracle on the rounded resized map."""
    U = resized(a, size)
    return torch.from_numpy(oracle_depthwise3x3(U.float().numpy(), w.float().numpy(), 1)).to(a.dtype)


def restated(a, w, size):
    """Header section 13 element by element in float64: per output the nine taps in (ky, kx) order, each tap the blend of
    its four source values in section 8's order rounded to the type, a tap outside U `w * (+0.0)`."""
    dtype = a.dtype
    N, C, h, wi = a.shape
    Ho, Wo = size
    a64, w64 = a.double().numpy(), w.double().numpy()
    same = (h, wi) == (Ho, Wo)
    y0, y1, ly0, ly1 = _axis(h, Ho)
    x0, x1, lx0, lx1 = _axis(wi, Wo)

    def u(p, Y, X):
        if same:
            return p[Y, X]
        with np.errstate(all="ignore"):
            top = lx0[X] * p[y0[Y], x0[X]] + lx1[X] * p[y0[Y], x1[X]]
            bot = lx0[X] * p[y1[Y], x0[X]] + lx1[X] * p[y1[Y], x1[X]]
            v = ly0[Y] * top + ly1[Y] * bot
        return np.float64(torch.tensor(v, dtype=torch.float64).to(dtype).double().item())

    out = np.zeros((N, C, Ho, Wo), np.float64)
    for n in range(N):
        for c in range(C):
            p = a64[n, c]
            for Y in range(Ho):
                for X in range(Wo):
                    acc = np.float64(0.0)
                    for ky in range(3):
                        for kx in range(3):
                            r, q = Y + ky - 1, X + kx - 1
                            tap = u(p, r, q) if 0 <= r < Ho and 0 <= q < Wo else np.float64(0.0)
                            with np.errstate(all="ignore"):
                                acc = acc + w64[c, 0, ky, kx] * tap
                    out[n, c, Y, X] = acc
    with np.errstate(all="ignore"):
        return torch.from_numpy(out.astype(np.float32)).to(dtype)


def tapped_by(case, i, j):
    """(Ho, Wo) bool: the elements of U whose blend reads source element (i, j) -- no tap is skipped, whatever its weight."""
    (_, _, h, w), (Ho, Wo) = case
    if (h, w) == (Ho, Wo):
        m = np.zeros((Ho, Wo), bool)
        m[i, j] = True
        return m
    y0, y1, _, _ = _axis(h, Ho)
    x0, x1, _, _ = _axis(w, Wo)
    return ((y0 == i) | (y1 == i))[:, None] & ((x0 == j) | (x1 == j))[None, :]


def window_of(mask):
    """(Ho, Wo) bool -> the outputs whose 3x3 window holds a marked element."""
    Ho, Wo = mask.shape
    p = np.zeros((Ho + 2, Wo + 2), bool)
    p[1:-1, 1:-1] = mask
    out = np.zeros((Ho, Wo), bool)
    for ky in range(3):
        for kx in range(3):
            out |= p[ky:ky + Ho, kx:kx + Wo]
    return out


def random_problem(case, dtype, seed):
    """N(0, 1) data and weights of `dtype` on the CPU."""
    (N, C, h, w), _ = case
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, C, h, w, generator=g).to(dtype), torch.randn(C, 1, 3, 3, generator=g).to(dtype)


@functools.lru_cache(maxsize=None)
def problem(case, dtype):
    """The table's problem for (case, dtype) with its reference, computed once per session and not modified: -> a, w, y."""
    a, w = random_problem(case, dtype, seed=sum(case[0]) + sum(case[1]))
    return a, w, reference(a, w, case[1])
