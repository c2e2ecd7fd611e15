"""Shared by test_depthwise_backward_abi.py (CPU) and test_gpu_depthwise_backward.py: the problems of the native depthwise
3x3 backward, its oracle for dx, its reference and bound for dweight, and the mirrors of the host's rules; no
test in here.  The shapes, x, the weights, `out_size` and the dtypes are those of depthwise_cases.py, which is imported
unchanged; dy is drawn as instancenorm_backward_cases.random_dy draws it (N(0,1) scaled by 2^(plane % 5 - 2)).

dx -- the oracle is the recipe of include/rroi_align_hip.h section 5b in numpy float64, compared as bits: dy is dilated by
the stride and zero-extended, then nine shifted `acc = acc + w64 * tap` in the order (ky, kx) = (2,2), (2,1) ... (0,0) --
which visits dy in row-major order -- at the positions whose parity the recipe admits (all of them at stride 1), then
`.astype(float32)`; a 16-bit expectation is `.to(dtype)` of that, one plain conversion.

dweight -- the reference is the sum of section 5b in np.longdouble, with the sum of the terms' absolute values beside it:
    |got - ref| <= 2 u |ref| + 2^-40 sum |terms| + 2^-25
u the unit roundoff of the dtype: one rounding from double to T (2 u leaves room for the half-ulp of a result next to a
binade's edge), a double sum whose longest chain of additions stays below 8192 = 2^13 terms (2^13 * 2^-53), and half the
smallest float16 subnormal.  NaN positions must agree.  Nothing is left out."""
import functools

import numpy as np
import torch

import depthwise_cases as D
from instancenorm_backward_cases import random_dy
from instancenorm_cases import UNIT_ROUNDOFF

LD = np.longdouble
THREADS = 256          # a workgroup of every launch (kDwThreads)


def plan_of(N, C, H, W, stride):
    """Mirror of plan_depthwise_backward (csrc/rroi_depthwise_backward_host.h): change both together.  All three launches
    stream rows of dy, TILE_W columns per thread, and take the forward's band rule on dy's planes; the partials launch gives
    every plane ceil(items / 256) workgroups of its own.  -> (band, items per plane, segments)."""
    band = D.band_of(N, C, H, W, stride)
    ho, wo = D.out_size(H, stride), D.out_size(W, stride)
    items = -(-ho // band) * -(-wo // D.TILE_W)
    return band, items, -(-items // THREADS)


def oracle_dx(dy, w, H, W, stride, rounded=True):
    """dy (N,C,Ho,Wo) float32 (a 16-bit tensor widened), w (C,1,3,3) float32 -> dx (N,C,H,W) float32 (rounded=False: the
    float64 accumulator before its rounding, for the comparison with autograd)."""
    d64 = np.asarray(dy, np.float32).astype(np.float64)
    w64 = np.asarray(w, np.float32).astype(np.float64)
    N, C, ho, wo = d64.shape
    s = stride
    assert (ho, wo) == (D.out_size(H, s), D.out_size(W, s))
    ext = np.zeros((N, C, H + 2, W + 2), np.float64)          # index 1 + s * oy, 1 + s * ox; index 0 and H + 1 lie outside
    ext[:, :, 1:2 + s * (ho - 1):s, 1:2 + s * (wo - 1):s] = d64
    rows = (np.arange(H + 2) - 1) % s == 0                     # the positions a tap may read: the right parity, inside or not
    cols = (np.arange(W + 2) - 1) % s == 0
    acc = np.zeros((N, C, H, W), np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for ky in (2, 1, 0):
            for kx in (2, 1, 0):
                tap = ext[:, :, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]          # dilated position (iy + 1 - ky, ix + 1 - kx)
                admit = rows[2 - ky:2 - ky + H, None] & cols[None, 2 - kx:2 - kx + W]
                acc = np.where(admit, acc + w64[None, :, 0, ky, kx, None, None] * tap, acc)
        return acc.astype(np.float32) if rounded else acc


def expected_dx(dy, w, H, W, stride):
    """The expectation for tensors dy, w of one dtype (any device), as a CPU tensor of that dtype."""
    o = oracle_dx(dy.detach().float().cpu().numpy(), w.detach().float().cpu().numpy(), H, W, stride)
    return torch.from_numpy(o).to(dy.dtype)


class DweightReference:
    """ref, bound: (C,1,3,3) float64 tensors for tensors dy (N,C,Ho,Wo) and x (N,C,H,W) of one dtype on the CPU."""

    def __init__(self, dy, x, stride):
        u = UNIT_ROUNDOFF[x.dtype]
        N, C, H, W = x.shape
        ho, wo = dy.shape[2:]
        s = stride
        with np.errstate(all="ignore"):
            dl = dy.double().numpy().astype(LD)
            xp = np.zeros((N, C, H + 2, W + 2), LD)
            xp[:, :, 1:H + 1, 1:W + 1] = x.double().numpy()
            ref, mag = np.zeros((C, 1, 3, 3), LD), np.zeros((C, 1, 3, 3), LD)
            for ky in range(3):
                for kx in range(3):
                    terms = dl * xp[:, :, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s]
                    ref[:, 0, ky, kx] = terms.sum(axis=(0, 2, 3))
                    mag[:, 0, ky, kx] = np.abs(terms).sum(axis=(0, 2, 3))
            lim = 2 * u * np.abs(ref) + LD(2.0 ** -40) * mag + LD(2.0 ** -25)
        t = lambda z: torch.from_numpy(np.asarray(z, dtype=np.float64))
        self.ref, self.bound = t(ref), t(lim)

    def check(self, got):
        """-> (ok, worst |got - ref| / bound over the finite reference elements); the NaN positions must agree."""
        got = got.detach().cpu()
        nan_ok = bool(torch.equal(got.isnan(), self.ref.isnan()))
        fin = self.ref.isfinite()
        if not bool(fin.any()):
            return nan_ok, 0.0
        ratio = (got.double() - self.ref).abs()[fin] / self.bound[fin]
        return nan_ok and bool((ratio <= 1).all()), float(ratio.max())


# dx at stride 2: H and W both even, both odd, mixed -- the even sizes are where the last dx row and column see a dy outside
# -- are (1,2,4,8), (1,2,5,9) of the forward's table and (1,3,6,7); W = 15, 16, 17 is one below, at and above two of a
# thread's eight dx columns.
# dweight partials, from plan_of: one workgroup per plane is most of the forward's table; (1,1,514,4) at stride 1 has 257
# items -- one more than a workgroup -- and (3,2,54,76) has 513 with N = 3, so three segments per plane in the finish's
# (n, segment) order; (3,2,107,76) at stride 2 has 270; (3,33,5,17) of the forward's table has 15 items per plane, of
# which seventeen planes' worth would fit one workgroup: it checks that workgroups are plane-aligned.
EXTRA = [((1, 3, 6, 7), 2), ((1, 2, 9, 15), 2), ((1, 2, 9, 16), 2), ((1, 2, 9, 17), 2), ((1, 2, 9, 16), 1),
         ((1, 1, 514, 4), 1), ((3, 2, 54, 76), 1), ((3, 2, 107, 76), 2)]
CASES = list(dict.fromkeys(D.CASES + EXTRA))
case_id = D.case_id


def random_case(case, dtype, seed=None):
    """(x, w, dy) of `dtype` on the CPU for ((N,C,H,W), stride)."""
    (N, C, H, W), s = case
    seed = sum((N, C, H, W)) + s if seed is None else seed
    x, w = D.random_problem((N, C, H, W), dtype, seed)
    return x, w, random_dy((N, C, D.out_size(H, s), D.out_size(W, s)), dtype, seed)


@functools.lru_cache(maxsize=12)
def problem(case, dtype):
    """(x, w, dy) of the table's case, computed once and not modified."""
    return random_case(case, dtype)


@functools.lru_cache(maxsize=12)
def reference(case, dtype):
    """(expected dx, DweightReference) of the table's case, computed once and not modified."""
    x, w, dy = problem(case, dtype)
    return expected_dx(dy, w, x.size(2), x.size(3), case[1]), DweightReference(dy, x, case[1])
