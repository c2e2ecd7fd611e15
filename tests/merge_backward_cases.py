"""Shared by test_merge_backward_abi.py (CPU) and test_gpu_merge_backward.py: the problems of the native gated merge's
backward and of the stand-alone resize with its backward, their references and bounds, and the mirrors of the
host's rules; no test in here.  The table, the resize, `_axis`, the dtypes and the bit comparison are those of
merge_cases.py, which is imported unchanged; dy is drawn as instancenorm_backward_cases.random_dy draws it.

df and the stand-alone forward -- float64 restatements compared as bits: df = (T)(float)(dy64 * G) with G = resize64(gate)
(1 without a gate), y = (T)(float)resize64(x).

dx = R^T dy and dgate -- the sum of terms and the sum of their absolute values in np.longdouble.  Weights come from
merge_cases._axis: output pixel (Y, X) gives ly0 lx0, ly0 lx1, ly1 lx0, ly1 lx1 to source elements (y0, x0), (y0, x1),
(y1, x0), (y1, x1) -- all four always, so a zero weight against an infinity is NaN and where y1 == y0 both weights meet in
one element.  A term is the double-rounded (wy * wx) * dy for dx, (wy * wx) * (dy * f) for dgate (dy * f is exact in double),
the latter summed over c as well.
    |got - ref| <= 2 u |ref| + 2^-40 sum |terms| + 2^-25
u the unit roundoff of the dtype: one rounding from double to T (2 u leaves room for the half-ulp of a result next to a
binade's edge), a double sum whose longest chain of additions stays below 8192 = 2^13 terms (2^13 * 2^-53), and half the
smallest float16 subnormal.  NaN positions must agree.  Nothing is left out."""
import functools

import numpy as np
import torch

import merge_cases as M
from instancenorm_backward_cases import random_dy

LD = np.longdouble
DTYPES, IDS, UNIT_ROUNDOFF = M.DTYPES, M.IDS, M.UNIT_ROUNDOFF
THREADS = 256
MIN_BLOCK, MAX_BLOCK, MAX_BLOCKS, MAX_FOOTPRINT = 32, 2048, 4096, 4096      # kMgbMinChannels, kMgbMaxBlock, kMgbMaxBlocks, kRsMaxFootprint
NETWORK_PAIRS = ((22, 44), (40, 80), (44, 88), (80, 160), (88, 176), (160, 320), (1023, 700))

# ((N, C, H, W), a's size, the gate's size or None).  Beyond merge_cases.CASES: a gate of f's size with C = 64 (the dgate
# gather is the identity, K = 2 blocks are summed), an ungated merge, 2100 channels on a one-pixel plane of 1024 images
# (the rule asks for one block, the cap makes two: 2048 and 52), and sources of one row / one element (every output row
# reaches element 0).
EXTRA = (
    ((1, 64, 6, 10), (3, 5), (6, 10)),
    ((2, 5, 11, 23), (6, 12), None),
    ((1024, 2100, 1, 1), (1, 1), (1, 1)),
    ((1, 2, 9, 40), (1, 1), (1, 3)),
)
CASES = M.CASES + EXTRA


def case_id(case):
    return "-".join("x".join(str(v) for v in part) if part is not None else "nogate" for part in case)


# --------------------------------------------------------------------------- mirrors of csrc/rroi_merge_backward_host.h
def footprint_bound(n_in, n_out):
    """rs_max_footprint: an upper bound of the output indices that meet in one source index."""
    if n_out == 1:
        return 1
    if n_in == 1:
        return n_out
    return min(n_out, int(2.0 / (np.float64(n_in - 1) / np.float64(n_out - 1))) + 2)


def footprints(n_in, n_out):
    """For every source index i the set {Y : i0(Y) == i or i1(Y) == i} by merge_cases._axis, as sorted lists."""
    i0, i1, _, _ = M._axis(n_in, n_out)
    return [sorted(set(np.nonzero((i0 == i) | (i1 == i))[0].tolist())) for i in range(n_in)]


def merge_backward_plan_of(shape, gate_size):
    """(K, channels per block, tiles, grid, gate tiles, workspace bytes, launches) by plan_merge_backward: plan_merge's rule
    for an `a` of f's size (V = 4) at 256 CUs on every device with at least 32 channels in the last block, then blocks of at
    most 2048 channels."""
    N, C, H, W = shape
    V = 4
    tiles = -(-H * W // (THREADS * V))
    K = 1
    while K < C and N * tiles * K < M.GROUPS_PER_CU * 256:
        K *= 2
    while K > 1 and C - (K - 1) * -(-C // K) < MIN_BLOCK:
        K //= 2
    cb = min(-(-C // K), MAX_BLOCK)
    K = -(-C // cb)
    if gate_size is None:
        return K, cb, tiles, N * K * tiles, 0, 0, 1
    gt = -(-gate_size[0] * gate_size[1] // THREADS)
    return K, cb, tiles, N * K * tiles, gt, -(-(N * K * H * W * 8) // 256) * 256, 3 if K > 1 else 2


def resize_backward_plan_of(N, C, in_size, cus=M.CUS):
    """(K, channels per block, tiles, grid) by plan_resize_backward: a lane per dx element, plan_merge's block rule."""
    tiles = -(-in_size[0] * in_size[1] // THREADS)
    K = 1
    while K < C and N * tiles * K < M.GROUPS_PER_CU * cus:
        K *= 2
    while K > 1 and C - (K - 1) * -(-C // K) < M.MIN_CHANNELS:
        K //= 2
    return K, -(-C // K), tiles, N * K * tiles


# --------------------------------------------------------------------------- references
def expected_resize(x, H, W):
    """The stand-alone forward for a tensor x of any of the dtypes, as a CPU tensor of that dtype."""
    out, _ = M.resize64(x.detach().double().cpu().numpy(), H, W)
    return torch.from_numpy(out).to(x.dtype)


def expected_df(dy, gate, rounded=True):
    """df = dy * G, G the gate resized to dy's plane (None: 1): a CPU tensor of dy's dtype (rounded=False: float64)."""
    d = dy.detach().double().cpu().numpy()
    if gate is not None:
        G, _ = M.resize64(gate.detach().double().cpu().numpy(), *dy.shape[-2:])
        with np.errstate(all="ignore"):
            d = d * G
    out = torch.from_numpy(d)
    return out.to(dy.dtype) if rounded else out


class GatherReference:
    """ref, bound: (N, C', h, w) float64 tensors of R^T v for v (N, C, H, W) float64 (numpy), summed over the channels into
    one (C' = 1) where `reduce_channels`; `check` compares a tensor of `dtype`."""

    def __init__(self, v, in_size, dtype, reduce_channels=False):
        h, w = in_size
        N, C, H, W = v.shape
        Co = 1 if reduce_channels else C
        ref, mag = np.zeros((N, Co, h, w), LD), np.zeros((N, Co, h, w), LD)
        red = (lambda t: t.sum(axis=1, keepdims=True)) if reduce_channels else (lambda t: t)
        with np.errstate(all="ignore"):
            if (h, w) == (H, W):
                ref, mag = red(v.astype(LD)), red(np.abs(v).astype(LD))
            else:
                y0, y1, ly0, ly1 = M._axis(h, H)
                x0, x1, lx0, lx1 = M._axis(w, W)
                for ys, wy in ((y0, ly0), (y1, ly1)):
                    for xs, wx in ((x0, lx0), (x1, lx1)):
                        terms = ((wy[:, None] * wx[None, :]) * v).astype(LD)
                        idx = (slice(None), slice(None), ys[:, None], xs[None, :])
                        np.add.at(ref, idx, red(terms))
                        np.add.at(mag, idx, red(np.abs(terms)))
            lim = 2 * UNIT_ROUNDOFF[dtype] * np.abs(ref) + LD(2.0 ** -40) * mag + LD(2.0 ** -25)
        t = lambda z: torch.from_numpy(np.asarray(z, dtype=np.float64))  # noqa: E731
        self.ref, self.bound = t(ref), t(lim)

    def check(self, got):
        """-> (ok, worst |got - ref| / bound over the finite reference elements); the NaN positions must agree."""
        got = got.detach().cpu()
        assert got.shape == self.ref.shape, (got.shape, self.ref.shape)
        inf = self.ref.isinf()
        nan_ok = bool(torch.equal(got.isnan(), self.ref.isnan())) and bool(torch.equal(got.double()[inf], self.ref[inf]))
        fin = self.ref.isfinite()
        if not bool(fin.any()):
            return nan_ok, 0.0
        ratio = (got.double() - self.ref).abs()[fin] / self.bound[fin]
        return nan_ok and bool((ratio <= 1).all()), float(ratio.max())


def dx_reference(dy, in_size):
    """dx = R^T dy for a tensor dy of any of the dtypes."""
    return GatherReference(dy.detach().double().cpu().numpy(), in_size, dy.dtype)


def dgate_reference(dy, f, gate_size):
    """dgate = R_g^T sum_c dy * f."""
    with np.errstate(all="ignore"):
        v = dy.detach().double().cpu().numpy() * f.detach().double().cpu().numpy()
    return GatherReference(v, gate_size, dy.dtype, reduce_channels=True)


# --------------------------------------------------------------------------- problems
def random_case(case, dtype, seed=None):
    """(a, f, gate or None, dy) of `dtype` on the CPU."""
    shape, a_size, g_size = case
    seed = sum(shape) if seed is None else seed
    a, f, gate = M.random_problem((shape, a_size, g_size or (1, 1)), dtype, seed)
    return a, f, (gate if g_size is not None else None), random_dy(shape, dtype, seed)


@functools.lru_cache(maxsize=None)
def problem(case, dtype):
    """(a, f, gate, dy) of the table's case, computed once per session and not modified."""
    return random_case(case, dtype)


@functools.lru_cache(maxsize=None)
def reference(case, dtype):
    """(expected y = R a, expected df, dx reference for da, dgate reference or None) of the table's case, computed once."""
    a, f, gate, dy = problem(case, dtype)
    H, W = f.shape[-2:]
    return (expected_resize(a, H, W), expected_df(dy, gate), dx_reference(dy, a.shape[-2:]),
            None if gate is None else dgate_reference(dy, f, gate.shape[-2:]))
