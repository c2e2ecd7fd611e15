"""Shared by test_instancenorm_backward_abi.py (CPU) and test_gpu_instancenorm_backward.py: the problems of the native
InstanceNorm2d backward, its reference and the bounds of the comparison.  The shapes, x, gamma and beta are
those of instancenorm_cases.py, which is imported unchanged.

The reference is header section 6c in np.longdouble, from `plane_statistics(x)` (two passes in longdouble):
    a = gamma / sqrt(var + eps), b = beta - mean a, v = x a + b, d = v > 0 ? 1 : slope, g = dy d
    rs = 1 / sqrt(var + eps), xh = (x - mean) rs, t1 = sum g, t2 = sum g xh
    dx = A (g - t1 / n - xh t2 / n), A = gamma rs;  dbeta[c] = sum_n t1(n, c), dgamma[c] = sum_n t2(n, c)

Bounds, u the unit roundoff of the dtype (one rounding to float and one to T, plus half the smallest fp16 subnormal):
    dx      |got - ref| <= 2 u (|A g| + |A t1 / n| + |A xh t2 / n|) + 2^-25
    params  |got - ref| <= 2 u |ref| + 2^-40 sum |terms| + 2^-25
A plane holding an element with |v| <= 2^-40 (|x a| + |b|) is left out (with its channel's parameter gradients): the
kernel forms v from its own double statistics, and so close to 0 its mask may legitimately differ.  At most 1 % of the
planes of a case may be left out.

A CONSTANT plane is never left out, although without affine parameters its v is 0 in every element.  The table has such
planes in every case -- a one-element plane; a 16-bit plane whose offset is 10^4 times its spread, which rounds to one
value -- and the rule as first written left out 6 of 6, 1 of 2 or 3 of 15 planes of those cases, over the cap whatever the
kernel did.  Nothing can differ there: all elements equal give s1 = s2 = 0, so mean = K = x and var = 0 exactly, in the
kernel as in the reference, and v = x a + (beta - x a) has one exact value in both -- 0 where beta is 0.  So these planes
are compared in full, which asks more of the kernel than leaving them out.
"""
import functools

import numpy as np
import torch

import instancenorm_cases as I

LD = np.longdouble
LEFT_OUT_CAP = 0.01


def random_dy(shape, dtype, seed):
    """dy = N(0,1) * 2^(k % 5 - 2) for plane k, rounded to `dtype`."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed + 1000)
    k = torch.arange(N * C)
    scale = 2.0 ** ((k % 5).double() - 2)
    dy = torch.randn(N * C, H * W, generator=g, dtype=torch.float64) * scale[:, None]
    return dy.view(N, C, H, W).to(dtype)


@functools.lru_cache(maxsize=None)
def problem(shape, dtype):
    """(x, gamma, beta, stats, dy) of the table's case, computed once per session and not modified."""
    x, gamma, beta, stats = I.problem(shape, dtype)
    return x, gamma, beta, stats, random_dy(shape, dtype, sum(shape))


class Reference:
    """dx (N,C,H,W), dgamma, dbeta (C) as float64 tensors, their bounds, and the planes / channels that are left out."""

    def __init__(self, x, dy, gamma=None, beta=None, eps=I.EPS, slope=1.0, stats=None):
        N, C, H, W = x.shape
        n = H * W
        u = I.UNIT_ROUNDOFF[x.dtype]
        mean, var = stats if stats is not None else I.plane_statistics(x)
        with np.errstate(all="ignore"):
            mean, var = mean.astype(LD), var.astype(LD)
            xl, dl = x.double().numpy().astype(LD), dy.double().numpy().astype(LD)
            g = (np.ones(C) if gamma is None else gamma.double().numpy()).astype(LD).reshape(1, C, 1, 1)
            bt = (np.zeros(C) if beta is None else beta.double().numpy()).astype(LD).reshape(1, C, 1, 1)
            rs = 1 / np.sqrt(var + LD(eps))
            a = g / np.sqrt(var + LD(eps))
            b = bt - mean * a
            v = xl * a + b
            d = np.where(v > 0, LD(1), LD(np.float32(slope)))
            gd = dl * d
            xh = (xl - mean) * rs
            t1 = gd.sum(axis=(2, 3), keepdims=True)
            t2 = (gd * xh).sum(axis=(2, 3), keepdims=True)
            A = g * rs
            dx = A * (gd - t1 / n - xh * t2 / n)
            lim = 2 * u * (np.abs(A * gd) + np.abs(A * t1 / n) + np.abs(A * xh * t2 / n)) + LD(2.0 ** -25)
            dbeta, dgamma = t1.sum(axis=0).reshape(C), t2.sum(axis=0).reshape(C)
            sb, sg = np.abs(gd).sum(axis=(0, 2, 3)), np.abs(gd * xh).sum(axis=(0, 2, 3))
            tie = (np.abs(v) <= LD(2.0 ** -40) * (np.abs(xl * a) + np.abs(b))).any(axis=(2, 3)) & (var.reshape(N, C) != 0)
            if float(np.float32(slope)) == 1.0:           # no activation, no mask
                tie = np.zeros((N, C), dtype=bool)
        t = lambda z: torch.from_numpy(np.asarray(z, dtype=np.float64))
        self.dx, self.dx_bound = t(dx), t(lim)
        self.dgamma, self.dbeta = t(dgamma), t(dbeta)
        self.dgamma_bound = t(2 * u * np.abs(dgamma) + LD(2.0 ** -40) * sg + LD(2.0 ** -25))
        self.dbeta_bound = t(2 * u * np.abs(dbeta) + LD(2.0 ** -40) * sb + LD(2.0 ** -25))
        self.left_out = torch.from_numpy(tie)                       # (N, C) planes
        self.left_out_channels = self.left_out.any(dim=0)          # (C,)
        self.planes = N * C
        self.v = t(v)

    def cap_ok(self):
        return int(self.left_out.sum()) <= LEFT_OUT_CAP * self.planes

    def check_dx(self, got):
        """-> (ok, worst |got - ref| / bound) over the finite reference elements of the planes that are compared; the NaN
        positions of those planes must agree."""
        keep = ~self.left_out[:, :, None, None].expand_as(self.dx)
        fin = self.dx.isfinite() & keep
        nan_ok = bool(torch.equal(got.isnan()[keep], self.dx.isnan()[keep]))
        if not bool(fin.any()):
            return nan_ok, 0.0
        ratio = ((got.double() - self.dx).abs()[fin] / self.dx_bound[fin])
        return nan_ok and bool((ratio <= 1).all()), float(ratio.max())

    def check_params(self, dgamma, dbeta):
        worst, ok = 0.0, True
        for got, ref, lim in ((dgamma, self.dgamma, self.dgamma_bound), (dbeta, self.dbeta, self.dbeta_bound)):
            keep = ~self.left_out_channels & ref.isfinite()
            ok = ok and bool(torch.equal(got.isnan()[~self.left_out_channels], ref.isnan()[~self.left_out_channels]))
            if bool(keep.any()):
                ratio = (got.double() - ref).abs()[keep] / lim[keep]
                ok, worst = ok and bool((ratio <= 1).all()), max(worst, float(ratio.max()))
        return ok, worst


@functools.lru_cache(maxsize=None)
def reference(shape, dtype, affine, slope):
    """The reference of the table's case, computed once per session and not modified."""
    x, gamma, beta, stats, dy = problem(shape, dtype)
    return Reference(x, dy, gamma if affine else None, beta if affine else None, I.EPS, slope, stats)
