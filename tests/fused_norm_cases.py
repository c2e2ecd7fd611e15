"""Shared by test_fused_norm_abi.py (CPU) and test_gpu_fused_norm.py: the reference and the bound of the fused InstanceNorm
epilogues, built from instancenorm_cases.py -- the same case table, the same longdouble statistics.

Residual:  a, b are the coefficients of instancenorm_cases.reference;  v32 = float32(x64 * a + b);  u = v32 + float32(r) in
torch fp32;  u = u < 0 ? u * float32(slope) : u;  one conversion to the tensor's type.  ref64 is the float64 value before any
rounding.  Mirror is the same reference on cat(x, -x) with parameters of 2C channels (and no residual).

Condition (a) allows |got - ref64| <= instancenorm_cases.bound(x, a, b) + 2 u |r|, u the unit roundoff of the type: the
bound of the plain norm, one more fp32 rounding (the sum) and the final rounding of a sum that r enters.
"""
import functools

import numpy as np
import torch

import instancenorm_cases as I


def reference(x, gamma=None, beta=None, eps=I.EPS, slope=1.0, stats=None, r=None):
    """-> (out of x's dtype, ref64, a, b (float64, (N, C, 1, 1)))."""
    _, _, a, b = I.reference(x, gamma, beta, eps, 1.0, stats)
    v64 = x.double() * a + b
    s32 = torch.tensor(np.float32(slope))
    u = v64.float()
    t64 = v64
    if r is not None:
        u = u + r.float()
        t64 = v64 + r.double()
    out = torch.where(u < 0, u * s32, u).to(x.dtype)
    ref64 = torch.where(t64 < 0, t64 * s32.double(), t64)
    return out, ref64, a, b


def bound(x, a, b, r=None):
    lim = I.bound(x, a, b)
    return lim if r is None else lim + 2 * I.UNIT_ROUNDOFF[x.dtype] * r.double().abs()


def within_bound(got, ref64, x, a, b, r=None):
    """Condition (a) on every finite element of the reference; -> (ok, worst |got - ref64| / bound)."""
    finite = ref64.isfinite()
    if not bool(finite.any()):
        return True, 0.0
    err = (got.double() - ref64).abs()[finite]
    lim = bound(x, a, b, r)[finite]
    return bool((err <= lim).all()), float((err / lim).max())


def mirrored(x):
    return torch.cat((x, -x), 1)


@functools.lru_cache(maxsize=None)
def residual_of(shape, dtype):
    """N(0, 1) rounded to `dtype`; computed once per session and not modified."""
    g = torch.Generator().manual_seed(1000 + sum(shape))
    return torch.randn(shape, generator=g, dtype=torch.float64).to(dtype)


@functools.lru_cache(maxsize=None)
def mirror_problem(shape, dtype):
    """x of the table's problem, cat(x, -x), gamma and beta of 2C channels and the statistics of the concatenated tensor;
    computed once per session and not modified."""
    x = I.problem(shape, dtype)[0]
    g = torch.Generator().manual_seed(2000 + sum(shape))
    C2 = 2 * shape[1]
    gamma = (torch.randn(C2, generator=g, dtype=torch.float64) * 0.5 + 1.0).to(dtype)
    beta = torch.randn(C2, generator=g, dtype=torch.float64).to(dtype)
    x2 = mirrored(x)
    return x, x2, gamma, beta, I.plane_statistics(x2)


def mirror_is_exact_case(shape, dtype):
    """Where the fused mirror must give the bits of the plain kernel on cat(x, -x): every plane of both tensors on a
    16-byte boundary, and the plans of (N, C, H, W) and (N, 2C, H, W) the same form with the same segment length."""
    N, C, H, W = shape
    size = 4 if dtype == torch.float32 else 2
    p1, p2 = I.plan_of(N, C, H, W), I.plan_of(N, 2 * C, H, W)
    return (H * W * size) % 16 == 0 and p1[0] == p2[0] and p1[2] == p2[2]
