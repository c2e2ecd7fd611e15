"""Shared by test_conv3x3_abi.py (CPU) and test_gpu_conv3x3.py: the case table of the native dense 3x3 convolution
(DESIGN 5.15), its float64 reference, the derived bound, the exact-integer generator and the mirrored plan rule.

The kernel sums K = 9 Cin exact products (two bf16 or two fp16 values multiply exactly in fp32) in fp32, in the matrix
core's own order, and rounds once to the tensor's type after the activation.  With `ref` the float64 convolution of the
same 16-bit inputs and S the float64 convolution of |x| with |w|, every finite output satisfies
    |y - act(ref)| <= K 2^-23 S + u |act(ref)| + t
u = 2^-8 (bf16) / 2^-11 (fp16): one rounding to the type; t = 2^-25 for fp16's subnormal range, 0 for bf16; the first term
is twice the round-to-nearest bound on K fp32 additions (the factor 2 covers an accumulator that truncates).  act is
1-Lipschitz for the slopes used here, so the error of the sum passes through it unamplified.  Derived, not tuned: a CPU
fp32-accumulate convolution of random normal data reaches 0.52-0.95 of it.

Exact cases: x and w in {-1, 0, 1} with at most 28 non-zero input channels per output channel, so every partial sum is an
integer of magnitude <= 252, exact in fp32, bf16 and fp16: the output equals the float64 reference whatever the order.
"""
import functools

import torch
import torch.nn.functional as F

DTYPES = (torch.bfloat16, torch.float16)
IDS = ("bf16", "fp16")
SLOPES = (1.0, 0.0, 0.01)
UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUBNORMAL_TERM = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}

# The plan rule of csrc/rroi_conv3x3_host.h (plan_conv3x3), mirrored: change both together.
TILE_M, TILE_H, TILE_W, K_CHUNK = 32, 4, 32, 16


def out_size(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def plan_of(case):
    """(tile_m, tile_h, k_chunks, grid) by the mirrored rule: one form, 32 channels x 4 rows x 32 columns, K chunks of 16."""
    N, Cin, Cout, H, W, stride = case
    Ho, Wo = out_size(H, W, stride)
    return TILE_M, TILE_H, -(-Cin // K_CHUNK), N * -(-Cout // TILE_M) * -(-Ho // TILE_H) * -(-Wo // TILE_W)


# (N, Cin, Cout, H, W, stride).  Cin 1, 3, 16, 17, 32, 64, 144: a tail of the 16-wide K step, one to nine K chunks.
# Cout 1, 16, 31, 32, 48, 64, 96: masked rows, one to three channel tiles.  Maps 1x1, 1x7, 5x1, 5x7, 9x33 and one pixel
# narrower / wider than the 4 x 32 tile, for both strides; rows of 128 tiles and one more.  Stride 2 on odd and even H and W.
CASES = (
    (1, 1, 1, 1, 1, 1),                # the smallest case
    (2, 3, 16, 1, 7, 1),               # one row
    (3, 16, 31, 5, 1, 1),              # one column, a masked channel row
    (1, 17, 32, 5, 7, 1),              # a K tail of one channel
    (2, 32, 48, 9, 33, 1),             # the second channel tile half masked, three y tiles, two x tiles
    (3, 17, 96, 9, 33, 1),             # three channel tiles, an odd K tail
    (1, 64, 64, 5, 7, 2),              # stride 2, odd H and W
    (1, 144, 96, 6, 8, 2),             # stride 2, even H and W, nine K chunks
    (1, 16, 1, 7, 9, 2),               # stride 2, one output channel
    (2, 1, 64, 4, 6, 2),               # stride 2, one input channel
    (1, 3, 16, 3, 31, 1),              # tile 4 x 32: one narrower in both directions
    (1, 3, 16, 5, 33, 1),              # ... one wider
    (1, 16, 16, 6, 62, 2),             # stride 2: output 3 x 31
    (1, 16, 16, 9, 65, 2),             # stride 2: output 5 x 33
    (2, 3, 16, 7, 4095, 1),            # 128 x tiles, the last one pixel short; two y tiles, the second one row short
    (1, 3, 16, 9, 4097, 1),            # 129 x tiles, the last of one pixel; three y tiles, the last of one row
    (1, 3, 48, 18, 8194, 2),           # likewise at stride 2, even H and W: output 9 x 4097
    (2, 17, 31, 13, 8192, 2),          # stride 2, odd H, a K tail: output 7 x 4096
    (1, 3, 64, 9, 4097, 1),            # two channel tiles over a wide map
)
# every form the table is meant to reach: (tile_m, tile_h, stride)
FORMS = {(32, 4, 1), (32, 4, 2)}

# the dense 3x3 convolutions of FOTSNet on a 704 x 1280 image (stem, layer0_1, layer1, layer2) and of its recogniser on
# crops of 11 x 96 (conv5 - conv9): (Cin, Cout, H, W, stride)
NETWORK_SHAPES = (
    (3, 16, 704, 1280, 1), (32, 32, 704, 1280, 2), (64, 64, 352, 640, 1), (64, 64, 352, 640, 2), (64, 64, 176, 320, 1),
    (64, 128, 176, 320, 2), (128, 128, 88, 160, 1),
)
RECOGNISER_SHAPES = ((64, 128, 11, 96, 1), (128, 128, 11, 96, 1), (128, 256, 5, 96, 1), (256, 256, 5, 96, 1))


def case_id(case):
    return "x".join(str(v) for v in case)


def act64(t, slope):
    return torch.where(t < 0, t * slope, t)


def reference(x, w, stride):
    """-> (ref, S): the float64 convolution of the 16-bit inputs, and that of their magnitudes."""
    xd, wd = x.double(), w.double()
    return F.conv2d(xd, wd, stride=stride, padding=1), F.conv2d(xd.abs(), wd.abs(), stride=stride, padding=1)


def bound(ref, S, cin, dtype, slope):
    """-> (act(ref), lim), both float64."""
    a = act64(ref, slope)
    return a, 9 * cin * 2.0 ** -23 * S + UNIT_ROUNDOFF[dtype] * a.abs() + SUBNORMAL_TERM[dtype]


def within(got, want, lim):
    """|got - want| <= lim on every finite output; -> (ok, worst error / bound, 0 where the bound is 0 and met)."""
    finite = got.isfinite() & want.isfinite() & lim.isfinite()
    if not bool(finite.any()):
        return True, 0.0
    err = (got.double() - want)[finite].abs()
    lim = lim[finite]
    ok = bool((err <= lim).all())
    pos = lim > 0
    return ok, float((err[pos] / lim[pos]).max()) if bool(pos.any()) else 0.0


def bits(t):
    return t.contiguous().view(torch.int16)


def random_problem(case, dtype, seed):
    """x = N(0, 1), w = N(0, 1) / sqrt(9 Cin), rounded to `dtype` (the reference sees the rounded values)."""
    N, Cin, Cout, H, W, _ = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g).to(dtype)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).to(dtype)
    return x, w


def integer_problem(case, dtype, seed):
    """x and w in {-1, 0, 1}; per output channel at most 28 input channels carry a non-zero weight."""
    N, Cin, Cout, H, W, _ = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (N, Cin, H, W), generator=g).to(dtype)
    w = torch.randint(-1, 2, (Cout, Cin, 3, 3), generator=g).float()
    if Cin > 28:
        keep = torch.zeros(Cout, Cin)
        for co in range(Cout):
            keep[co, torch.randperm(Cin, generator=g)[:28]] = 1.0
        w = w * keep[:, :, None, None]
    assert int((w.abs().sum((2, 3)) > 0).sum(1).max()) <= 28
    return x, w.to(dtype)


@functools.lru_cache(maxsize=None)
def problem(case, dtype):
    """The table's random problem for (case, dtype) with its reference, computed once per session and not modified:
    -> x, w, ref, S."""
    x, w = random_problem(case, dtype, seed=sum(case))
    return (x, w) + reference(x, w, case[5])


@functools.lru_cache(maxsize=None)
def exact_problem(case, dtype):
    """Likewise for the exact-integer problem: -> x, w, ref (integers of magnitude <= 252)."""
    x, w = integer_problem(case, dtype, seed=1000 + sum(case))
    ref, S = reference(x, w, case[5])
    assert float(S.max()) <= 252.0
    return x, w, ref
