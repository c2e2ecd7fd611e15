"""Shared by test_remainder_abi.py (CPU) and test_gpu_conv2x3.py: the case table of the native (2,3) convolution
(DESIGN 5.19), its float64 reference, the derived bound, the exact-integer generator and the mirrored plan rule.

The reasoning is conv3x3_cases.py's with K = 6 Cin: the kernel sums K exact products (two bf16 or two fp16 values multiply
exactly in fp32) in fp32, in the matrix core's own order, and rounds once to the tensor's type after the activation.  With
`ref` the float64 convolution of the same 16-bit inputs and S the float64 convolution of |x| with |w|, every finite output
satisfies
    |y - act(ref)| <= K 2^-23 S + u |act(ref)| + t
u = 2^-8 (bf16) / 2^-11 (fp16): one rounding to the type; t = 2^-25 for fp16's subnormal range, 0 for bf16; the first term
is twice the round-to-nearest bound on K fp32 additions (the factor 2 covers an accumulator that truncates).  act is
1-Lipschitz for the slopes used here.  Derived, not tuned.

Exact cases: x and w in {-1, 0, 1} with at most 42 non-zero input channels per output channel, so every partial sum is an
integer of magnitude <= 6 * 42 = 252, exact in fp32, bf16 and fp16: the output equals the float64 reference whatever the
order.
"""
import functools

import torch
import torch.nn.functional as F

from conv3x3_cases import SLOPES, SUBNORMAL_TERM, UNIT_ROUNDOFF, act64, bits, within  # noqa: F401  (one definition of each)

DTYPES = (torch.bfloat16, torch.float16)
IDS = ("bf16", "fp16")
LIVE_CHANNELS = 42

# The plan rule of csrc/rroi_conv2x3_host.h (plan_conv2x3), mirrored: change both together.
TILE_M, TILE_W, WAVE_ITEMS, K_CHUNK = 32, 32, 4, 32


def plan_of(case):
    """(k_chunks, items, grid) by the mirrored rule: items of one output row x 32 columns, four per workgroup (one per
    wave), 32 output channels per workgroup, K chunks of 32."""
    N, Cin, Cout, H, W = case
    items = N * (H - 1) * -(-W // TILE_W)
    return -(-Cin // K_CHUNK), items, -(-items // WAVE_ITEMS) * -(-Cout // TILE_M)


# (N, Cin, Cout, H, W).  Cin 3, 20, 256: below one 8-channel group, a group half full, eight K chunks; 70 and 100: three
# chunks (an odd number for the two register sets) and four, the last of six and of four channels.  Cout 1, 40, 256: one
# masked channel tile, a second tile a quarter full, eight tiles.  W 1, 8, 33, 70, 96: one column, a quarter tile, one
# column into the second tile, a third tile of six columns, three whole tiles.  H 2, 3, 5: one, two and four output rows.
# N 1 and 5, so that the item count (10, 15) is no multiple of the four waves.
CASES = (
    (1, 3, 1, 2, 1),                   # the smallest case: one item, three idle waves
    (5, 3, 40, 2, 33),                 # 10 items: the third workgroup has two
    (1, 20, 40, 3, 8),                 # two output rows, a K tail
    (5, 20, 1, 5, 70),                 # four output rows, three x tiles, one output channel
    (1, 3, 256, 3, 96),                # eight channel tiles over three whole x tiles
    (1, 256, 40, 5, 33),               # eight K chunks, a masked second channel tile
    (2, 70, 40, 3, 33),                # three K chunks, the last of six channels
    (1, 100, 1, 2, 70),                # four K chunks, the last of four channels
    (5, 20, 40, 2, 96),                # 15 items
    (4, 256, 256, 2, 40),              # the network's own: network_cases.CROPS["4x11x40"] in front of conv10_s
    (1, 256, 256, 2, 8),               # ... and "1x11x8"
    (24, 256, 256, 2, 64),             # 24 crops of 64 columns
)
NETWORK_CASES = ((4, 256, 256, 2, 40), (1, 256, 256, 2, 8))


def case_id(case):
    return "x".join(str(v) for v in case)


def reference(x, w):
    """-> (ref, S): the float64 convolution of the 16-bit inputs, and that of their magnitudes."""
    xd, wd = x.double(), w.double()
    return F.conv2d(xd, wd, padding=(0, 1)), F.conv2d(xd.abs(), wd.abs(), padding=(0, 1))


def bound(ref, S, cin, dtype, slope):
    """-> (act(ref), lim), both float64."""
    a = act64(ref, slope)
    return a, 6 * cin * 2.0 ** -23 * S + UNIT_ROUNDOFF[dtype] * a.abs() + SUBNORMAL_TERM[dtype]


def random_problem(case, dtype, seed):
    """x = N(0, 1), w = N(0, 1) / sqrt(6 Cin), rounded to `dtype` (the reference sees the rounded values)."""
    N, Cin, Cout, H, W = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g).to(dtype)
    w = (torch.randn(Cout, Cin, 2, 3, generator=g) / (6 * Cin) ** 0.5).to(dtype)
    return x, w


def integer_problem(case, dtype, seed):
    """x and w in {-1, 0, 1}; per output channel at most 42 input channels carry a non-zero weight."""
    N, Cin, Cout, H, W = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (N, Cin, H, W), generator=g).to(dtype)
    w = torch.randint(-1, 2, (Cout, Cin, 2, 3), generator=g).float()
    if Cin > LIVE_CHANNELS:
        keep = torch.zeros(Cout, Cin)
        for co in range(Cout):
            keep[co, torch.randperm(Cin, generator=g)[:LIVE_CHANNELS]] = 1.0
        w = w * keep[:, :, None, None]
    assert int((w.abs().sum((2, 3)) > 0).sum(1).max()) <= LIVE_CHANNELS
    return x, w.to(dtype)


@functools.lru_cache(maxsize=None)
def problem(case, dtype):
    """The table's random problem for (case, dtype) with its reference, computed once per session and not modified:
    -> x, w, ref, S."""
    x, w = random_problem(case, dtype, seed=sum(case))
    return (x, w) + reference(x, w)


@functools.lru_cache(maxsize=None)
def exact_problem(case, dtype):
    """Likewise for the exact-integer problem: -> x, w, ref (integers of magnitude <= 252)."""
    x, w = integer_problem(case, dtype, seed=1000 + sum(case))
    ref, S = reference(x, w)
    assert float(S.max()) <= 252.0
    return x, w, ref
