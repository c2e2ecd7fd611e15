"""Shared by test_conv1x1_abi.py (CPU) and test_gpu_conv1x1.py: the case table of the native 1x1 convolution with its folded
BatchNorm, its float64 reference, the two bounds, the exact-integer generator and the mirrored plan rule.

The kernel sums Cin exact products (two bf16 or two fp16 values multiply exactly in fp32) in fp32, in the matrix core's own
order, and rounds once to the tensor's type after the activation.  With `ref` the float64 sum over the same 16-bit inputs
and A the float64 sum of |w| |x|, every finite output satisfies
    plain:  |y - act(ref)| <= Cin 2^-23 A + u |act(ref)| + tau
u = 2^-8 (bf16) / 2^-11 (fp16): one rounding to the type; tau = 2^-25 for fp16's subnormal range, 0 for bf16; the first term
is twice the round-to-nearest bound on Cin fp32 additions (the factor 2 covers an accumulator that truncates) -- the bound
of conv3x3_cases.py with K = Cin.  act is 1-Lipschitz for the slopes used here.
With a norm the kernel computes s = g / sqrt(var + eps), t = b - mean * s and s * sum + t in fp32.  With s, t in float64 from
the 16-bit vectors and z = s ref + t,
    norm:   |y - act(z)| <= |s| Cin 2^-23 A + 2^-20 (|s| (A + |mean|) + |b|) + u |act(z)| + tau
The 2^-20 term is sixteen fp32 half-ulps on each magnitude that enters: the reciprocal square root (an add, a square root
and a division: three roundings of s, which scales A and mean), the product mean * s and the subtraction that folds t (on
|mean| |s| + |b|), and the final multiply and add (on |s| A + |t|) -- eight roundings at most on any magnitude, so sixteen
half-ulps leave a factor two.  Derived, not tuned; test_conv1x1_abi.py checks that an fp32-accumulating CPU emulation of
the same formula stays within both on the whole table.

Exact cases: x and w in {-1, 0, 1}, no norm: every partial sum is an integer of magnitude <= Cin <= 144, exact in fp32,
bf16 and fp16, so the output equals the float64 reference whatever the order.
"""
import functools

import torch
import torch.nn.functional as F

DTYPES = (torch.bfloat16, torch.float16)
IDS = ("bf16", "fp16")
SLOPES = (1.0, 0.0, 0.01)
UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUBNORMAL_TERM = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}

# The plan rule of csrc/rroi_conv1x1_host.h (plan_conv1x1), mirrored: change both together.
TILE_P, K_CHUNK, MIN_GROUPS = 128, 64, 256


def out_size(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def plan_of(case):
    """(tile_m, k_chunks, grid) by the mirrored rule: 128 output pixels (flat) per workgroup, K chunks of 64, 64 output
    channels per workgroup where Cout > 32 and that leaves at least 256 workgroups, 32 otherwise."""
    N, Cin, Cout, H, W, stride = case
    Ho, Wo = out_size(H, W, stride)
    p_tiles = -(-(Ho * Wo) // TILE_P)
    tile_m = 64 if Cout > 32 and N * -(-Cout // 64) * p_tiles >= MIN_GROUPS else 32
    return tile_m, -(-Cin // K_CHUNK), N * -(-Cout // tile_m) * p_tiles


# (N, Cin, Cout, H, W, stride).  Cin 1, 3, 16, 17, 32, 64, 65, 144: a tail of the 16-wide K step and of the 64-wide chunk,
# one to three chunks.  Cout 1, 31, 32, 33, 65, 96: masked rows, one to three channel tiles of 32, two of 64.  Maps 1x1, 1x7,
# 5x1; 127 and 129 output pixels (the pixel tile is 128) at both strides; an odd W with N > 1 (channel planes off a 16-byte
# boundary); stride 2 on odd and even H and W; wide maps whose last pixel tile holds one pixel; the 64-channel form (at
# least 256 workgroups) at both strides and with three K chunks.
CASES = (
    (1, 1, 1, 1, 1, 1),                # the smallest case
    (2, 3, 33, 1, 7, 1),               # one row, the second channel tile of one row
    (3, 16, 31, 5, 1, 1),              # one column, a masked channel row
    (2, 17, 32, 5, 7, 1),              # a K tail of one channel; planes of 35 elements: off 16 bytes
    (1, 32, 96, 1, 127, 1),            # one pixel short of the tile; three channel tiles
    (1, 64, 33, 3, 43, 1),             # 129 pixels: one more than the tile; one full chunk
    (1, 65, 32, 9, 33, 1),             # a second chunk of one channel
    (3, 144, 96, 9, 33, 1),            # three chunks, the last of one 16-channel step; three pixel tiles
    (1, 64, 64, 5, 7, 2),              # stride 2, odd H and W
    (1, 144, 96, 6, 8, 2),             # stride 2, even H and W
    (1, 16, 1, 7, 9, 2),               # stride 2, one output channel
    (2, 1, 33, 4, 6, 2),               # stride 2, one input channel
    (1, 3, 31, 1, 253, 2),             # stride 2: 127 output pixels
    (2, 17, 32, 5, 85, 2),             # stride 2: 3 x 43 = 129 output pixels, odd W with N > 1
    (1, 3, 33, 1, 4097, 1),            # 33 pixel tiles, the last of one pixel
    (1, 17, 31, 3, 8193, 2),           # stride 2: output 2 x 4097, 65 pixel tiles, rows that straddle tiles
    (2, 3, 96, 1, 8193, 1),            # 260 workgroups of 64 channels: the second channel tile half masked
    (2, 17, 96, 3, 16385, 2),          # likewise at stride 2: output 2 x 8193
    (1, 144, 65, 1, 16400, 1),         # 64 channels per workgroup over three chunks; the second channel tile of one row
)
# every form the table is meant to reach: (tile_m, stride)
FORMS = {(32, 1), (32, 2), (64, 1), (64, 2)}

# the bias-free 1x1 convolutions of FOTSNet on a 704 x 1280 image: (Cin, Cout, H, W, stride)
NETWORK_SHAPES = (
    (128, 256, 44, 80, 1), (256, 256, 44, 80, 1),                                  # layer3: conv_sep1[1], conv2[3]
    (256, 512, 22, 40, 1), (512, 512, 22, 40, 1),                                  # layer4
    (64, 128, 176, 320, 2), (128, 256, 88, 160, 2), (256, 512, 44, 80, 2),         # layerN.0.downsample[0]
    (64, 256, 176, 320, 1), (128, 256, 88, 160, 1), (512, 256, 22, 40, 1),         # feature1, 2, 4 (feature3: row 2)
    (256, 256, 88, 160, 1), (256, 256, 176, 320, 1),                               # upconv1[1], upconv2[1]
)
SHORTCUT_SHAPES = NETWORK_SHAPES[4:7]
NORM_KINDS = ("affine", "plain", "tiny_var")


def case_id(case):
    return "x".join(str(v) for v in case)


def act64(t, slope):
    return torch.where(t < 0, t * slope, t)


def reference(x, w, stride):
    """-> (ref, A): the float64 1x1 convolution of the 16-bit inputs, and that of their magnitudes."""
    xd, wd = x.double(), w.double().reshape(w.size(0), w.size(1), 1, 1)
    return F.conv2d(xd, wd, stride=stride), F.conv2d(xd.abs(), wd.abs(), stride=stride)


def fold64(norm):
    """(s, t, |mean|, |b|) in float64, each (1, Cout, 1, 1), of a norm (g or None, b or None, mean, var, eps)."""
    g, b, mean, var, eps = norm
    gd = torch.ones_like(mean, dtype=torch.float64) if g is None else g.double()
    bd = torch.zeros_like(mean, dtype=torch.float64) if b is None else b.double()
    s = gd / torch.sqrt(var.double() + eps)
    t = bd - mean.double() * s
    return tuple(v.reshape(1, -1, 1, 1) for v in (s, t, mean.double().abs(), bd.abs()))


def bound(ref, A, cin, dtype, slope, norm=None):
    """-> (act(ref) or act(s ref + t), lim), both float64."""
    if norm is None:
        a = act64(ref, slope)
        return a, cin * 2.0 ** -23 * A + UNIT_ROUNDOFF[dtype] * a.abs() + SUBNORMAL_TERM[dtype]
    s, t, mean, b = fold64(norm)
    a = act64(s * ref + t, slope)
    lim = (s.abs() * cin * 2.0 ** -23 * A + 2.0 ** -20 * (s.abs() * (A + mean) + b) + UNIT_ROUNDOFF[dtype] * a.abs()
           + SUBNORMAL_TERM[dtype])
    return a, lim


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
    """x = N(0, 1), w = N(0, 1) / sqrt(Cin) as (Cout, Cin, 1, 1), rounded to `dtype` (the reference sees the rounded values)."""
    N, Cin, Cout, H, W, _ = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g).to(dtype)
    w = (torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5).to(dtype)
    return x, w


def random_norm(cout, dtype, kind, seed):
    """(g or None, b or None, mean, var, eps) in `dtype`: affine, without affine parameters, or with a variance of at most
    1e-6 -- zeros among them in fp16 -- so that eps = 1e-5 dominates and s is about 300 g."""
    g = torch.Generator().manual_seed(seed)
    gamma = (1.0 + 0.5 * torch.randn(cout, generator=g)).to(dtype)
    beta = (0.5 * torch.randn(cout, generator=g)).to(dtype)
    mean = (0.5 * torch.randn(cout, generator=g)).to(dtype)
    var = (0.5 + torch.rand(cout, generator=g)).to(dtype)
    if kind == "tiny_var":
        var = (1e-6 * torch.rand(cout, generator=g)).to(dtype)
    if kind == "plain":
        return None, None, mean, var, 1e-5
    assert kind in ("affine", "tiny_var")
    return gamma, beta, mean, var, 1e-5


def integer_problem(case, dtype, seed):
    """x and w in {-1, 0, 1}."""
    N, Cin, Cout, H, W, _ = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (N, Cin, H, W), generator=g).to(dtype)
    w = torch.randint(-1, 2, (Cout, Cin, 1, 1), generator=g).to(dtype)
    return x, w


def emulate_fp32(x, w, stride, slope, norm, dtype):
    """The kernel's formula with every step in fp32 on the CPU (whatever order its convolution sums in), rounded once."""
    v = F.conv2d(x.float(), w.float().reshape(w.size(0), w.size(1), 1, 1), stride=stride)
    if norm is not None:
        g, b, mean, var, eps = norm
        one = torch.ones(w.size(0)) if g is None else g.float()
        zero = torch.zeros(w.size(0)) if b is None else b.float()
        s = one / torch.sqrt(var.float() + torch.tensor(eps, dtype=torch.float32))
        t = zero - mean.float() * s
        v = v * s.reshape(1, -1, 1, 1) + t.reshape(1, -1, 1, 1)
    return torch.where(v < 0, v * torch.tensor(slope, dtype=torch.float32), v).to(dtype)


@functools.lru_cache(maxsize=None)
def problem(case, dtype):
    """The table's random problem for (case, dtype) with its reference, computed once per session and not modified:
    -> x, w, ref, A."""
    x, w = random_problem(case, dtype, seed=sum(case))
    return (x, w) + reference(x, w, case[5])


@functools.lru_cache(maxsize=None)
def norm_of(case, dtype):
    """The norm that goes with the table's problem: the three kinds in turn along the table."""
    kind = NORM_KINDS[CASES.index(case) % 3] if case in CASES else "affine"
    return random_norm(case[2], dtype, kind, seed=2000 + sum(case))


@functools.lru_cache(maxsize=None)
def exact_problem(case, dtype):
    """Likewise for the exact-integer problem: -> x, w, ref (integers of magnitude <= Cin <= 144)."""
    x, w = integer_problem(case, dtype, seed=1000 + sum(case))
    ref, A = reference(x, w, case[5])
    assert float(A.max()) <= 144.0
    return x, w, ref
