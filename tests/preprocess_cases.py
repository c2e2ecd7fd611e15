"""Shared by test_preprocess_abi.py (CPU) and test_gpu_preprocess.py: the float64 restatement of native preprocessing
(include/rroi_align_hip.h section 14), the case table, the packing of a batch and the mirrored plan rule.

The restatement is the header's recipe in exactly its order, every operation a separate numpy float64 operation (numpy
contracts nothing): per axis  n0 == n: i0 = i1 = i, l = 0;  otherwise  s = max(0, (i + 0.5) * (n0 / n) - 0.5),
i0 = min(floor(s), n0 - 1), i1 = min(i0 + 1, n0 - 1), l = s - i0;  top = (1 - lx) * p[y0][x0] + lx * p[y0][x1], bot likewise
on row y1, v = (1 - ly) * top + ly * bot, out = v / 128 - 1.  `rounded` is the one rounding the kernel makes: (T)(float)."""
import numpy as np
import torch

DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def axis(n0, n):
    i = np.arange(n, dtype=np.float64)
    if n0 == n:
        idx = np.arange(n, dtype=np.int64)
        return idx, idx, np.zeros(n, np.float64)
    s = np.maximum(0.0, (i + 0.5) * (np.float64(n0) / np.float64(n)) - 0.5)
    i0 = np.minimum(np.floor(s).astype(np.int64), n0 - 1)
    i1 = np.minimum(i0 + 1, n0 - 1)
    return i0, i1, s - i0.astype(np.float64)


def ref64(im, size):
    """(H0, W0, 3) uint8 -> (3, H, W) float64."""
    H, W = size
    p = im.astype(np.float64).transpose(2, 0, 1)               # (3, H0, W0): bytes are exact in double
    y0, y1, ly = axis(im.shape[0], H)
    x0, x1, lx = axis(im.shape[1], W)
    lx0 = 1.0 - lx
    top = lx0 * p[:, y0][:, :, x0] + lx * p[:, y0][:, :, x1]
    bot = lx0 * p[:, y1][:, :, x0] + lx * p[:, y1][:, :, x1]
    v = (1.0 - ly)[None, :, None] * top + ly[None, :, None] * bot
    return v / 128.0 - 1.0


def ref_batch(ims, size):
    """-> (N, 3, H, W) float64."""
    if len(ims) == 0:
        return np.zeros((0, 3) + tuple(size), np.float64)
    return np.stack([ref64(im, size) for im in ims])


def rounded(ref, dtype):
    """(T)(float)ref as a CPU tensor: numpy rounds double to float to nearest-even, torch float to bf16 / fp16 likewise."""
    t = torch.from_numpy(np.ascontiguousarray(ref.astype(np.float32)))
    return t if dtype == torch.float32 else t.to(dtype)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def image(h, w, fill, seed):
    if fill == "full":
        return np.full((h, w, 3), 255, np.uint8)
    if fill == "checker":                                        # 0 and 255 alternate along both axes and the channels
        yy, xx, cc = np.mgrid[0:h, 0:w, 0:3]
        return (((yy + xx + cc) & 1) * 255).astype(np.uint8)
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# (source sizes, output size, pixel content): the smallest at which each branch can break
CASES = (
    (((64, 96),), (64, 96), "random"),                 # identity
    (((90, 161),), (88, 160), "random"),               # the workload's kind of slight downscale, scale not a float
    (((33, 70),), (64, 96), "random"),                 # upscale, taps clamped at the far edge
    (((50, 37),), (32, 32), "random"),                 # downscale past 1.5
    (((20, 30),), (64, 96), "random"),                 # scale_up's x3 (and more)
    (((1, 1),), (32, 32), "random"),                   # one-pixel axes
    (((7, 1),), (5, 7), "random"),                     # odd outputs with no full vector
    (((45, 77),), (1, 1), "random"),                   # one-pixel output
    (((33, 71), (35, 68), (64, 96)), (64, 96), "random"),   # different sources, one output; offsets 7029 and 14169: odd
    ((), (8, 8), "random"),                            # N = 0
    (((33, 70),), (64, 96), "full"),                   # the extremes of v
    (((90, 161),), (88, 160), "checker"),
    (((64, 96),), (64, 96), "checker"),
    (((5, 9), (5, 9), (5, 9), (5, 9), (5, 9)), (37, 1283), "random"),   # a wide odd row: 161 strips of 8, several workgroups
)
RESIZING = tuple(c for c in CASES if c[0] and any(s != c[1] for s in c[0]))


def images_of(case, seed=0):
    return [image(h, w, case[2], seed + 17 * k) for k, (h, w) in enumerate(case[0])]


def pack(ims):
    """-> (bytes of the images back to back, (N, 4) int32 table {offset, H0, W0, 0})."""
    table = np.zeros((len(ims), 4), np.int32)
    at = 0
    for k, im in enumerate(ims):
        table[k] = (at, im.shape[0], im.shape[1], 0)
        at += im.size
    src = np.concatenate([im.reshape(-1) for im in ims]) if ims else np.zeros(0, np.uint8)
    return src, table


def plan_of(n, size, dtype):
    """The plan rule, mirrored: (columns, rows per thread, strips, bands, items, grid, wide)."""
    H, W = size
    V = 4 if dtype == torch.float32 else 8
    strips = -(-W // V)
    band = 1
    while band < 4 and band * 2 <= H and (n * H * strips) // (band * 2) >= 1024 * 64:
        band *= 2
    bands = -(-H // band)
    items = n * bands * strips
    return V, band, strips, bands, items, -(-items // 256), int(W % V == 0)


def stock_error_bound(h0, w0):
    """What the stock chain (fp32 F.interpolate, then / 128 - 1 in fp32) may differ from the float64 value by, from its own
    arithmetic: it evaluates the source coordinate scale * (i + 0.5) - 0.5 in fp32 -- the scale, the product and the
    difference each rounded, at most 3 * 2^-24 relative to a coordinate below the source extent -- so each axis' weight is
    off by at most 3 * 2^-24 * n0 and the blend by that times the largest byte difference, 255 (the blend is continuous
    across a tap change); its two blends and their weights add at most 8 roundings of values up to 255; then / 128, and two
    roundings of results below 2."""
    u = 2.0 ** -24
    return (3 * (h0 + w0) + 8) * u * 255 / 128 + 2 * 2 * u
