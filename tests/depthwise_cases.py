"""The oracle and the case table of the depthwise 3x3 tests; no test in here.

The oracle is the recipe of include/rroi_align_hip.h section 5, in numpy: zero-pad, then nine shifted
`acc = acc + w64 * x64` over float64 arrays in (ky, kx) order, then `.astype(float32)`.  A 16-bit expectation is
`torch.from_numpy(that).to(dtype)` -- one plain conversion, to nearest even."""
import numpy as np
import torch

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
IDS = ["fp32", "bf16", "fp16"]

# the kernel's geometry (csrc/rroi_depthwise_kernels.h, rroi_depthwise_host.h): a thread owns TILE_W output columns over
# `band` output rows; the host takes the tallest band of 8, 4, 2 that still gives 65536 threads
TILE_W = 4
BANDS = (8, 4, 2)


def out_size(n, stride):
    return (n - 1) // stride + 1


def band_of(N, C, H, W, stride):
    """Mirror of depthwise_band (host): which band height a shape runs with."""
    ho, wo = out_size(H, stride), out_size(W, stride)
    strips = -(-wo // TILE_W)
    for band in BANDS[:-1]:
        if N * C * -(-ho // band) * strips >= 65536:
            return band
    return BANDS[-1]


def oracle_depthwise3x3(x, w, stride):
    """x (N,C,H,W) float32 (a 16-bit tensor widened), w (C,1,3,3) float32 -> (N,C,Ho,Wo) float32."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    w64 = np.asarray(w, np.float32).astype(np.float64)
    N, C, H, W = x64.shape
    ho, wo = out_size(H, stride), out_size(W, stride)
    xp = np.zeros((N, C, H + 2, W + 2), np.float64)
    xp[:, :, 1:H + 1, 1:W + 1] = x64
    acc = np.zeros((N, C, ho, wo), np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for ky in range(3):
            for kx in range(3):
                tap = xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
                acc = acc + w64[None, :, 0, ky, kx, None, None] * tap
        return acc.astype(np.float32)


def expected(x, w, stride):
    """The expectation for tensors x, w of one dtype (any device), as a CPU tensor of that dtype."""
    o = oracle_depthwise3x3(x.detach().float().cpu().numpy(), w.detach().float().cpu().numpy(), stride)
    return torch.from_numpy(o).to(x.dtype)


def random_problem(shape, dtype, seed):
    """N(0, 1) data and weights of `dtype` on the CPU."""
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    return torch.randn(N, C, H, W, generator=g).to(dtype), torch.randn(C, 1, 3, 3, generator=g).to(dtype)


# (N, C, H, W), strides.  Both strides unless the shape is one of the network's.
# Tile width 4: Wo = 3, 4, 5 are W = 3, 4, 5 at stride 1 and W = 5, 7, 9 at stride 2.  Band heights: small shapes run
# band 2 (Ho = 1, 2, 3: H = 1, 2, 3 at stride 1; H = 1, 3, 5 at stride 2); the C = 10923 shapes are the smallest that
# reach band 4 (Ho = 9 = two bands + 1: H = 9 / 17) and band 8 (Ho = 17: H = 17 / 33), with Wo = 5 (one above the tile).
GENERAL = [
    (1, 1, 1, 1), (1, 3, 1, 7), (2, 3, 7, 1), (1, 5, 2, 2), (3, 33, 5, 17),
    (1, 4, 3, 67), (1, 2, 50, 320), (1, 2, 51, 319), (2, 7, 22, 40), (1, 512, 22, 40),
    (8, 16, 44, 80),
    (1, 2, 3, 3), (1, 2, 2, 4), (1, 3, 3, 5), (1, 2, 5, 7), (1, 2, 4, 8), (1, 2, 5, 9),
]
CASES = [(s, 1) for s in GENERAL] + [(s, 2) for s in GENERAL] + [
    # the network's six shapes at 1280 x 704, the large ones at reduced C
    ((1, 32, 176, 320), 1), ((1, 32, 88, 160), 1), ((1, 32, 88, 160), 2),
    ((1, 256, 44, 80), 1), ((1, 256, 44, 80), 2), ((1, 512, 22, 40), 1),
    # band 4 and band 8, one row above a whole number of bands
    ((1, 10923, 9, 5), 1), ((1, 10923, 17, 9), 2), ((1, 10923, 17, 5), 1), ((1, 10923, 33, 9), 2),
]
CASES = list(dict.fromkeys(CASES))   # ((1, 512, 22, 40), 1) is in both lists


def case_id(case):
    (N, C, H, W), s = case
    return f"{N}x{C}x{H}x{W}-s{s}"


# the six distinct shapes of FOTSNet's depthwise convolutions for a 1280 x 704 image: (C, H, W, stride)
NETWORK_SHAPES = [(256, 176, 320, 1), (256, 88, 160, 1), (128, 88, 160, 2), (256, 44, 80, 1), (256, 44, 80, 2), (512, 22, 40, 1)]
