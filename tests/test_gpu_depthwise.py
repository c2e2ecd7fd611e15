"""GPU (MI355X): the native depthwise 3x3 convolution against the numpy oracle of depthwise_cases.py,
compared as integers ("both NaN" counts as equal): shapes chosen for the kernel's tile, special values, misaligned base
addresses, nothing written outside the output, graph capture, the module switch, and the 22 convolutions of the network
on the inputs they really see."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import depthwise_cases as D
from test_gpu_bucketed import NAN_PATTERN, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def raw_call(ext, x, w, y, shape, stride):
    """The C ABI on tensors (or views) as they are: nothing is made contiguous or aligned on the way."""
    N, C, H, W = shape
    st = ext._lib.rroi_depthwise3x3_forward_hip(ext.dtype_code(x.dtype), x.data_ptr(), w.data_ptr(), y.data_ptr(), N, C, H, W,
                                                stride, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


# ---------------------------------------------------------------- bit-exact against the oracle
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.IDS)
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_bit_exact_against_the_oracle(ext, case, dtype):
    """Tile width 4 and band heights 2 / 4 / 8: the table holds output widths 3, 4, 5 and, for every band height, an output
    height one above a whole number of bands (test_depthwise_abi.test_case_table_reaches_every_band_height)."""
    shape, stride = case
    x, w = D.random_problem(shape, dtype, seed=sum(shape) + stride)
    got = ext.depthwise3x3(x.cuda(), w.cuda(), stride)
    want = D.expected(x, w, stride)
    assert got.shape == want.shape and got.is_contiguous()
    assert same_bits(got.cpu(), want)


def test_empty_batch_returns_without_a_call(ext):
    out = ext.depthwise3x3(torch.zeros(0, 4, 9, 9, device="cuda"), torch.zeros(4, 1, 3, 3, device="cuda"), 2)
    assert out.shape == (0, 4, 5, 5)


# ---------------------------------------------------------------- special values
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.IDS)
def test_special_values(ext, dtype, stride):
    x, w = D.random_problem((2, 4, 9, 11), dtype, seed=5)
    nan, inf = float("nan"), float("inf")
    x[0, 0, 0, 0], x[0, 0, 0, 5], x[0, 0, 8, 10], x[0, 0, 4, 0], x[0, 0, 4, 5] = nan, inf, -inf, -0.0, nan
    x[0, 1, 0, :], x[0, 1, :, 10], x[0, 1, 8, :], x[0, 1, 3:6, 3:6] = -0.0, -0.0, -0.0, -0.0
    x[1, 0, 8, 0], x[1, 0, 0, 10], x[1, 0, 5, 6], x[1, 1, 4, 4] = inf, -inf, inf, -inf
    w[2, 0, 0, 0] = inf                        # channel 2: the top-left tap is in the padding for row 0 and column 0: inf * +0.0
    w[3] = w[3].abs()                          # channel 3: -0.0 everywhere gives w * -0.0 = -0.0 nine times: +0.0 + -0.0 = +0.0
    x[:, 3] = -0.0
    got = ext.depthwise3x3(x.cuda(), w.cuda(), stride).cpu()
    assert same_bits(got, D.expected(x, w, stride))
    assert got[:, 2, 0, :].isnan().all() and got[:, 2, :, 0].isnan().all()
    assert not got[:, 2, 1:, 1:].isnan().any()                # elsewhere inf * x is +-inf, a number
    assert not got[:, 3].view(torch.int32 if dtype == torch.float32 else torch.int16).any()   # +0.0, bit for bit


@pytest.mark.parametrize("stride", (1, 2))
def test_fp32_subnormals_are_kept(ext, stride):
    rng = np.random.default_rng(11)
    shape = (1, 3, 10, 13)
    tiny = np.float32(2.0 ** -130)             # subnormal: below 2^-126
    cases = {
        "subnormal inputs": (rng.standard_normal(shape).astype(np.float32) * tiny, rng.standard_normal((3, 1, 3, 3)).astype(np.float32)),
        "subnormal weights": (rng.standard_normal(shape).astype(np.float32), rng.standard_normal((3, 1, 3, 3)).astype(np.float32) * tiny),
        "subnormal products": (rng.standard_normal(shape).astype(np.float32) * np.float32(2.0 ** -70),
                               rng.standard_normal((3, 1, 3, 3)).astype(np.float32) * np.float32(2.0 ** -65)),
    }
    for name, (x, w) in cases.items():
        want = D.oracle_depthwise3x3(x, w, stride)
        mag = np.abs(want[want != 0])
        assert mag.size > want.size // 2 and mag.max() < 2.0 ** -126, name       # the outputs ARE subnormal
        got = ext.depthwise3x3(torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda(), stride).cpu()
        assert same_bits(got, torch.from_numpy(want)), name


# ---------------------------------------------------------------- addresses
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.IDS)
def test_any_element_aligned_base_address(ext, dtype, stride):
    """x, w and y each 1, 2 and 3 elements into an aligned allocation, through the raw ABI (W = 24: rows keep the base's
    misalignment, so the element path runs everywhere; offset 0 of the other two keeps their vector paths in the call)."""
    shape = (2, 3, 9, 24)
    N, C, H, W = shape
    x, w = D.random_problem(shape, dtype, seed=21)
    want = D.expected(x, w, stride)
    for which in range(3):
        for off in (1, 2, 3):
            offs = [off if k == which else 0 for k in range(3)]
            xb = torch.zeros(x.numel() + 4, dtype=dtype, device="cuda")
            wb = torch.zeros(w.numel() + 4, dtype=dtype, device="cuda")
            yb = torch.zeros(want.numel() + 4, dtype=dtype, device="cuda")
            xv, wv, yv = xb[offs[0]:offs[0] + x.numel()], wb[offs[1]:offs[1] + w.numel()], yb[offs[2]:offs[2] + want.numel()]
            xv.copy_(x.reshape(-1))
            wv.copy_(w.reshape(-1))
            assert xv.data_ptr() == xb.data_ptr() + offs[0] * x.element_size()
            assert raw_call(ext, xv, wv, yv, shape, stride) == 1
            assert same_bits(yv.cpu().view(want.shape), want), (which, off)


# ---------------------------------------------------------------- nothing else is written
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.IDS)
@pytest.mark.parametrize("shape", [(2, 5, 7, 13), (1, 3, 16, 32)], ids=["odd", "aligned"])
def test_nothing_outside_the_output_is_written(ext, shape, dtype, stride):
    N, C, H, W = shape
    x, w = D.random_problem(shape, dtype, seed=31)
    want = D.expected(x, w, stride)
    itype = torch.int32 if dtype == torch.float32 else torch.int16
    for start in (64, 67):                     # y on a 16-byte boundary of the buffer, and 3 elements past one
        buf = torch.full((start + want.numel() + 64,), NAN_PATTERN[dtype], dtype=itype, device="cuda")
        before = buf.clone()
        yv = buf[start:start + want.numel()].view(dtype)
        assert raw_call(ext, x.cuda(), w.cuda(), yv, shape, stride) == 1
        inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
        inside[start:start + want.numel()] = True
        assert torch.equal(buf[~inside], before[~inside]), "a byte outside y was written"
        assert not (buf[inside] == before[inside]).any(), "an element of y was left unwritten"
        assert same_bits(yv.cpu().view(want.shape), want)


# ---------------------------------------------------------------- graph capture
def test_graph_capture_reproduces_the_eager_bits(ext):
    for dtype, stride in ((torch.float32, 1), (torch.bfloat16, 2)):
        x, w = D.random_problem((2, 16, 44, 80), dtype, seed=41)
        x, w = x.cuda(), w.cuda()
        ext.depthwise3x3(x, w, stride)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                out = ext.depthwise3x3(x, w, stride)
        for k in range(2):
            x.copy_(D.random_problem((2, 16, 44, 80), dtype, seed=42 + k)[0])   # x changes in place
            out.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert same_bits(out, ext.depthwise3x3(x, w, stride))
            assert same_bits(out.cpu(), D.expected(x, w, stride))


# ---------------------------------------------------------------- the module really runs the kernel
def test_switched_module_runs_the_kernel_and_falls_back(ext, monkeypatch):
    from fots_e2e.native import DepthwiseConv3x3, native_ok, use_native_depthwise
    net = nn.Sequential(nn.Conv2d(8, 8, 3, 2, 1, groups=8, bias=False), nn.Conv2d(8, 8, 1)).cuda()
    assert use_native_depthwise(net) == 1 and type(net[0]) is DepthwiseConv3x3 and type(net[1]) is nn.Conv2d
    m = net[0]
    x = torch.randn(2, 8, 13, 17, device="cuda")
    stock = F.conv2d

    def refuse(*a, **k):
        raise AssertionError("the stock convolution was called")
    monkeypatch.setattr(F, "conv2d", refuse)
    with torch.no_grad():
        assert native_ok(m, x)
        y = m(x)                                            # works although F.conv2d raises: the kernel ran
    assert same_bits(y.cpu(), D.expected(x, m.weight, 2))
    with pytest.raises(AssertionError, match="stock convolution"):
        m(x.requires_grad_(True))                           # grad enabled + requires_grad: the stock path (which raises here)
    monkeypatch.setattr(F, "conv2d", stock)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        xa = x.detach()
        assert not native_ok(m, xa)                         # autocast: the stock module's bf16 output, not the fp32 kernel's
        assert m(xa).dtype == torch.bfloat16
    xg = x.detach().clone().requires_grad_(True)
    assert not native_ok(m, xg)
    yg = m(xg)
    assert yg.requires_grad and torch.equal(yg, stock(xg, m.weight, None, 2, 1, 1, 8))
    yg.sum().backward()
    assert xg.grad is not None and m.weight.grad is not None  # training is untouched
    with torch.no_grad():
        xc = x.detach().to(memory_format=torch.channels_last)
        assert not native_ok(m, xc)
        assert torch.equal(m(xc), stock(xc, m.weight, None, 2, 1, 1, 8))


# ---------------------------------------------------------------- in the network
def abs_sum(x, w, stride):
    """sum |w| |x| over the nine taps, in float64 on the device (the scale of the rounding bound)."""
    xa = F.pad(x.double().abs(), (1, 1, 1, 1))
    wa = w.double().abs()
    ho, wo = D.out_size(x.size(2), stride), D.out_size(x.size(3), stride)
    s = torch.zeros((x.size(0), x.size(1), ho, wo), dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            s += wa[None, :, 0, ky, kx, None, None] * xa[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
    return s


def ulp_at(y):
    """One ulp of y's 16-bit type at |y| (the smallest subnormal at 0), as float64."""
    p, emin = (7, -126) if y.dtype == torch.bfloat16 else (10, -14)
    _, e = torch.frexp(y.double().abs())                    # |y| = m * 2^e, m in [0.5, 1)
    e = torch.where(y == 0, torch.full_like(e, emin), torch.clamp(e - 1, min=emin))
    return torch.ldexp(torch.ones_like(y, dtype=torch.float64), e - p)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=["fp32", "bf16"])
def test_the_22_convolutions_of_the_network(ext, dtype):
    """Each depthwise convolution of FOTSNet on the input it sees in a stock pass over a 1280 x 704 image: the switched
    module equals the oracle bit for bit, and lies within |y_native - y_stock| <= 10 * 2^-24 * sum|w x| + eps_T of the stock
    module (eps_T: 0 for fp32, one ulp of T at |y| for 16-bit outputs, which covers a truncating conversion on the stock
    side).  The stock path's accumulation is not ours to specify: a sanity bound, not a parity claim."""
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import DepthwiseConv3x3, _static_ok, use_native_depthwise
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet()).eval().cuda().to(dtype)
    mods = [(n, m) for n, m in net.named_modules() if type(m) is nn.Conv2d and _static_ok(m)]
    assert len(mods) == 22
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, inp, out, n=n: seen.__setitem__(n, (inp[0].detach(), out.detach()))) for n, m in mods]
    x = torch.randn(1, 3, 704, 1280, generator=torch.Generator().manual_seed(77)).cuda().to(dtype)
    with torch.no_grad():
        net(x)
    for h in hooks:
        h.remove()
    assert len(seen) == 22
    assert {(m.in_channels, seen[n][0].size(2), seen[n][0].size(3), m.stride[0]) for n, m in mods} == set(D.NETWORK_SHAPES)
    assert use_native_depthwise(net) == 22
    with torch.no_grad():
        for n, m in mods:
            assert type(m) is DepthwiseConv3x3
            xin, y_stock = seen[n]
            y = m(xin)
            assert same_bits(y.cpu(), D.expected(xin, m.weight, m.stride[0])), n
            bound = 10 * 2.0 ** -24 * abs_sum(xin, m.weight, m.stride[0])
            if dtype != torch.float32:
                bound = bound + ulp_at(y)
            err = (y.double() - y_stock.double()).abs()
            worst = float((err / bound.clamp_min(1e-300)).max())
            print(f"{n}: max |native - stock| / bound = {worst:.3f}")
            assert bool((err <= bound).all()), (n, worst)
