"""CPU: the depthwise 3x3 entry point is exported, declared and host-checked; the Python surface refuses CPU tensors and
mismatched arguments; `native_ok` / `use_native_depthwise` do what fots_e2e.native says; the tests' oracle is pinned
against torch.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import depthwise_cases as D
from test_abi import declared_functions


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def test_symbol_is_exported_and_declared(ext):
    assert "rroi_depthwise3x3_forward_hip" in declared_functions()
    assert "rroi_depthwise3x3_forward_hip" in ext.EXPORTS
    assert hasattr(ctypes.CDLL(ext.LIB_PATH), "rroi_depthwise3x3_forward_hip")


def test_refusals_return_zero_before_any_launch(ext):
    f = ext._lib.rroi_depthwise3x3_forward_hip
    P = 0x7f0000000000   # non-null, never dereferenced: every call below is refused on the host
    assert f(3, P, P, P, 1, 4, 8, 8, 1, None) == 0          # unknown dtype
    assert f(-1, P, P, P, 1, 4, 8, 8, 1, None) == 0
    for stride in (0, 3, -1, 4):
        assert f(0, P, P, P, 1, 4, 8, 8, stride, None) == 0
    for dims in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (-1, 4, 8, 8), (1, 4, 8, -3)):
        assert f(0, P, P, P, *dims, 1, None) == 0, dims
    for dims in ((1, 1 << 11, 1 << 10, 1 << 10), (1 << 16, 1 << 15, 1, 1), (2, 2, 1 << 15, 1 << 14),
                 (0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff)):
        for dtype in (0, 1, 2):
            assert f(dtype, P, P, P, *dims, 2, None) == 0, dims   # N * C * H * W >= 2^31
    # null pointers with valid sizes
    for dtype in (0, 1, 2):
        assert f(dtype, None, P, P, 1, 4, 8, 8, 1, None) == 0
        assert f(dtype, P, None, P, 1, 4, 8, 8, 2, None) == 0
        assert f(dtype, P, P, None, 1, 4, 8, 8, 1, None) == 0
        assert f(dtype, None, None, None, 1, 4, 8, 8, 1, None) == 0


def test_python_surface_refuses_cpu_tensors_and_mismatches(ext):
    x, w = torch.zeros(2, 3, 8, 8), torch.zeros(3, 1, 3, 3)
    for dtype in D.DTYPES:
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.depthwise3x3(x.to(dtype), w.to(dtype))
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.depthwise3x3(x.to(dtype), w.to(dtype), stride=2)
    with pytest.raises(ValueError):
        ext.depthwise3x3(x, w.to(torch.bfloat16))                 # dtypes differ
    with pytest.raises(ValueError):
        ext.depthwise3x3(x.half(), w)
    with pytest.raises(ValueError):
        ext.depthwise3x3(x, torch.zeros(4, 1, 3, 3))              # channels differ
    with pytest.raises(ValueError):
        ext.depthwise3x3(x, torch.zeros(3, 3, 3, 3))              # not depthwise
    with pytest.raises(ValueError):
        ext.depthwise3x3(x, torch.zeros(3, 1, 5, 5))
    with pytest.raises(ValueError):
        ext.depthwise3x3(x[0], w)                                 # not 4-D
    with pytest.raises(ValueError):
        ext.depthwise3x3(x, w, stride=3)


def qualifying(c=4, **kw):
    args = dict(kernel_size=3, stride=1, padding=1, groups=c, bias=False)
    args.update(kw)
    return nn.Conv2d(c, args.pop("out_channels", c), **args)


class FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: `native_ok` is pure, so its other conditions can be asked without one."""
    is_cuda = True


def fake_cuda(t):
    return t.as_subclass(FakeCuda)


def test_native_ok_declines_each_disqualifying_property(monkeypatch):
    from fots_e2e.native import native_ok
    x = fake_cuda(torch.zeros(2, 4, 8, 8))
    with torch.no_grad():
        assert native_ok(qualifying(), x)
        assert native_ok(qualifying(stride=2), x)
        for dtype in (torch.bfloat16, torch.float16):
            assert native_ok(qualifying().to(dtype), fake_cuda(torch.zeros(2, 4, 8, 8, dtype=dtype)))
        # a CPU tensor: everything else qualifies
        assert not native_ok(qualifying(), torch.zeros(2, 4, 8, 8))
        # the tensor
        assert not native_ok(qualifying(), fake_cuda(torch.zeros(4, 8, 8)))                      # not 4-D
        assert not native_ok(qualifying(), fake_cuda(torch.zeros(2, 4, 8, 8).to(memory_format=torch.channels_last)))
        assert not native_ok(qualifying(), fake_cuda(torch.zeros(2, 4, 8, 16)[:, :, :, ::2]))    # strided view
        assert not native_ok(qualifying(), fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.float64)))
        assert not native_ok(qualifying(), fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.bfloat16)))  # not the weight's
        assert not native_ok(qualifying().double(), fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.float64)))
        # the module
        assert not native_ok(qualifying(kernel_size=5, padding=2), x)
        assert not native_ok(qualifying(kernel_size=(3, 1), padding=(1, 0)), x)
        assert not native_ok(qualifying(padding=0), x)
        assert not native_ok(qualifying(padding=2, dilation=2), x)
        assert not native_ok(qualifying(stride=3), x)
        assert not native_ok(qualifying(stride=(1, 2)), x)
        assert not native_ok(qualifying(groups=2), x)
        assert not native_ok(qualifying(groups=1), x)
        assert not native_ok(qualifying(out_channels=8), x)                                      # a channel multiplier
        assert not native_ok(qualifying(bias=True), x)
        assert not native_ok(qualifying(padding_mode="reflect"), x)
        # 2^31 elements (a view of one element: nothing that large is allocated)
        assert not native_ok(qualifying(c=1 << 11), fake_cuda(torch.zeros(1).expand(1, 1 << 11, 1 << 10, 1 << 10)))
    # a gradient is needed: of the weight (a fresh module's default), of the input
    m = qualifying()
    assert m.weight.requires_grad and not native_ok(m, x)
    with torch.no_grad():
        assert native_ok(m, x)
    m.weight.requires_grad_(False)
    assert native_ok(m, x)
    with monkeypatch.context() as mp:                       # under autocast the stock module returns 16 bits: declined
        mp.setattr(torch, "is_autocast_enabled", lambda *a: True)   # (torch.autocast("cuda") switches itself off without a GPU)
        assert not native_ok(m, x)
    assert native_ok(m, x)
    xg = fake_cuda(torch.zeros(2, 4, 8, 8)).requires_grad_(True)
    assert not native_ok(m, xg)
    with torch.no_grad():
        assert native_ok(m, xg)


def test_use_native_depthwise_switches_22_modules_of_the_network_and_back():
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import DepthwiseConv3x3, use_native_depthwise
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet()).eval()
    keys = list(net.state_dict().keys())
    ptrs = {k: p.data_ptr() for k, p in net.named_parameters()}
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        stock = net(x)
    assert use_native_depthwise(net) == 22
    switched = [n for n, m in net.named_modules() if type(m) is DepthwiseConv3x3]
    assert len(switched) == 22
    assert all(".conv_sep1.0" in n or ".conv2.0" in n or n in ("upconv1.0", "upconv2.0") for n in switched), switched
    assert list(net.state_dict().keys()) == keys
    assert {k: p.data_ptr() for k, p in net.named_parameters()} == ptrs
    assert use_native_depthwise(net) == 0                       # nothing left to switch
    # on CPU input the switched network takes the stock path: exactly the stock network's output
    with torch.no_grad():
        again = net(x)
    for a, b in zip(stock, again):
        for s, t in zip(a, b):
            assert torch.equal(s, t)
    assert use_native_depthwise(net, enable=False) == 22
    assert all(type(m) is nn.Conv2d for m in net.modules() if isinstance(m, nn.Conv2d))
    assert list(net.state_dict().keys()) == keys
    assert {k: p.data_ptr() for k, p in net.named_parameters()} == ptrs


def test_case_table_reaches_every_band_height():
    """The GPU cases are chosen for the kernel's tile: every band height under both strides, and output widths and heights
    one below, at and one above the tile width and the band heights."""
    seen = {(D.band_of(*shape, s), s) for shape, s in D.CASES}
    assert seen == {(b, s) for b in D.BANDS for s in (1, 2)}
    for s in (1, 2):
        wos = {D.out_size(shape[3], s) for shape, st in D.CASES if st == s}
        assert {D.TILE_W - 1, D.TILE_W, D.TILE_W + 1} <= wos
        for band in D.BANDS:
            hos = {D.out_size(shape[2], s) % band for shape, st in D.CASES if st == s and D.band_of(*shape, s) == band}
            assert 1 in hos, (s, band)      # one row above a whole number of bands
        hos2 = {D.out_size(shape[2], s) for shape, st in D.CASES if st == s and D.band_of(*shape, s) == 2}
        assert {1, 2, 3} <= hos2
    assert {(C, H, W, s) for C, H, W, s in D.NETWORK_SHAPES} == {(256, 176, 320, 1), (256, 88, 160, 1), (128, 88, 160, 2),
                                                                   (256, 44, 80, 1), (256, 44, 80, 2), (512, 22, 40, 1)}


def test_oracle_is_pinned_against_torch():
    """200 random small fp32 problems, both strides: the oracle equals torch's double convolution rounded to fp32, except
    where the two double sums (the oracle's order is fixed, torch's is not) round to different floats -- at most 1 element
    in 10^5.  (Measured when the seeds were chosen: 0 of 136,327 elements differ.)"""
    rng = np.random.default_rng(20261018)
    total = differ = 0
    for i in range(200):
        N, C, H, W = (int(v) for v in (rng.integers(1, 4), rng.integers(1, 9), rng.integers(1, 20), rng.integers(1, 24)))
        s = 1 + i % 2
        x, w = D.random_problem((N, C, H, W), torch.float32, seed=1000 + i)
        got = torch.from_numpy(D.oracle_depthwise3x3(x.numpy(), w.numpy(), s))
        want = F.conv2d(x.double(), w.double(), padding=1, stride=s, groups=C).float()
        assert got.shape == want.shape == (N, C, D.out_size(H, s), D.out_size(W, s))
        total += got.numel()
        differ += int((got.view(torch.int32) != want.view(torch.int32)).sum())
    print(f"oracle vs torch: {differ} of {total} elements differ")
    assert total > 100000 and differ * 100000 <= total, (differ, total)
