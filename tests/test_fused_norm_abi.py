"""CPU: the fused InstanceNorm entry point is exported, declared and host-checked; the Python surface raises
as documented; `use_native_blocks` switches classes only, composes with the other three switches and leaves a CPU pass
bit for bit stock; `fused_norm_ok` declines every disqualifying property; the tests' own reference is pinned against torch
and stays inside its bound.  No kernel is launched here."""
import ctypes
import itertools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import fused_norm_cases as FN
import instancenorm_cases as I
from test_abi import declared_functions
from test_depthwise_abi import fake_cuda

NAME = "rroi_instancenorm_fused_forward_hip"
SPLIT_SHAPE = (1, 2, 128, 256)      # needs a workspace
PLANE_SHAPE = (1, 4, 8, 8)          # needs none


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def test_symbol_is_exported_and_declared(ext):
    lib = ctypes.CDLL(ext.LIB_PATH)
    assert NAME in declared_functions() and NAME in ext.EXPORTS and hasattr(lib, NAME)
    assert callable(ext.instance_norm_fused) and callable(ext._instance_norm_fused_run)


def test_refusals_return_zero_before_any_launch(ext):
    f = ext._lib.rroi_instancenorm_fused_forward_hip
    P = 0x7f0000000000   # non-null, a multiple of 256, never dereferenced: every call below is refused on the host
    ok = dict(dtype=0, x=P, gamma=P, beta=P, r=P, y=P, shape=PLANE_SHAPE, mirror=0, eps=1e-5, slope=0.01, ws=None, nbytes=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["dtype"], a["x"], a["gamma"], a["beta"], a["r"], a["y"], *a["shape"], a["mirror"], a["eps"], a["slope"],
                 a["ws"], a["nbytes"], None)

    modes = (dict(), dict(mirror=1, r=None), dict(r=None))     # residual, mirror, neither (the plain call)
    for mode in modes:
        for dtype in (3, -1, 100):
            assert call(dtype=dtype, **mode) == 0
        for shape in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (-1, 4, 8, 8), (1, 4, 8, -3)):
            assert call(shape=shape, **mode) == 0, shape
        for shape in ((1, 1 << 11, 1 << 10, 1 << 10), (1 << 16, 1 << 15, 1, 1), (2, 2, 1 << 15, 1 << 14),
                      (0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff)):
            for dtype in (0, 1, 2):
                assert call(dtype=dtype, shape=shape, ws=P, nbytes=1 << 40, **mode) == 0, shape    # N * C * H * W >= 2^31
        for dtype in (0, 1, 2):
            assert call(dtype=dtype, x=None, **mode) == 0
            assert call(dtype=dtype, y=None, **mode) == 0
            assert call(dtype=dtype, gamma=None, **mode) == 0                                       # exactly one of gamma / beta
            assert call(dtype=dtype, beta=None, **mode) == 0
        for eps in (0.0, -1e-5, float("nan"), float("inf"), -float("inf")):
            assert call(eps=eps, **mode) == 0, eps
            assert call(eps=eps, gamma=None, beta=None, **mode) == 0, eps
        for slope in (float("nan"), float("inf"), -float("inf")):
            assert call(slope=slope, **mode) == 0, slope
        need = ext.instance_norm_workspace_bytes(*SPLIT_SHAPE)                                      # x's shape, in every mode
        assert need > 0
        for dtype in (0, 1, 2):
            assert call(dtype=dtype, shape=SPLIT_SHAPE, ws=None, nbytes=need, **mode) == 0
            for off in (1, 16, 255):
                assert call(dtype=dtype, shape=SPLIT_SHAPE, ws=P + off, nbytes=need + 256, **mode) == 0, off
            assert call(dtype=dtype, shape=SPLIT_SHAPE, ws=P, nbytes=need - 1, **mode) == 0
            assert call(dtype=dtype, shape=SPLIT_SHAPE, ws=P, nbytes=0, **mode) == 0
    # what this entry point refuses on its own
    for dtype in (0, 1, 2):
        assert call(dtype=dtype, mirror=1) == 0                                                     # mirror with a residual
        for mirror in (2, -1, 256):
            assert call(dtype=dtype, mirror=mirror) == 0
            assert call(dtype=dtype, mirror=mirror, r=None) == 0
        # N * 2C * H * W = 2^31 at a shape the plain call accepts (its plan exists)
        big = (1, 1 << 10, 1 << 10, 1 << 10)
        assert ext.instance_norm_plan(*big, dtype=dtype).form == I.PLANE
        assert call(dtype=dtype, shape=big, mirror=1, r=None, ws=P, nbytes=1 << 40) == 0


def test_python_surface_raises_as_documented(ext):
    x, w, b = torch.zeros(2, 3, 8, 8), torch.ones(3), torch.zeros(3)
    w2, b2 = torch.ones(6), torch.zeros(6)
    r = torch.zeros(2, 3, 8, 8)
    for dtype in I.DTYPES:
        for kw in (dict(residual=r.to(dtype)), dict(mirror=True), dict()):
            with pytest.raises(RuntimeError, match="GPU only"):
                ext.instance_norm_fused(x.to(dtype), **kw)
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.instance_norm_fused(x.to(dtype), w.to(dtype), b.to(dtype), negative_slope=0.01, residual=r.to(dtype))
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.instance_norm_fused(x.to(dtype), w2.to(dtype), b2.to(dtype), negative_slope=0.01, mirror=True)
    with pytest.raises(TypeError):
        ext.instance_norm_fused([1.0])
    with pytest.raises(TypeError):
        ext.instance_norm_fused(x, residual=[1.0])
    # the exceptions of instance_norm
    for bad in (dict(x=x[0]), dict(weight=w.to(torch.bfloat16), bias=b.to(torch.bfloat16)), dict(weight=w, bias=b.half()),
                dict(weight=torch.ones(4), bias=torch.zeros(4)), dict(weight=w, bias=None), dict(weight=None, bias=b)):
        args = dict(dict(x=x, residual=r), **bad)
        if args["x"].dim() != 4:
            args["residual"] = None
        with pytest.raises(ValueError):
            ext.instance_norm_fused(**args)
    # the residual
    with pytest.raises(ValueError, match="shape"):
        ext.instance_norm_fused(x, w, b, residual=torch.zeros(2, 3, 8, 9))
    with pytest.raises(ValueError, match="shape"):
        ext.instance_norm_fused(x, w, b, residual=torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="dtype"):
        ext.instance_norm_fused(x, w, b, residual=r.half())
    with pytest.raises(ValueError, match="device"):
        ext.instance_norm_fused(x, w, b, residual=torch.zeros(2, 3, 8, 8, device="meta"))
    # the mirror
    with pytest.raises(ValueError, match="residual"):
        ext.instance_norm_fused(x, w2, b2, residual=r, mirror=True)
    with pytest.raises(ValueError):
        ext.instance_norm_fused(x, w, b, mirror=True)                 # (C,), not (2C,)
    with pytest.raises(ValueError):
        ext.instance_norm_fused(x, w2, b2)                            # (2C,) without mirror
    with pytest.raises(ValueError):
        ext.instance_norm_fused(x, w2, b, mirror=True)


# ---------------------------------------------------------------- the switch
def outputs_equal(a, b):
    return all(torch.equal(s, t) for u, v in zip(a, b) for s, t in zip(u, v))


def test_use_native_blocks_switches_classes_only_and_composes():
    from fots_e2e.model import FOTSNet, _MirrorNorm, _PlainBlock, _SeparableBlock
    from fots_e2e.native import (NativeMirrorNorm, NativePlainBlock, NativeSeparableBlock, use_native_blocks,
                                 use_native_depthwise, use_native_heads, use_native_instancenorm)
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet()).eval()
    keys = list(net.state_dict().keys())
    ptrs = {k: p.data_ptr() for k, p in net.named_parameters()}
    classes = {n: type(m) for n, m in net.named_modules()}
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    crops = torch.randn(3, 64, 11, 24, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        stock, stock_ocr = net(x), net.forward_ocr(crops)

    def unchanged():
        return list(net.state_dict().keys()) == keys and {k: p.data_ptr() for k, p in net.named_parameters()} == ptrs

    def same_as_stock():
        with torch.no_grad():           # on CPU input the switched network takes the stock path: the same bits
            return outputs_equal(stock, net(x)) and torch.equal(stock_ocr, net.forward_ocr(crops))

    def count(cls):
        return sum(type(m) is cls for m in net.modules())

    # alone
    assert use_native_blocks(net) == (2, 7, 10)
    assert use_native_blocks(net) == (0, 0, 0)
    assert (count(NativeMirrorNorm), count(NativePlainBlock), count(NativeSeparableBlock)) == (2, 7, 10)
    assert count(_MirrorNorm) == count(_PlainBlock) == count(_SeparableBlock) == 0
    assert unchanged() and same_as_stock()
    assert use_native_blocks(net, enable=False) == (2, 7, 10)
    assert {n: type(m) for n, m in net.named_modules()} == classes and unchanged()
    assert use_native_blocks(net, enable=False) == (0, 0, 0)

    # with the three other switches, in two different orders
    others = (lambda on: use_native_depthwise(net, on) == 22,
              lambda on: use_native_instancenorm(net, on) == (52, 20),
              lambda on: use_native_heads(net, on) is True)
    blocks = lambda on: use_native_blocks(net, on) == (2, 7, 10)   # noqa: E731
    for order in ((blocks,) + others, others[::-1] + (blocks,)):
        for switch in order:
            assert switch(True)
        assert unchanged() and same_as_stock()
        assert (count(NativeMirrorNorm), count(NativePlainBlock), count(NativeSeparableBlock)) == (2, 7, 10)
        fused = [n for n, m in net.named_modules() if getattr(m, "fused_slope", None) is not None]
        assert len(fused) == 20                                    # the other switch's pairs are what they were
        for switch in order:                                        # undone in the order they were made ...
            assert switch(False)
        assert {n: type(m) for n, m in net.named_modules()} == classes and unchanged() and same_as_stock()
    # ... and undone in another order than made
    for switch in (others[1], blocks, others[0], others[2]):
        assert switch(True)
    for switch in (blocks, others[2], others[1], others[0]):
        assert switch(False)
    assert {n: type(m) for n, m in net.named_modules()} == classes and unchanged()

    # exact types only: a subclass of a block is left alone
    class Mine(_PlainBlock):
        pass
    other = nn.Sequential(Mine(4, 4, 1, None), _PlainBlock(4, 4, 1, None), _MirrorNorm(2), _SeparableBlock(4, 4, 1, None))
    assert use_native_blocks(other) == (1, 1, 1) and type(other[0]) is Mine


# ---------------------------------------------------------------- the predicate
def norm(c=4, **kw):
    return nn.InstanceNorm2d(c, **kw)


def test_fused_norm_ok_declines_each_disqualifying_property():
    from fots_e2e.native import NativeInstanceNorm2d, fused_norm_ok, instancenorm_ok
    t = fake_cuda(torch.zeros(2, 4, 8, 8))
    r = fake_cuda(torch.zeros(2, 4, 8, 8))
    with torch.no_grad():
        for m in (norm(), norm(affine=True)):
            assert fused_norm_ok(m, t) and fused_norm_ok(m, t, residual=r)
        for dtype in (torch.bfloat16, torch.float16):
            td, rd = fake_cuda(torch.zeros(2, 4, 8, 8, dtype=dtype)), fake_cuda(torch.zeros(2, 4, 8, 8, dtype=dtype))
            assert fused_norm_ok(norm(affine=True).to(dtype), td, residual=rd)
        # everything instancenorm_ok declines
        for bad in (torch.zeros(2, 4, 8, 8), fake_cuda(torch.zeros(2, 5, 8, 8)), fake_cuda(torch.zeros(2, 4, 1, 1)),
                    fake_cuda(torch.zeros(2, 4, 8, 8).to(memory_format=torch.channels_last))):
            assert not instancenorm_ok(norm(), bad)
            assert not fused_norm_ok(norm(), bad) and not fused_norm_ok(norm(), bad, residual=fake_cuda(torch.zeros_like(bad)))
        assert not fused_norm_ok(norm(track_running_stats=True), t, residual=r)
        # the residual
        assert not fused_norm_ok(norm(), t, residual=torch.zeros(2, 4, 8, 8))                            # on the CPU
        assert not fused_norm_ok(norm(), t, residual=fake_cuda(torch.zeros(2, 4, 8, 9)))                 # another shape
        assert not fused_norm_ok(norm(), t, residual=fake_cuda(torch.zeros(1, 4, 8, 8).expand(2, 4, 8, 8)))
        assert not fused_norm_ok(norm(), t, residual=fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.bfloat16)))
        assert not fused_norm_ok(norm(), t, residual=fake_cuda(torch.zeros(2, 4, 8, 16)[:, :, :, ::2]))  # strided
        assert not fused_norm_ok(norm(), t, residual=fake_cuda(torch.zeros(2, 4, 8, 8).to(memory_format=torch.channels_last)))
        assert not fused_norm_ok(norm(), t, residual=[0.0])
        # the mirror: an affine norm of twice the channels, no residual
        assert fused_norm_ok(norm(8, affine=True), t, mirror=True)
        assert not fused_norm_ok(norm(8), t, mirror=True)                                                # not affine
        assert not fused_norm_ok(norm(4, affine=True), t, mirror=True)                                   # C, not 2C
        assert not fused_norm_ok(norm(16, affine=True), t, mirror=True)
        assert not fused_norm_ok(norm(8, affine=True), t, residual=r, mirror=True)
        assert not fused_norm_ok(norm(8, affine=True), torch.zeros(2, 4, 8, 8), mirror=True)             # a CPU tensor
        # 2 t.numel() = 2^31 (on the meta device: contiguous, and nothing is allocated); one column fewer passes
        wide = nn.InstanceNorm2d(1 << 11, affine=True, device="meta")
        assert not fused_norm_ok(wide, fake_cuda(torch.empty(1, 1 << 10, 1 << 10, 1 << 10, device="meta")), mirror=True)
        assert fused_norm_ok(wide, fake_cuda(torch.empty(1, 1 << 10, 1 << 10, (1 << 10) - 1, device="meta")), mirror=True)
        # a norm that use_native_instancenorm has given an activation of its own
        m = norm(affine=True)
        m.__class__ = NativeInstanceNorm2d
        assert fused_norm_ok(m, t, residual=r) and fused_norm_ok(m, t)
        m.fused_slope = 0.01
        assert not fused_norm_ok(m, t, residual=r) and not fused_norm_ok(m, t)
        m8 = norm(8, affine=True)
        m8.__class__ = NativeInstanceNorm2d
        assert fused_norm_ok(m8, t, mirror=True)
        m8.fused_slope = 0.0                                          # (0.0 is a slope too: ReLU)
        assert not fused_norm_ok(m8, t, mirror=True)
    # a residual that needs a gradient, under grad mode (the norm's own parameters need none here)
    m = norm()
    rg = fake_cuda(torch.zeros(2, 4, 8, 8)).requires_grad_(True)
    assert fused_norm_ok(m, t, residual=r)
    assert not fused_norm_ok(m, t, residual=rg)
    with torch.no_grad():
        assert fused_norm_ok(m, t, residual=rg)


def test_blocks_in_training_mode_or_on_cpu_input_run_the_stock_forward(monkeypatch):
    """The gate in front of a block's work: nothing native is asked for, so nothing is computed twice."""
    import fots_e2e.native as native
    from fots_e2e.model import _PlainBlock, _SeparableBlock

    def refuse(*a, **k):
        raise AssertionError("a predicate was asked")
    x = torch.randn(1, 4, 6, 6, generator=torch.Generator().manual_seed(2))
    for cls in (_PlainBlock, _SeparableBlock):
        block = cls(4, 4, 1, None).eval()
        with torch.no_grad():
            want = block(x)
        assert sum(native.use_native_blocks(block)) == 1
        with monkeypatch.context() as mp:
            mp.setattr(native, "fused_norm_ok", refuse)
            with torch.no_grad():
                assert torch.equal(block(x), want)                                # CPU input
            assert block(x.clone().requires_grad_(True)).requires_grad
        with torch.no_grad():
            assert native._block_input_ok(block, fake_cuda(x))
            assert not native._block_input_ok(block, x)
            assert not native._block_input_ok(block, fake_cuda(x.double()))
            assert not native._block_input_ok(block, fake_cuda(x[0]))
            block.train()
            assert not native._block_input_ok(block, fake_cuda(x))                # training mode, whatever the input
            block.eval()
        assert not native._block_input_ok(block, fake_cuda(x))                    # a gradient is needed: the parameters'
        for p in block.parameters():
            p.requires_grad_(False)
        assert native._block_input_ok(block, fake_cuda(x))
        assert not native._block_input_ok(block, fake_cuda(x.clone()).requires_grad_(True))   # ... the input's


# ---------------------------------------------------------------- the reference
def test_fused_reference_is_pinned_against_torch():
    """In float64, F.leaky_relu(F.instance_norm(x64, ...) + r64, slope) lies within 2^-40 (|x a| + |b|) of ref64: the
    bound of test_instancenorm_abi.test_reference_is_pinned_against_torch, for the same reason (the sum with r64 and the
    activation add no error of that order: r64 is exact in both, and a product with the slope scales both alike)."""
    worst, total = 0.0, 0
    for shape in I.CASES[1:7]:                  # (torch refuses planes of one element)
        x, gamma, beta, stats = I.problem(shape, torch.float32)
        r = FN.residual_of(shape, torch.float32)
        for slope in I.SLOPES:
            out, ref64, a, b = FN.reference(x, gamma, beta, I.EPS, slope, stats, r)
            want = F.leaky_relu(F.instance_norm(x.double(), weight=gamma.double(), bias=beta.double(), use_input_stats=True,
                                                eps=I.EPS) + r.double(), float(torch.tensor(slope, dtype=torch.float32)))
            scale = (x.double() * a).abs() + b.abs()
            worst = max(worst, float(((ref64 - want).abs() / scale).max()))
            total += out.numel()
        # the mirror is the same reference on the concatenated tensor
        x, x2, g2, b2, stats2 = FN.mirror_problem(shape, torch.float32)
        out, ref64, a, b = FN.reference(x2, g2, b2, I.EPS, 0.01, stats2)
        want = F.leaky_relu(F.instance_norm(torch.cat((x, -x), 1).double(), weight=g2.double(), bias=b2.double(),
                                            use_input_stats=True, eps=I.EPS), float(torch.tensor(0.01, dtype=torch.float32)))
        scale = (x2.double() * a).abs() + b.abs()
        worst = max(worst, float(((ref64 - want).abs() / scale).max()))
        # the two halves of the mirror's statistics are each other's negation: a alike, the means opposite
        C = shape[1]
        assert torch.equal(torch.from_numpy(stats2[0][:, :C]), -torch.from_numpy(stats2[0][:, C:]))
        assert torch.equal(torch.from_numpy(stats2[1][:, :C]), torch.from_numpy(stats2[1][:, C:]))
    print(f"fused reference vs torch float64: worst relative difference {worst:.3g} over {total} elements")
    assert worst <= 2.0 ** -40, worst
    assert total > 100000
    # without a residual and without the mirror it is the reference of the plain norm
    x, gamma, beta, stats = I.problem(I.CASES[1], torch.bfloat16)
    for slope in I.SLOPES:
        assert torch.equal(FN.reference(x, gamma, beta, I.EPS, slope, stats)[0], I.reference(x, gamma, beta, I.EPS, slope, stats)[0])


@pytest.mark.parametrize("dtype", I.DTYPES, ids=I.IDS)
def test_the_reference_alone_stays_inside_the_bound(dtype):
    """Condition (a) of the GPU tests, asked of the rounded reference itself over the whole table, both modes."""
    for shape, slope in itertools.product(I.CASES, I.SLOPES):
        x, gamma, beta, stats = I.problem(shape, dtype)
        r = FN.residual_of(shape, dtype)
        out, ref64, a, b = FN.reference(x, gamma, beta, I.EPS, slope, stats, r)
        ok, worst = FN.within_bound(out, ref64, x, a, b, r)
        assert ok, (shape, slope, worst)
        _, x2, g2, b2, stats2 = FN.mirror_problem(shape, dtype)
        out, ref64, a, b = FN.reference(x2, g2, b2, I.EPS, slope, stats2)
        ok, worst = FN.within_bound(out, ref64, x2, a, b)
        assert ok, (shape, slope, worst)
