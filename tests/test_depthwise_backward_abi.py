"""CPU: the depthwise 3x3 backward entry points (header section 5b) are exported, declared and host-checked;
the plan and workspace queries agree with the case module's mirror of the host rules over the whole table; the Python
surface raises what it documents; `TrainableDepthwiseConv3x3` / `use_trainable_depthwise` do what fots_e2e.native_train
says; the tests' oracle and reference are pinned against torch's float64 autograd.  No kernel is launched here."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import depthwise_backward_cases as B
import depthwise_cases as D
from test_abi import declared_functions
from test_depthwise_abi import fake_cuda, qualifying

NAMES = ("rroi_depthwise3x3_backward_hip", "rroi_depthwise3x3_backward_workspace_bytes", "rroi_depthwise3x3_backward_plan")
SHAPE = (2, 4, 8, 8)
P = 0x7f0000000000   # non-null, a multiple of 256, never dereferenced: every call below is refused on the host
FAR = 1 << 32        # between two fake tensors: they do not overlap


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def test_symbols_are_exported_and_declared(ext):
    lib = ctypes.CDLL(ext.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions() and name in ext.EXPORTS and hasattr(lib, name)
    for name in ("depthwise3x3_backward", "run_depthwise3x3_backward", "depthwise3x3_backward_plan",
                 "depthwise3x3_backward_workspace_bytes"):
        assert callable(getattr(ext, name))
    from rroi_align import conv
    assert callable(conv.depthwise3x3)
    assert ext.version() == "rroi_align_hip 0.10.0 gfx950"


def test_plan_and_workspace_queries_agree_with_the_mirror_over_the_table(ext):
    segs, bands = set(), set()
    for (shape, s) in B.CASES + [((1, c, h, w), st) for c, h, w, st in D.NETWORK_SHAPES] + [((8, c, h, w), st) for c, h, w, st in D.NETWORK_SHAPES]:
        N, C, H, W = shape
        band, items, nseg = B.plan_of(N, C, H, W, s)
        ho, wo = D.out_size(H, s), D.out_size(W, s)
        for dtype in D.DTYPES:
            p = ext.depthwise3x3_backward_plan(N, C, H, W, s, dtype=dtype)
            assert p.block == B.THREADS and p.launches == 3
            assert (p.dx_band, p.dx_cols, p.dw_band) == (band * s, D.TILE_W * s, band), (shape, s)
            assert p.dx_grid_x == -(-(N * C * items) // B.THREADS)
            assert p.segments == nseg and p.dw_grid_x == N * C * nseg
            assert (nseg - 1) * B.THREADS < -(-ho // band) * -(-wo // D.TILE_W) <= nseg * B.THREADS
        need = ext.depthwise3x3_backward_workspace_bytes(N, C, H, W, s)
        assert need == -(-(72 * N * C * nseg) // 256) * 256 and need > 0
        segs.add(nseg)
        bands.add((band, s))
    assert bands == {(b, s) for b in D.BANDS for s in (1, 2)} and {1, 2, 3} <= segs
    # the cases the table was extended for (the case module's comment)
    assert B.plan_of(1, 1, 514, 4, 1)[1:] == (257, 2) and B.plan_of(3, 2, 54, 76, 1)[1:] == (513, 3)
    assert B.plan_of(3, 2, 107, 76, 2)[1:] == (270, 2) and B.plan_of(3, 33, 5, 17, 1)[1:] == (15, 1)
    assert ext.depthwise3x3_backward_plan(1, 256, 176, 320, 1).segments == 7          # the network's largest plane
    # the grid of the partials launch is capped; the workspace is not
    many = ext.depthwise3x3_backward_plan(1 << 23, 1, 1, 1, 1)
    assert many.segments == 1 and many.dw_grid_x == 1 << 22
    assert ext.depthwise3x3_backward_workspace_bytes(1 << 23, 1, 1, 1, 1) == 72 << 23
    assert ext._lib.rroi_depthwise3x3_backward_plan(0, *SHAPE, 1, None) == 0
    for bad in ((1, 0, 8, 8, 1), (1, 4, 8, 8, 3), (1, 1 << 11, 1 << 10, 1 << 10, 1)):
        with pytest.raises(ValueError):
            ext.depthwise3x3_backward_plan(*bad)
        assert ext.depthwise3x3_backward_workspace_bytes(*bad) == 0
    with pytest.raises(ValueError):
        ext.depthwise3x3_backward_plan(1, 4, 8, 8, 1, dtype=7)


def test_refusals_return_zero_before_any_launch(ext):
    f = ext._lib.rroi_depthwise3x3_backward_hip
    need = ext.depthwise3x3_backward_workspace_bytes(*SHAPE, 1)
    ok = dict(dtype=0, dy=P, x=P + FAR, w=P + 2 * FAR, dx=P + 3 * FAR, dw=P + 4 * FAR, shape=SHAPE, stride=1, ws=P + 5 * FAR,
              nbytes=need)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["dtype"], a["dy"], a["x"], a["w"], a["dx"], a["dw"], *a["shape"], a["stride"], a["ws"], a["nbytes"], None)

    # everything section 5 refuses
    for dtype in (3, -1, 100):
        assert call(dtype=dtype) == 0
    for stride in (0, 3, -1, 4):
        assert call(stride=stride) == 0
    for shape in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (-1, 4, 8, 8), (1, 4, 8, -3)):
        assert call(shape=shape, nbytes=1 << 40) == 0, shape
    for shape in ((1, 1 << 11, 1 << 10, 1 << 10), (1 << 16, 1 << 15, 1, 1), (2, 2, 1 << 15, 1 << 14), (0x7fffffff,) * 4):
        for dtype in (0, 1, 2):
            assert call(dtype=dtype, shape=shape, stride=2, nbytes=1 << 40) == 0, shape
    for dtype in (0, 1, 2):
        for stride in (1, 2):
            kw = dict(dtype=dtype, stride=stride)
            # the backward's own: dy always, both outputs NULL, what the requested outputs need
            assert call(dy=None, **kw) == 0
            assert call(dx=None, dw=None, **kw) == 0
            assert call(w=None, **kw) == 0 and call(w=None, dw=None, **kw) == 0          # dx needs the weight
            assert call(x=None, **kw) == 0 and call(x=None, dx=None, **kw) == 0          # dweight needs x
            esize = 4 if dtype == 0 else 2
            dy_bytes = 2 * 4 * (64 if stride == 1 else 16) * esize
            dx_bytes = 2 * 4 * 64 * esize
            assert call(dx=ok["dy"], **kw) == 0                                           # dx overlapping dy
            assert call(dx=ok["dy"] + dy_bytes - 2, **kw) == 0
            assert call(dx=ok["dy"] - dx_bytes + 2, **kw) == 0
            assert call(dx=ok["x"], **kw) == 0                                            # ... or x, which dweight reads
            # the workspace, where dweight is wanted
            for extra in (dict(), dict(dx=None)):
                assert call(ws=None, **kw, **extra) == 0 and call(ws=None, nbytes=0, **kw, **extra) == 0
                for off in (1, 16, 128, 255):
                    assert call(ws=ok["ws"] + off, nbytes=need + 256, **kw, **extra) == 0, off
                assert call(ws=ok["ws"], nbytes=ext.depthwise3x3_backward_workspace_bytes(*SHAPE, stride) - 1, **kw, **extra) == 0
                assert call(ws=ok["ws"], nbytes=0, **kw, **extra) == 0


def test_python_surface_raises_what_it_documents(ext):
    from rroi_align import conv
    x, w = torch.zeros(2, 3, 8, 8), torch.zeros(3, 1, 3, 3)
    dy2 = torch.zeros(2, 3, 4, 4)
    for dtype in D.DTYPES:
        with pytest.raises(RuntimeError, match="GPU only"):
            conv.depthwise3x3(x.to(dtype), w.to(dtype))
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.depthwise3x3_backward(dy2.to(dtype), x.to(dtype), w.to(dtype), 2)
    for f in (conv.depthwise3x3, lambda a, b, stride=1: ext.depthwise3x3_backward(a, a, b, stride)):
        with pytest.raises(ValueError):
            f(x, w.to(torch.bfloat16))
        with pytest.raises(ValueError):
            f(x, torch.zeros(4, 1, 3, 3))
        with pytest.raises(ValueError):
            f(x, torch.zeros(3, 3, 3, 3))
        with pytest.raises(ValueError):
            f(x[0], w)
        with pytest.raises(ValueError):
            f(x, w, stride=3)
        with pytest.raises(TypeError):
            f([1.0], w)
    bw = ext.depthwise3x3_backward
    with pytest.raises(ValueError, match="dy must be"):
        bw(x, x, w, 2)                                            # dy's shape is the output's
    with pytest.raises(ValueError, match="dy must be"):
        bw(dy2, x, w, 1)
    with pytest.raises(ValueError, match="one dtype"):
        bw(x.half(), x, w)
    with pytest.raises(TypeError):
        bw(None, x, w)
    xc, wc = fake_cuda(x), fake_cuda(w)
    with pytest.raises(ValueError, match="no gradient"):
        bw(xc, xc, wc, need_dx=False, need_dweight=False)


def test_trainable_depthwise_ok_is_native_ok_without_its_gradient_clause(monkeypatch):
    from fots_e2e import native_train as T
    from fots_e2e.native import native_ok
    x = fake_cuda(torch.zeros(2, 4, 8, 8))
    xg = fake_cuda(torch.zeros(2, 4, 8, 8)).requires_grad_(True)
    m = qualifying()
    assert m.weight.requires_grad and not native_ok(m, x) and T.trainable_depthwise_ok(m, x)
    frozen = qualifying(stride=2)
    frozen.weight.requires_grad_(False)
    assert not native_ok(frozen, xg) and T.trainable_depthwise_ok(frozen, xg)
    assert torch.is_grad_enabled()                                            # asking leaves grad mode as it was
    for dtype in (torch.bfloat16, torch.float16):
        assert T.trainable_depthwise_ok(qualifying().to(dtype), fake_cuda(torch.zeros(2, 4, 8, 8, dtype=dtype)))
    for bad in (torch.zeros(2, 4, 8, 8), fake_cuda(torch.zeros(2, 4, 8, 8).to(memory_format=torch.channels_last)),
                fake_cuda(torch.zeros(2, 4, 8, 16)[:, :, :, ::2]), fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.float64)),
                fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.bfloat16)), fake_cuda(torch.zeros(2, 5, 8, 8)),
                fake_cuda(torch.zeros(0, 4, 8, 8)), fake_cuda(torch.zeros(4, 8, 8))):
        assert not T.trainable_depthwise_ok(m, bad)
    for mod in (qualifying(kernel_size=5, padding=2), qualifying(padding=0), qualifying(stride=3), qualifying(groups=2),
                qualifying(bias=True), qualifying(padding_mode="reflect"), qualifying(out_channels=8)):
        assert not T.trainable_depthwise_ok(mod, x)
    with monkeypatch.context() as mp:
        mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert not T.trainable_depthwise_ok(m, x)
    with monkeypatch.context() as mp:                                         # this module's own hook declines a shape
        seen = []
        mp.setattr(T, "_dw_backward_slower", lambda t, stride: (seen.append(stride), True)[1])
        assert not T.trainable_depthwise_ok(m, x) and not T.trainable_depthwise_ok(frozen, xg) and seen == [1, 2]
    assert T.trainable_depthwise_ok(m, x)
    # the six shapes of the network, one and eight images, every dtype: no class is declined (views of one element: nothing
    # that large is allocated)
    for n in (1, 8):
        for c, h, w, s in D.NETWORK_SHAPES:
            for dtype in D.DTYPES:
                assert not T._dw_backward_slower(fake_cuda(torch.zeros(1, dtype=dtype).expand(n, c, h, w)), s)


def test_use_trainable_depthwise_switches_classes_only_and_back():
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import DepthwiseConv3x3, use_native_depthwise
    from fots_e2e.native_remainder import use_native_upconv
    from fots_e2e.native_train import TrainableDepthwiseConv3x3, use_trainable_depthwise
    net = FOTSNet()
    keys = list(net.state_dict().keys())
    params = [id(p) for p in net.parameters()]
    assert use_trainable_depthwise(net) == 0                                  # off by default; nothing to switch yet
    assert use_native_depthwise(net) == 22
    assert not any(type(m) is TrainableDepthwiseConv3x3 for m in net.modules())
    assert use_trainable_depthwise(net) == 22
    switched = [n for n, m in net.named_modules() if type(m) is TrainableDepthwiseConv3x3]
    assert len(switched) == 22 and not any(type(m) is DepthwiseConv3x3 for m in net.modules())
    assert all(".conv_sep1.0" in n or ".conv2.0" in n or n in ("upconv1.0", "upconv2.0") for n in switched), switched
    assert list(net.state_dict().keys()) == keys and [id(p) for p in net.parameters()] == params
    assert use_trainable_depthwise(net) == 0
    # with the fused resize + depthwise switched on as well the two upconv convolutions are still modules of the network
    use_native_upconv(net)
    assert sum(type(m) is TrainableDepthwiseConv3x3 for m in net.modules()) == 22
    use_native_upconv(net, enable=False)
    assert use_trainable_depthwise(net, enable=False) == 22
    assert sum(type(m) is DepthwiseConv3x3 for m in net.modules()) == 22
    assert use_native_depthwise(net, enable=False) == 22
    assert all(type(m) is nn.Conv2d for m in net.modules() if isinstance(m, nn.Conv2d))
    assert list(net.state_dict().keys()) == keys and [id(p) for p in net.parameters()] == params


def test_a_cpu_call_of_the_switched_module_is_its_parents():
    """On the CPU the predicate fails, so the module is DepthwiseConv3x3, which is nn.Conv2d there."""
    from fots_e2e.native import use_native_depthwise
    from fots_e2e.native_train import TrainableDepthwiseConv3x3, use_trainable_depthwise
    net = nn.Sequential(qualifying(stride=2))
    assert use_native_depthwise(net) == 1 and use_trainable_depthwise(net) == 1 and type(net[0]) is TrainableDepthwiseConv3x3
    x = torch.randn(2, 4, 5, 7, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    y = net(x)
    assert torch.equal(y, F.conv2d(x, net[0].weight, None, 2, 1, 1, 4))
    y.sum().backward()
    assert x.grad is not None and net[0].weight.grad is not None


@pytest.mark.parametrize("stride", (1, 2))
def test_the_oracle_and_the_reference_are_torchs_float64_autograd(stride):
    """The case module's dx formula and dweight sums against autograd of F.conv2d in float64 on the same
    (float32-representable) values: the formula is the gradient, to float64 summation order."""
    shapes = ((1, 1, 1, 1), (1, 2, 4, 8), (1, 2, 5, 9), (1, 3, 6, 7), (2, 3, 7, 1), (3, 5, 9, 16), (1, 2, 9, 17), (2, 4, 22, 40),
              (1, 2, 51, 31))
    worst_dx = worst_dw = 0.0
    for shape in shapes:
        x, w, dy = B.random_case((shape, stride), torch.float32)
        N, C, H, W = shape
        xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
        F.conv2d(xr, wr, None, stride, 1, 1, C).backward(dy.double())
        got = torch.from_numpy(B.oracle_dx(dy.numpy(), w.numpy(), H, W, stride, rounded=False))
        scale = float(xr.grad.abs().max()) or 1.0
        worst_dx = max(worst_dx, float((got - xr.grad).abs().max()) / scale)
        assert float((got - xr.grad).abs().max()) <= 1e-12 * scale, shape
        assert torch.equal(torch.from_numpy(B.oracle_dx(dy.numpy(), w.numpy(), H, W, stride)), got.float())
        ref = B.DweightReference(dy, x, stride)
        ok, ratio = ref.check(wr.grad)
        worst_dw = max(worst_dw, ratio)
        assert ok and ratio <= 1e-3, (shape, ratio)
        assert float((ref.ref - wr.grad).abs().max()) <= 1e-12 * max(1.0, float(wr.grad.abs().max())), shape
    print(f"stride {stride}: dx oracle vs float64 autograd {worst_dx:.3g} of the largest gradient, "
          f"float64 autograd's dweight at {worst_dw:.3g} of the bound")


def test_the_bound_holds_the_reference_rounded_to_the_dtype():
    """The reference's dweight rounded once to the dtype is inside its own bound -- within half of it, and a little, where
    the result is a normal number -- so the bound is not tighter than a correct kernel can meet."""
    for case in (((3, 33, 5, 17), 1), ((2, 7, 22, 40), 2), ((1, 2, 9, 16), 1)):
        for dtype in D.DTYPES:
            _, ref = B.reference(case, dtype)
            ok, worst = ref.check(ref.ref.to(dtype))
            assert ok and worst <= 0.5 + 1e-9, (case, dtype, worst)
