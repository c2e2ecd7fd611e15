"""CPU: the InstanceNorm2d training entry points (header section 6c) are exported, declared and host-checked;
the backward's plan and workspace queries are consistent with each other and with the forward's plan; the Python surface
raises what it documents; `TrainableInstanceNorm2d` / `use_trainable_instancenorm` do what fots_e2e.native_train says; the
tests' reference is pinned against torch's float64 autograd.  No kernel is launched here."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import instancenorm_backward_cases as B
import instancenorm_cases as I
from test_abi import declared_functions
from test_depthwise_abi import fake_cuda

NAMES = ("rroi_instancenorm_forward_train_hip", "rroi_instancenorm_backward_hip",
         "rroi_instancenorm_backward_workspace_bytes", "rroi_instancenorm_backward_plan")
SPLIT_SHAPE = (1, 2, 128, 256)
PLANE_SHAPE = (1, 4, 8, 8)
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
    for name in ("instance_norm_train", "instance_norm_backward", "instance_norm_backward_plan",
                 "instance_norm_backward_workspace_bytes", "run_instance_norm_train", "run_instance_norm_backward"):
        assert callable(getattr(ext, name))
    assert ext.version() == "rroi_align_hip 0.10.0 gfx950"


def test_training_forward_refuses_what_section_6_refuses_and_a_null_stats(ext):
    f = ext._lib.rroi_instancenorm_forward_train_hip
    ok = dict(dtype=0, x=P, gamma=P, beta=P, y=P + FAR, stats=P + 2 * FAR, shape=PLANE_SHAPE, eps=1e-5, slope=0.01, ws=None, nbytes=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["dtype"], a["x"], a["gamma"], a["beta"], a["y"], a["stats"], *a["shape"], a["eps"], a["slope"], a["ws"],
                 a["nbytes"], None)

    assert call(dtype=3) == 0 and call(dtype=-1) == 0
    for shape in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (1, 1 << 11, 1 << 10, 1 << 10)):
        assert call(shape=shape, ws=P, nbytes=1 << 40) == 0, shape
    for dtype in (0, 1, 2):
        for null in ("x", "y", "stats", "gamma", "beta"):
            assert call(dtype=dtype, **{null: None}) == 0, null
    for eps in (0.0, -1e-5, float("nan"), float("inf")):
        assert call(eps=eps) == 0
    assert call(slope=float("nan")) == 0 and call(slope=float("inf")) == 0
    need = ext.instance_norm_workspace_bytes(*SPLIT_SHAPE)                  # the forward's workspace, the forward's plan
    assert need > 0
    assert call(shape=SPLIT_SHAPE, ws=None, nbytes=need) == 0
    assert call(shape=SPLIT_SHAPE, ws=P + 16, nbytes=need + 256) == 0
    assert call(shape=SPLIT_SHAPE, ws=P, nbytes=need - 1) == 0


def test_backward_refusals_return_zero_before_any_launch(ext):
    f = ext._lib.rroi_instancenorm_backward_hip
    need_plane = ext.instance_norm_backward_workspace_bytes(*PLANE_SHAPE)
    ok = dict(dtype=0, dy=P, x=P + FAR, stats=P + 2 * FAR, gamma=P + 3 * FAR, beta=P + 4 * FAR, dx=P + 5 * FAR, dgamma=P + 6 * FAR,
              dbeta=P + 7 * FAR, shape=PLANE_SHAPE, eps=1e-5, slope=0.01, ws=P + 8 * FAR, nbytes=need_plane)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["dtype"], a["dy"], a["x"], a["stats"], a["gamma"], a["beta"], a["dx"], a["dgamma"], a["dbeta"], *a["shape"],
                 a["eps"], a["slope"], a["ws"], a["nbytes"], None)

    # everything section 6 refuses
    for dtype in (3, -1, 100):
        assert call(dtype=dtype) == 0
    for shape in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (-1, 4, 8, 8), (1, 4, 8, -3)):
        assert call(shape=shape, nbytes=1 << 40) == 0, shape
        assert ext.instance_norm_backward_workspace_bytes(*shape) == 0
    for shape in ((1, 1 << 11, 1 << 10, 1 << 10), (1 << 16, 1 << 15, 1, 1), (0x7fffffff,) * 4):
        for dtype in (0, 1, 2):
            assert call(dtype=dtype, shape=shape, nbytes=1 << 40) == 0, shape
    for eps in (0.0, -1e-5, float("nan"), float("inf"), -float("inf")):
        assert call(eps=eps) == 0, eps
    for slope in (float("nan"), float("inf"), -float("inf")):
        assert call(slope=slope) == 0, slope
    for dtype in (0, 1, 2):
        assert call(dtype=dtype, gamma=None, dgamma=None, dbeta=None) == 0      # exactly one of gamma / beta
        assert call(dtype=dtype, beta=None, dgamma=None, dbeta=None) == 0
        # the backward's own
        for null in ("dy", "x", "stats"):
            assert call(dtype=dtype, **{null: None}) == 0, null
        assert call(dtype=dtype, dgamma=None) == 0 and call(dtype=dtype, dbeta=None) == 0   # they come together
        assert call(dtype=dtype, gamma=None, beta=None) == 0                    # dgamma without gamma
        assert call(dtype=dtype, dx=None, dgamma=None, dbeta=None) == 0         # dx may be NULL only where dgamma is not
        size = 4 * 64 * (4 if dtype == 0 else 2)
        for src in ("x", "dy"):                                                # dx overlapping x or dy
            assert call(dtype=dtype, dx=ok[src]) == 0
            assert call(dtype=dtype, dx=ok[src] + size - 2) == 0
            assert call(dtype=dtype, dx=ok[src] - size + 2) == 0
    # the workspace, where the plan needs one: parameter gradients in either form, the split form always
    need_split = ext.instance_norm_backward_workspace_bytes(*SPLIT_SHAPE)
    assert need_plane > 0 and need_plane % 256 == 0 and need_split > need_plane and need_split % 256 == 0
    for dtype in (0, 1, 2):
        for shape, need, params in ((PLANE_SHAPE, need_plane, True), (SPLIT_SHAPE, need_split, True), (SPLIT_SHAPE, need_split, False)):
            kw = dict(dtype=dtype, shape=shape) if params else dict(dtype=dtype, shape=shape, dgamma=None, dbeta=None)
            assert call(ws=None, nbytes=need, **kw) == 0
            assert call(ws=None, nbytes=0, **kw) == 0
            for off in (1, 16, 128, 255):
                assert call(ws=ok["ws"] + off, nbytes=need + 256, **kw) == 0, off
            assert call(ws=ok["ws"], nbytes=need - 1, **kw) == 0
            assert call(ws=ok["ws"], nbytes=0, **kw) == 0


def test_plan_and_workspace_queries_agree_with_each_other_and_with_the_forward(ext):
    """The backward starts from the forward's rule: wherever the two plans name one form, segments and grid are equal too.
    The workspace is one pair of doubles per plane, and in the split form one more per workgroup, each region rounded up
    to 256 bytes."""
    up = lambda v: -(-v // 256) * 256
    forms = set()
    for shape in I.CASES + (PLANE_SHAPE, SPLIT_SHAPE, (8, 64, 24, 40), (24, 256, 1, 64), (1, 255, 256, 256), (1, 256, 256, 256)):
        N, C, H, W = shape
        for dtype in I.DTYPES:
            bp, fp = ext.instance_norm_backward_plan(*shape, dtype=dtype), ext.instance_norm_plan(*shape, dtype=dtype)
            forms.add(bp.form)
            assert bp.block == 256 and bp.vector_elems == (4 if dtype == torch.float32 else 8)
            assert bp.grid_x == (N * C * bp.segments if bp.form == ext.INORM_SPLIT else min(N * C, 1 << 20))
            if bp.form == ext.INORM_PLANE:
                assert bp.segments == 1 and bp.segment_elems == H * W and bp.launches == 2
            else:
                assert bp.launches == 3 and 1 < bp.segments <= 256 and bp.segment_elems % 2048 == 0
                assert (bp.segments - 1) * bp.segment_elems < H * W <= bp.segments * bp.segment_elems
            if bp.form == fp.form:
                assert bp[2:] == fp[2:]                       # all but form and launches
            need = ext.instance_norm_backward_workspace_bytes(*shape)
            assert need == up(16 * N * C) + (up(16 * bp.grid_x) if bp.form == ext.INORM_SPLIT else 0)
    assert forms == {ext.INORM_PLANE, ext.INORM_SPLIT}
    assert ext._lib.rroi_instancenorm_backward_plan(0, *PLANE_SHAPE, None) == 0
    with pytest.raises(ValueError):
        ext.instance_norm_backward_plan(1, 0, 8, 8)
    with pytest.raises(ValueError):
        ext.instance_norm_backward_plan(1, 1 << 11, 1 << 10, 1 << 10)
    with pytest.raises(ValueError):
        ext.instance_norm_backward_plan(1, 4, 8, 8, dtype=7)


def test_python_surface_raises_what_it_documents(ext):
    from rroi_align import norm
    x, w, b = torch.zeros(2, 3, 8, 8), torch.ones(3), torch.zeros(3)
    stats = torch.zeros(2, 3, 2, dtype=torch.float64)
    for f in (ext.instance_norm_train, norm.instance_norm):
        for dtype in I.DTYPES:
            with pytest.raises(RuntimeError, match="GPU only"):
                f(x.to(dtype), w.to(dtype), b.to(dtype), negative_slope=0.01)
        with pytest.raises(ValueError):
            f(x[0])
        with pytest.raises(ValueError):
            f(x, w.half(), b.half())
        with pytest.raises(ValueError):
            f(x, torch.ones(4), torch.zeros(4))
        with pytest.raises(ValueError):
            f(x, w, None)
        with pytest.raises(TypeError):
            f([1.0])
    bw = ext.instance_norm_backward
    with pytest.raises(RuntimeError, match="GPU only"):
        bw(x, x, stats, w, b)
    with pytest.raises(ValueError):
        bw(x[:, :, :4], x, stats, w, b)                          # dy's shape
    with pytest.raises(ValueError):
        bw(x.half(), x, stats, w, b)                             # dy's dtype
    with pytest.raises(ValueError):
        bw(x, x, stats, w, None)
    with pytest.raises(ValueError):
        bw(x, x, stats, torch.ones(4), torch.zeros(4))
    with pytest.raises(TypeError):
        bw(None, x, stats)
    xc = fake_cuda(x)
    with pytest.raises(ValueError, match="stats"):
        bw(xc, xc, fake_cuda(stats.float()))                     # stats is float64 ...
    with pytest.raises(ValueError, match="stats"):
        bw(xc, xc, fake_cuda(stats[:1]))                         # ... and (N, C, 2)
    with pytest.raises(ValueError, match="no gradient"):
        bw(xc, xc, fake_cuda(stats), need_dx=False, need_param_grads=False)
    with pytest.raises(ValueError, match="no gradient"):
        bw(xc, xc, fake_cuda(stats), need_dx=False)              # parameter gradients of a norm without parameters


def norm2d(c=4, **kw):
    return nn.InstanceNorm2d(c, **kw)


def test_trainable_norm_ok_is_instancenorm_ok_without_its_gradient_clause(monkeypatch):
    from fots_e2e import native_train as T
    from fots_e2e.native import instancenorm_ok
    x = fake_cuda(torch.zeros(2, 4, 8, 8))
    xg = fake_cuda(torch.zeros(2, 4, 8, 8)).requires_grad_(True)
    m = norm2d(affine=True)
    assert not instancenorm_ok(m, x) and T.trainable_norm_ok(m, x)            # the parameters need a gradient
    assert not instancenorm_ok(norm2d(), xg) and T.trainable_norm_ok(norm2d(), xg)
    assert torch.is_grad_enabled()                                            # asking leaves grad mode as it was
    for bad in (torch.zeros(2, 4, 8, 8), fake_cuda(torch.zeros(2, 4, 8, 8).to(memory_format=torch.channels_last)),
                fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.float64)), fake_cuda(torch.zeros(2, 5, 8, 8)),
                fake_cuda(torch.zeros(2, 4, 1, 1)), fake_cuda(torch.zeros(0, 4, 8, 8))):
        assert not T.trainable_norm_ok(norm2d(), bad)
    assert not T.trainable_norm_ok(norm2d(track_running_stats=True), x)
    assert not T.trainable_norm_ok(norm2d(256), fake_cuda(torch.zeros(192, 256, 1, 64)))     # the forward's slower class
    with monkeypatch.context() as mp:
        mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert not T.trainable_norm_ok(m, x)
    with monkeypatch.context() as mp:                                         # this module's own hook declines a shape
        mp.setattr(T, "_inorm_backward_slower", lambda t, slope: True)
        assert not T.trainable_norm_ok(m, x)
    # the class that measured no faster: 16 bits, no activation, few planes of 32,768 to 131,071 elements
    for dtype in (torch.bfloat16, torch.float16):
        big = fake_cuda(torch.zeros(1, 64, 176, 320, dtype=dtype))
        plain, act = norm2d(64), norm2d(64)
        act.fused_slope = 0.01
        assert not T.trainable_norm_ok(plain, big) and T.trainable_norm_ok(act, big)
        assert T.trainable_norm_ok(plain, fake_cuda(torch.zeros(1, 64, 128, 255, dtype=dtype)))      # 32,640 elements
        assert T.trainable_norm_ok(norm2d(129), fake_cuda(torch.zeros(1, 129, 176, 320, dtype=dtype)))  # 129 planes
    assert T.trainable_norm_ok(norm2d(64), fake_cuda(torch.zeros(1, 64, 176, 320)))                  # float32
    assert T._needs_grad(m, x) and T._needs_grad(norm2d(), xg) and not T._needs_grad(norm2d(), x)
    with torch.no_grad():
        assert not T._needs_grad(m, xg)


def test_use_trainable_instancenorm_switches_classes_only_and_back():
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import NativeInstanceNorm2d, use_native_instancenorm
    from fots_e2e.native_train import TrainableInstanceNorm2d, use_trainable_instancenorm
    net = FOTSNet()
    keys = list(net.state_dict().keys())
    params = [id(p) for p in net.parameters()]
    assert use_trainable_instancenorm(net) == 0                               # off by default; nothing to switch yet
    assert use_native_instancenorm(net) == (52, 20)
    assert not any(type(m) is TrainableInstanceNorm2d for m in net.modules())
    slopes = {n: m.fused_slope for n, m in net.named_modules() if type(m) is NativeInstanceNorm2d}
    assert use_trainable_instancenorm(net) == 52
    assert not any(type(m) is NativeInstanceNorm2d for m in net.modules())
    assert {n: m.fused_slope for n, m in net.named_modules() if type(m) is TrainableInstanceNorm2d} == slopes
    assert list(net.state_dict().keys()) == keys and [id(p) for p in net.parameters()] == params
    assert use_trainable_instancenorm(net) == 0
    assert use_trainable_instancenorm(net, enable=False) == 52
    assert {n: m.fused_slope for n, m in net.named_modules() if type(m) is NativeInstanceNorm2d} == slopes
    assert use_native_instancenorm(net, enable=False) == (52, 20)
    assert not any(isinstance(m, NativeInstanceNorm2d) for m in net.modules())
    assert list(net.state_dict().keys()) == keys and [id(p) for p in net.parameters()] == params


def test_a_cpu_call_of_the_switched_module_is_its_parents(monkeypatch):
    """On the CPU the predicate fails, so the module is NativeInstanceNorm2d, which is nn.InstanceNorm2d plus the slope."""
    from fots_e2e.native import use_native_instancenorm
    from fots_e2e.native_train import TrainableInstanceNorm2d, use_trainable_instancenorm
    net = nn.Sequential(nn.InstanceNorm2d(4, affine=True), nn.LeakyReLU(0.01))
    use_native_instancenorm(net)
    assert use_trainable_instancenorm(net) == 1 and type(net[0]) is TrainableInstanceNorm2d
    x = torch.randn(2, 4, 5, 7, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    y = net(x)
    want = F.leaky_relu(F.instance_norm(x, weight=net[0].weight, bias=net[0].bias, use_input_stats=True, eps=net[0].eps), 0.01)
    assert torch.equal(y, want)
    y.sum().backward()
    assert x.grad is not None and net[0].weight.grad is not None


@pytest.mark.parametrize("slope", I.SLOPES)
@pytest.mark.parametrize("affine", (True, False), ids=["affine", "plain"])
def test_the_reference_is_torchs_float64_autograd(affine, slope):
    """The case module's longdouble formulas against autograd of F.leaky_relu(F.instance_norm(...)) in float64 on the same
    (float32-representable) values, to 1e-12 of the largest gradient, on planes away from ties -- where the two could
    pick different masks."""
    s32 = float(torch.tensor(slope, dtype=torch.float32))
    for shape in ((2, 3, 7, 9), (3, 5, 24, 40)):
        g = torch.Generator().manual_seed(sum(shape))
        x = (torch.randn(shape, generator=g, dtype=torch.float64) * 2 + 0.5).float()
        dy = torch.randn(shape, generator=g, dtype=torch.float64).float()
        C = shape[1]
        gamma = (torch.randn(C, generator=g, dtype=torch.float64) * 0.5 + 1.0).float() if affine else None
        beta = torch.randn(C, generator=g, dtype=torch.float64).float() if affine else None
        ref = B.Reference(x, dy, gamma, beta, I.EPS, slope)
        assert not bool(ref.left_out.any()) and float(ref.v.abs().min()) > 1e-9
        xr = x.double().requires_grad_(True)
        gr, br = (gamma.double().requires_grad_(True), beta.double().requires_grad_(True)) if affine else (None, None)
        y = F.instance_norm(xr, weight=gr, bias=br, use_input_stats=True, eps=I.EPS)
        if slope != 1.0:
            y = F.leaky_relu(y, s32)
        y.backward(dy.double())
        assert float((ref.dx - xr.grad).abs().max()) <= 1e-12 * float(xr.grad.abs().max())
        if affine:
            assert float((ref.dgamma - gr.grad).abs().max()) <= 1e-12 * float(gr.grad.abs().max())
            assert float((ref.dbeta - br.grad).abs().max()) <= 1e-12 * float(br.grad.abs().max())


def test_the_bounds_hold_the_reference_rounded_to_the_dtype():
    """The reference's dx rounded once to the dtype is inside its own bound -- within half of it for float32 and bfloat16,
    whose results here are normal numbers (one rounding is u |dx|, the bound at least 2 u |dx|); float16 reaches its
    subnormals, where one rounding is up to 2^-25, the bound's last term -- and no plane of the table is left out: the
    bound is not tighter than a correct kernel can meet, and the cap is not eaten by the table itself."""
    for shape in I.CASES[:6]:
        for dtype in I.DTYPES:
            for slope in I.SLOPES:
                for affine in (True, False):
                    ref = B.reference(shape, dtype, affine, slope)
                    assert int(ref.left_out.sum()) == 0 and ref.cap_ok()
                    ok, worst = ref.check_dx(ref.dx.to(dtype))
                    assert ok and worst <= (1.0 if dtype == torch.float16 else 0.5 + 1e-9), (shape, dtype, slope, worst)
