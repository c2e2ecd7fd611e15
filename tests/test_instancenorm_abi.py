"""CPU: the InstanceNorm2d entry points are exported, declared and host-checked; the plan query reaches both forms and every
threshold with the case table; the Python surface refuses CPU tensors and mismatched arguments; `instancenorm_ok` /
`use_native_instancenorm` do what fots_e2e.native says; the tests' reference is pinned against torch.  No kernel is
launched here."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import instancenorm_cases as I
from test_abi import declared_functions
from test_depthwise_abi import fake_cuda

NAMES = ("rroi_instancenorm_forward_hip", "rroi_instancenorm_workspace_bytes", "rroi_instancenorm_plan")
SPLIT_SHAPE = (1, 2, 128, 256)      # needs a workspace
PLANE_SHAPE = (1, 4, 8, 8)          # needs none


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def test_symbols_are_exported_and_declared(ext):
    lib = ctypes.CDLL(ext.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions()
        assert name in ext.EXPORTS
        assert hasattr(lib, name)
    assert callable(ext.instance_norm) and callable(ext.instance_norm_plan) and callable(ext.instance_norm_workspace_bytes)


def test_refusals_return_zero_before_any_launch(ext):
    f = ext._lib.rroi_instancenorm_forward_hip
    P = 0x7f0000000000   # non-null, a multiple of 256, never dereferenced: every call below is refused on the host
    ok = dict(dtype=0, x=P, gamma=P, beta=P, y=P, shape=PLANE_SHAPE, eps=1e-5, slope=0.01, ws=None, nbytes=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["dtype"], a["x"], a["gamma"], a["beta"], a["y"], *a["shape"], a["eps"], a["slope"], a["ws"], a["nbytes"], None)

    for dtype in (3, -1, 100):
        assert call(dtype=dtype) == 0
    for shape in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (-1, 4, 8, 8), (1, 4, 8, -3)):
        assert call(shape=shape) == 0, shape
        assert ext.instance_norm_workspace_bytes(*shape) == 0
    for shape in ((1, 1 << 11, 1 << 10, 1 << 10), (1 << 16, 1 << 15, 1, 1), (2, 2, 1 << 15, 1 << 14),
                  (0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff)):
        for dtype in (0, 1, 2):
            assert call(dtype=dtype, shape=shape, ws=P, nbytes=1 << 40) == 0, shape      # N * C * H * W >= 2^31
    for dtype in (0, 1, 2):
        assert call(dtype=dtype, x=None) == 0
        assert call(dtype=dtype, y=None) == 0
        assert call(dtype=dtype, gamma=None) == 0                                         # exactly one of gamma / beta
        assert call(dtype=dtype, beta=None) == 0
    for eps in (0.0, -1e-5, float("nan"), float("inf"), -float("inf")):
        assert call(eps=eps) == 0, eps
        assert call(eps=eps, gamma=None, beta=None) == 0, eps
    for slope in (float("nan"), float("inf"), -float("inf")):
        assert call(slope=slope) == 0, slope
    # a plan that needs the workspace
    need = ext.instance_norm_workspace_bytes(*SPLIT_SHAPE)
    assert need > 0 and need % 256 == 0 and ext.instance_norm_workspace_bytes(*PLANE_SHAPE) == 0
    for dtype in (0, 1, 2):
        assert call(dtype=dtype, shape=SPLIT_SHAPE, ws=None, nbytes=need) == 0
        assert call(dtype=dtype, shape=SPLIT_SHAPE, ws=None, nbytes=0) == 0
        for off in (1, 4, 16, 128, 255):
            assert call(dtype=dtype, shape=SPLIT_SHAPE, ws=P + off, nbytes=need + 256) == 0, off
        assert call(dtype=dtype, shape=SPLIT_SHAPE, ws=P, nbytes=need - 1) == 0
        assert call(dtype=dtype, shape=SPLIT_SHAPE, ws=P, nbytes=0) == 0
    # the plan query refuses what the call refuses, and a NULL result
    plan = ext._lib.rroi_instancenorm_plan
    assert plan(0, *PLANE_SHAPE, None) == 0
    with pytest.raises(ValueError):
        ext.instance_norm_plan(1, 0, 8, 8)
    with pytest.raises(ValueError):
        ext.instance_norm_plan(1, 1 << 11, 1 << 10, 1 << 10)
    with pytest.raises(ValueError):
        ext.instance_norm_plan(1, 4, 8, 8, dtype=7)


def test_python_surface_refuses_cpu_tensors_and_mismatches(ext):
    x, w, b = torch.zeros(2, 3, 8, 8), torch.ones(3), torch.zeros(3)
    for dtype in I.DTYPES:
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.instance_norm(x.to(dtype))
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.instance_norm(x.to(dtype), w.to(dtype), b.to(dtype), negative_slope=0.01)
    with pytest.raises(ValueError):
        ext.instance_norm(x[0])                                   # not 4-D
    with pytest.raises(ValueError):
        ext.instance_norm(x.view(2, 3, 8, 8, 1))
    with pytest.raises(ValueError):
        ext.instance_norm(x, w.to(torch.bfloat16), b.to(torch.bfloat16))   # dtypes differ
    with pytest.raises(ValueError):
        ext.instance_norm(x, w, b.half())
    with pytest.raises(ValueError):
        ext.instance_norm(x.half(), w, b)
    with pytest.raises(ValueError):
        ext.instance_norm(x, torch.ones(4), torch.zeros(4))       # not (C,)
    with pytest.raises(ValueError):
        ext.instance_norm(x, torch.ones(3, 1), torch.zeros(3, 1))
    with pytest.raises(ValueError):
        ext.instance_norm(x, w, torch.zeros(2))
    with pytest.raises(ValueError):
        ext.instance_norm(x, w, None)                             # one of the two missing
    with pytest.raises(ValueError):
        ext.instance_norm(x, None, b)


def norm(c=4, **kw):
    return nn.InstanceNorm2d(c, **kw)


def test_instancenorm_ok_declines_each_disqualifying_property(monkeypatch):
    from fots_e2e.native import instancenorm_ok
    x = fake_cuda(torch.zeros(2, 4, 8, 8))
    with torch.no_grad():
        assert instancenorm_ok(norm(), x)
        assert instancenorm_ok(norm(affine=True), x)
        for dtype in (torch.bfloat16, torch.float16):
            xt = fake_cuda(torch.zeros(2, 4, 8, 8, dtype=dtype))
            assert instancenorm_ok(norm(), xt) and instancenorm_ok(norm(affine=True).to(dtype), xt)
        assert not instancenorm_ok(norm(), torch.zeros(2, 4, 8, 8))                              # a CPU tensor
        assert not instancenorm_ok(norm(), fake_cuda(torch.zeros(4, 8, 8)))                      # not 4-D
        assert not instancenorm_ok(norm(), fake_cuda(torch.zeros(2, 4, 8, 8).to(memory_format=torch.channels_last)))
        assert not instancenorm_ok(norm(), fake_cuda(torch.zeros(2, 4, 8, 16)[:, :, :, ::2]))    # strided view
        assert not instancenorm_ok(norm(), fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.float64)))
        assert not instancenorm_ok(norm(affine=True), fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.bfloat16)))  # not the weight's
        assert not instancenorm_ok(norm(affine=True).double(), fake_cuda(torch.zeros(2, 4, 8, 8, dtype=torch.float64)))
        assert not instancenorm_ok(norm(), fake_cuda(torch.zeros(2, 5, 8, 8)))                   # not num_features
        assert not instancenorm_ok(norm(track_running_stats=True), x)                           # running statistics
        assert not instancenorm_ok(norm(track_running_stats=True).eval(), x)
        assert not instancenorm_ok(norm(), fake_cuda(torch.zeros(0, 4, 8, 8)))                   # nothing to do
        assert not instancenorm_ok(norm(), fake_cuda(torch.zeros(2, 4, 1, 1)))                   # the stock module raises: left to it
        # the one class measured slower than stock: float32, more than 16,384 planes of at most 128 elements
        assert not instancenorm_ok(norm(256), fake_cuda(torch.zeros(192, 256, 1, 64)))
        assert not instancenorm_ok(norm(256), fake_cuda(torch.zeros(65, 256, 2, 64)))
        assert instancenorm_ok(norm(256), fake_cuda(torch.zeros(64, 256, 2, 64)))                # 16,384 planes
        assert instancenorm_ok(norm(256), fake_cuda(torch.zeros(65, 256, 3, 43)))                # 129 elements
        assert instancenorm_ok(norm(256), fake_cuda(torch.zeros(192, 256, 1, 64, dtype=torch.bfloat16)))
        # 2^31 elements (a view of one element: nothing that large is allocated)
        assert not instancenorm_ok(norm(1 << 11), fake_cuda(torch.zeros(1).expand(1, 1 << 11, 1 << 10, 1 << 10)))
    # a gradient is needed: of the parameters (a fresh affine module's default), of the input
    m = norm(affine=True)
    assert m.weight.requires_grad and not instancenorm_ok(m, x)
    with torch.no_grad():
        assert instancenorm_ok(m, x)
    m.weight.requires_grad_(False)
    assert not instancenorm_ok(m, x)                            # the bias still needs one
    m.bias.requires_grad_(False)
    assert instancenorm_ok(m, x)
    with monkeypatch.context() as mp:                           # autocast: left to the stock module
        mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert not instancenorm_ok(m, x)
    assert instancenorm_ok(m, x)
    xg = fake_cuda(torch.zeros(2, 4, 8, 8)).requires_grad_(True)
    assert not instancenorm_ok(m, xg) and not instancenorm_ok(norm(), xg)
    with torch.no_grad():
        assert instancenorm_ok(m, xg)


def outputs_equal(a, b):
    return all(torch.equal(s, t) for u, v in zip(a, b) for s, t in zip(u, v))


def test_use_native_instancenorm_switches_the_network_and_back():
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import (AbsorbedLeakyReLU, AbsorbedReLU, NativeInstanceNorm2d, use_native_depthwise,
                                 use_native_instancenorm)
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

    for fuse, pairs in ((True, 20), (False, 0)):
        assert use_native_instancenorm(net, fuse_activation=fuse) == (52, pairs)
        assert use_native_instancenorm(net, fuse_activation=fuse) == (0, 0)             # nothing left to switch
        assert unchanged()
        norms = [n for n, m in net.named_modules() if type(m) is NativeInstanceNorm2d]
        assert len(norms) == 52 and not any(type(m) is nn.InstanceNorm2d for m in net.modules())
        fused = [n for n, m in net.named_modules() if type(m) is NativeInstanceNorm2d and m.fused_slope is not None]
        absorbed = [n for n, m in net.named_modules() if type(m) in (AbsorbedLeakyReLU, AbsorbedReLU)]
        assert len(fused) == len(absorbed) == pairs
        assert all(n.endswith(".conv_sep1.2") or n.endswith(".conv2.1") for n in fused), fused
        assert all(n.endswith(".conv_sep1.3") or n.endswith(".conv2.2") for n in absorbed), absorbed
        assert all(net.get_submodule(n).fused_slope == 0.01 for n in fused)
        with torch.no_grad():                       # on CPU input the switched network takes the stock path: the same bits
            assert outputs_equal(stock, net(x))
            assert torch.equal(stock_ocr, net.forward_ocr(crops))
        assert use_native_instancenorm(net, enable=False) == (52, pairs)
        assert {n: type(m) for n, m in net.named_modules()} == classes
        assert not any("fused_slope" in m.__dict__ for m in net.modules())
        assert unchanged()
    # a later call may still fuse what an earlier one left separate
    assert use_native_instancenorm(net, fuse_activation=False) == (52, 0)
    assert use_native_instancenorm(net) == (0, 20)
    assert use_native_depthwise(net) == 22                      # the other switch is untouched by this one
    with torch.no_grad():
        assert outputs_equal(stock, net(x))
    assert use_native_depthwise(net, enable=False) == 22
    assert use_native_instancenorm(net, enable=False) == (52, 20)
    assert {n: type(m) for n, m in net.named_modules()} == classes


def test_fusing_takes_a_relu_and_leaves_shared_modules_alone():
    from fots_e2e.native import AbsorbedReLU, use_native_instancenorm
    a = nn.Sequential(nn.Conv2d(3, 4, 1), nn.InstanceNorm2d(4, affine=True), nn.ReLU(), nn.InstanceNorm2d(4), nn.Tanh()).eval()
    x = torch.randn(2, 3, 5, 7, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = a(x)
    assert use_native_instancenorm(a) == (2, 1)
    assert type(a[2]) is AbsorbedReLU and a[1].fused_slope == 0.0 and a[3].fused_slope is None
    with torch.no_grad():
        assert torch.equal(a(x), want)
    assert use_native_instancenorm(a, enable=False) == (2, 1) and type(a[2]) is nn.ReLU
    act = nn.LeakyReLU(0.2)                                     # one activation module behind two norms: not fused
    shared = nn.ModuleList([nn.Sequential(nn.InstanceNorm2d(3), act), nn.Sequential(nn.InstanceNorm2d(3), act)])
    assert use_native_instancenorm(shared) == (2, 0) and type(act) is nn.LeakyReLU


def test_case_table_reaches_both_forms_and_every_threshold(ext):
    """Asked through the plan query (256 CUs, with or without a GPU of that size)."""
    plans = {}
    for shape in I.CASES:
        for dtype in I.DTYPES:
            p = ext.instance_norm_plan(*shape, dtype=dtype)
            form, nseg, seg = I.plan_of(*shape)
            assert (p.form, p.segments, p.segment_elems) == (form, nseg, seg), (shape, p)      # the mirror is the rule
            assert p.launches == (2 if form == I.SPLIT else 1) and p.block == 256
            assert p.grid_x == shape[0] * shape[1] * nseg
            assert p.vector_elems == (4 if dtype == torch.float32 else 8)
            assert (ext.instance_norm_workspace_bytes(*shape) > 0) == (form == I.SPLIT)
            plans[shape, dtype] = p
    for dtype in I.DTYPES:
        forms = {p.form for (s, d), p in plans.items() if d == dtype}
        assert forms == {I.PLANE, I.SPLIT}, dtype                                        # both forms in every dtype
    sizes = {s[2] * s[3]: s for s in I.CASES}
    assert 1 in sizes and {1023, 1024, 1025} <= set(sizes)
    assert any((s[2] * s[3]) % 2 == 1 and s[0] * s[1] > 1 for s in I.CASES)              # odd planes, more than one
    t = I.SPLIT_MIN_PLANE                                                                # the rule's one plane-size threshold
    assert {t - 1, t, t + 1} <= set(sizes)
    assert I.plan_of(*sizes[t - 1])[0] == I.PLANE and I.plan_of(*sizes[t])[0] == I.SPLIT and I.plan_of(*sizes[t + 1])[0] == I.SPLIT
    assert any(I.plan_of(*s)[0] == I.SPLIT and (s[2] * s[3]) % I.plan_of(*s)[2] == 1 for s in I.CASES)   # a last segment of 1
    assert any(I.plan_of(*s)[0] == I.SPLIT and s[0] > 1 and s[1] > 1 for s in I.CASES)
    # the rule's other threshold, the plane count against the CU count, needs no launch to be asked
    for planes, form in ((I.CUS - 1, I.SPLIT), (I.CUS, I.PLANE), (I.CUS + 1, I.PLANE)):
        assert ext.instance_norm_plan(1, planes, 128, 256).form == form, planes
    # the network's shapes at 704 x 1280, one image: the stem and layer1 are split, everything below is not
    for C, H, W, form in ((32, 704, 1280, I.SPLIT), (64, 352, 640, I.SPLIT), (64, 176, 320, I.SPLIT), (128, 88, 160, I.PLANE),
                          (256, 44, 80, I.PLANE), (512, 22, 40, I.PLANE)):
        p = ext.instance_norm_plan(1, C, H, W)
        assert p.form == form and p.segments <= I.MAX_SEGS and p.segments * p.segment_elems >= H * W, (C, H, W, p)
        assert (p.segments - 1) * p.segment_elems < H * W                                 # no empty segment


def test_reference_is_pinned_against_torch():
    """The longdouble reference against F.instance_norm in float64 on the table's own inputs (|mean| / std up to 10^4):
    |ref64 - torch| <= 2^-40 (|x a| + |b|) -- torch's float64 statistics carry a relative error of a few 2^-53 in the mean,
    which the ratio 10^4 amplifies to 2^-40 at most; measured 3.6e-15.  (How many fp32 roundings of the two differ is printed, not asserted:
    at ratio 10^4 a difference of 10^-13 of the scale is 10^-9 absolute, a few percent of an fp32 ulp of the result.)"""
    total = differ = 0
    worst = 0.0
    for shape in I.CASES[1:7]:                  # (torch refuses planes of one element)
        x, gamma, beta, stats = I.problem(shape, torch.float32)
        for affine in (True, False):
            g, bt = (gamma, beta) if affine else (None, None)
            out, ref64, a, b = I.reference(x, g, bt, I.EPS, 1.0, stats)
            want = F.instance_norm(x.double(), weight=None if g is None else g.double(), bias=None if bt is None else bt.double(),
                                   use_input_stats=True, eps=I.EPS)
            scale = (x.double() * a).abs() + b.abs()
            worst = max(worst, float(((ref64 - want).abs() / scale).max()))
            d, nan_ok = I.differing(out, want.float())
            assert nan_ok
            total += out.numel()
            differ += d
    print(f"reference vs torch float64: worst relative difference {worst:.3g}, {differ} of {total} fp32 results differ")
    assert worst <= 2.0 ** -40, worst
    assert total > 100000
    # the activation of the reference is torch's
    x, gamma, beta, stats = I.problem(I.CASES[1], torch.float32)
    for slope in I.SLOPES:
        out = I.reference(x, gamma, beta, I.EPS, slope, stats)[0]
        assert torch.equal(out, F.leaky_relu(I.reference(x, gamma, beta, I.EPS, 1.0, stats)[0], slope))
    # a plane with a NaN or an inf is NaN throughout and alone
    x = x.clone()
    x[0, 1, 2, 3], x[1, 0, 0, 0] = float("nan"), float("inf")
    out = I.reference(x, gamma, beta)[0]
    assert out[0, 1].isnan().all() and out[1, 0].isnan().all() and int(out.isnan().sum()) == 2 * 63
