"""GPU (MI355X): the native InstanceNorm2d with its activation against the longdouble reference of
instancenorm_cases.py: the bound and the bit count of the contract over the whole table, special values, misaligned
views with guards around output and workspace, determinism, graph capture, the module switch, and the 49 norms of the
network on the inputs they really see."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import instancenorm_cases as I
from test_gpu_bucketed import NAN_PATTERN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def raw_call(ext, x, gamma, beta, y, shape, slope, ws=None, nbytes=0, eps=I.EPS):
    """The C ABI on tensors (or views) as they are: nothing is made contiguous or aligned on the way."""
    st = ext._lib.rroi_instancenorm_forward_hip(
        ext.dtype_code(x.dtype), x.data_ptr(), None if gamma is None else gamma.data_ptr(), None if beta is None else beta.data_ptr(),
        y.data_ptr(), *shape, eps, slope, None if ws is None else ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def same_bits(got, want):
    d, nan_ok = I.differing(got.cpu(), want.cpu())
    return d == 0 and nan_ok


# ---------------------------------------------------------------- against the reference: conditions (a) and (b)
@pytest.mark.parametrize("dtype", I.DTYPES, ids=I.IDS)
def test_against_the_reference_over_the_whole_table(ext, dtype):
    """Every case x affine on / off x slope {1, 0, 0.01}, inputs N(0,1) * scale + offset with |offset| / scale up to 10^4:
    (a) every finite element within 2 u (|x a| + |b|) + 2^-25 of the float64 value, NaN positions equal;
    (b) over the whole table at most 1 element in 10^4, of at least 10^6, differs in bits from the rounded reference."""
    total = differ = 0
    for shape in I.CASES:
        x, gamma, beta, stats = I.problem(shape, dtype)
        xg, gg, bg = x.cuda(), gamma.cuda(), beta.cuda()
        assert ext.instance_norm_plan(*shape, dtype=dtype).form == I.plan_of(*shape)[0]
        for affine in (True, False):
            for slope in I.SLOPES:
                got = (ext.instance_norm(xg, gg, bg, I.EPS, slope) if affine else ext.instance_norm(xg, eps=I.EPS, negative_slope=slope)).cpu()
                want, ref64, a, b = I.reference(x, gamma if affine else None, beta if affine else None, I.EPS, slope, stats)
                assert got.shape == want.shape and got.dtype == dtype and got.is_contiguous()
                d, nan_ok = I.differing(got, want)
                ok, worst = I.within_bound(got, ref64, x, a, b)
                print(f"{I.case_id(shape)} affine={affine} slope={slope}: {d} of {got.numel()} differ, worst error / bound {worst:.3f}")
                assert nan_ok, (shape, affine, slope)
                assert ok, (shape, affine, slope, worst)
                total += got.numel()
                differ += d
    print(f"{dtype}: {differ} of {total} elements differ in bits from the reference")
    assert total >= 10 ** 6 and differ * 10 ** 4 <= total, (differ, total)


def test_empty_batch_returns_without_a_call(ext):
    out = ext.instance_norm(torch.zeros(0, 4, 9, 9, device="cuda"))
    assert out.shape == (0, 4, 9, 9)


# ---------------------------------------------------------------- special values
@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (1, 2, 99, 331)], ids=["plane", "split"])
@pytest.mark.parametrize("dtype", I.DTYPES, ids=I.IDS)
def test_special_values(ext, dtype, shape):
    """A NaN, an inf and a -inf each take their own plane and no other (first element, which is K, and elsewhere); a
    constant plane gives beta within (a); -0.0 inputs."""
    N, C, H, W = shape
    x, gamma, beta = I.random_problem(shape, dtype, seed=5)
    planes = x.view(N * C, H * W)                       # (a view: writes go to x)
    nan, inf = float("nan"), float("inf")
    if N * C >= 6:
        planes[0, 17], planes[1, 0], planes[2, H * W - 1], planes[3, :] = nan, inf, -inf, 1.5
        planes[4, ::2] = -0.0
        bad, const = (0, 1, 2), 3
    else:
        planes[0, 0] = -inf
        bad, const = (0,), None
    for slope in (1.0, 0.01):
        got = ext.instance_norm(x.cuda(), gamma.cuda(), beta.cuda(), I.EPS, slope).cpu()
        want, ref64, a, b = I.reference(x, gamma, beta, I.EPS, slope)
        gp = got.view(N * C, H * W)
        for p in range(N * C):
            assert bool(gp[p].isnan().all()) == (p in bad), p
        assert I.differing(got, want)[1]
        assert I.within_bound(got, ref64, x, a, b)[0]
        if const is not None:
            c = const % C
            lim = I.bound(x, a, b).view(N * C, H * W)[const]
            act = float(beta[c]) if float(beta[c]) >= 0 or slope == 1.0 else float(beta[c]) * float(torch.tensor(slope, dtype=torch.float32))
            assert bool(((gp[const].double() - act).abs() <= lim).all())
    # an inf at the plane's first element with a NaN-free rest, affine off
    y = ext.instance_norm(x.cuda()).cpu().view(N * C, H * W)
    assert all(bool(y[p].isnan().all()) == (p in bad) for p in range(N * C))


def test_fp32_subnormal_inputs_are_not_flushed(ext):
    shape = (2, 3, 7, 9)
    x = (torch.randn(shape, generator=torch.Generator().manual_seed(8), dtype=torch.float64) * 2.0 ** -130).float()
    assert float(x.abs().max()) < 2.0 ** -126 and int((x != 0).sum()) > x.numel() // 2
    eps = 1e-80                                         # the planes' variance is about 2^-260 = 5e-79: eps must not drown it
    for slope in (1.0, 0.01):
        got = ext.instance_norm(x.cuda(), eps=eps, negative_slope=slope).cpu()
        want, ref64, a, b = I.reference(x, None, None, eps, slope)
        assert float(want.abs().max()) > 0.5            # the reference sees the subnormals (a flushed plane would be constant)
        assert I.within_bound(got, ref64, x, a, b)[0]   # (flushed inputs give a constant plane: off by the plane's whole spread)
    # subnormal OUTPUTS: gamma tiny
    x, gamma, beta = I.random_problem(shape, torch.float32, seed=9)
    gamma, beta = gamma * 2.0 ** -135, beta * 0
    got = ext.instance_norm(x.cuda(), gamma.cuda(), beta.cuda()).cpu()
    want, ref64, a, b = I.reference(x, gamma, beta)
    assert 0 < float(want.abs().max()) < 2.0 ** -126
    assert int((got != 0).sum()) > got.numel() // 2
    assert I.within_bound(got, ref64, x, a, b)[0]


# ---------------------------------------------------------------- addresses, guards, workspace
@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (1, 2, 99, 331)], ids=["plane", "split"])
@pytest.mark.parametrize("dtype", I.DTYPES, ids=I.IDS)
def test_views_guards_and_workspace(ext, dtype, shape):
    """x and y 0 .. 3 elements past a 16-byte boundary, independently (the same offset: vector loads and stores; different
    ones: element loads), through the raw ABI.  Nothing but y's elements is written in y's buffer, nothing but the queried
    bytes in the workspace's; what the workspace held before -- 0xFF, 0x00, another call's leftovers -- changes no bit."""
    x, gamma, beta, stats = I.problem(shape, dtype)
    slope = 0.01
    want, ref64, a, b = I.reference(x, gamma, beta, I.EPS, slope, stats)
    n = x.numel()
    itype = torch.int32 if dtype == torch.float32 else torch.int16
    need = ext.instance_norm_workspace_bytes(*shape)
    assert (need > 0) == (I.plan_of(*shape)[0] == I.SPLIT)
    gg, bg = gamma.cuda(), beta.cuda()
    GUARD = 256
    by_x_offset = {}
    for k, (ox, oy) in enumerate(((0, 0), (1, 1), (2, 2), (3, 3), (1, 0), (0, 2), (3, 1))):
        xb = torch.zeros(n + 8, dtype=dtype, device="cuda")
        xv = xb[ox:ox + n]
        xv.copy_(x.reshape(-1))
        assert xv.data_ptr() == xb.data_ptr() + ox * x.element_size() and xb.data_ptr() % 16 == 0
        buf = torch.full((64 + n + 64,), NAN_PATTERN[dtype], dtype=itype, device="cuda")
        before = buf.clone()
        yv = buf[64 + oy:64 + oy + n].view(dtype)
        wsb = torch.full((GUARD + need + GUARD,), (0xFF, 0x00, 0xA5)[k % 3], dtype=torch.uint8, device="cuda")
        if k == 3 and need:
            wsb[GUARD:GUARD + need] = torch.randint(0, 256, (need,), dtype=torch.uint8, device="cuda")
        wsb[:GUARD], wsb[GUARD + need:] = 0x3C, 0x3C
        ws = wsb[GUARD:GUARD + need] if need else None
        assert raw_call(ext, xv, gg, bg, yv, shape, slope, ws, need) == 1
        inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
        inside[64 + oy:64 + oy + n] = True
        assert torch.equal(buf[~inside], before[~inside]), "a byte outside y was written"
        assert not (buf[inside] == before[inside]).any(), "an element of y was left unwritten"
        assert bool((wsb[:GUARD] == 0x3C).all()) and bool((wsb[GUARD + need:] == 0x3C).all()), "a byte outside the workspace was written"
        assert bool((xb[:ox] == 0).all()) and bool((xb[ox + n:] == 0).all()) and torch.equal(xv.cpu(), x.reshape(-1))
        got = yv.cpu().view(shape)
        assert I.differing(got, want)[1] and I.within_bound(got, ref64, x, a, b)[0], (ox, oy)
        # the sums follow x's address alone: the same x offset gives the same bits whatever y's offset and the workspace held
        assert same_bits(got, by_x_offset.setdefault(ox, got)), (ox, oy)
    assert len(by_x_offset) == 4


def test_plane_form_leaves_a_workspace_alone(ext):
    shape = (2, 3, 7, 9)
    x, gamma, beta, _ = I.problem(shape, torch.float32)
    ws = torch.full((1024,), 0x5A, dtype=torch.uint8, device="cuda")
    y = torch.empty(shape, device="cuda")
    assert raw_call(ext, x.cuda(), gamma.cuda(), beta.cuda(), y, shape, 1.0, ws, 1024) == 1
    assert bool((ws == 0x5A).all())
    y2 = torch.empty(shape, device="cuda")
    assert raw_call(ext, x.cuda(), gamma.cuda(), beta.cuda(), y2, shape, 1.0, None, 0) == 1
    assert same_bits(y, y2)


# ---------------------------------------------------------------- determinism, streams, capture
@pytest.mark.parametrize("shape", [(3, 5, 24, 40), (2, 2, 128, 257)], ids=["plane", "split"])
def test_two_calls_and_a_second_stream_give_identical_bits(ext, shape):
    for dtype in (torch.float32, torch.bfloat16):
        x, gamma, beta, _ = I.problem(shape, dtype)
        x, gamma, beta = x.cuda(), gamma.cuda(), beta.cuda()
        first = ext.instance_norm(x, gamma, beta, I.EPS, 0.01)
        second = ext.instance_norm(x, gamma, beta, I.EPS, 0.01)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            third = ext.instance_norm(x, gamma, beta, I.EPS, 0.01)
        side.synchronize()
        assert same_bits(first, second) and same_bits(first, third)


@pytest.mark.parametrize("shape", [(3, 5, 24, 40), (2, 2, 128, 257)], ids=["plane", "split"])
def test_graph_capture_reproduces_the_eager_bits(ext, shape):
    dtype = torch.bfloat16 if shape[0] == 3 else torch.float32
    x, gamma, beta, _ = I.problem(shape, dtype)
    x, gamma, beta = x.cuda(), gamma.cuda(), beta.cuda()
    ext.instance_norm(x, gamma, beta, I.EPS, 0.01)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = ext.instance_norm(x, gamma, beta, I.EPS, 0.01)
    x.copy_(I.random_problem(shape, dtype, seed=77)[0])          # x changes in place
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, ext.instance_norm(x, gamma, beta, I.EPS, 0.01))


# ---------------------------------------------------------------- the module really runs the kernel
def test_switched_module_runs_the_kernel_and_falls_back(ext, monkeypatch):
    from fots_e2e.native import AbsorbedLeakyReLU, NativeInstanceNorm2d, instancenorm_ok, use_native_instancenorm
    net = nn.Sequential(nn.InstanceNorm2d(8, affine=True), nn.LeakyReLU(0.01), nn.Conv2d(8, 8, 1)).cuda()
    assert use_native_instancenorm(net) == (1, 1)
    m = net[0]
    assert type(m) is NativeInstanceNorm2d and type(net[1]) is AbsorbedLeakyReLU and m.fused_slope == 0.01
    x = torch.randn(2, 8, 13, 17, device="cuda")
    stock = F.instance_norm

    def refuse(*a, **k):
        raise AssertionError("the stock instance norm was called")
    monkeypatch.setattr(F, "instance_norm", refuse)
    with torch.no_grad():
        assert instancenorm_ok(m, x)
        y = net[1](m(x))                                    # works although F.instance_norm raises: the kernel ran
    want, ref64, a, b = I.reference(x.cpu(), m.weight.detach().cpu(), m.bias.detach().cpu(), m.eps, 0.01)
    assert I.within_bound(y.cpu(), ref64, x.cpu(), a, b)[0] and I.differing(y.cpu(), want)[0] * 1000 <= y.numel()
    with pytest.raises(AssertionError, match="stock instance norm"):
        m(x.clone().requires_grad_(True))                   # a gradient is needed: the stock path (which raises here)
    monkeypatch.setattr(F, "instance_norm", stock)
    xg = x.clone().requires_grad_(True)
    assert not instancenorm_ok(m, xg)
    yg = m(xg)                                              # the stock path applies the absorbed activation too
    assert yg.requires_grad and torch.equal(yg, F.leaky_relu(stock(xg, weight=m.weight, bias=m.bias, use_input_stats=True, eps=m.eps), 0.01))
    yg.sum().backward()
    assert xg.grad is not None and m.weight.grad is not None     # training is untouched
    with torch.no_grad():
        xc = x.to(memory_format=torch.channels_last)
        assert not instancenorm_ok(m, xc)
        assert torch.equal(m(xc), F.leaky_relu(stock(xc, weight=m.weight, bias=m.bias, use_input_stats=True, eps=m.eps), 0.01))
        assert torch.allclose(m(xc), y, atol=1e-5)


# ---------------------------------------------------------------- in the network
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=["fp32", "bf16"])
def test_the_49_norms_of_the_network(ext, dtype, monkeypatch):
    """FOTSNet on a 64 x 96 image and 11 x 24 crops with every norm switched: 49 native calls, each output within (a) of the
    reference of its own input.  With the activations absorbed, each of the 20 pairs gives F.leaky_relu of the un-fused
    native output -- bit for bit in fp32.  In bf16 the fused module rounds (float)v * slope once, as the contract fixes it,
    where the un-fused pair rounds v to bf16 first and the product again: bit for bit wherever the output is not negative;
    where it is, with t = v * slope, |got - t| <= u |t| (one rounding), |t - bf16(v) * slope| <= u |t| and the un-fused
    pair's second rounding adds u (1 + u) |t|, so |got - want| <= 3 u (1 + 2^-6) |want| with u = 2^-8.  With both native
    switches on, the network runs."""
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import NativeInstanceNorm2d, use_native_depthwise, use_native_instancenorm
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet()).eval().cuda().to(dtype)
    image = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(7)).cuda().to(dtype)
    crops = torch.randn(3, 64, 11, 24, generator=torch.Generator().manual_seed(8)).cuda().to(dtype)
    assert use_native_instancenorm(net, fuse_activation=False) == (52, 0)
    calls = []
    run = ext._instance_norm_run
    monkeypatch.setattr(ext, "_instance_norm_run", lambda *a: (calls.append(a[4]), run(*a))[1])
    seen = {}
    mods = [(n, m) for n, m in net.named_modules() if type(m) is NativeInstanceNorm2d]
    hooks = [m.register_forward_hook(lambda mod, inp, out, n=n: seen.__setitem__(n, (inp[0].detach(), out.detach()))) for n, m in mods]
    with torch.no_grad():
        plain = net(image)
        plain_ocr = net.forward_ocr(crops)
    for h in hooks:
        h.remove()
    assert len(calls) == 49 == len(seen) and set(calls) == {1.0}
    for n, m in mods:
        if n not in seen:
            continue
        xin, y = seen[n][0].cpu(), seen[n][1].cpu()
        p = m._parameters
        w, bt = (p["weight"].detach().cpu(), p["bias"].detach().cpu()) if p.get("weight") is not None else (None, None)
        want, ref64, a, b = I.reference(xin, w, bt, m.eps, 1.0)
        ok, worst = I.within_bound(y, ref64, xin, a, b)
        assert I.differing(y, want)[1] and ok, (n, worst)
    # absorb the activations
    del calls[:]
    assert use_native_instancenorm(net) == (0, 20)
    fused = [(n, m) for n, m in mods if m.fused_slope is not None]
    assert len(fused) == 20 and all(n in seen for n, _ in fused)
    with torch.no_grad():
        for n, m in fused:
            xin, y = seen[n]
            got, want = m(xin), F.leaky_relu(y, m.fused_slope)
            if dtype == torch.float32:
                assert same_bits(got, want), n
            else:
                keep = want >= 0
                assert same_bits(got[keep], want[keep]), n
                assert bool(((got.double() - want.double()).abs() <= 3 * 2.0 ** -8 * (1 + 2.0 ** -6) * want.double().abs()).all()), n
        both = net(image)
        both_ocr = net.forward_ocr(crops)
    assert len(calls) == 20 + 49 and calls.count(0.01) == 20 + 20
    assert use_native_depthwise(net) == 22
    with torch.no_grad():
        all_native = net(image)
    for a, b in zip(list(plain) + [[plain_ocr]], list(both) + [[both_ocr]]):
        for s, t in zip(a, b):
            assert s.shape == t.shape and bool(t.isfinite().all())     # (the stock convolutions between the norms are not
            #                                                            held to equal bits from pass to pass: no comparison here)
    assert all(bool(t.isfinite().all()) for a in all_native for t in a)
