"""GPU (MI355X): the native InstanceNorm2d training forward and backward against the longdouble reference of
instancenorm_backward_cases.py: the bounds of the contract over the whole table in both forms, the two partial calls,
misaligned views with guards, determinism, a NaN plane, the workspace, graph capture, the autograd function, the module
switch, and the 49 norms of the network in one training step."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import instancenorm_backward_cases as B
import instancenorm_cases as I
from test_gpu_bucketed import NAN_PATTERN

pytestmark = pytest.mark.gpu

PLANE_SHAPE, SPLIT_SHAPE = (3, 5, 24, 40), (2, 2, 128, 257)


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def same_bits(got, want):
    d, nan_ok = I.differing(got.cpu(), want.cpu())
    return d == 0 and nan_ok


def ptr(t):
    return None if t is None else t.data_ptr()


def raw_backward(ext, dy, x, stats, gamma, beta, dx, dgamma, dbeta, shape, slope, ws=None, nbytes=0, eps=I.EPS):
    """The C ABI on tensors (or views) as they are: nothing is made contiguous or aligned on the way."""
    st = ext._lib.rroi_instancenorm_backward_hip(
        ext.dtype_code(x.dtype), ptr(dy), ptr(x), ptr(stats), ptr(gamma), ptr(beta), ptr(dx), ptr(dgamma), ptr(dbeta), *shape, eps,
        slope, ptr(ws), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def on_gpu(shape, dtype):
    x, gamma, beta, stats, dy = B.problem(shape, dtype)
    return x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda()


def threshold_shapes(ext):
    """The table's shapes, and -- read from the plan query, not from a copy of the rule -- the largest plane of the plane
    form and the smallest of the split form for two planes, wherever the backward's rule has put that line."""
    lo, hi = 1, 1 << 20                                   # rows of 16 elements: 2 planes of 16 .. 16 * 2^20
    assert ext.instance_norm_backward_plan(1, 2, lo, 16).form == ext.INORM_PLANE
    assert ext.instance_norm_backward_plan(1, 2, hi, 16).form == ext.INORM_SPLIT
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ext.instance_norm_backward_plan(1, 2, mid, 16).form == ext.INORM_SPLIT:
            hi = mid
        else:
            lo = mid
    extra = tuple(s for s in ((1, 2, lo, 16), (1, 2, hi, 16)) if s[2] * 16 <= 1 << 18)
    return I.CASES + tuple(s for s in extra if s not in I.CASES)


# ---------------------------------------------------------------- against the reference
@pytest.mark.parametrize("dtype", I.DTYPES, ids=I.IDS)
def test_against_the_reference_over_the_whole_table(ext, dtype):
    """Every case x affine on / off x slope {1, 0, 0.01}: the training forward's y bit for bit the inference call's and its
    statistics those of the longdouble reference; dx, dgamma and dbeta within the bounds of the case module; no plane of
    the table left out; both forms reached."""
    forms = set()
    worst_dx = worst_p = 0.0
    for shape in threshold_shapes(ext):
        N, C, H, W = shape
        if shape in I.CASES:
            x, gamma, beta, stats, dy = B.problem(shape, dtype)
        else:
            x, gamma, beta = I.random_problem(shape, dtype, seed=sum(shape))
            stats, dy = I.plane_statistics(x), B.random_dy(shape, dtype, sum(shape))
        xg, gg, bg, dg = x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda()
        forms.add(ext.instance_norm_backward_plan(*shape, dtype=dtype).form)
        mean, var = (torch.from_numpy(s).reshape(N, C) for s in stats)
        for affine in (True, False):
            w, b = (gg, bg) if affine else (None, None)
            for slope in I.SLOPES:
                y, st = ext.instance_norm_train(xg, w, b, I.EPS, slope)
                assert same_bits(y, ext.instance_norm(xg, w, b, I.EPS, slope)), (shape, affine, slope)
                assert st.shape == (N, C, 2) and st.dtype == torch.float64
                # sums of up to 2^18 doubles, shifted by the plane's first element K with |K - mean| of a few standard
                # deviations: n 2^-53 relative to sum |x - K| <= n (|K - mean| + std), and mean = K + m rounded once
                sd = var.sqrt()
                assert bool(((st[..., 0].cpu() - mean).abs() <= 2.0 ** -31 * sd + 2.0 ** -50 * mean.abs()).all()), shape
                assert bool(((st[..., 1].cpu() - var).abs() <= 2.0 ** -30 * var).all()), shape
                ref = B.reference(shape, dtype, affine, slope) if shape in I.CASES else \
                    B.Reference(x, dy, gamma if affine else None, beta if affine else None, I.EPS, slope, stats)
                assert int(ref.left_out.sum()) == 0
                dx, dw, db = ext.instance_norm_backward(dg, xg, st, w, b, I.EPS, slope)
                assert dx.shape == x.shape and dx.dtype == dtype and dx.is_contiguous()
                ok, worst = ref.check_dx(dx.cpu())
                print(f"{I.case_id(shape)} affine={affine} slope={slope}: dx worst error / bound {worst:.3f}")
                worst_dx = max(worst_dx, worst)
                assert ok, (shape, affine, slope, worst)
                if H * W == 1:
                    assert bool((dx == 0).all())              # a one-element plane: xh = 0 and g - t1 = 0 exactly
                if affine:
                    assert dw.shape == db.shape == (C,) and dw.dtype == db.dtype == dtype
                    ok, worst = ref.check_params(dw.cpu(), db.cpu())
                    print(f"{I.case_id(shape)} slope={slope}: parameter gradients worst error / bound {worst:.3f}")
                    worst_p = max(worst_p, worst)
                    assert ok, (shape, slope, worst)
                else:
                    assert dw is None and db is None
    print(f"{dtype}: worst ratio dx {worst_dx:.3f}, parameter gradients {worst_p:.3f}")
    assert forms == {ext.INORM_PLANE, ext.INORM_SPLIT}


@pytest.mark.parametrize("shape", [PLANE_SHAPE, SPLIT_SHAPE], ids=["plane", "split"])
@pytest.mark.parametrize("dtype", I.DTYPES, ids=I.IDS)
def test_partial_calls_give_the_full_calls_bits(ext, dtype, shape):
    """need_dx=False skips the map pass, need_param_grads=False the parameter-gradient kernel; what is left has the bits of
    the call that computes everything.  An empty batch returns without a call."""
    x, gamma, beta, dy = on_gpu(shape, dtype)
    _, st = ext.instance_norm_train(x, gamma, beta, I.EPS, 0.01)
    dx, dw, db = ext.instance_norm_backward(dy, x, st, gamma, beta, I.EPS, 0.01)
    none, dw2, db2 = ext.instance_norm_backward(dy, x, st, gamma, beta, I.EPS, 0.01, need_dx=False)
    assert none is None and same_bits(dw2, dw) and same_bits(db2, db)
    dx3, nw, nb = ext.instance_norm_backward(dy, x, st, gamma, beta, I.EPS, 0.01, need_param_grads=False)
    assert nw is None and nb is None and same_bits(dx3, dx)
    ref = B.reference(shape, dtype, True, 0.01)
    assert ref.check_dx(dx3.cpu())[0] and ref.check_params(dw2.cpu(), db2.cpu())[0]
    e = torch.zeros(0, shape[1], 4, 4, dtype=dtype, device="cuda")
    ye, se = ext.instance_norm_train(e, gamma, beta)
    dxe, dwe, dbe = ext.instance_norm_backward(e, e, se, gamma, beta)
    assert ye.shape == dxe.shape == e.shape and se.shape == (0, shape[1], 2) and bool((dwe == 0).all()) and bool((dbe == 0).all())


# ---------------------------------------------------------------- addresses, guards, workspace
@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (1, 2, 99, 331)], ids=["plane", "split"])
@pytest.mark.parametrize("dtype", I.DTYPES, ids=I.IDS)
def test_views_guards_and_workspace(ext, dtype, shape):
    """dy, x and dx each 0 .. 3 elements past a 16-byte boundary through the raw ABI (equal offsets: vector loads; different
    ones: element loads).  Nothing but dx's elements is written in dx's buffer and nothing but the queried bytes in the
    workspace's; what the workspace held before changes no bit."""
    x, gamma, beta, stats, dy = B.problem(shape, dtype)
    ref = B.reference(shape, dtype, True, 0.01)
    n = x.numel()
    itype = torch.int32 if dtype == torch.float32 else torch.int16
    need = ext.instance_norm_backward_workspace_bytes(*shape)
    gg, bg = gamma.cuda(), beta.cuda()
    _, st = ext.instance_norm_train(x.cuda(), gg, bg, I.EPS, 0.01)
    GUARD = 256
    by_x_offset = {}
    for k, (ox, od, oo) in enumerate(((0, 0, 0), (1, 1, 1), (3, 3, 3), (1, 0, 1), (1, 1, 0), (0, 2, 3), (3, 1, 2))):
        xb, db_ = torch.zeros(n + 8, dtype=dtype, device="cuda"), torch.zeros(n + 8, dtype=dtype, device="cuda")
        xv, dv = xb[ox:ox + n], db_[od:od + n]
        xv.copy_(x.reshape(-1))
        dv.copy_(dy.reshape(-1))
        assert xb.data_ptr() % 16 == 0 and db_.data_ptr() % 16 == 0 and xv.data_ptr() == xb.data_ptr() + ox * x.element_size()
        buf = torch.full((64 + n + 64,), NAN_PATTERN[dtype], dtype=itype, device="cuda")
        before = buf.clone()
        ov = buf[64 + oo:64 + oo + n].view(dtype)
        wsb = torch.full((GUARD + need + GUARD,), (0xFF, 0x00, 0xA5)[k % 3], dtype=torch.uint8, device="cuda")
        wsb[:GUARD], wsb[GUARD + need:] = 0x3C, 0x3C
        dw, db = torch.empty_like(gg), torch.empty_like(gg)
        assert raw_backward(ext, dv, xv, st, gg, bg, ov, dw, db, shape, 0.01, wsb[GUARD:GUARD + need], need) == 1
        inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
        inside[64 + oo:64 + oo + n] = True
        assert torch.equal(buf[~inside], before[~inside]), "a byte outside dx was written"
        assert not (buf[inside] == before[inside]).any(), "an element of dx was left unwritten"
        assert bool((wsb[:GUARD] == 0x3C).all()) and bool((wsb[GUARD + need:] == 0x3C).all()), "a byte outside the workspace was written"
        assert torch.equal(xv.cpu(), x.reshape(-1)) and torch.equal(dv.cpu(), dy.reshape(-1))
        got = ov.cpu().view(shape)
        assert ref.check_dx(got)[0] and ref.check_params(dw.cpu(), db.cpu())[0], (ox, od, oo)
        # the sums follow x's address alone: the same x offset gives the same bits whatever the others and the workspace held
        first = by_x_offset.setdefault(ox, (got, dw.cpu(), db.cpu()))
        assert same_bits(got, first[0]) and same_bits(dw, first[1]) and same_bits(db, first[2]), (ox, od, oo)
    assert len(by_x_offset) == 3


def test_plane_form_without_parameter_gradients_needs_no_workspace_and_leaves_one_alone(ext):
    shape = (2, 3, 7, 9)
    x, gamma, beta, dy = on_gpu(shape, torch.float32)
    _, st = ext.instance_norm_train(x, gamma, beta, I.EPS, 0.0)
    ws = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    dx = torch.empty_like(x)
    assert raw_backward(ext, dy, x, st, gamma, beta, dx, None, None, shape, 0.0, ws, 4096) == 1
    assert bool((ws == 0x5A).all())
    dx2 = torch.empty_like(x)
    assert raw_backward(ext, dy, x, st, gamma, beta, dx2, None, None, shape, 0.0, None, 0) == 1
    assert same_bits(dx, dx2) and B.reference(shape, torch.float32, True, 0.0).check_dx(dx.cpu())[0]
    # refused where the workspace is needed, and nothing is written then
    dx3 = torch.full_like(x, 7.0)
    dw = torch.full_like(gamma, 7.0)
    assert raw_backward(ext, dy, x, st, gamma, beta, dx3, dw, dw.clone(), shape, 0.0, None, 0) == 0
    assert bool((dx3 == 7.0).all()) and bool((dw == 7.0).all())


# ---------------------------------------------------------------- determinism, special values, capture
@pytest.mark.parametrize("shape", [PLANE_SHAPE, SPLIT_SHAPE], ids=["plane", "split"])
def test_two_calls_and_a_second_stream_give_identical_bits(ext, shape):
    for dtype in (torch.float32, torch.bfloat16):
        x, gamma, beta, dy = on_gpu(shape, dtype)
        _, st = ext.instance_norm_train(x, gamma, beta, I.EPS, 0.01)
        _, st2 = ext.instance_norm_train(x, gamma, beta, I.EPS, 0.01)
        assert torch.equal(st.view(torch.int64), st2.view(torch.int64))
        first = ext.instance_norm_backward(dy, x, st, gamma, beta, I.EPS, 0.01)
        second = ext.instance_norm_backward(dy, x, st, gamma, beta, I.EPS, 0.01)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            third = ext.instance_norm_backward(dy, x, st, gamma, beta, I.EPS, 0.01)
        side.synchronize()
        for a, b, c in zip(first, second, third):
            assert same_bits(a, b) and same_bits(a, c)


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), SPLIT_SHAPE], ids=["plane", "split"])
@pytest.mark.parametrize("where", ["x", "dy"])
def test_a_nan_stays_in_its_plane_and_its_channel(ext, shape, where):
    N, C, H, W = shape
    dtype = torch.float32
    x, gamma, beta, stats, dy = B.problem(shape, dtype)
    x, dy = x.clone(), dy.clone()
    bad = 1                                               # plane (n = 0, c = 1)
    (x if where == "x" else dy).view(N * C, H * W)[bad, 17] = float("nan")
    _, st = ext.instance_norm_train(x.cuda(), gamma.cuda(), beta.cuda(), I.EPS, 0.01)
    dx, dw, db = ext.instance_norm_backward(dy.cuda(), x.cuda(), st, gamma.cuda(), beta.cuda(), I.EPS, 0.01)
    planes = dx.cpu().view(N * C, H * W)
    for p in range(N * C):
        assert bool(planes[p].isnan().all()) == (p == bad), p
        assert p == bad or bool(planes[p].isfinite().all())
    for c in range(C):
        assert c == bad % C or (bool(dw[c].isfinite()) and bool(db[c].isfinite())), c
    # dgamma takes it through xh either way; dbeta = sum dy d only from dy: where v is NaN, d is the slope, as in torch
    assert bool(dw[bad % C].isnan()) and bool(db[bad % C].isnan()) == (where == "dy")
    ref = B.Reference(x, dy, gamma, beta, I.EPS, 0.01)
    assert ref.check_dx(dx.cpu())[0] and ref.check_params(dw.cpu(), db.cpu())[0]


@pytest.mark.parametrize("shape", [PLANE_SHAPE, SPLIT_SHAPE], ids=["plane", "split"])
def test_graph_capture_reproduces_the_eager_bits(ext, shape):
    """One linear chain -- training forward, backward -- captured on a side stream and replayed on changed inputs."""
    dtype = torch.bfloat16 if shape[0] == 3 else torch.float32
    x, gamma, beta, dy = on_gpu(shape, dtype)
    x, dy = x.clone(), dy.clone()
    ext.instance_norm_backward(dy, x, ext.instance_norm_train(x, gamma, beta, I.EPS, 0.01)[1], gamma, beta, I.EPS, 0.01)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            y, st = ext.instance_norm_train(x, gamma, beta, I.EPS, 0.01)
            out = ext.instance_norm_backward(dy, x, st, gamma, beta, I.EPS, 0.01)
    x.copy_(I.random_problem(shape, dtype, seed=77)[0])          # the inputs change in place
    dy.copy_(B.random_dy(shape, dtype, 78))
    for t in out:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    y2, st2 = ext.instance_norm_train(x, gamma, beta, I.EPS, 0.01)
    want = ext.instance_norm_backward(dy, x, st2, gamma, beta, I.EPS, 0.01)
    assert same_bits(y, y2) and all(same_bits(a, b) for a, b in zip(out, want))


# ---------------------------------------------------------------- autograd
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=["fp32", "bf16"])
def test_autograd_function_under_deterministic_algorithms(ext, dtype):
    """rroi_align.norm.instance_norm: the forward's bits are the inference call's, the gradients are the backward call's,
    only what needs_input_grad wants is computed, a non-contiguous dy is taken, and without any gradient needed it is the
    plain inference call.  All of it with torch.use_deterministic_algorithms(True)."""
    from rroi_align import norm
    shape = PLANE_SHAPE
    x, gamma, beta, dy = on_gpu(shape, dtype)
    torch.use_deterministic_algorithms(True)
    try:
        xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        y = norm.instance_norm(xr, gr, br, I.EPS, 0.01)
        assert y.requires_grad and same_bits(y, ext.instance_norm(x, gamma, beta, I.EPS, 0.01))
        y.backward(dy)
        _, st = ext.instance_norm_train(x, gamma, beta, I.EPS, 0.01)
        dx, dw, db = ext.instance_norm_backward(dy, x, st, gamma, beta, I.EPS, 0.01)
        assert same_bits(xr.grad, dx) and same_bits(gr.grad, dw) and same_bits(br.grad, db)
        ref = B.reference(shape, dtype, True, 0.01)
        assert ref.check_dx(xr.grad.cpu())[0] and ref.check_params(gr.grad.cpu(), br.grad.cpu())[0]
        # only x, without parameters; a dy that is a permuted view
        calls = []
        run = norm.run_instance_norm_backward
        norm.run_instance_norm_backward = lambda *a: (calls.append(a), run(*a))[1]
        try:
            xr2 = x.clone().requires_grad_(True)
            y2 = norm.instance_norm(xr2, eps=I.EPS, negative_slope=0.0)
            dyt = dy.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
            assert not dyt.is_contiguous()
            y2.backward(dyt)
            assert calls[-1][0].is_contiguous() and calls[-1][7:] == (True, False)
            assert B.reference(shape, dtype, False, 0.0).check_dx(xr2.grad.cpu())[0]
            # only the parameters
            gr3, br3 = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
            norm.instance_norm(x, gr3, br3, I.EPS, 0.01).backward(dy)
            assert calls[-1][7:] == (False, True) and same_bits(gr3.grad, dw) and same_bits(br3.grad, db)
            # no gradient needed: the plain call, nothing saved
            n = len(calls)
            y4 = norm.instance_norm(x, gamma, beta, I.EPS, 0.01)
            with torch.no_grad():
                y5 = norm.instance_norm(xr, gr, br, I.EPS, 0.01)
            assert y4.grad_fn is None and y5.grad_fn is None and same_bits(y4, y) and same_bits(y5, y) and len(calls) == n
        finally:
            norm.run_instance_norm_backward = run
    finally:
        torch.use_deterministic_algorithms(False)


# ---------------------------------------------------------------- the module really runs the kernels
def test_trainable_module_runs_the_kernels_where_a_gradient_is_needed(ext, monkeypatch):
    from fots_e2e.native import NativeInstanceNorm2d, use_native_instancenorm
    from fots_e2e.native_train import TrainableInstanceNorm2d, trainable_norm_ok, use_trainable_instancenorm
    net = nn.Sequential(nn.InstanceNorm2d(8, affine=True), nn.LeakyReLU(0.01), nn.Conv2d(8, 8, 1)).cuda()
    assert use_native_instancenorm(net) == (1, 1) and use_trainable_instancenorm(net) == 1
    m = net[0]
    assert type(m) is TrainableInstanceNorm2d and m.fused_slope == 0.01
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 13, 17, generator=g).cuda()
    dy = torch.randn(2, 8, 13, 17, generator=g).cuda()
    stock = F.instance_norm

    def refuse(*a, **k):
        raise AssertionError("the stock instance norm was called")
    monkeypatch.setattr(F, "instance_norm", refuse)
    xg = x.clone().requires_grad_(True)
    assert trainable_norm_ok(m, xg)
    y = net[1](m(xg))                                       # works although F.instance_norm raises: the kernels ran
    y.backward(dy)
    w, b = m.weight.detach().cpu(), m.bias.detach().cpu()
    ref = B.Reference(x.cpu(), dy.cpu(), w, b, m.eps, 0.01)
    assert not bool(ref.left_out.any())
    assert ref.check_dx(xg.grad.cpu())[0] and ref.check_params(m.weight.grad.cpu(), m.bias.grad.cpu())[0]
    want, ref64, a, bb = I.reference(x.cpu(), w, b, m.eps, 0.01)
    assert I.within_bound(y.detach().cpu(), ref64, x.cpu(), a, bb)[0]
    with torch.no_grad():                                   # no gradient needed: the parent's native inference call
        assert same_bits(m(x), y.detach())
    # the fall-backs take the stock path (which raises here): channels-last, autocast, running statistics
    with pytest.raises(AssertionError, match="stock instance norm"):
        m(x.to(memory_format=torch.channels_last).requires_grad_(True))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(AssertionError, match="stock instance norm"):
            m(xg)
    r = nn.Sequential(nn.InstanceNorm2d(8, affine=True, track_running_stats=True)).cuda()
    use_native_instancenorm(r)
    assert use_trainable_instancenorm(r) == 1
    with pytest.raises(AssertionError, match="stock instance norm"):
        r(xg)
    monkeypatch.setattr(F, "instance_norm", stock)
    # ... and compute what the stock module does, activation included
    xc = x.to(memory_format=torch.channels_last).requires_grad_(True)
    assert torch.equal(m(xc), F.leaky_relu(stock(xc, weight=m.weight, bias=m.bias, use_input_stats=True, eps=m.eps), 0.01))
    # enable=False restores the class, and with it today's behaviour: the stock path where a gradient is needed
    assert use_trainable_instancenorm(net, enable=False) == 1 and type(m) is NativeInstanceNorm2d
    monkeypatch.setattr(F, "instance_norm", refuse)
    with pytest.raises(AssertionError, match="stock instance norm"):
        m(xg)


# ---------------------------------------------------------------- in the network
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=["fp32", "bf16"])
def test_one_training_step_of_the_network(ext, dtype, monkeypatch):
    """FOTSNet in train mode on a 64 x 96 image and 11 x 24 crops with both switches: one forward + forward_ocr + a scalar
    loss + backward makes 49 native backward calls, each within the bounds of the reference of its own (x, dy), and every
    parameter that took part has a finite gradient."""
    from rroi_align import norm
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import use_native_instancenorm
    from fots_e2e.native_train import use_trainable_instancenorm
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet()).train().cuda().to(dtype)
    image = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(7)).cuda().to(dtype)
    crops = torch.randn(3, 64, 11, 24, generator=torch.Generator().manual_seed(8)).cuda().to(dtype)
    assert use_native_instancenorm(net) == (52, 20) and use_trainable_instancenorm(net) == 52
    calls = []
    run = norm.run_instance_norm_backward

    def record(*a):
        out = run(*a)
        calls.append((a, out))
        return out
    monkeypatch.setattr(norm, "run_instance_norm_backward", record)
    monkeypatch.setattr(F, "instance_norm", lambda *a, **k: pytest.fail("the stock instance norm was called"))
    outs = [t for group in net(image) for t in group] + [net.forward_ocr(crops)]
    loss = sum((t.float() * torch.linspace(-1, 1, t.numel(), device="cuda").view_as(t)).sum() for t in outs)
    loss.backward()
    torch.cuda.synchronize()
    assert len(calls) == 49
    worst_dx = worst_p = 0.0
    for (dy, x, st, w, b, eps, slope, need_dx, need_params), (dx, dw, db) in calls:
        assert need_dx and need_params == (w is not None)
        cpu = lambda t: None if t is None else t.detach().cpu()
        ref = B.Reference(cpu(x), cpu(dy), cpu(w), cpu(b), eps, slope)
        assert ref.cap_ok(), (tuple(x.shape), int(ref.left_out.sum()))
        ok, worst = ref.check_dx(cpu(dx))
        worst_dx = max(worst_dx, worst)
        assert ok, (tuple(x.shape), slope, worst)
        if w is not None:
            ok, worst = ref.check_params(cpu(dw), cpu(db))
            worst_p = max(worst_p, worst)
            assert ok, (tuple(x.shape), slope, worst)
    print(f"{dtype}: 49 backward calls, worst ratio dx {worst_dx:.3f}, parameter gradients {worst_p:.3f}")
    with_grad = [p for p in net.parameters() if p.grad is not None]
    assert len(with_grad) >= 0.9 * len(list(net.parameters()))       # (three norms and little else take no part in a pass)
    assert all(bool(p.grad.isfinite().all()) for p in with_grad)
