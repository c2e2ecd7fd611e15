"""GPU (MI355X): the native depthwise 3x3 backward against the oracle and the reference of
depthwise_backward_cases.py: dx bit for bit and dweight within the bound over the whole table, the two partial calls,
misaligned views with guards, the overlap and workspace refusals, determinism, graph capture, NaN locality, the autograd
function, the module switch, and the 22 convolutions of the network in one training step."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import depthwise_backward_cases as B
import depthwise_cases as D
from instancenorm_cases import differing
from test_gpu_bucketed import NAN_PATTERN

pytestmark = pytest.mark.gpu

ONE_SEG, THREE_SEGS, STRIDE2, STRIDE2_SEGS = ((2, 7, 22, 40), 1), ((3, 2, 54, 76), 1), ((1, 3, 6, 7), 2), ((3, 2, 107, 76), 2)


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def same_bits(got, want):
    d, nan_ok = differing(got.cpu(), want.cpu())
    return d == 0 and nan_ok


def ptr(t):
    return None if t is None else t.data_ptr()


def raw_backward(ext, dy, x, w, dx, dw, shape, stride, ws=None, nbytes=0):
    """The C ABI on tensors (or views) as they are: nothing is made contiguous or aligned on the way."""
    st = ext._lib.rroi_depthwise3x3_backward_hip(ext.dtype_code(dy.dtype), ptr(dy), ptr(x), ptr(w), ptr(dx), ptr(dw), *shape, stride,
                                                 ptr(ws), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def on_gpu(case, dtype):
    return tuple(t.cuda() for t in B.problem(case, dtype))


# ---------------------------------------------------------------- against the oracle and the reference
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.IDS)
@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_against_the_oracle_and_the_reference_over_the_whole_table(ext, case, dtype):
    """dx bit for bit the oracle's, every element written; dweight within the bound of the case module."""
    shape, s = case
    x, w, dy = on_gpu(case, dtype)
    want_dx, ref = B.reference(case, dtype)
    dx, dw = ext.depthwise3x3_backward(dy, x, w, s)
    assert dx.shape == x.shape and dx.dtype == dtype and dx.is_contiguous()
    assert dw.shape == w.shape and dw.dtype == dtype and dw.is_contiguous()
    d, nan_ok = differing(dx.cpu(), want_dx)
    ok, worst = ref.check(dw)
    print(f"{B.case_id(case)} {dtype}: dx elements differing {d} of {dx.numel()}, dweight worst error / bound {worst:.4f}")
    assert d == 0 and nan_ok, (case, d)
    assert ok, (case, worst)


@pytest.mark.parametrize("case", [ONE_SEG, THREE_SEGS, STRIDE2, STRIDE2_SEGS], ids=B.case_id)
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.IDS)
def test_partial_calls_give_the_full_calls_bits(ext, dtype, case):
    """need_dx=False skips the dx launch, need_dweight=False the two dweight launches; what is left has the bits of the call
    that computes everything.  An empty batch returns without a call."""
    shape, s = case
    x, w, dy = on_gpu(case, dtype)
    dx, dw = ext.depthwise3x3_backward(dy, x, w, s)
    none, dw2 = ext.depthwise3x3_backward(dy, x, w, s, need_dx=False)
    dx3, none3 = ext.depthwise3x3_backward(dy, x, w, s, need_dweight=False)
    assert none is None and none3 is None and same_bits(dw2, dw) and same_bits(dx3, dx)
    want_dx, ref = B.reference(case, dtype)
    assert same_bits(dx3, want_dx) and ref.check(dw2)[0]
    e = torch.zeros(0, shape[1], 5, 7, dtype=dtype, device="cuda")
    dxe, dwe = ext.depthwise3x3_backward(e[:, :, :D.out_size(5, s), :D.out_size(7, s)], e, w, s)
    assert dxe.shape == e.shape and dwe.shape == w.shape and bool((dwe == 0).all())


# ---------------------------------------------------------------- addresses, guards, workspace
@pytest.mark.parametrize("case", [((2, 3, 7, 9), 1), ((1, 2, 9, 17), 2), ((1, 2, 8, 16), 2)], ids=B.case_id)
@pytest.mark.parametrize("dtype", D.DTYPES, ids=D.IDS)
def test_views_guards_and_workspace(ext, dtype, case):
    """dy, x and dx each 0 .. 3 elements past a 16-byte boundary through the raw ABI.  Nothing but dx's elements is written
    in dx's buffer and nothing but the queried bytes in the workspace's; dy, x and the weight are left as they were; what
    the workspace held before changes no bit, and neither do the offsets: the order of every sum is the shape's alone."""
    shape, s = case
    N, C, H, W = shape
    x, w, dy = B.random_case(case, dtype)
    want_dx = B.expected_dx(dy, w, H, W, s)
    ref = B.DweightReference(dy, x, s)
    n, ny = x.numel(), dy.numel()
    itype = torch.int32 if dtype == torch.float32 else torch.int16
    need = ext.depthwise3x3_backward_workspace_bytes(*shape, s)
    wg = w.cuda()
    GUARD = 256
    first = None
    for k, (ox, od, oo) in enumerate(((0, 0, 0), (1, 1, 1), (3, 3, 3), (1, 0, 1), (1, 1, 0), (0, 2, 3), (3, 1, 2))):
        xb, db_ = torch.zeros(n + 8, dtype=dtype, device="cuda"), torch.zeros(ny + 8, dtype=dtype, device="cuda")
        xv, dv = xb[ox:ox + n], db_[od:od + ny]
        xv.copy_(x.reshape(-1))
        dv.copy_(dy.reshape(-1))
        assert xb.data_ptr() % 16 == 0 and db_.data_ptr() % 16 == 0 and dv.data_ptr() == db_.data_ptr() + od * dy.element_size()
        buf = torch.full((64 + n + 64,), NAN_PATTERN[dtype], dtype=itype, device="cuda")
        before = buf.clone()
        ov = buf[64 + oo:64 + oo + n].view(dtype)
        wsb = torch.full((GUARD + need + GUARD,), (0xFF, 0x00, 0xA5)[k % 3], dtype=torch.uint8, device="cuda")
        wsb[:GUARD], wsb[GUARD + need:] = 0x3C, 0x3C
        dw = torch.empty_like(wg)
        assert raw_backward(ext, dv, xv, wg, ov, dw, shape, s, wsb[GUARD:GUARD + need], need) == 1
        inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
        inside[64 + oo:64 + oo + n] = True
        assert torch.equal(buf[~inside], before[~inside]), "a byte outside dx was written"
        assert not (buf[inside] == before[inside]).any(), "an element of dx was left unwritten"
        assert bool((wsb[:GUARD] == 0x3C).all()) and bool((wsb[GUARD + need:] == 0x3C).all()), "a byte outside the workspace was written"
        assert torch.equal(xv.cpu(), x.reshape(-1)) and torch.equal(dv.cpu(), dy.reshape(-1)) and torch.equal(wg.cpu(), w)
        got = ov.cpu().view(shape)
        assert same_bits(got, want_dx) and ref.check(dw)[0], (ox, od, oo)
        first = dw.cpu() if first is None else first
        assert same_bits(dw, first), (ox, od, oo)


def test_overlap_and_workspace_refusals_write_nothing_and_an_unneeded_workspace_is_left_alone(ext):
    case = ((2, 3, 7, 9), 1)
    shape, s = case
    x, w, dy = on_gpu(case, torch.float32)
    need = ext.depthwise3x3_backward_workspace_bytes(*shape, s)
    ws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    # dx alone needs no workspace: NULL / 0 is accepted, and a buffer that is handed over is left alone
    dx = torch.empty_like(x)
    assert raw_backward(ext, dy, None, w, dx, None, shape, s, ws, need) == 1
    assert bool((ws == 0x5A).all())
    dx2 = torch.empty_like(x)
    assert raw_backward(ext, dy, None, w, dx2, None, shape, s, None, 0) == 1
    assert same_bits(dx, dx2) and same_bits(dx, B.reference(case, torch.float32)[0])
    # dweight alone needs neither the weight nor dx
    dw = torch.empty_like(w)
    assert raw_backward(ext, dy, x, None, None, dw, shape, s, ws, need) == 1
    assert B.reference(case, torch.float32)[1].check(dw)[0]
    # refused where the workspace is needed and is missing, misaligned or short -- and nothing is written then
    dx3, dw3 = torch.full_like(x, 7.0), torch.full_like(w, 7.0)
    ws.fill_(0x5A)
    assert raw_backward(ext, dy, x, w, dx3, dw3, shape, s, None, 0) == 0
    assert raw_backward(ext, dy, x, w, dx3, dw3, shape, s, ws[16:], need) == 0
    assert raw_backward(ext, dy, x, w, dx3, dw3, shape, s, ws, need - 1) == 0
    # dx overlapping dy (one buffer holds both, dx beginning inside dy), and dx overlapping x where dweight reads it
    both = torch.zeros(2 * x.numel(), device="cuda")
    both[:dy.numel()].copy_(dy.reshape(-1))
    keep = both.clone()
    assert raw_backward(ext, both[:dy.numel()], x, w, both[dy.numel() - 1:dy.numel() - 1 + x.numel()], dw3, shape, s, ws, need) == 0
    assert raw_backward(ext, both[:dy.numel()], x, w, both[:x.numel()], None, shape, s, None, 0) == 0
    assert raw_backward(ext, dy, x, w, x, dw3, shape, s, ws, need) == 0
    assert torch.equal(both, keep) and bool((dx3 == 7.0).all()) and bool((dw3 == 7.0).all()) and bool((ws == 0x5A).all())
    assert torch.equal(x.cpu(), B.problem(case, torch.float32)[0])


# ---------------------------------------------------------------- determinism, special values, capture
@pytest.mark.parametrize("case", [ONE_SEG, THREE_SEGS, STRIDE2_SEGS], ids=B.case_id)
def test_two_calls_and_a_second_stream_give_identical_bits(ext, case):
    shape, s = case
    for dtype in (torch.float32, torch.bfloat16):
        x, w, dy = on_gpu(case, dtype)
        first = ext.depthwise3x3_backward(dy, x, w, s)
        second = ext.depthwise3x3_backward(dy, x, w, s)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            third = ext.depthwise3x3_backward(dy, x, w, s)
        side.synchronize()
        for a, b, c in zip(first, second, third):
            assert same_bits(a, b) and same_bits(a, c)


@pytest.mark.parametrize("case", [THREE_SEGS, STRIDE2_SEGS], ids=B.case_id)
def test_graph_capture_reproduces_the_eager_bits(ext, case):
    """One linear chain -- forward, backward -- captured on a side stream and replayed on changed inputs."""
    shape, s = case
    dtype = torch.bfloat16 if s == 2 else torch.float32
    x, w, dy = (t.clone() for t in on_gpu(case, dtype))
    ext.depthwise3x3_backward(dy, x, w, s)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            y = ext.depthwise3x3(x, w, s)
            out = ext.depthwise3x3_backward(dy, x, w, s)
    x2, w2, dy2 = B.random_case(case, dtype, seed=77)
    x.copy_(x2)                                                   # the inputs change in place
    dy.copy_(dy2)
    for t in out:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want = ext.depthwise3x3_backward(dy, x, w, s)
    assert same_bits(y, ext.depthwise3x3(x, w, s)) and all(same_bits(a, b) for a, b in zip(out, want))
    assert same_bits(out[0], B.expected_dx(dy2, w.cpu(), shape[2], shape[3], s)) and B.DweightReference(dy2, x2, s).check(out[1])[0]


@pytest.mark.parametrize("case", [((2, 3, 7, 9), 1), ((2, 3, 8, 10), 2), ((2, 3, 7, 9), 2)], ids=B.case_id)
def test_a_nan_in_dy_reaches_exactly_the_oracles_elements_and_its_channels_dweight(ext, case):
    shape, s = case
    N, C, H, W = shape
    x, w, dy = (t.clone() for t in B.random_case(case, torch.float32))
    ho, wo = dy.shape[2:]
    bad_n, bad_c = 1, 1
    for oy, ox in ((0, 0), (ho - 1, wo - 1), (ho // 2, wo // 2)):
        d = dy.clone()
        d[bad_n, bad_c, oy, ox] = float("nan")
        dx, dw = ext.depthwise3x3_backward(d.cuda(), x.cuda(), w.cuda(), s)
        want = B.expected_dx(d, w, H, W, s)
        assert same_bits(dx, want)
        nan = dx.cpu().isnan()
        assert bool(nan.any()) and int(nan.sum()) <= 9 and bool(nan[bad_n, bad_c].any()) and int(nan.sum()) == int(nan[bad_n, bad_c].sum())
        for c in range(C):
            assert bool(dw[c].isnan().all()) == (c == bad_c) and (c == bad_c or bool(dw[c].isfinite().all())), c
        assert B.DweightReference(d, x, s).check(dw)[0]


# ---------------------------------------------------------------- autograd
@pytest.mark.parametrize("case", [((3, 5, 24, 40), 1), ((3, 5, 23, 40), 2)], ids=B.case_id)
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=["fp32", "bf16"])
def test_autograd_function_under_deterministic_algorithms(ext, dtype, case):
    """rroi_align.conv.depthwise3x3: the forward's bits are the inference call's, the gradients are the backward call's,
    only what needs_input_grad wants is computed, a non-contiguous dy is taken, and without any gradient needed it is the
    plain inference call.  All of it with torch.use_deterministic_algorithms(True)."""
    from rroi_align import conv
    shape, s = case
    x, w, dy = (t.cuda() for t in B.random_case(case, dtype))
    torch.use_deterministic_algorithms(True)
    try:
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = conv.depthwise3x3(xr, wr, s)
        assert y.requires_grad and same_bits(y, ext.depthwise3x3(x, w, s))
        y.backward(dy)
        dx, dw = ext.depthwise3x3_backward(dy, x, w, s)
        assert same_bits(xr.grad, dx) and same_bits(wr.grad, dw)
        assert same_bits(dx, B.expected_dx(dy, w, shape[2], shape[3], s)) and B.DweightReference(dy.cpu(), x.cpu(), s).check(dw)[0]
        calls = []
        run = conv.run_depthwise3x3_backward
        conv.run_depthwise3x3_backward = lambda *a: (calls.append(a), run(*a))[1]
        try:
            # only x; a dy that is a permuted view
            xr2 = x.clone().requires_grad_(True)
            y2 = conv.depthwise3x3(xr2, w, s)
            dyt = dy.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
            assert not dyt.is_contiguous()
            y2.backward(dyt)
            assert calls[-1][0].is_contiguous() and calls[-1][3:] == (s, True, False)
            assert same_bits(xr2.grad, dx)
            # only the weight
            wr3 = w.clone().requires_grad_(True)
            conv.depthwise3x3(x, wr3, s).backward(dy)
            assert calls[-1][3:] == (s, False, True) and same_bits(wr3.grad, dw)
            # no gradient needed: the plain call, nothing saved
            n = len(calls)
            y4 = conv.depthwise3x3(x, w, s)
            with torch.no_grad():
                y5 = conv.depthwise3x3(xr, wr, s)
            assert y4.grad_fn is None and y5.grad_fn is None and same_bits(y4, y) and same_bits(y5, y) and len(calls) == n
        finally:
            conv.run_depthwise3x3_backward = run
    finally:
        torch.use_deterministic_algorithms(False)


# ---------------------------------------------------------------- the module really runs the kernels
@pytest.mark.parametrize("stride", (1, 2))
def test_trainable_module_runs_the_kernels_where_a_gradient_is_needed(ext, monkeypatch, stride):
    from fots_e2e.native import DepthwiseConv3x3, use_native_depthwise
    from fots_e2e.native_train import TrainableDepthwiseConv3x3, trainable_depthwise_ok, use_trainable_depthwise
    net = nn.Sequential(nn.Conv2d(8, 8, 3, stride, 1, groups=8, bias=False)).cuda()
    assert use_native_depthwise(net) == 1 and use_trainable_depthwise(net) == 1
    m = net[0]
    assert type(m) is TrainableDepthwiseConv3x3
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 13, 17, generator=g).cuda()
    dy = torch.randn(2, 8, D.out_size(13, stride), D.out_size(17, stride), generator=g).cuda()
    stock_conv2d, stock_forward = F.conv2d, nn.Conv2d._conv_forward

    def refuse(*a, **k):
        raise AssertionError("the stock convolution was called")
    monkeypatch.setattr(F, "conv2d", refuse)
    monkeypatch.setattr(nn.Conv2d, "_conv_forward", refuse)
    xg = x.clone().requires_grad_(True)
    assert trainable_depthwise_ok(m, xg)
    y = m(xg)                                               # works although the stock convolution raises: the kernels ran
    y.backward(dy)
    w = m.weight.detach()
    assert same_bits(y.detach(), D.expected(x, w, stride))
    assert same_bits(xg.grad, B.expected_dx(dy, w, 13, 17, stride))
    assert B.DweightReference(dy.cpu(), x.cpu(), stride).check(m.weight.grad)[0]
    with torch.no_grad():                                   # no gradient needed: the parent's native inference call
        assert same_bits(m(x), y.detach())
    # the fall-backs take the stock path (which raises here): channels-last, autocast
    with pytest.raises(AssertionError, match="stock convolution"):
        m(x.to(memory_format=torch.channels_last).requires_grad_(True))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(AssertionError, match="stock convolution"):
            m(xg)
    monkeypatch.setattr(F, "conv2d", stock_conv2d)
    monkeypatch.setattr(nn.Conv2d, "_conv_forward", stock_forward)
    # ... and compute what the stock module does
    xc = x.to(memory_format=torch.channels_last).requires_grad_(True)
    assert torch.equal(m(xc), F.conv2d(xc, m.weight, None, stride, 1, 1, 8))
    # enable=False restores the class, and with it today's behaviour: the stock path where a gradient is needed
    assert use_trainable_depthwise(net, enable=False) == 1 and type(m) is DepthwiseConv3x3
    monkeypatch.setattr(nn.Conv2d, "_conv_forward", refuse)
    with pytest.raises(AssertionError, match="stock convolution"):
        m(xg)


# ---------------------------------------------------------------- in the network
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=["fp32", "bf16"])
def test_one_training_step_of_the_network(ext, dtype, monkeypatch):
    """FOTSNet in train mode on a 64 x 96 image and 11 x 24 crops with both switches: one forward + forward_ocr + a scalar
    loss + backward makes exactly 22 native backward calls, each with dx the oracle's bits and dweight within the bound of
    the reference of its own recorded (dy, x, w), and every parameter that took part has a finite gradient."""
    from rroi_align import conv
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import use_native_depthwise
    from fots_e2e.native_train import use_trainable_depthwise
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet()).train().cuda().to(dtype)
    image = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(7)).cuda().to(dtype)
    crops = torch.randn(3, 64, 11, 24, generator=torch.Generator().manual_seed(8)).cuda().to(dtype)
    assert use_native_depthwise(net) == 22 and use_trainable_depthwise(net) == 22
    calls = []
    run = conv.run_depthwise3x3_backward

    def record(*a):
        out = run(*a)
        calls.append((a, out))
        return out
    monkeypatch.setattr(conv, "run_depthwise3x3_backward", record)
    outs = [t for group in net(image) for t in group] + [net.forward_ocr(crops)]
    loss = sum((t.float() * torch.linspace(-1, 1, t.numel(), device="cuda").view_as(t)).sum() for t in outs)
    loss.backward()
    torch.cuda.synchronize()
    assert len(calls) == 22
    worst = 0.0
    for (dy, x, w, s, need_dx, need_dw), (dx, dw) in calls:
        assert need_dx and need_dw and dy.dtype == x.dtype == w.dtype == dtype
        cpu = lambda t: t.detach().cpu()
        assert same_bits(dx, B.expected_dx(dy, w, x.size(2), x.size(3), s)), (tuple(x.shape), s)
        ok, ratio = B.DweightReference(cpu(dy), cpu(x), s).check(dw)
        worst = max(worst, ratio)
        assert ok, (tuple(x.shape), s, ratio)
    print(f"{dtype}: 22 backward calls, dx bit for bit, dweight worst error / bound {worst:.4f}")
    with_grad = [p for p in net.parameters() if p.grad is not None]
    assert len(with_grad) >= 0.9 * len(list(net.parameters()))       # (three norms and little else take no part in a pass)
    assert all(bool(p.grad.isfinite().all()) for p in with_grad)
    depthwise = [m for m in net.modules() if type(m).__name__ == "TrainableDepthwiseConv3x3"]
    assert len(depthwise) == 22 and all(m.weight.grad is not None for m in depthwise)
