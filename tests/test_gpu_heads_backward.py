"""GPU (MI355X): the native training forward and backward of the detection heads and the attention gate
against the reference of heads_backward_cases.py: the training forward's outputs bit for bit the inference call's and z,
dx, dw and db within their bounds over the whole table, the partial calls, misaligned views with guards, determinism at
two workspace addresses, a stale workspace, graph capture, NaN locality, the autograd functions, and the two heads and
three gates of the network in one training step."""
import pytest
import torch

import heads_backward_cases as B
import heads_cases as H
from heads_cases import differing
from test_gpu_bucketed import NAN_PATTERN as _NAN_PATTERNS

pytestmark = pytest.mark.gpu

NAN_PATTERN = _NAN_PATTERNS[torch.float32]      # the workspace's stale contents, as 32-bit words

ONE_ROW, TWO_ROWS, CROSSING, TWO_PASSES, ODD = (2, 3, 7, 9), (1, 64, 5, 13), (3, 3, 181, 242), (2, 515, 3, 5), (3, 257, 7, 9)


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def same_bits(got, want):
    if got is None or want is None:
        return got is None and want is None
    d, nan_ok = differing(got.cpu(), want.cpu())
    return d == 0 and nan_ok


def flat(result):
    """(dx, dw, db) of either backward as one list of tensors / Nones."""
    dx, dw, db = result
    return [dx] + (list(dw) if isinstance(dw, tuple) else [dw]) + (list(db) if isinstance(db, tuple) else [db])


def on_gpu(shape, dtype):
    x, hp, gp, hg, gg = B.problem(shape, dtype)
    cu = lambda ts: tuple(t.cuda() for t in ts)  # noqa: E731
    return x.cuda(), cu(hp), cu(gp), cu(hg), cu(gg)


def heads_call(ext, x, hp, hg, z=None, **need):
    z = ext.heads_train(x, *hp)[3] if z is None else z
    return ext.heads_backward(*hg, x, z, hp[0], hp[2], hp[4], **need)


def gate_call(ext, x, gp, gg, z=None, **need):
    z = ext.gate_train(x, *gp)[1] if z is None else z
    return ext.gate_backward(gg[0], x, z, gp[0], **need)


# ---------------------------------------------------------------- against the reference
@pytest.mark.parametrize("dtype", H.DTYPES, ids=H.IDS)
@pytest.mark.parametrize("shape", B.CASES, ids=B.case_id)
def test_training_forward_and_backward_over_the_whole_table(ext, shape, dtype):
    """heads_train / gate_train: the outputs bit for bit `heads` / `gate`, z within its bound; heads_backward /
    gate_backward: dx, dw and db within the bounds of the case module, every element written."""
    x, hp, gp, hg, gg = on_gpu(shape, dtype)
    Rh, Rg = B.reference(shape, dtype)
    *outs, z = ext.heads_train(x, *hp)
    assert all(same_bits(a, b) for a, b in zip(outs, ext.heads(x, *hp)))
    y, zg = ext.gate_train(x, *gp)
    assert same_bits(y, ext.gate(x, *gp))
    zs = [B.check(z, Rh.z, Rh.z_lim), B.check(zg, Rg.z, Rg.z_lim)]
    dx, dw, db = ext.heads_backward(*hg, x, z, hp[0], hp[2], hp[4])
    assert dx.shape == x.shape and dx.dtype == dtype and [t.shape for t in dw] == [hp[0].shape, hp[2].shape, hp[4].shape]
    ok_h, worst_h = B.check_all(Rh, dx, dw, db)
    gdx, gdw, gdb = ext.gate_backward(gg[0], x, zg, gp[0])
    ok_g, worst_g = B.check_all(Rg, gdx, gdw, gdb)
    print(f"{B.case_id(shape)} {dtype}: worst error / bound: z {zs[0][1]:.4f} {zs[1][1]:.4f}, heads {worst_h}, gate {worst_g}")
    assert zs[0][0] and zs[1][0], zs
    assert ok_h, worst_h
    assert ok_g, worst_g


# ---------------------------------------------------------------- partial calls
@pytest.mark.parametrize("dtype", H.DTYPES, ids=H.IDS)
@pytest.mark.parametrize("shape", (TWO_ROWS, ODD), ids=B.case_id)
def test_partial_calls_give_the_full_calls_bits(ext, shape, dtype):
    """Each need_* flag off, and each output gradient None against the same gradient given as zeros."""
    x, hp, gp, hg, gg = on_gpu(shape, dtype)
    z, zg = ext.heads_train(x, *hp)[3], ext.gate_train(x, *gp)[1]
    full_h, full_g = flat(heads_call(ext, x, hp, hg, z)), flat(gate_call(ext, x, gp, gg, zg))
    for off in ("need_dx", "need_dweight", "need_dbias"):
        for full, part in ((full_h, flat(heads_call(ext, x, hp, hg, z, **{off: False}))),
                           (full_g, flat(gate_call(ext, x, gp, gg, zg, **{off: False})))):
            assert any(t is None for t in part)
            assert all(t is None or same_bits(t, f) for t, f in zip(part, full)), off
    only_dx = heads_call(ext, x, hp, hg, z, need_dweight=False, need_dbias=False)
    assert same_bits(only_dx[0], full_h[0]) and only_dx[1] == (None,) * 3 and only_dx[2] == (None,) * 3
    for i in range(3):
        with_none = [g if j != i else None for j, g in enumerate(hg)]
        with_zero = [g if j != i else torch.zeros_like(g) for j, g in enumerate(hg)]
        assert all(same_bits(a, b) for a, b in zip(flat(heads_call(ext, x, hp, with_none, z)), flat(heads_call(ext, x, hp, with_zero, z))))
    with pytest.raises(ValueError):
        heads_call(ext, x, hp, (None, None, None), z)
    with pytest.raises(ValueError):
        heads_call(ext, x, hp, hg, z, need_dx=False, need_dweight=False, need_dbias=False)


# ---------------------------------------------------------------- the C ABI on views
def ptr(t):
    return None if t is None else t.data_ptr()


def guarded(t, lead=3, tail=5, fill=None):
    """-> (buffer, view): a copy of t (fill given: not copied) `lead` elements into a buffer of NaNs."""
    buf = torch.full((lead + t.numel() + tail,), float("nan"), dtype=t.dtype, device="cuda")
    view = buf[lead:lead + t.numel()].view(t.shape)
    if fill is None:
        view.copy_(t)
    return buf, view


def guards_intact(buf, view, lead=3):
    return bool(buf[:lead].isnan().all()) and bool(buf[lead + view.numel():].isnan().all())


@pytest.mark.parametrize("dtype", H.DTYPES, ids=H.IDS)
@pytest.mark.parametrize("shape", (ODD, TWO_ROWS), ids=B.case_id)
def test_misaligned_views_with_guard_bands_are_left_intact(ext, shape, dtype):
    """Every tensor one or three elements into its allocation, every output between guard bands of the NaN pattern, the
    workspace filled with it: the bits of the wrapper's call, the guards untouched."""
    x, hp, gp, hg, gg = on_gpu(shape, dtype)
    N, C, Hh, W = shape
    z = ext.heads_train(x, *hp)[3]
    want = flat(ext.heads_backward(*hg, x, z, hp[0], hp[2], hp[4]))
    ins = [guarded(t, lead=1)[1] for t in (*hg, x, hp[0], hp[2], hp[4])]
    outs = [guarded(t, fill=0) for t in want]
    nbytes = ext.heads_backward_workspace_bytes(N, C, Hh, W)
    assert nbytes == B.workspace_bytes(N, C, Hh, W, 7)
    ws = torch.full((nbytes // 4 + 64,), NAN_PATTERN, dtype=torch.int32, device="cuda")
    off = (-ws.data_ptr() % 256) // 4
    st = ext._lib.rroi_heads_backward_hip(ext.dtype_code(dtype), ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), ptr(z),
                                          ptr(ins[4]), ptr(ins[5]), ptr(ins[6]), ptr(outs[0][1]), ptr(outs[1][1]),
                                          ptr(outs[4][1]), ptr(outs[2][1]), ptr(outs[5][1]), ptr(outs[3][1]), ptr(outs[6][1]),
                                          N, C, Hh, W, H.RBOX_SCALE, ws[off:].data_ptr(), nbytes,
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 1
    assert all(same_bits(view, w) for (_, view), w in zip(outs, want))
    assert all(guards_intact(buf, view) for buf, view in outs)
    tail = ws[off + nbytes // 4:]
    assert bool((tail == NAN_PATTERN).all()) and bool((ws[:off] == NAN_PATTERN).all())


# ---------------------------------------------------------------- determinism, the workspace, graphs
@pytest.mark.parametrize("shape", (CROSSING, TWO_PASSES, (3, 256, 16, 24)), ids=B.case_id)
def test_same_bits_twice_at_another_workspace_address_and_over_a_stale_workspace(ext, shape):
    """Two calls agree bit for bit; so does a raw call at a different workspace address whose bytes are the NaN pattern."""
    dtype = torch.float32
    x, hp, gp, hg, gg = on_gpu(shape, dtype)
    N, C, Hh, W = shape
    z = ext.heads_train(x, *hp)[3]
    first, second = flat(heads_call(ext, x, hp, hg, z)), flat(heads_call(ext, x, hp, hg, z))
    assert all(same_bits(a, b) for a, b in zip(first, second))
    g1, g2 = flat(gate_call(ext, x, gp, gg)), flat(gate_call(ext, x, gp, gg))
    assert all(same_bits(a, b) for a, b in zip(g1, g2))
    nbytes = ext.heads_backward_workspace_bytes(N, C, Hh, W)
    ws = torch.full((nbytes // 4 + 256,), NAN_PATTERN, dtype=torch.int32, device="cuda")
    off = (-ws.data_ptr() % 256) // 4 + 64                     # another 256-byte-aligned address, stale contents
    outs = [torch.empty_like(t) for t in first]
    st = ext._lib.rroi_heads_backward_hip(ext.dtype_code(dtype), ptr(hg[0]), ptr(hg[1]), ptr(hg[2]), ptr(x), ptr(z), ptr(hp[0]),
                                          ptr(hp[2]), ptr(hp[4]), ptr(outs[0]), ptr(outs[1]), ptr(outs[4]), ptr(outs[2]),
                                          ptr(outs[5]), ptr(outs[3]), ptr(outs[6]), N, C, Hh, W, H.RBOX_SCALE,
                                          ws[off:].data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 1 and all(same_bits(a, b) for a, b in zip(outs, first))
    ok, worst = B.check_all(B.reference(shape, dtype)[0], first[0], tuple(first[1:4]), tuple(first[4:7]))
    assert ok, worst


@pytest.mark.parametrize("shape", (TWO_ROWS, (3, 256, 16, 24)), ids=B.case_id)
def test_graph_capture_and_replay_give_the_eager_bits(ext, shape):
    dtype = torch.bfloat16
    x, hp, gp, hg, gg = on_gpu(shape, dtype)
    eager = flat(heads_call(ext, x, hp, hg)) + flat(gate_call(ext, x, gp, gg))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            captured = flat(heads_call(ext, x, hp, hg)) + flat(gate_call(ext, x, gp, gg))
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
    stream.synchronize()
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(captured, eager))


# ---------------------------------------------------------------- NaN locality
@pytest.mark.parametrize("dtype", (torch.float32, torch.float16), ids=["fp32", "fp16"])
def test_a_poisoned_pixel_changes_its_own_dx_column_and_the_parameter_gradients_only(ext, dtype):
    shape = (2, 255, 11, 23)
    x, hp, gp, hg, gg = on_gpu(shape, dtype)
    z = ext.heads_train(x, *hp)[3]
    clean = heads_call(ext, x, hp, hg, z)
    n, py, pxl = 1, 4, 17
    poisoned = [g.clone() for g in hg]
    poisoned[2][n, 0, py, pxl] = float("nan")                         # dangle_0 of one pixel
    dx, dw, db = heads_call(ext, x, hp, poisoned, z)
    column = torch.zeros_like(dx, dtype=torch.bool)
    column[n, :, py, pxl] = True
    assert bool(dx[column].isnan().all()) and same_bits(dx.masked_fill(column, 0), clean[0].masked_fill(column, 0))
    # both angle rows see the pixel (g_5 and g_6 share u . dangle); score and rbox do not
    assert bool(dw[2].isnan().all()) and bool(db[2].isnan().all())
    assert same_bits(dw[0], clean[1][0]) and same_bits(dw[1], clean[1][1]) and same_bits(db[0], clean[2][0]) and same_bits(db[1], clean[2][1])
    # r = 0: z_5 = z_6 = 0 gives a = 0, u = 0 / 0: NaN in that pixel's column, nowhere else in dx
    z0 = z.clone()
    z0[n, 5:7, py, pxl] = 0.0
    dx0 = heads_call(ext, x, hp, hg, z0)[0]
    assert bool(dx0[column].isnan().all()) and not bool(dx0.masked_fill(column, 0).isnan().any())
    # the gate: a NaN in x reaches the pixel's column of dx through z, and dw / db
    xg = x.clone()
    xg[n, 3, py, pxl] = float("nan")
    gdx, gdw, gdb = gate_call(ext, xg, gp, gg)
    assert bool(gdx[column].isnan().all()) and not bool(gdx.masked_fill(column, 0).isnan().any())
    assert bool(gdw.isnan().all()) and bool(gdb.isnan().all())


# ---------------------------------------------------------------- autograd
def stock_heads(x, hp, scale=H.RBOX_SCALE):
    """FOTSNet._heads's expression on plain tensors."""
    import torch.nn.functional as F
    C = x.size(1)
    conv = lambda w, b: F.conv2d(x, w.reshape(-1, C, 1, 1), b)  # noqa: E731
    score = torch.sigmoid(conv(hp[0], hp[1]))
    dist = torch.sigmoid(conv(hp[2], hp[3])) * scale
    ang = torch.sigmoid(conv(hp[4], hp[5])) * 2 - 1
    ang = ang / torch.sqrt(ang[:, 0] * ang[:, 0] + ang[:, 1] * ang[:, 1]).unsqueeze(1)
    return score, dist, ang


@pytest.mark.parametrize("dtype", H.DTYPES, ids=H.IDS)
@pytest.mark.parametrize("shape", ((3, 256, 16, 24), ODD), ids=B.case_id)
def test_autograd_functions_against_float64_stock_autograd(ext, shape, dtype):
    """detection_heads / attention_gate: gradients within the bounds against float64 autograd of the stock expressions on
    the same (rounded) values; an unused output arrives as None; without a gradient needed they are the inference calls."""
    import torch.nn.functional as F
    from rroi_align.heads import attention_gate, detection_heads
    x, hp, gp, hg, gg = on_gpu(shape, dtype)
    Rh, Rg = B.reference(shape, dtype)
    leaves = [t.clone().requires_grad_(True) for t in (x, *hp)]
    outs = detection_heads(*leaves)
    assert all(same_bits(a, b) for a, b in zip(outs, ext.heads(x, *hp)))
    torch.autograd.backward(outs, hg)
    ok, worst = B.check_all(Rh, leaves[0].grad, (leaves[1].grad, leaves[3].grad, leaves[5].grad),
                            (leaves[2].grad, leaves[4].grad, leaves[6].grad))
    assert ok, worst
    # float64 stock autograd on the CPU agrees with the longdouble reference far inside the bounds
    l64 = [t.detach().double().cpu().requires_grad_(True) for t in (x, *hp)]
    torch.autograd.backward(stock_heads(l64[0], l64[1:]), [g.double().cpu() for g in hg])
    for got, want in ((leaves[0].grad, l64[0].grad), (leaves[1].grad, l64[1].grad), (leaves[6].grad, l64[6].grad)):
        fin = want.isfinite()
        lim = 4 * H.UNIT_ROUNDOFF[dtype] * want.abs().max() + 2.0 ** -20
        assert bool(((got.double().cpu().reshape(want.shape) - want).abs()[fin] <= lim).all())
    # the score alone: rbox and angle arrive as None
    leaves = [t.clone().requires_grad_(True) for t in (x, *hp)]
    detection_heads(*leaves)[0].backward(hg[0])
    Rs = B.Reference(x.cpu(), [t.cpu() for t in hp], (hg[0].cpu(), None, None))
    ok, worst = B.check_all(Rs, leaves[0].grad, (leaves[1].grad, leaves[3].grad, leaves[5].grad),
                            (leaves[2].grad, leaves[4].grad, leaves[6].grad))
    assert ok, worst
    gl = [t.clone().requires_grad_(True) for t in (x, *gp)]
    y = attention_gate(*gl)
    assert same_bits(y, ext.gate(x, *gp))
    y.backward(gg[0])
    ok, worst = B.check_all(Rg, gl[0].grad, gl[1].grad, gl[2].grad)
    assert ok, worst
    g64 = [t.detach().double().cpu().requires_grad_(True) for t in (x, *gp)]
    torch.sigmoid(F.conv2d(g64[0], g64[1].reshape(1, -1, 1, 1), g64[2])).backward(gg[0].double().cpu())
    assert torch.allclose(gl[1].grad.double().cpu(), g64[1].grad, rtol=8 * H.UNIT_ROUNDOFF[dtype],
                          atol=8 * H.UNIT_ROUNDOFF[dtype] * float(g64[1].grad.abs().max()))
    with torch.no_grad():
        assert all(same_bits(a, b) for a, b in zip(detection_heads(x, *hp), ext.heads(x, *hp)))
    assert not attention_gate(x, *gp).requires_grad


def test_the_stock_chains_backward_does_not_raise_under_deterministic_algorithms():
    """What `trainable_heads_ok` relies on when it asks `_heads_backward_slower` in that mode too: the stock expressions of
    `_heads` and of the gate train there, so determinism alone is no reason to leave them."""
    import torch.nn.functional as F
    x, hp, gp, hg, gg = on_gpu((3, 256, 16, 24), torch.float32)
    leaves = [t.clone().requires_grad_(True) for t in (x, *hp, *gp)]
    torch.use_deterministic_algorithms(True)
    try:
        torch.autograd.backward(stock_heads(leaves[0], leaves[1:7]), hg)
        torch.sigmoid(F.conv2d(leaves[0], leaves[7].reshape(1, -1, 1, 1), leaves[8])).backward(gg[0])
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(False)
    assert all(t.grad is not None and bool(t.grad.isfinite().all()) for t in leaves)


# ---------------------------------------------------------------- in the network
def small_net(dtype):
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    return deterministic_init(FOTSNet()).train().cuda().to(dtype)


def all_trainable_switches(net):
    from fots_e2e import native as nat, native_train as T
    from fots_e2e.native_train_heads import use_trainable_heads
    nat.use_native_instancenorm(net)
    assert T.use_trainable_instancenorm(net) > 0
    assert nat.use_native_depthwise(net) == 22 and T.use_trainable_depthwise(net) == 22
    assert nat.use_native_heads(net) and nat.use_native_merge(net) and T.use_trainable_merge(net)
    assert use_trainable_heads(net)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=["fp32", "bf16"])
def test_one_training_step_of_the_network(ext, dtype, monkeypatch):
    """FOTSNet in train mode on a 64 x 96 image with all four trainable switches on, under
    torch.use_deterministic_algorithms(True): a forward + a scalar loss + backward completes, makes exactly two heads and
    three gate backward calls, each within its bound on its own recorded tensors, and two runs give identical gradient bits
    for `act`, `rbox`, `angle` and `conv_attenton`."""
    from rroi_align import heads as fn
    net = small_net(dtype)
    all_trainable_switches(net)
    calls = {"heads": [], "gate": []}
    run_h, run_g = fn.run_heads_backward, fn.run_gate_backward

    def rec_h(*a):
        out = run_h(*a)
        calls["heads"].append((a, out))
        return out

    def rec_g(*a):
        out = run_g(*a)
        calls["gate"].append((a, out))
        return out
    monkeypatch.setattr(fn, "run_heads_backward", rec_h)
    monkeypatch.setattr(fn, "run_gate_backward", rec_g)
    image = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(7)).cuda().to(dtype)
    own = [p for m in (net.act, net.rbox, net.angle, net.conv_attenton) for p in m.parameters()]
    runs = []
    torch.use_deterministic_algorithms(True)
    try:
        for _ in range(2):
            net.zero_grad(set_to_none=True)
            torch.manual_seed(3)                                        # the dropouts draw the same masks
            outs = [t for group in net(image)[:3] for t in group]
            loss = sum((t.float() * torch.linspace(-1, 1, t.numel(), device="cuda").view_as(t)).sum() for t in outs)
            loss.backward()
            torch.cuda.synchronize()
            runs.append([p.grad.clone() for p in own])
    finally:
        torch.use_deterministic_algorithms(False)
    assert len(calls["heads"]) == 4 and len(calls["gate"]) == 6           # two runs of two and three
    assert all(same_bits(a, b) for a, b in zip(*runs)) and all(bool(g.isfinite().all()) for g in runs[0])
    params = [t.detach().cpu() for m in (net.act, net.rbox, net.angle) for t in (m.weight, m.bias)]
    for (ds, dr, da, x, z, ws, wr, wa, scale, ndx, ndw, ndb), (dx, dw, db) in calls["heads"][:2]:
        assert ndx and ndw and ndb and scale == 128.0 and x.dtype == dtype and x.size(1) == 256
        cpu = lambda t: None if t is None else t.cpu()  # noqa: E731
        ok, worst = B.check_all(B.Reference(x.cpu(), params, (cpu(ds), cpu(dr), cpu(da))), dx, dw, db)
        assert ok, worst
    gp = [net.conv_attenton.weight.detach().cpu(), net.conv_attenton.bias.detach().cpu()]
    for (dy, x, z, w, ndx, ndw, ndb), (dx, dw, db) in calls["gate"][:3]:
        assert ndx and ndw and ndb
        ok, worst = B.check_all(B.Reference(x.cpu(), gp, (dy.cpu(),)), dx, dw, db)
        assert ok, worst
    assert sorted(tuple(a[0][3].shape[2:]) for a in calls["heads"][:2]) == [(8, 12), (16, 24)]
    assert sorted(tuple(a[0][1].shape[2:]) for a in calls["gate"][:3]) == [(2, 3), (4, 6), (8, 12)]
