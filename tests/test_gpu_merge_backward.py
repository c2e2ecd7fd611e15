"""GPU (MI355X): the native gated merge's backward, the stand-alone resize and its backward against the
references of merge_backward_cases.py: df and the forward bit for bit, dx and dgate within the bound over the whole table,
the partial calls, misaligned views with guards, the overlap and workspace refusals, determinism, graph capture, NaN
locality, the autograd functions under deterministic algorithms, the network's `_merge` with the stock resize patched to
raise, and one whole training step."""
import pytest
import torch
import torch.nn.functional as F

import merge_backward_cases as B
from merge_cases import differing
from test_gpu_bucketed import NAN_PATTERN

pytestmark = pytest.mark.gpu

UPSCALE, DOWNSCALE, BLOCKS, SAME_GATE = B.CASES[2], B.CASES[7], B.CASES[5], B.EXTRA[0]


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def same_bits(got, want):
    d, nan_ok = differing(got.detach().cpu(), want.detach().cpu())
    return d == 0 and nan_ok


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def raw_merge_backward(ext, dy, f, gate, df, dg, shape, g_size, ws=None, nbytes=0):
    """The C ABI on tensors (or views) as they are: nothing is made contiguous or aligned on the way."""
    st = ext._lib.rroi_merge_backward_hip(ext.dtype_code(dy.dtype), ptr(dy), ptr(f), ptr(gate), ptr(df), ptr(dg), *shape, *g_size,
                                          ptr(ws), nbytes, stream())
    torch.cuda.synchronize()
    return st


def raw_resize(ext, fn, src, dst, N, C, in_size, size):
    st = fn(ext.dtype_code(src.dtype), ptr(src), ptr(dst), N, C, *in_size, *size, stream())
    torch.cuda.synchronize()
    return st


def on_gpu(case, dtype):
    return tuple(None if t is None else t.cuda() for t in B.problem(case, dtype))


# ---------------------------------------------------------------- against the references
@pytest.mark.parametrize("dtype", B.DTYPES, ids=B.IDS)
@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_against_the_references_over_the_whole_table(ext, case, dtype):
    """The stand-alone forward and df differ in 0 elements; dx = R^T dy and dgate are within the bound of the case module,
    NaN positions equal, every element compared."""
    a, f, gate, dy = on_gpu(case, dtype)
    H, W = f.shape[2:]
    want_y, want_df, da_ref, dg_ref = B.reference(case, dtype)
    y = ext.resize_bilinear(a, (H, W))
    dx = ext.resize_bilinear_backward(dy, a.shape[2:])
    df, dg = ext.gated_merge_backward(dy, f, gate)
    assert y.shape == f.shape and dx.shape == a.shape and df.shape == f.shape
    assert all(t.dtype == dtype and t.is_contiguous() for t in (y, dx, df))
    d_y, nan_y = differing(y.cpu(), want_y)
    d_f, nan_f = differing(df.cpu(), want_df)
    ok_x, worst_x = da_ref.check(dx)
    ok_g, worst_g = (True, 0.0)
    if gate is None:
        assert dg is None
    else:
        assert dg.shape == gate.shape and dg.dtype == dtype
        ok_g, worst_g = dg_ref.check(dg)
    print(f"{B.case_id(case)} {dtype}: forward differing {d_y}, df differing {d_f} of {df.numel()}, "
          f"dx worst error / bound {worst_x:.4f}, dgate {worst_g:.4f}")
    assert d_y == 0 and nan_y and d_f == 0 and nan_f, (case, d_y, d_f)
    assert ok_x and ok_g, (case, worst_x, worst_g)


@pytest.mark.parametrize("case", [UPSCALE, DOWNSCALE, BLOCKS, SAME_GATE], ids=B.case_id)
@pytest.mark.parametrize("dtype", B.DTYPES, ids=B.IDS)
def test_partial_calls_give_the_full_calls_bits(ext, dtype, case):
    """need_df=False skips df's store, need_dgate=False the sums and the second launch; what is left has the full call's
    bits.  Without a gate df is dy.  An empty batch returns without a call."""
    a, f, gate, dy = on_gpu(case, dtype)
    df, dg = ext.gated_merge_backward(dy, f, gate)
    none, dg2 = ext.gated_merge_backward(dy, f, gate, need_df=False)
    df3, none3 = ext.gated_merge_backward(dy, f, gate, need_dgate=False)
    assert none is None and none3 is None and same_bits(dg2, dg) and same_bits(df3, df)
    df4, none4 = ext.gated_merge_backward(dy, f, None)
    assert none4 is None and same_bits(df4, dy)
    e = torch.zeros(0, f.size(1), 5, 7, dtype=dtype, device="cuda")
    dfe, dge = ext.gated_merge_backward(e, e, torch.zeros(0, 1, 3, 4, dtype=dtype, device="cuda"))
    assert dfe.shape == e.shape and dge.shape == (0, 1, 3, 4)
    assert ext.resize_bilinear(e, (9, 3)).shape == (0, f.size(1), 9, 3) and ext.resize_bilinear_backward(e, (2, 2)).shape == (0, f.size(1), 2, 2)


# ---------------------------------------------------------------- addresses, guards, workspace
@pytest.mark.parametrize("case", [B.CASES[1], B.CASES[2], DOWNSCALE], ids=B.case_id)
@pytest.mark.parametrize("dtype", B.DTYPES, ids=B.IDS)
def test_views_guards_and_workspace(ext, dtype, case):
    """dy, f, df and dx each 0 .. 3 elements past a 16-byte boundary through the raw ABI.  Nothing but the outputs' elements
    is written in their buffers and nothing but the queried bytes in the workspace's; every output element is written; what
    the workspace held before changes no bit, and neither do the offsets."""
    shape, a_size, g_size = case
    N, C, H, W = shape
    a, f, gate, dy = B.problem(case, dtype)
    want_y, want_df, da_ref, dg_ref = B.reference(case, dtype)
    itype = torch.int32 if dtype == torch.float32 else torch.int16
    need = ext.merge_backward_workspace_bytes(*shape, g_size, dtype=dtype)
    gg = gate.cuda()
    GUARD = 256
    first = None

    def view_of(t, off):
        buf = torch.zeros(t.numel() + 8, dtype=dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + t.numel()]
        v.copy_(t.reshape(-1))
        return v

    def guarded(n, off):
        buf = torch.full((64 + n + 64,), NAN_PATTERN[dtype], dtype=itype, device="cuda")
        return buf, buf.clone(), buf[64 + off:64 + off + n].view(dtype)

    def only_inside_written(buf, before, n, off, what):
        inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
        inside[64 + off:64 + off + n] = True
        assert torch.equal(buf[~inside], before[~inside]), f"a byte outside {what} was written"
        assert not (buf[inside] == before[inside]).any(), f"an element of {what} was left unwritten"

    for k, (od, of, oo, ox) in enumerate(((0, 0, 0, 0), (1, 1, 1, 1), (3, 3, 3, 3), (1, 0, 2, 3), (2, 3, 0, 1), (0, 2, 3, 2))):
        dv, fv, av = view_of(dy, od), view_of(f, of), view_of(a, ox)
        dfb, dfbefore, dfv = guarded(f.numel(), oo)
        dgb, dgbefore, dgv = guarded(gate.numel(), (oo + 1) % 4)
        dxb, dxbefore, dxv = guarded(a.numel(), ox)
        yb, ybefore, yv = guarded(f.numel(), (ox + 1) % 4)
        wsb = torch.full((GUARD + need + GUARD,), (0xFF, 0x00, 0xA5)[k % 3], dtype=torch.uint8, device="cuda")
        wsb[:GUARD], wsb[GUARD + need:] = 0x3C, 0x3C
        assert raw_merge_backward(ext, dv, fv, gg, dfv, dgv, shape, g_size, wsb[GUARD:GUARD + need], need) == 1
        assert raw_resize(ext, ext._lib.rroi_resize_backward_hip, dv, dxv, N, C, a_size, (H, W)) == 1
        assert raw_resize(ext, ext._lib.rroi_resize_forward_hip, av, yv, N, C, a_size, (H, W)) == 1
        only_inside_written(dfb, dfbefore, f.numel(), oo, "df")
        only_inside_written(dgb, dgbefore, gate.numel(), (oo + 1) % 4, "dgate")
        only_inside_written(dxb, dxbefore, a.numel(), ox, "dx")
        only_inside_written(yb, ybefore, f.numel(), (ox + 1) % 4, "y")
        assert bool((wsb[:GUARD] == 0x3C).all()) and bool((wsb[GUARD + need:] == 0x3C).all()), "a byte outside the workspace was written"
        assert torch.equal(dv.cpu(), dy.reshape(-1)) and torch.equal(fv.cpu(), f.reshape(-1)) and torch.equal(gg.cpu(), gate)
        assert same_bits(dfv.cpu().view(shape), want_df) and same_bits(yv.cpu().view(shape), want_y)
        assert da_ref.check(dxv.cpu().view(a.shape))[0] and dg_ref.check(dgv.cpu().view(gate.shape))[0], (od, of, oo, ox)
        got = (dgv.cpu().clone(), dxv.cpu().clone())
        first = got if first is None else first
        assert same_bits(got[0], first[0]) and same_bits(got[1], first[1]), (od, of, oo, ox)


def test_overlap_and_workspace_refusals_write_nothing_and_an_unneeded_workspace_is_left_alone(ext):
    case = B.CASES[1]
    shape, a_size, g_size = case
    a, f, gate, dy = on_gpu(case, torch.float32)
    want_y, want_df, da_ref, dg_ref = B.reference(case, torch.float32)
    need = ext.merge_backward_workspace_bytes(*shape, g_size)
    ws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    # df alone needs no workspace: NULL / 0 is accepted, and a buffer that is handed over is left alone
    df = torch.empty_like(f)
    assert raw_merge_backward(ext, dy, f, gate, df, None, shape, g_size, ws, need) == 1
    assert bool((ws == 0x5A).all())
    df2 = torch.empty_like(f)
    assert raw_merge_backward(ext, dy, f, gate, df2, None, shape, g_size, None, 0) == 1
    assert same_bits(df, df2) and same_bits(df, want_df)
    # without a gate df is dy's values
    df5 = torch.empty_like(f)
    assert raw_merge_backward(ext, dy, f, None, df5, None, shape, (1, 1), None, 0) == 1 and same_bits(df5, dy)
    # refused where the workspace is needed and is missing, misaligned or short -- and nothing is written then
    df3, dg3 = torch.full_like(f, 7.0), torch.full_like(gate, 7.0)
    ws.fill_(0x5A)
    assert raw_merge_backward(ext, dy, f, gate, df3, dg3, shape, g_size, None, 0) == 0
    assert raw_merge_backward(ext, dy, f, gate, df3, dg3, shape, g_size, ws[16:], need) == 0
    assert raw_merge_backward(ext, dy, f, gate, df3, dg3, shape, g_size, ws, need - 1) == 0
    assert raw_merge_backward(ext, dy, f, None, df3, dg3, shape, g_size, ws, need) == 0          # dgate without the gate
    # an output overlapping an input, or the other output
    both = torch.zeros(2 * f.numel(), device="cuda")
    both[:dy.numel()].copy_(dy.reshape(-1))
    keep = both.clone()
    n = f.numel()
    assert raw_merge_backward(ext, both[:n], f, gate, both[n - 1:2 * n - 1], dg3, shape, g_size, ws, need) == 0
    assert raw_merge_backward(ext, both[:n], f, gate, both[:n], None, shape, g_size, None, 0) == 0
    assert raw_merge_backward(ext, dy, f, gate, f, dg3, shape, g_size, ws, need) == 0
    assert raw_merge_backward(ext, dy, f, gate, df3, gate, shape, g_size, ws, need) == 0
    assert raw_merge_backward(ext, dy, f, gate, df3, df3.view(-1)[:gate.numel()], shape, g_size, ws, need) == 0
    N, C, H, W = shape
    assert raw_resize(ext, ext._lib.rroi_resize_backward_hip, both[:n], both[n - 1:], N, C, a_size, (H, W)) == 0
    assert raw_resize(ext, ext._lib.rroi_resize_forward_hip, both[:a.numel()], both[a.numel() - 1:], N, C, a_size, (H, W)) == 0
    assert torch.equal(both, keep) and bool((df3 == 7.0).all()) and bool((dg3 == 7.0).all()) and bool((ws == 0x5A).all())
    assert torch.equal(f.cpu(), B.problem(case, torch.float32)[1]) and torch.equal(gate.cpu(), B.problem(case, torch.float32)[2])


# ---------------------------------------------------------------- determinism, capture, special values
@pytest.mark.parametrize("case", [UPSCALE, BLOCKS, SAME_GATE], ids=B.case_id)
def test_two_calls_and_a_second_stream_give_identical_bits(ext, case):
    for dtype in (torch.float32, torch.bfloat16):
        a, f, gate, dy = on_gpu(case, dtype)
        run = lambda: ext.gated_merge_backward(dy, f, gate) + (ext.resize_bilinear_backward(dy, a.shape[2:]),)  # noqa: E731
        first, second = run(), run()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            third = run()
        side.synchronize()
        for x, y, z in zip(first, second, third):
            assert same_bits(x, y) and same_bits(x, z)


@pytest.mark.parametrize("case", [UPSCALE, BLOCKS], ids=B.case_id)
def test_graph_capture_reproduces_the_eager_bits(ext, case):
    """One linear chain -- merge forward, its backward, the resize and its backward -- captured on a side stream and
    replayed on changed inputs."""
    dtype = torch.bfloat16 if case is BLOCKS else torch.float32
    a, f, gate, dy = (t.clone() for t in on_gpu(case, dtype))
    size, a_size = tuple(f.shape[2:]), tuple(a.shape[2:])
    ext.gated_merge_backward(dy, f, gate)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            y = ext.gated_merge(a, f, gate)
            df, dg = ext.gated_merge_backward(dy, f, gate)
            r = ext.resize_bilinear(a, size)
            dx = ext.resize_bilinear_backward(dy, a_size)
    a2, f2, gate2, dy2 = B.random_case(case, dtype, seed=77)
    for t, t2 in ((a, a2), (f, f2), (gate, gate2), (dy, dy2)):       # the inputs change in place
        t.copy_(t2)
    for t in (y, df, dg, r, dx):
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want_df, want_dg = ext.gated_merge_backward(dy, f, gate)
    assert same_bits(y, ext.gated_merge(a, f, gate)) and same_bits(df, want_df) and same_bits(dg, want_dg)
    assert same_bits(r, ext.resize_bilinear(a, size)) and same_bits(dx, ext.resize_bilinear_backward(dy, a_size))
    assert same_bits(df, B.expected_df(dy2, gate2)) and same_bits(r, B.expected_resize(a2, *size))
    assert B.dx_reference(dy2, a_size).check(dx)[0] and B.dgate_reference(dy2, f2, gate2.shape[2:]).check(dg)[0]


@pytest.mark.parametrize("case", [UPSCALE, DOWNSCALE, SAME_GATE], ids=B.case_id)
def test_a_nan_in_dy_reaches_exactly_the_references_elements(ext, case):
    a, f, gate, dy = B.random_case(case, torch.float32)
    N, C, H, W = f.shape
    for Y, X in ((0, 0), (H - 1, W - 1), (H // 2, W // 2)):
        d = dy.clone()
        d[N - 1, C - 1, Y, X] = float("nan")
        df, dg = ext.gated_merge_backward(d.cuda(), f.cuda(), gate.cuda())
        dx = ext.resize_bilinear_backward(d.cuda(), a.shape[2:])
        assert same_bits(df, B.expected_df(d, gate)) and int(df.isnan().sum()) == 1
        rx, rg = B.dx_reference(d, a.shape[2:]), B.dgate_reference(d, f, gate.shape[2:])
        assert rx.check(dx)[0] and rg.check(dg)[0]
        nan = dx.cpu().isnan()
        assert 1 <= int(nan.sum()) <= 4 and int(nan.sum()) == int(nan[N - 1, C - 1].sum())   # its plane only, its taps only
        assert 1 <= int(dg.isnan().sum()) <= 4 and not bool(dg[:N - 1].isnan().any())


def test_an_infinity_beside_a_zero_weight_is_the_references_nan(ext):
    """Output pixel (0, 0) of an upscale gives weight 1 to source element (0, 0) and weight 0 to its three neighbours: no tap
    is skipped, so an infinity there is an infinity in one element and NaN in three, as the forward's 0 * inf is."""
    case = UPSCALE
    a, f, gate, dy = B.random_case(case, torch.float32)
    d = dy.clone()
    d[0, 1, 0, 0] = float("inf")
    dx = ext.resize_bilinear_backward(d.cuda(), a.shape[2:]).cpu()
    ref = B.dx_reference(d, a.shape[2:])
    assert ref.check(dx)[0]
    assert bool(dx[0, 1, 0, 0] == float("inf")) and bool(dx[0, 1, 0, 1].isnan()) and bool(dx[0, 1, 1, 0].isnan()) and bool(dx[0, 1, 1, 1].isnan())
    assert int(dx.isnan().sum()) == 3 and int(dx.isinf().sum()) == 1
    ff = f.clone()
    ff[0, 1, 0, 0] = 1.0
    df, dg = ext.gated_merge_backward(d.cuda(), ff.cuda(), gate.cuda())
    assert B.dgate_reference(d, ff, gate.shape[2:]).check(dg)[0] and int(dg.isnan().sum()) == 3 and int(dg.isinf().sum()) == 1
    assert same_bits(df, B.expected_df(d, gate))


# ---------------------------------------------------------------- autograd
@pytest.mark.parametrize("case", [UPSCALE, B.CASES[8], B.EXTRA[1]], ids=B.case_id)
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=["fp32", "bf16"])
def test_autograd_functions_under_deterministic_algorithms(ext, dtype, case):
    """rroi_align.merge: the forward's bits are the inference call's, the gradients are the raw calls', only what
    needs_input_grad wants is computed, a non-contiguous dy is taken, da is dy where a has f's size, and without any
    gradient needed it is the plain inference call.  All of it with torch.use_deterministic_algorithms(True)."""
    from rroi_align import merge
    a, f, gate, dy = on_gpu(case, dtype)
    a_size, size = tuple(a.shape[2:]), tuple(f.shape[2:])
    torch.use_deterministic_algorithms(True)
    try:
        ar, fr = a.clone().requires_grad_(True), f.clone().requires_grad_(True)
        gr = None if gate is None else gate.clone().requires_grad_(True)
        y = merge.gated_merge(ar, fr, gr)
        assert y.requires_grad and same_bits(y, ext.gated_merge(a, f, gate))
        y.backward(dy)
        want_da = dy if a_size == size else ext.resize_bilinear_backward(dy, a_size)
        want_df, want_dg = (dy, None) if gate is None else ext.gated_merge_backward(dy, f, gate)
        assert same_bits(ar.grad, want_da) and same_bits(fr.grad, want_df) and (gate is None or same_bits(gr.grad, want_dg))
        _, ref_df, ref_da, ref_dg = B.reference(case, dtype)
        assert same_bits(fr.grad, ref_df) and ref_da.check(ar.grad)[0] and (gate is None or ref_dg.check(gr.grad)[0])
        # the stand-alone resize
        xr = a.clone().requires_grad_(True)
        r = merge.bilinear_resize(xr, size)
        assert same_bits(r, ext.resize_bilinear(a, size))
        if r.requires_grad:
            r.backward(dy)
            assert same_bits(xr.grad, want_da)
        merge_calls, resize_calls = [], []
        run_m, run_r = merge.run_gated_merge_backward, merge.run_resize_bilinear_backward
        merge.run_gated_merge_backward = lambda *x: (merge_calls.append(x), run_m(*x))[1]
        merge.run_resize_bilinear_backward = lambda *x: (resize_calls.append(x), run_r(*x))[1]
        try:
            dyt = dy.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
            assert not dyt.is_contiguous() or min(size) == 1
            # only a: no merge-backward call; a resize-backward call only where a is resized
            ar2 = a.clone().requires_grad_(True)
            merge.gated_merge(ar2, f, gate).backward(dyt)
            assert not merge_calls and len(resize_calls) == int(a_size != size) and same_bits(ar2.grad, want_da)
            assert all(c[0].is_contiguous() for c in resize_calls)
            # only f
            fr3 = f.clone().requires_grad_(True)
            merge.gated_merge(a, fr3, gate).backward(dyt)
            assert len(resize_calls) == int(a_size != size) and same_bits(fr3.grad, want_df)
            if gate is None:
                assert not merge_calls
            else:
                assert len(merge_calls) == 1 and merge_calls[-1][0].is_contiguous() and merge_calls[-1][3:] == (True, False)
                # only the gate
                gr4 = gate.clone().requires_grad_(True)
                merge.gated_merge(a, f, gr4).backward(dy)
                assert len(merge_calls) == 2 and merge_calls[-1][3:] == (False, True) and same_bits(gr4.grad, want_dg)
            # no gradient needed: the plain call, nothing saved
            n = len(merge_calls) + len(resize_calls)
            y5 = merge.gated_merge(a, f, gate)
            with torch.no_grad():
                y6, r6 = merge.gated_merge(ar, fr, gr), merge.bilinear_resize(xr, size)
            assert y5.grad_fn is None and y6.grad_fn is None and r6.grad_fn is None and same_bits(y5, y) and same_bits(y6, y)
            assert len(merge_calls) + len(resize_calls) == n
        finally:
            merge.run_gated_merge_backward, merge.run_resize_bilinear_backward = run_m, run_r
    finally:
        torch.use_deterministic_algorithms(False)


# ---------------------------------------------------------------- in the network
def small_net(dtype, attention=True):
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    return deterministic_init(FOTSNet(attention=attention)).train().cuda().to(dtype)


def feature_maps(dtype, seed=11):
    """Leaf tensors of a 64 x 96 image's feature sizes (1/4 .. 1/32), 256 channels, that require gradients."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, 256, h, w, generator=g).cuda().to(dtype).requires_grad_(True) for h, w in ((16, 24), (8, 12), (4, 6), (2, 3))]


def record_backward_calls(monkeypatch):
    from rroi_align import merge
    merges, resizes = [], []
    run_m, run_r = merge.run_gated_merge_backward, merge.run_resize_bilinear_backward

    def rec_m(*x):
        out = run_m(*x)
        merges.append((x, out))
        return out

    def rec_r(*x):
        out = run_r(*x)
        resizes.append((x, out))
        return out
    monkeypatch.setattr(merge, "run_gated_merge_backward", rec_m)
    monkeypatch.setattr(merge, "run_resize_bilinear_backward", rec_r)
    return merges, resizes


def refuse_interpolate(*a, **k):
    raise AssertionError("the stock resize was called")


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=["fp32", "bf16"])
def test_the_networks_merge_trains_without_the_stock_resize_under_deterministic_algorithms(ext, dtype, monkeypatch):
    """`net._merge` of a FOTSNet in training mode with `F.interpolate` patched to raise, under deterministic algorithms:
    it completes, makes exactly three merge-backward and three resize-backward calls (the two stand-alone resizes and `da`
    of the first merge), each within its bound on its own recorded tensors, and two runs agree bit for bit."""
    from fots_e2e.native import use_native_merge
    from fots_e2e.native_train import TrainableMergeFOTSNet, use_trainable_merge
    net = small_net(dtype)
    assert use_native_merge(net) and use_trainable_merge(net) and type(net) is TrainableMergeFOTSNet
    merges, resizes = record_backward_calls(monkeypatch)
    stock = F.interpolate
    monkeypatch.setattr(F, "interpolate", refuse_interpolate)
    g = torch.Generator().manual_seed(12)
    d1, d2 = (torch.randn(1, 256, h, w, generator=g).cuda().to(dtype) for h, w in ((16, 24), (8, 12)))
    torch.use_deterministic_algorithms(True)
    try:
        grads = []
        for _ in range(2):
            fs = feature_maps(dtype)
            net.zero_grad(set_to_none=True)
            m1, m2 = net._merge(*fs)
            assert m1.shape == fs[0].shape and m2.shape == fs[1].shape
            torch.autograd.backward([m1, m2], [d1, d2])
            torch.cuda.synchronize()
            grads.append([t.grad.clone() for t in fs] + [p.grad.clone() for p in net.conv_attenton.parameters()]
                         + [m1.detach().clone(), m2.detach().clone()])
        assert all(same_bits(x, y) for x, y in zip(*grads))
        assert all(bool(t.isfinite().all()) for t in grads[0])
    finally:
        torch.use_deterministic_algorithms(False)
    assert len(merges) == 6 and len(resizes) == 6                     # two runs of three and three
    worst = 0.0
    for (dy, f, gate, need_df, need_dg), (df, dg) in merges[:3]:
        assert need_df and need_dg and dy.dtype == f.dtype == gate.dtype == dtype and gate.size(1) == 1
        assert same_bits(df, B.expected_df(dy, gate))
        ok, ratio = B.dgate_reference(dy, f, gate.shape[2:]).check(dg)
        worst = max(worst, ratio)
        assert ok, (tuple(f.shape), ratio)
    for (dy, h, w), dx in resizes[:3]:
        ok, ratio = B.dx_reference(dy, (h, w)).check(dx)
        worst = max(worst, ratio)
        assert ok, (tuple(dy.shape), h, w, ratio)
    assert sorted((tuple(dy.shape[2:]), (h, w)) for (dy, h, w), _ in resizes[:3]) == \
        [((4, 6), (2, 3)), ((8, 12), (4, 6)), ((16, 24), (8, 12))]
    print(f"{dtype}: three merge and three resize backward calls, worst error / bound {worst:.4f}")
    # enable=False restores today's behaviour: the stock path is called
    monkeypatch.setattr(F, "interpolate", stock)
    assert use_trainable_merge(net, enable=False)
    monkeypatch.setattr(F, "interpolate", refuse_interpolate)
    with pytest.raises(AssertionError, match="stock resize"):
        net._merge(*feature_maps(dtype))
    assert len(merges) == 6 and len(resizes) == 6


def test_the_fall_backs_take_the_stock_path(ext, monkeypatch):
    """Autocast, channels-last maps and a network without gradients needed keep the path they have today; a network without
    attention merges natively without a gate."""
    from fots_e2e.native import use_native_merge
    from fots_e2e.native_train import use_trainable_merge
    net = small_net(torch.float32)
    assert use_native_merge(net) and use_trainable_merge(net)
    merges, resizes = record_backward_calls(monkeypatch)
    fs = feature_maps(torch.float32)
    want = [t.detach().clone() for t in net._merge(*fs)]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        m1, m2 = net._merge(*feature_maps(torch.float32))
    (m1.float().sum() + m2.float().sum()).backward()
    cl = [t.detach().to(memory_format=torch.channels_last).requires_grad_(True) for t in feature_maps(torch.float32)]
    m1, m2 = net._merge(*cl)
    (m1.sum() + m2.sum()).backward()
    assert not merges and not resizes and torch.allclose(m1, want[0], rtol=1e-4, atol=1e-4)
    with monkeypatch.context() as mp:
        mp.setattr(F, "interpolate", refuse_interpolate)
        with pytest.raises(AssertionError, match="stock resize"):
            net._merge(*cl)
        # no gradient needed in training mode: the parent's method, which is the stock one in training mode
        for p in net.parameters():
            p.requires_grad_(False)
        with pytest.raises(AssertionError, match="stock resize"):
            net._merge(*(t.detach() for t in fs))
    plain = small_net(torch.float32, attention=False)
    assert use_native_merge(plain) and use_trainable_merge(plain)
    with monkeypatch.context() as mp:
        mp.setattr(F, "interpolate", refuse_interpolate)
        fs = feature_maps(torch.float32)
        m1, m2 = plain._merge(*fs)
        (m1.sum() + m2.sum()).backward()
    assert not merges and len(resizes) == 3 and all(t.grad is not None for t in fs)   # ungated: df is dy, no merge-backward call


@pytest.mark.parametrize("deterministic", (False, True), ids=["default", "deterministic"])
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=["fp32", "bf16"])
def test_one_training_step_of_the_network(ext, dtype, deterministic, monkeypatch):
    """FOTSNet in train mode on a 64 x 96 image and 11 x 24 crops with the three trainable switches on: one forward +
    forward_ocr + a scalar loss + backward makes three merge-backward and three resize-backward calls, and at least nine
    parameters in ten have a finite gradient.  In default mode and under torch.use_deterministic_algorithms(True): with the
    three switches on no operator of the pass raises there."""
    from fots_e2e.native import use_native_depthwise, use_native_instancenorm, use_native_merge
    from fots_e2e.native_train import use_trainable_depthwise, use_trainable_instancenorm, use_trainable_merge
    net = small_net(dtype)
    image = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(7)).cuda().to(dtype)
    crops = torch.randn(3, 64, 11, 24, generator=torch.Generator().manual_seed(8)).cuda().to(dtype)
    use_native_instancenorm(net)
    assert use_trainable_instancenorm(net) > 0
    assert use_native_depthwise(net) == 22 and use_trainable_depthwise(net) == 22
    assert use_native_merge(net) and use_trainable_merge(net)
    merges, resizes = record_backward_calls(monkeypatch)
    torch.use_deterministic_algorithms(deterministic)
    try:
        with monkeypatch.context() as mp:
            mp.setattr(F, "interpolate", refuse_interpolate)
            outs = [t for group in net(image) for t in group] + [net.forward_ocr(crops)]
            loss = sum((t.float() * torch.linspace(-1, 1, t.numel(), device="cuda").view_as(t)).sum() for t in outs)
            loss.backward()
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(False)
    assert len(merges) == 3 and len(resizes) == 3
    for (dy, f, gate, need_df, need_dg), (df, dg) in merges:
        assert need_df and need_dg and same_bits(df, B.expected_df(dy, gate))
        assert B.dgate_reference(dy, f, gate.shape[2:]).check(dg)[0]
    for (dy, h, w), dx in resizes:
        assert B.dx_reference(dy, (h, w)).check(dx)[0]
    with_grad = [p for p in net.parameters() if p.grad is not None]
    assert len(with_grad) >= 0.9 * len(list(net.parameters()))
    assert all(bool(p.grad.isfinite().all()) for p in with_grad)
    assert all(p.grad is not None for p in net.conv_attenton.parameters())
