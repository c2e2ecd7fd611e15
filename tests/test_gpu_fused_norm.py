"""GPU (MI355X): the fused InstanceNorm epilogues -- the residual add of a block's tail and the stem's mirror
-- against the reference of fused_norm_cases.py over the case table of instancenorm_cases.py, against the plain kernel
bit for bit where the contract says so, special values, misaligned views with guards, determinism and capture, and the
wiring of `use_native_blocks` in the network."""
import pytest
import torch

import fused_norm_cases as FN
import instancenorm_cases as I
from test_gpu_bucketed import NAN_PATTERN

pytestmark = pytest.mark.gpu

PLANE_ODD, SPLIT_ODD = (2, 3, 7, 9), (1, 2, 99, 331)      # odd planes: the base alignment changes from plane to plane


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def raw_call(ext, x, gamma, beta, r, y, shape, mirror, slope, ws=None, nbytes=0, eps=I.EPS):
    """The C ABI on tensors (or views) as they are: nothing is made contiguous or aligned on the way."""
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    st = ext._lib.rroi_instancenorm_fused_forward_hip(
        ext.dtype_code(x.dtype), ptr(x), ptr(gamma), ptr(beta), ptr(r), ptr(y), *shape, int(mirror), eps, slope, ptr(ws), nbytes,
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def same_bits(got, want):
    d, nan_ok = I.differing(got.cpu(), want.cpu())
    return d == 0 and nan_ok


def activate(t, slope):
    return torch.where(t < 0, t * torch.tensor(slope, dtype=torch.float32, device=t.device).to(t.dtype), t)


# ---------------------------------------------------------------- 1. residual against the reference
@pytest.mark.parametrize("dtype", I.DTYPES, ids=I.IDS)
def test_residual_against_the_reference_over_the_whole_table(ext, dtype):
    """Every case x affine on / off x slope {1, 0, 0.01}, r = N(0, 1) rounded to the type:
    (a) every finite element within bound(x, a, b) + 2 u |r| of the float64 value, NaN positions equal;
    (b) over the whole table at most 1 element in 10^4, of at least 10^6, differs in bits from the rounded reference."""
    total = differ = 0
    for shape in I.CASES:
        x, gamma, beta, stats = I.problem(shape, dtype)
        r = FN.residual_of(shape, dtype)
        xg, gg, bg, rg = x.cuda(), gamma.cuda(), beta.cuda(), r.cuda()
        for affine in (True, False):
            g, bt = (gamma, beta) if affine else (None, None)
            for slope in I.SLOPES:
                got = (ext.instance_norm_fused(xg, gg, bg, I.EPS, slope, residual=rg) if affine
                       else ext.instance_norm_fused(xg, eps=I.EPS, negative_slope=slope, residual=rg)).cpu()
                want, ref64, a, b = FN.reference(x, g, bt, I.EPS, slope, stats, r)
                assert got.shape == want.shape and got.dtype == dtype and got.is_contiguous()
                d, nan_ok = I.differing(got, want)
                ok, worst = FN.within_bound(got, ref64, x, a, b, r)
                print(f"{I.case_id(shape)} affine={affine} slope={slope}: {d} of {got.numel()} differ, worst error / bound {worst:.3f}")
                assert nan_ok, (shape, affine, slope)
                assert ok, (shape, affine, slope, worst)
                total += got.numel()
                differ += d
    print(f"{dtype}: {differ} of {total} elements differ in bits from the reference")
    assert total >= 10 ** 6 and differ * 10 ** 4 <= total, (differ, total)


# ---------------------------------------------------------------- 2. residual, fp32, no tolerance
def test_residual_fp32_equals_the_plain_kernel_plus_torch(ext):
    """The statistics pass is shared with the plain kernel and the epilogue is fp32 arithmetic torch can repeat: nothing
    may differ."""
    for shape in I.CASES:
        x, gamma, beta, _ = I.problem(shape, torch.float32)
        xg, gg, bg, rg = x.cuda(), gamma.cuda(), beta.cuda(), FN.residual_of(shape, torch.float32).cuda()
        t = ext.instance_norm(xg, gg, bg, I.EPS, 1.0) + rg
        for slope in I.SLOPES:
            got = ext.instance_norm_fused(xg, gg, bg, I.EPS, slope, residual=rg)
            assert same_bits(got, activate(t, slope)), (shape, slope)


# ---------------------------------------------------------------- 3. mirror against the reference
@pytest.mark.parametrize("dtype", I.DTYPES, ids=I.IDS)
def test_mirror_against_the_reference_over_the_whole_table(ext, dtype):
    """The same (a) and (b) on the 2C output planes, the reference being that of cat(x, -x)."""
    total = differ = 0
    for shape in I.CASES:
        x, x2, gamma, beta, stats = FN.mirror_problem(shape, dtype)
        xg, gg, bg = x.cuda(), gamma.cuda(), beta.cuda()
        for affine in (True, False):
            g, bt = (gamma, beta) if affine else (None, None)
            for slope in I.SLOPES:
                got = (ext.instance_norm_fused(xg, gg, bg, I.EPS, slope, mirror=True) if affine
                       else ext.instance_norm_fused(xg, eps=I.EPS, negative_slope=slope, mirror=True)).cpu()
                want, ref64, a, b = FN.reference(x2, g, bt, I.EPS, slope, stats)
                assert got.shape == want.shape == x2.shape and got.dtype == dtype and got.is_contiguous()
                d, nan_ok = I.differing(got, want)
                ok, worst = FN.within_bound(got, ref64, x2, a, b)
                print(f"{I.case_id(shape)} affine={affine} slope={slope}: {d} of {got.numel()} differ, worst error / bound {worst:.3f}")
                assert nan_ok, (shape, affine, slope)
                assert ok, (shape, affine, slope, worst)
                total += got.numel()
                differ += d
    print(f"{dtype}: {differ} of {total} elements differ in bits from the reference")
    assert total >= 10 ** 6 and differ * 10 ** 4 <= total, (differ, total)


# ---------------------------------------------------------------- 4. mirror, no tolerance
@pytest.mark.parametrize("dtype", I.DTYPES, ids=I.IDS)
def test_mirror_equals_the_plain_kernel_on_the_concatenated_tensor(ext, dtype):
    """Where every plane of x and of cat(x, -x) starts on a 16-byte boundary and both shapes plan alike, the plain kernel
    adds the concatenated tensor's planes in the order the fused one adds x's: the same bits."""
    chosen = [s for s in I.CASES if FN.mirror_is_exact_case(s, dtype)]
    forms = {I.plan_of(*s)[0] for s in chosen}
    assert forms == {I.PLANE, I.SPLIT}, (dtype, chosen)
    for shape in chosen:
        x, x2, gamma, beta, _ = FN.mirror_problem(shape, dtype)
        N, C, H, W = shape
        p1, p2 = ext.instance_norm_plan(N, C, H, W, dtype=dtype), ext.instance_norm_plan(N, 2 * C, H, W, dtype=dtype)
        assert (p1.form, p1.segment_elems) == (p2.form, p2.segment_elems) == (I.plan_of(*shape)[0], I.plan_of(*shape)[2])
        xg, gg, bg = x.cuda(), gamma.cuda(), beta.cuda()
        cat = torch.cat((xg, -xg), 1)
        assert xg.data_ptr() % 16 == 0 and cat.data_ptr() % 16 == 0
        for slope in I.SLOPES:
            assert same_bits(ext.instance_norm_fused(xg, gg, bg, I.EPS, slope, mirror=True),
                             ext.instance_norm(cat, gg, bg, I.EPS, slope)), (shape, slope)
        assert same_bits(ext.instance_norm_fused(xg, eps=I.EPS, negative_slope=0.01, mirror=True),
                         ext.instance_norm(cat, eps=I.EPS, negative_slope=0.01)), shape


def test_empty_batch_returns_without_a_call(ext):
    x = torch.zeros(0, 4, 9, 9, device="cuda")
    assert ext.instance_norm_fused(x, residual=x).shape == (0, 4, 9, 9)
    assert ext.instance_norm_fused(x, mirror=True).shape == (0, 8, 9, 9)


def test_neither_residual_nor_mirror_is_the_plain_call(ext):
    for shape in (PLANE_ODD, SPLIT_ODD):
        x, gamma, beta, _ = I.problem(shape, torch.bfloat16)
        xg, gg, bg = x.cuda(), gamma.cuda(), beta.cuda()
        y = torch.empty_like(xg)
        need = ext.instance_norm_workspace_bytes(*shape)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda") if need else None
        assert raw_call(ext, xg, gg, bg, None, y, shape, 0, 0.01, ws, need) == 1
        assert same_bits(y, ext.instance_norm(xg, gg, bg, I.EPS, 0.01))
        assert same_bits(y, ext.instance_norm_fused(xg, gg, bg, I.EPS, 0.01))


# ---------------------------------------------------------------- 5. special values
@pytest.mark.parametrize("shape", [PLANE_ODD, SPLIT_ODD], ids=["plane", "split"])
@pytest.mark.parametrize("dtype", I.DTYPES, ids=I.IDS)
def test_special_values(ext, dtype, shape):
    """A NaN and an infinity in r touch their own elements only; a NaN in a plane of x takes that plane -- under mirror
    that plane and its twin -- and no other."""
    N, C, H, W = shape
    n = H * W
    x, gamma, beta = I.random_problem(shape, dtype, seed=5)
    r = FN.residual_of(shape, dtype).clone()
    rp = r.view(N * C, n)
    rp[0, 3], rp[1, 0], rp[1, n - 1] = float("nan"), float("inf"), -float("inf")
    for slope in (1.0, 0.01):
        got = ext.instance_norm_fused(x.cuda(), gamma.cuda(), beta.cuda(), I.EPS, slope, residual=r.cuda()).cpu()
        want, ref64, a, b = FN.reference(x, gamma, beta, I.EPS, slope, None, r)
        assert torch.equal(got.isnan(), r.isnan()) and torch.equal(got.isinf(), r.isinf())
        assert float(got.view(N * C, n)[1, 0]) == float("inf")
        assert float(got.view(N * C, n)[1, n - 1]) == -float("inf")
        assert I.differing(got, want)[1] and FN.within_bound(got, ref64, x, a, b, r)[0]
    # a NaN in x: plane 1 of image 0 (and, mirrored, its twin C + 1)
    xn = x.clone()
    xn[0, 1, H // 2, W // 3] = float("nan")
    r = FN.residual_of(shape, dtype)
    got = ext.instance_norm_fused(xn.cuda(), gamma.cuda(), beta.cuda(), I.EPS, 0.01, residual=r.cuda()).cpu()
    nan_planes = got.view(N * C, n).isnan()
    assert [bool(p.all()) for p in nan_planes] == [p == 1 for p in range(N * C)] and int(nan_planes.sum()) == n
    _, _, g2, b2, _ = FN.mirror_problem(shape, dtype)
    got = ext.instance_norm_fused(xn.cuda(), g2.cuda(), b2.cuda(), I.EPS, 0.01, mirror=True).cpu()
    nan_planes = got.view(N * 2 * C, n).isnan()
    assert [bool(p.all()) for p in nan_planes] == [p in (1, C + 1) for p in range(N * 2 * C)] and int(nan_planes.sum()) == 2 * n
    want, ref64, a, b = FN.reference(FN.mirrored(xn), g2, b2, I.EPS, 0.01)
    assert I.differing(got, want)[1] and FN.within_bound(got, ref64, FN.mirrored(xn), a, b)[0]


def test_fp32_subnormals_in_x_and_r_are_kept(ext):
    shape = (2, 3, 7, 9)
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * 2.0 ** -130).float()
    assert float(x.abs().max()) < 2.0 ** -126 and int((x != 0).sum()) > x.numel() // 2
    eps = 1e-80                                         # the planes' variance is about 2^-260: eps must not drown it
    r = FN.residual_of(shape, torch.float32)
    for slope in (1.0, 0.01):
        got = ext.instance_norm_fused(x.cuda(), eps=eps, negative_slope=slope, residual=r.cuda()).cpu()
        want, ref64, a, b = FN.reference(x, None, None, eps, slope, None, r)
        assert FN.within_bound(got, ref64, x, a, b, r)[0]      # (flushed inputs give a constant plane: off by its whole spread)
        got = ext.instance_norm_fused(x.cuda(), eps=eps, negative_slope=slope, mirror=True).cpu()
        want, ref64, a, b = FN.reference(FN.mirrored(x), None, None, eps, slope)
        assert float(want.abs().max()) > 0.5 and FN.within_bound(got, ref64, FN.mirrored(x), a, b)[0]
    # a subnormal residual on a zero map: gamma = beta = 0, so y = act(0 + r) = act(r), exactly
    x, gamma, beta = I.random_problem(shape, torch.float32, seed=9)
    rs = (torch.randn(shape, generator=g, dtype=torch.float64) * 2.0 ** -130).float()
    assert float(rs.abs().max()) < 2.0 ** -126
    got = ext.instance_norm_fused(x.cuda(), (gamma * 0).cuda(), (beta * 0).cuda(), I.EPS, 1.0, residual=rs.cuda()).cpu()
    assert int((got != 0).sum()) > got.numel() // 2 and torch.equal(got, rs + 0.0)


# ---------------------------------------------------------------- 6. views and guards
OFFSETS = ((0, 0, 0, 0), (1, 1, 1, 1), (2, 0, 2, 3), (0, 3, 1, 2), (3, 2, 0, 1), (1, 0, 3, 0), (2, 2, 3, 2), (3, 3, 3, 3))


@pytest.mark.parametrize("mirror", [False, True], ids=["residual", "mirror"])
@pytest.mark.parametrize("shape", [PLANE_ODD, SPLIT_ODD], ids=["plane", "split"])
@pytest.mark.parametrize("dtype", I.DTYPES, ids=I.IDS)
def test_views_and_guards(ext, dtype, shape, mirror):
    """x, r and y 0 .. 3 elements past a 16-byte boundary, independently of one another, and the workspace 0 .. 3 times
    256 bytes into its buffer (the call refuses a workspace anywhere else), through the raw ABI.  Nothing but y's elements
    is written in y's buffer and nothing but the queried bytes in the workspace's; the results stay within (a).  Under
    mirror the two output planes of an odd plane differ in alignment: the two-pass path, asserted through the addresses."""
    N, C, H, W = shape
    n_in = N * C * H * W
    if mirror:
        x, x2, gamma, beta, stats = FN.mirror_problem(shape, dtype)
        r = None
        want, ref64, a, b = FN.reference(x2, gamma, beta, I.EPS, 0.01, stats)
        bx, n_out = x2, 2 * n_in
    else:
        x, gamma, beta, stats = I.problem(shape, dtype)
        r = FN.residual_of(shape, dtype)
        want, ref64, a, b = FN.reference(x, gamma, beta, I.EPS, 0.01, stats, r)
        bx, n_out = x, n_in
    itype = torch.int32 if dtype == torch.float32 else torch.int16
    size = x.element_size()
    need = ext.instance_norm_workspace_bytes(*shape)            # x's shape in both modes
    assert (need > 0) == (I.plan_of(*shape)[0] == I.SPLIT)
    gg, bg = gamma.cuda(), beta.cuda()
    GUARD = 1024
    by_x_offset = {}
    for k, (ox, orr, oy, ow) in enumerate(OFFSETS):
        xb = torch.zeros(n_in + 8, dtype=dtype, device="cuda")
        xv = xb[ox:ox + n_in]
        xv.copy_(x.reshape(-1))
        rv = None
        if r is not None:
            rb = torch.zeros(n_in + 8, dtype=dtype, device="cuda")
            rv = rb[orr:orr + n_in]
            rv.copy_(r.reshape(-1))
            assert rb.data_ptr() % 16 == 0 and rv.data_ptr() == rb.data_ptr() + orr * size
        buf = torch.full((64 + n_out + 64,), NAN_PATTERN[dtype], dtype=itype, device="cuda")
        before = buf.clone()
        yv = buf[64 + oy:64 + oy + n_out].view(dtype)
        assert xb.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0 and yv.data_ptr() == buf.data_ptr() + (64 + oy) * size
        if mirror:                                              # planes (0, 0) and (0, C) of y: another offset from a boundary
            assert (yv.data_ptr() % 16) != ((yv.data_ptr() + C * H * W * size) % 16)
        wsb = torch.full((GUARD + need + GUARD,), (0xFF, 0x00, 0xA5)[k % 3], dtype=torch.uint8, device="cuda")
        lo = 256 * ow
        wsb[:lo], wsb[lo + need:] = 0x3C, 0x3C
        ws = wsb[lo:lo + need] if need else None
        assert ws is None or ws.data_ptr() % 256 == 0
        assert raw_call(ext, xv, gg, bg, rv, yv, shape, mirror, 0.01, ws, need) == 1
        inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
        inside[64 + oy:64 + oy + n_out] = True
        assert torch.equal(buf[~inside], before[~inside]), "a byte outside y was written"
        assert not (buf[inside] == before[inside]).any(), "an element of y was left unwritten"
        assert bool((wsb[:lo] == 0x3C).all()) and bool((wsb[lo + need:] == 0x3C).all()), "a byte outside the workspace was written"
        assert bool((xb[:ox] == 0).all()) and bool((xb[ox + n_in:] == 0).all()) and torch.equal(xv.cpu(), x.reshape(-1))
        if r is not None:
            assert bool((rb[:orr] == 0).all()) and bool((rb[orr + n_in:] == 0).all()) and torch.equal(rv.cpu(), r.reshape(-1))
        got = yv.cpu().view(bx.shape)
        ok, worst = FN.within_bound(got, ref64, bx, a, b, r)
        assert I.differing(got, want)[1] and ok, (ox, orr, oy, ow, worst)
        # the sums follow x's address alone: the same x offset gives the same bits whatever the other three are
        assert same_bits(got, by_x_offset.setdefault(ox, got)), (ox, orr, oy, ow)
    assert len(by_x_offset) == 4


# ---------------------------------------------------------------- 7. determinism, streams, capture
def _call(ext, shape, dtype, mirror):
    if mirror:
        x, _, gamma, beta, _ = FN.mirror_problem(shape, dtype)
        x, gamma, beta = x.cuda(), gamma.cuda(), beta.cuda()
        return x, lambda: ext.instance_norm_fused(x, gamma, beta, I.EPS, 0.01, mirror=True)
    x, gamma, beta, _ = I.problem(shape, dtype)
    x, gamma, beta, r = x.cuda(), gamma.cuda(), beta.cuda(), FN.residual_of(shape, dtype).cuda()
    return x, lambda: ext.instance_norm_fused(x, gamma, beta, I.EPS, 0.01, residual=r)


@pytest.mark.parametrize("mirror", [False, True], ids=["residual", "mirror"])
@pytest.mark.parametrize("shape", [(3, 5, 24, 40), (2, 2, 128, 257)], ids=["plane", "split"])
def test_two_calls_and_a_second_stream_give_identical_bits(ext, shape, mirror):
    for dtype in (torch.float32, torch.bfloat16):
        _, call = _call(ext, shape, dtype, mirror)
        first, second = call(), call()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            third = call()
        side.synchronize()
        assert same_bits(first, second) and same_bits(first, third)


@pytest.mark.parametrize("mirror", [False, True], ids=["residual", "mirror"])
@pytest.mark.parametrize("shape", [(3, 5, 24, 40), (2, 2, 128, 257)], ids=["plane", "split"])
def test_graph_capture_reproduces_the_eager_bits(ext, shape, mirror):
    """One call captured on a single stream (no parallel branches), replayed after x changed in place."""
    dtype = torch.bfloat16 if shape[0] == 3 else torch.float32
    x, call = _call(ext, shape, dtype, mirror)
    call()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = call()
    x.copy_(I.random_problem(shape, dtype, seed=77)[0])          # x changes in place
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, call())


# ---------------------------------------------------------------- 8. wiring
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=["fp32", "bf16"])
def test_the_network_makes_19_fused_calls(ext, dtype, monkeypatch):
    """One forward of the switched FOTSNet on a 1 x 3 x 64 x 96 input: 2 mirror calls (slope 0.01) and 17 residual calls
    (0.0 for the seven plain blocks, 0.01 for the ten separable ones); the residual is the block's input where the block
    has no shortcut branch; every block returns the call's output; every call satisfies property 2 (fp32) or condition (a).
    With the predicate forced false and the fused call made to raise, the network still runs and gives the stock bits."""
    import fots_e2e.native as native
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    # The stock 1 x 1 convolutions of layer3 / layer4 at this size do not repeat their own bits from pass to pass (the
    # stock network differs from itself); with deterministic algorithms asked for they do, and the comparison of the
    # fallback with the stock network means something.
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    net = deterministic_init(FOTSNet()).eval().cuda().to(dtype)
    image = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(7)).cuda().to(dtype)
    with torch.no_grad():
        first = net(image)
        stock = net(image)
    assert all(torch.equal(s, t) for u, v in zip(first, stock) for s, t in zip(u, v)), "the stock network does not repeat its bits"
    assert native.use_native_blocks(net) == (2, 7, 10)
    calls = []
    run = ext._instance_norm_fused_run

    def recording(x, weight, bias, eps, slope, residual, mirror):
        out = run(x, weight, bias, eps, slope, residual, mirror)
        calls.append(dict(x=x, weight=weight, bias=bias, eps=eps, slope=slope, residual=residual, mirror=mirror, out=out))
        return out
    monkeypatch.setattr(ext, "_instance_norm_fused_run", recording)
    seen = []
    kinds = (native.NativeMirrorNorm, native.NativePlainBlock, native.NativeSeparableBlock)
    hooks = [m.register_forward_hook(lambda mod, inp, out: seen.append((mod, inp[0], out)))
             for m in net.modules() if type(m) in kinds]
    with torch.no_grad():
        net(image)
    for h in hooks:
        h.remove()
    assert len(calls) == 19 == len(seen)
    assert sum(c["mirror"] for c in calls) == 2 and sum(c["residual"] is not None for c in calls) == 17
    shortcuts = 0
    for c, (mod, xin, out) in zip(calls, seen):          # a block's one fused call is its last step: the same order
        assert out is c["out"], type(mod)
        if type(mod) is native.NativeMirrorNorm:
            assert c["mirror"] and c["residual"] is None and c["slope"] == 0.01 and c["x"] is xin
            assert out.shape == (xin.size(0), 2 * xin.size(1)) + xin.shape[2:]
            continue
        assert not c["mirror"] and c["slope"] == (0.0 if type(mod) is native.NativePlainBlock else 0.01)
        if mod.downsample is None:
            assert c["residual"].data_ptr() == xin.data_ptr()
        else:
            shortcuts += 1
            assert c["residual"].shape == out.shape and c["residual"].data_ptr() != xin.data_ptr()
    assert shortcuts == 3
    assert [c["slope"] for c in calls].count(0.0) == 7 and [c["slope"] for c in calls].count(0.01) == 12
    for c in calls:
        x, w, b, r = c["x"], c["weight"], c["bias"], c["residual"]
        if c["mirror"] or dtype != torch.float32:
            xc = FN.mirrored(x.cpu()) if c["mirror"] else x.cpu()
            rc = None if r is None else r.cpu()
            want, ref64, ca, cb = FN.reference(xc, w.detach().cpu(), b.detach().cpu(), c["eps"], c["slope"], None, rc)
            ok, worst = FN.within_bound(c["out"].cpu(), ref64, xc, ca, cb, rc)
            assert I.differing(c["out"].cpu(), want)[1] and ok, worst
        else:
            t = ext.instance_norm(x, w.detach(), b.detach(), c["eps"], 1.0) + r
            assert same_bits(c["out"], activate(t, c["slope"]))
    # the fallback: no predicate holds, the fused call raises -- the stock forward runs
    def refuse(*a, **k):
        raise AssertionError("the fused call was made")
    monkeypatch.setattr(ext, "_instance_norm_fused_run", refuse)
    with torch.no_grad():
        with pytest.raises(AssertionError, match="fused call was made"):
            net(image)
        monkeypatch.setattr(native, "fused_norm_ok", lambda *a, **k: False)
        fallback = net(image)
    for u, v in zip(stock, fallback):
        for s, t in zip(u, v):
            assert torch.equal(s, t)
