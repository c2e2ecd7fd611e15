"""CPU: the merge-backward and resize entry points (header section 8b) are exported, declared and
host-checked; `rroi_resize_footprint` is the definition's set for every source index; the plan and workspace queries agree
with the case module's mirror of the host rules; the Python surface raises what it documents; `use_trainable_merge` /
`trainable_merge_ok` do what fots_e2e.native_train says; the tests' references are pinned against torch's float64 autograd.
No kernel is launched here."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import merge_backward_cases as B
import merge_cases as M
from test_abi import declared_functions
from test_depthwise_abi import fake_cuda

NAMES = ("rroi_resize_forward_hip", "rroi_resize_backward_hip", "rroi_resize_footprint", "rroi_resize_backward_plan",
         "rroi_merge_backward_hip", "rroi_merge_backward_workspace_bytes", "rroi_merge_backward_plan")
P = 0x7f0000000000   # non-null, a multiple of 256, never dereferenced: every call below is refused on the host
FAR = 1 << 32        # between two fake tensors: they do not overlap
NETWORK = (((1, 256, 44, 80), (22, 40)), ((1, 256, 88, 160), (44, 80)), ((1, 256, 176, 320), (88, 160)),
           ((8, 256, 44, 80), (22, 40)), ((8, 256, 88, 160), (44, 80)), ((8, 256, 176, 320), (88, 160)))


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def test_symbols_are_exported_and_declared(ext):
    lib = ctypes.CDLL(ext.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions() and name in ext.EXPORTS and hasattr(lib, name)
    for name in ("resize_bilinear", "resize_bilinear_backward", "gated_merge_backward", "resize_backward_plan",
                 "merge_backward_plan", "merge_backward_workspace_bytes", "resize_footprint", "run_resize_bilinear",
                 "run_resize_bilinear_backward", "run_gated_merge_backward"):
        assert callable(getattr(ext, name))
    from rroi_align import merge
    assert callable(merge.gated_merge) and callable(merge.bilinear_resize)


def test_footprint_is_the_definitions_set_for_every_source_index(ext):
    """For every (in, out) in 1..40 x 1..40 and the network's pairs the range equals {Y : i0(Y) == i or i1(Y) == i} by the
    numpy `_axis`, the union over i covers every Y, and no range is longer than the bound the host refuses by."""
    pairs = [(a, b) for a in range(1, 41) for b in range(1, 41)] + list(B.NETWORK_PAIRS) + [(1, 5000), (5000, 1), (2, 4000)]
    longest = {}
    for n_in, n_out in pairs:
        want = B.footprints(n_in, n_out)
        covered = set()
        for i in range(n_in):
            lo, hi = ext.resize_footprint(n_in, n_out, i)
            assert 0 <= lo <= hi <= n_out and list(range(lo, hi)) == want[i], (n_in, n_out, i, lo, hi)
            covered.update(range(lo, hi))
            assert hi - lo <= B.footprint_bound(n_in, n_out), (n_in, n_out, i)
            longest[(n_in, n_out)] = max(longest.get((n_in, n_out), 0), hi - lo)
        assert covered == set(range(n_out)), (n_in, n_out)
    assert longest[(22, 44)] <= 5 and longest[(160, 320)] <= 5 and longest[(1, 5000)] == 5000 and longest[(5000, 1)] == 1
    for bad in ((0, 4, 0), (4, 0, 0), (4, 4, 4), (4, 4, -1)):
        with pytest.raises(ValueError):
            ext.resize_footprint(*bad)
    assert ext._lib.rroi_resize_footprint(4, 4, 0, None, None) == 0


def test_the_references_are_torchs_float64_autograd():
    """On the CPU the float64 restatements equal torch's float64 autograd of `up(a) + f * up(gate)` and of F.interpolate to
    1e-12 of the largest gradient, over the whole table: the restatement is the stock definition's gradient."""
    up = lambda t, like: t if t.shape[-2:] == like.shape[-2:] else F.interpolate(  # noqa: E731
        t, size=like.shape[-2:], mode="bilinear", align_corners=True)
    worst = 0.0
    for case in B.CASES:
        a, f, gate, dy = B.problem(case, torch.float32)
        ar, fr = a.double().requires_grad_(True), f.double().requires_grad_(True)
        gr = None if gate is None else gate.double().requires_grad_(True)
        y = up(ar, fr) + (fr if gr is None else fr * up(gr, fr))
        y.backward(dy.double())
        want_y, want_df, da_ref, dg_ref = B.reference(case, torch.float32)
        scale = max(float(t.grad.abs().max()) for t in (ar, fr) + (() if gr is None else (gr,))) or 1.0
        errs = [float((da_ref.ref - ar.grad).abs().max()), float((B.expected_df(dy, gate, rounded=False) - fr.grad).abs().max())]
        if gr is not None:
            errs.append(float((dg_ref.ref - gr.grad).abs().max()))
        fwd = torch.from_numpy(M.resize64(a.double().numpy(), *f.shape[-2:])[0])
        errs.append(float((fwd - up(a.double(), f)).abs().max()))
        assert torch.equal(fwd.float(), want_y)
        worst = max(worst, max(errs) / scale)
        assert max(errs) <= 1e-12 * scale, (case, errs, scale)
        # the stand-alone resize's backward is F.interpolate's
        if a.shape[-2:] != f.shape[-2:]:
            xr = a.double().requires_grad_(True)
            up(xr, f).backward(dy.double())
            assert float((da_ref.ref - xr.grad).abs().max()) <= 1e-12 * (float(xr.grad.abs().max()) or 1.0), case
    print(f"references against float64 autograd: worst {worst:.3g} of the largest gradient")


def test_the_bound_holds_the_reference_rounded_to_the_dtype():
    """The references rounded once to the dtype are inside their own bounds -- within half of it, and a little, where the
    result is a normal number -- so the bound is not tighter than a correct kernel can meet."""
    for case in (B.CASES[1], B.CASES[7], B.CASES[13]):
        for dtype in B.DTYPES:
            _, _, da_ref, dg_ref = B.reference(case, dtype)
            for ref in (da_ref, dg_ref):
                ok, worst = ref.check(ref.ref.to(dtype))
                assert ok and worst <= 1.0, (case, dtype, worst)
                normal = ref.ref.abs() >= 2.0 ** -13
                ratio = ((ref.ref.to(dtype).double() - ref.ref).abs() / ref.bound)[normal]
                assert float(ratio.max()) <= 0.5 + 1e-9, (case, dtype)


def test_plan_and_workspace_queries_agree_with_the_mirror(ext):
    table = [(c[0], c[1], c[2]) for c in B.CASES] + [(shape, g, g) for shape, g in NETWORK]
    blocks = set()
    for shape, a_size, g_size in table:
        N, C, H, W = shape
        K, cb, tiles, grid, gt, ws, launches = B.merge_backward_plan_of(shape, g_size)
        blocks.add(K)
        for dtype in B.DTYPES:
            p = ext.merge_backward_plan(N, C, H, W, g_size, dtype=dtype)
            assert (p.vector_elems, p.block, p.channel_groups, p.channel_block, p.tiles, p.grid_x) == (4, 256, K, cb, tiles, grid), shape
            assert cb <= B.MAX_BLOCK and (K - 1) * cb < C <= K * cb
            if g_size is None:
                assert (p.gate_tiles, p.gate_grid_x, p.launches, p.workspace_bytes, p.resize_gate) == (0, 0, 1, 0, 0)
                continue
            assert (p.gate_tiles, p.gate_grid_x, p.launches, p.workspace_bytes) == (gt, N * gt, launches, ws)
            assert p.resize_gate == int(tuple(g_size) != (H, W))
            assert (p.gate_scale_y, p.gate_scale_x) == tuple(0.0 if o == 1 else (i - 1) / (o - 1) for i, o in zip(g_size, (H, W)))
            assert ext.merge_backward_workspace_bytes(N, C, H, W, g_size, dtype=dtype) == ws > 0
            # the resize's backward for `a`
            rk, rcb, rt, rg = B.resize_backward_plan_of(N, C, a_size)
            r = ext.resize_backward_plan(N, C, a_size, (H, W), dtype=dtype)
            assert (r.vector_elems, r.block, r.channel_groups, r.channel_block, r.tiles, r.grid_x) == (1, 256, rk, rcb, rt, rg)
            assert r.identity == int(tuple(a_size) == (H, W))
            assert (r.max_rows, r.max_cols) == (B.footprint_bound(a_size[0], H), B.footprint_bound(a_size[1], W))
    assert {1, 2, 4, 8} <= blocks
    assert B.merge_backward_plan_of((1024, 2100, 1, 1), (1, 1))[:2] == (2, 2048)      # the cap decides, not the rule
    assert ext.merge_backward_plan(8, 256, 176, 320, (88, 160)).channel_groups == 4   # the network's largest merge
    # the blocks do not depend on the dtype
    assert len({ext.merge_backward_plan(3, 256, 16, 24, (8, 12), dtype=d)[:6] for d in B.DTYPES}) == 1
    assert ext._lib.rroi_merge_backward_plan(0, 2, 4, 8, 8, 4, 4, 1, None) == 0
    assert ext._lib.rroi_resize_backward_plan(0, 2, 4, 4, 4, 8, 8, None) == 0
    for bad in ((1, 0, 8, 8), (0, 4, 8, 8), (1, 4, 8, -1), (1, 1 << 11, 1 << 10, 1 << 10)):
        with pytest.raises(ValueError):
            ext.merge_backward_plan(*bad, (4, 4))
        assert ext.merge_backward_workspace_bytes(*bad, (4, 4)) == 0
    with pytest.raises(ValueError):
        ext.merge_backward_plan(1, 4, 8, 8, (4, 4), dtype=7)
    # the chain limits: more than 4096 output rows (columns) meeting in one source element, more than 4096 blocks
    with pytest.raises(ValueError):
        ext.merge_backward_plan(1, 2, 5000, 2, (1, 2))
    with pytest.raises(ValueError):
        ext.resize_backward_plan(1, 2, (2, 1), (2, 5000))
    assert ext.resize_backward_plan(1, 2, (2, 1), (2, 4096)).max_cols == 4096
    assert ext.resize_backward_plan(1, 2, (2, 5), (2, 8000)).max_cols == B.footprint_bound(5, 8000) == 4001
    with pytest.raises(ValueError):
        ext.resize_backward_plan(1, 2, (2, 3), (2, 8000))                # about 8000 columns reach the middle element
    with pytest.raises(ValueError):
        ext.merge_backward_plan(1, 2048 * 4096 + 1, 1, 1, (1, 1))        # the rule gives blocks of 2048: 4097 of them


def test_refusals_return_zero_before_any_launch(ext):
    mb, rf, rb = ext._lib.rroi_merge_backward_hip, ext._lib.rroi_resize_forward_hip, ext._lib.rroi_resize_backward_hip
    shape, g = (2, 4, 8, 8), (4, 4)
    need = ext.merge_backward_workspace_bytes(*shape, g)
    ok = dict(dtype=0, dy=P, f=P + FAR, gate=P + 2 * FAR, df=P + 3 * FAR, dg=P + 4 * FAR, shape=shape, g=g, ws=P + 5 * FAR,
              nbytes=need)

    def call(**kw):
        a = dict(ok, **kw)
        return mb(a["dtype"], a["dy"], a["f"], a["gate"], a["df"], a["dg"], *a["shape"], *a["g"], a["ws"], a["nbytes"], None)

    for dtype in (3, -1, 100):
        assert call(dtype=dtype) == 0
    for bad in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (-1, 4, 8, 8), (1, 1 << 11, 1 << 10, 1 << 10),
                (0x7fffffff,) * 4):
        assert call(shape=bad, nbytes=1 << 40) == 0, bad
    for bad_g in ((0, 4), (4, 0), (-1, 4)):
        assert call(g=bad_g) == 0
    assert call(shape=(1, 2, 5000, 2), g=(1, 2), nbytes=1 << 40) == 0                     # the chain limit
    for dtype in (0, 1, 2):
        kw = dict(dtype=dtype)
        esize = 4 if dtype == 0 else 2
        map_bytes, gate_bytes = 2 * 4 * 64 * esize, 2 * 16 * esize
        assert call(dy=None, **kw) == 0 and call(f=None, **kw) == 0 and call(f=None, dg=None, **kw) == 0
        assert call(df=None, dg=None, **kw) == 0
        assert call(gate=None, **kw) == 0                                                  # dgate needs the gate
        for out, nbytes in (("df", map_bytes), ("dg", gate_bytes)):
            for src, sbytes in (("dy", map_bytes), ("f", map_bytes), ("gate", gate_bytes)):
                assert call(**{out: ok[src]}, **kw) == 0, (out, src)
                assert call(**{out: ok[src] + sbytes - 2}, **kw) == 0, (out, src)
                assert call(**{out: ok[src] - nbytes + 2}, **kw) == 0, (out, src)
        assert call(dg=ok["df"] + map_bytes - 2, **kw) == 0                                # the two outputs overlap
        for extra in (dict(), dict(df=None)):
            assert call(ws=None, **kw, **extra) == 0 and call(ws=None, nbytes=0, **kw, **extra) == 0
            for off in (1, 16, 128, 255):
                assert call(ws=ok["ws"] + off, nbytes=need + 256, **kw, **extra) == 0, off
            assert call(nbytes=need - 1, **kw, **extra) == 0 and call(nbytes=0, **kw, **extra) == 0
    # the two resize calls: (dtype, in, out, N, C, h, w, H, W, stream)
    for fn in (rf, rb):
        good = [0, P, P + FAR, 2, 4, 4, 4, 8, 8, None]
        for at, bad in ((0, 3), (0, -1), (1, None), (2, None), (3, 0), (4, 0), (5, 0), (6, -1), (7, 0), (8, 0)):
            args = list(good)
            args[at] = bad
            assert fn(*args) == 0, (at, bad)
        assert fn(0, P, P + FAR, 1, 1 << 11, 4, 4, 1 << 10, 1 << 10, None) == 0
        assert fn(0, P, P + FAR, 1, 1 << 11, 1 << 10, 1 << 10, 4, 4, None) == 0
        assert fn(0, P, P, 2, 4, 4, 4, 8, 8, None) == 0 and fn(0, P, P + 16, 2, 4, 4, 4, 8, 8, None) == 0   # overlap
    assert rb(0, P, P + FAR, 1, 2, 2, 1, 2, 5000, None) == 0                               # the chain limit (backward only)


def test_python_surface_raises_what_it_documents(ext):
    from rroi_align import merge
    a, f, g = torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 8, 8), torch.zeros(2, 1, 4, 4)
    for dtype in B.DTYPES:
        with pytest.raises(RuntimeError, match="GPU only"):
            merge.gated_merge(a.to(dtype), f.to(dtype), g.to(dtype))
        with pytest.raises(RuntimeError, match="GPU only"):
            merge.bilinear_resize(a.to(dtype), (8, 8))
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.gated_merge_backward(f.to(dtype), f.to(dtype), g.to(dtype))
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.resize_bilinear_backward(f.to(dtype), (4, 4))
    a, f, g = fake_cuda(a), fake_cuda(f), fake_cuda(g)            # (the shape and dtype checks come before any call)
    for fn in (merge.gated_merge, lambda a_, f_, g_=None: ext.gated_merge_backward(f_, f_, g_)):
        with pytest.raises(ValueError):
            fn(a, f.half(), g)
        with pytest.raises(ValueError):
            fn(a, f, fake_cuda(torch.zeros(2, 2, 4, 4)))
        with pytest.raises(ValueError):
            fn(a, f, fake_cuda(torch.zeros(3, 1, 4, 4)))
        with pytest.raises(ValueError):
            fn(a, f[0], g)
        with pytest.raises(TypeError):
            fn(a, [1.0], g)
    with pytest.raises(ValueError, match="batch size and channels"):
        merge.gated_merge(fake_cuda(torch.zeros(2, 4, 4, 4)), f, g)
    with pytest.raises(ValueError, match="one shape"):
        ext.gated_merge_backward(a, f, g)
    fc, gc = f, g
    with pytest.raises(ValueError, match="no gradient"):
        ext.gated_merge_backward(fc, fc, gc, need_df=False, need_dgate=False)
    with pytest.raises(ValueError, match="no gradient"):
        ext.gated_merge_backward(fc, fc, None, need_df=False)                 # without a gate there is no dgate
    for fn in (merge.bilinear_resize, ext.resize_bilinear, ext.resize_bilinear_backward):
        for bad in ((0, 4), (4,), 4, (4, -1), "ab"):
            with pytest.raises(ValueError):
                fn(a, bad)
        with pytest.raises(ValueError):
            fn(a[0], (4, 4))
        with pytest.raises(TypeError):
            fn(None, (4, 4))


def test_trainable_merge_ok_is_merge_ok_without_its_gradient_clause(monkeypatch):
    from fots_e2e import native_train as T
    from fots_e2e.native import merge_ok
    z = lambda *s, dtype=torch.float32: fake_cuda(torch.zeros(*s, dtype=dtype))  # noqa: E731
    a, f, g = z(2, 4, 4, 4), z(2, 4, 8, 8), z(2, 1, 4, 4)
    ag = z(2, 4, 4, 4).requires_grad_(True)
    assert merge_ok(a, f, g) and not merge_ok(ag, f, g)
    assert T.trainable_merge_ok(ag, f, g) and T.trainable_merge_ok(a, f, g) and T.trainable_merge_ok(ag, f) and T.trainable_merge_ok(ag, f, None, True)
    assert torch.is_grad_enabled()                                            # asking leaves grad mode as it was
    for dtype in (torch.bfloat16, torch.float16):
        assert T.trainable_merge_ok(z(2, 4, 4, 4, dtype=dtype), z(2, 4, 8, 8, dtype=dtype), z(2, 1, 4, 4, dtype=dtype))
    for bad in ((torch.zeros(2, 4, 4, 4), f, g), (a, f, torch.zeros(2, 1, 4, 4)),
                (a, fake_cuda(torch.zeros(2, 4, 8, 8).to(memory_format=torch.channels_last)), g),
                (z(2, 4, 4, 4, dtype=torch.float64), z(2, 4, 8, 8, dtype=torch.float64), None),
                (z(2, 4, 4, 4, dtype=torch.bfloat16), f, g), (z(2, 5, 4, 4), f, g), (a, f, z(2, 2, 4, 4)), (a, f, z(3, 1, 4, 4)),
                (z(0, 4, 4, 4), z(0, 4, 8, 8), None), (z(4, 4, 4), f, g)):
        assert not T.trainable_merge_ok(*bad)
    # what the backward's gather refuses: more than 4096 output columns meeting in one source element
    wide = z(2, 4, 8, 5000)
    assert merge_ok(z(2, 4, 8, 1), wide) and not T.trainable_merge_ok(z(2, 4, 8, 1), wide)
    assert T.trainable_merge_ok(z(2, 4, 8, 5), wide) and not T.trainable_merge_ok(z(2, 4, 8, 5), wide, z(2, 1, 1, 1))
    assert [T._footprint_bound(i, o) for i, o in ((1, 1), (1, 7), (7, 1), (22, 44), (3, 8000), (2, 4000))] == \
        [B.footprint_bound(i, o) for i, o in ((1, 1), (1, 7), (7, 1), (22, 44), (3, 8000), (2, 4000))]
    with monkeypatch.context() as mp:
        mp.setattr(torch, "is_autocast_enabled", lambda *x: True)
        assert not T.trainable_merge_ok(a, f, g)
    with monkeypatch.context() as mp:                                         # this module's own hook declines a shape
        seen = []
        mp.setattr(T, "_merge_backward_slower", lambda a_, f_, g_, r: (seen.append(r), True)[1])
        assert not T.trainable_merge_ok(a, f, g) and not T.trainable_merge_ok(a, f, None, True) and seen == [False, True]
        with monkeypatch.context() as det:                                    # ... but not where the stock backward raises
            det.setattr(torch, "are_deterministic_algorithms_enabled", lambda: True)
            assert T.trainable_merge_ok(a, f, g) and seen == [False, True]
    assert T.trainable_merge_ok(a, f, g)
    # the 30 measured rows -- the network's three merges and two resizes at 704 x 1280, one and eight images, every dtype:
    # declined are exactly the rows that missed the bar in both runs (views of one element: nothing that large is allocated)
    e = lambda dtype, *s: fake_cuda(torch.zeros(1, dtype=dtype).expand(*s))  # noqa: E731
    declined = set()
    for n in (1, 8):
        for dtype in B.DTYPES:
            rows = {"merge1": (e(dtype, n, 256, 22, 40), e(dtype, n, 256, 44, 80), e(dtype, n, 1, 22, 40), False),
                    "merge2": (e(dtype, n, 256, 88, 160), e(dtype, n, 256, 88, 160), e(dtype, n, 1, 44, 80), False),
                    "merge3": (e(dtype, n, 256, 176, 320), e(dtype, n, 256, 176, 320), e(dtype, n, 1, 88, 160), False),
                    "resize1": (e(dtype, n, 256, 44, 80), e(dtype, n, 256, 88, 160), None, True),
                    "resize2": (e(dtype, n, 256, 88, 160), e(dtype, n, 256, 176, 320), None, True)}
            declined |= {(what, dtype, n) for what, args in rows.items() if T._merge_backward_slower(*args)}
    assert declined == {("merge2", d, 1) for d in B.DTYPES} | {("merge1", torch.float32, 1)}
    # the lines: half the measured size below, halfway to the next measured row above; the tests' small maps stay native
    f32 = torch.float32
    assert not T._merge_backward_slower(e(f32, 1, 256, 16, 24), e(f32, 1, 256, 16, 24), e(f32, 1, 1, 8, 12), False)
    assert not T._merge_backward_slower(e(f32, 1, 256, 2, 3), e(f32, 1, 256, 4, 6), e(f32, 1, 1, 2, 3), False)
    for n, want in ((1_799_999, False), (1_800_000, True), (8_999_999, True), (9_000_000, False)):
        assert T._merge_backward_slower(e(f32, 1, 1, 1, n), e(f32, 1, 1, 1, n), e(f32, 1, 1, 1, 1), False) == want, n
    for n, want in ((449_999, False), (450_000, True), (4_049_999, True), (4_050_000, False)):
        assert T._merge_backward_slower(e(f32, 1, 1, 1, 2), e(f32, 1, 1, 1, n), e(f32, 1, 1, 1, 1), False) == want, n
        assert not T._merge_backward_slower(e(torch.bfloat16, 1, 1, 1, 2), e(torch.bfloat16, 1, 1, 1, n), e(torch.bfloat16, 1, 1, 1, 1), False)
    assert not T._merge_backward_slower(e(f32, 1, 1, 1, 3_600_000), e(f32, 1, 1, 1, 3_600_000), None, False)   # ungated: not measured


def test_use_trainable_merge_switches_the_class_only_and_back():
    from fots_e2e import native as nat
    from fots_e2e import native_train as T
    from fots_e2e.model import FOTSNet
    net = FOTSNet()
    keys = list(net.state_dict().keys())
    params = [id(p) for p in net.parameters()]
    assert not T.use_trainable_merge(net) and type(net) is FOTSNet            # off by default; nothing to switch yet
    for first, second, native_type, trainable_type in (
            (nat.use_native_merge, nat.use_native_heads, nat.NativeHeadsMergeFOTSNet, T.TrainableHeadsMergeFOTSNet),
            (nat.use_native_heads, nat.use_native_merge, nat.NativeHeadsMergeFOTSNet, T.TrainableHeadsMergeFOTSNet)):
        assert first(net) and second(net) and type(net) is native_type        # the two compose in either order ...
        assert T.use_trainable_merge(net) and type(net) is trainable_type     # ... and the trainable switch goes on top
        assert isinstance(net, native_type) and not T.use_trainable_merge(net)
        assert list(net.state_dict().keys()) == keys and [id(p) for p in net.parameters()] == params
        assert not second(net, enable=False) and type(net) is trainable_type  # the other switches know their own types only
        assert T.use_trainable_merge(net, enable=False) and type(net) is native_type
        assert second(net, enable=False) and first(net, enable=False) and type(net) is FOTSNet
    for switches, native_type, trainable_type in (
            ((nat.use_native_merge,), nat.NativeMergeFOTSNet, T.TrainableMergeFOTSNet),
            ((nat.use_native_merge, nat.use_native_recogniser), nat.NativeMergeRecogniserFOTSNet, T.TrainableMergeRecogniserFOTSNet),
            ((nat.use_native_heads, nat.use_native_merge, nat.use_native_recogniser), nat.NativeHeadsMergeRecogniserFOTSNet,
             T.TrainableHeadsMergeRecogniserFOTSNet)):
        assert all(s(net) for s in switches) and type(net) is native_type
        assert T.use_trainable_merge(net) and type(net) is trainable_type
        assert T.use_trainable_merge(net, enable=False) and type(net) is native_type
        assert all(s(net, enable=False) for s in reversed(switches)) and type(net) is FOTSNet
    assert list(net.state_dict().keys()) == keys and [id(p) for p in net.parameters()] == params


def test_a_cpu_pass_of_the_switched_network_is_the_stock_merge():
    """On the CPU the predicate fails, so the trainable `_merge` computes `FOTSNet._merge`'s expression piece by piece."""
    from fots_e2e import native as nat
    from fots_e2e import native_train as T
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    for attention in (True, False):
        net = deterministic_init(FOTSNet(attention=attention)).train()
        g = torch.Generator().manual_seed(4)
        fs = [torch.randn(1, 256, h, w, generator=g).requires_grad_(True) for h, w in ((16, 24), (8, 12), (4, 6), (2, 3))]
        want = FOTSNet._merge(net, *fs)
        assert nat.use_native_merge(net) and T.use_trainable_merge(net)
        got = net._merge(*fs)
        assert all(torch.equal(x, y) for x, y in zip(got, want))
        sum(t.sum() for t in got).backward()
        assert all(t.grad is not None for t in fs)
