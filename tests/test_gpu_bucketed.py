"""GPU (MI355X): bucketed RoIRotate -- one pooled width per ROI, one launch chain.

Forward: every bucket equals, as integers, both the dense op on rois[index] at the bucket's width and the oracle;
nothing outside the crops is written and every crop element is.  Backward: under RROI_PATH_DETERMINISTIC the ragged
gradients give the bits of the existing ORDERED backward fed the same gradients zero-padded to the widest width (a
padded column adds w * (+0) to a double sum that starts at +0.0); the default plans stay within the per-element bound
of workloads.check_backward_elementwise against the oracle on the padded gradients.  Every case records the plan it ran;
the last test fails unless both forward plans and all three backward families were reached."""
import ctypes

import numpy as np
import pytest
import torch

import workloads as Wk
from test_gpu_deterministic import sandwich, torch_deterministic
from test_gpu_half import check_half_backward

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
IDS = ["fp32", "bf16", "fp16"]
RAN = set()   # plan families that ran


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(got, want):
    """Compared as integers; a NaN may carry any payload (the blend of a NaN tap)."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    ok = (bits(got) == bits(want)) | (got.isnan() & want.isnan())
    return bool(ok.all())


def multiples(rng, R, choices):
    return [int(v) for v in rng.choice(choices, R)]


def natural_widths(r, ph, quantum):
    """floor(roi_pooled_width) + 1 columns hold every live bin (pw <= rpw); rounded up to `quantum`."""
    rpw = np.float32(ph) * r[:, 4] / r[:, 3]
    return [int(-(-(int(np.floor(v)) + 1) // quantum) * quantum) for v in rpw]


def forward_case(name):
    rng = np.random.default_rng(len(name))
    if name == "one image":            # C = 64 on a 176 x 320 map, R = 24, widths {64, 96, 128, 416}
        f, r = Wk.bench_inputs(R=24, C=64, H=176, W=320, img=1280, seed=1)
        r[:, 2] *= 704 / 1280
        return f, r, 11, [64] * 9 + [96] * 8 + [128] * 6 + [416], 0.25, "patch"
    if name == "eight images":         # R = 192
        f, r = Wk.bench_inputs(R=192, C=64, H=176, W=320, img=1280, seed=2, batch=8)
        r[:, 2] *= 704 / 1280
        return f, r, 11, multiples(rng, 192, [64, 96, 128]), 0.25, "gather"
    if name == "configs[1] natural":   # C = 256 on 160 x 160, R = 512, PH = 8
        f, r = Wk.bench_inputs()
        return f, r, 8, natural_widths(r, 8, 16), 0.25, "gather"
    if name in ("arbitrary R=32", "arbitrary R=600"):
        R = 32 if name.endswith("32") else 600
        f, r = Wk.bench_inputs(R=R, C=64, H=120, W=160, img=640, seed=3, batch=2)
        return f, r, 11, multiples(rng, R, [1, 7, 83, 96, 100]), 0.25, "patch"
    if name in ("C=3", "C=33"):
        C = int(name[2:])
        f, r = Wk.bench_inputs(R=40, C=C, H=96, W=128, img=512, seed=4)
        return f, r, 8, multiples(rng, 40, [5, 32, 64, 66]), 0.25, "patch"
    if name == "C=33 gather":          # a partial last chunk in the ragged gather (named: the output is small)
        f, r = Wk.bench_inputs(R=96, C=33, H=96, W=128, img=512, seed=5)
        return f, r, 8, multiples(rng, 96, [16, 32, 64, 96]), 0.25, "tiled"
    if name == "edge + degenerate":    # + a bad batch index, NaN / +-inf in the map
        r = np.concatenate([Wk.edge_rois(), Wk.degenerate_rois(), Wk.bench_inputs(R=20, C=1)[1]])
        r[-3:, 0] = (7, -2, np.nan)
        f = rng.standard_normal((1, 16, 160, 160)).astype(np.float32)
        flat = f.reshape(-1)
        idx = rng.choice(flat.size, 300, replace=False)
        flat[idx[:100]], flat[idx[100:200]], flat[idx[200:]] = np.nan, np.inf, -np.inf
        return f, r, 8, multiples(rng, len(r), [16, 48, 64, 200]), 0.25, "patch"
    raise KeyError(name)


FORWARD_CASES = ["one image", "eight images", "configs[1] natural", "arbitrary R=32", "arbitrary R=600", "C=3", "C=33",
                 "C=33 gather", "edge + degenerate"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", FORWARD_CASES)
def test_forward_bit_exact(ext, oracle, name, dtype):
    f, r, ph, widths, scale, want_plan = forward_case(name)
    F, Rr = dev(f).to(dtype), dev(r)
    f_wide = F.float().cpu().numpy()
    B, C, H, W = f.shape
    path = ext.PATH_TILED if want_plan == "tiled" else ext.PATH_AUTO
    plan = ext.forward_bucketed_plan(B, C, H, W, ph, widths, path=path, dtype=dtype)
    assert plan.family == (ext.PLAN_FWD_DIRECT_K2P if want_plan == "patch" else ext.PLAN_FWD_TWO_LAUNCH), plan
    layout = ext.bucket_layout(widths)
    for trig in (ext.TRIG_DOUBLE, ext.TRIG_FP32):
        out = ext.forward_bucketed(F, Rr, ph, widths, scale, path=path, trig=trig)
        assert len(out) == len(layout)
        for (idx, crops), (w, want_idx) in zip(out, layout):
            assert idx.tolist() == want_idx and idx.dtype == torch.int64
            assert crops.shape == (len(want_idx), C, ph, w) and crops.dtype == dtype and crops.is_contiguous()
            dense = ext.forward(F, Rr[idx], ph, w, scale, trig=trig)
            assert same_bits(crops, dense), (name, trig, w, "differs from the dense op")
            if trig == ext.TRIG_DOUBLE:
                # (a batch index outside [0, B): the op writes zeros where the reference reads out of bounds)
                rb = r[want_idx].copy()
                bad = ~((rb[:, 0] > -1) & (rb[:, 0] < B)) & ~np.isnan(rb[:, 0])
                rb[bad, 0] = 0
                want = oracle.forward_c(f_wide, rb, ph, w, scale, threads=16)
                want[bad] = 0
                want = torch.from_numpy(want).to(dtype)
                assert same_bits(crops.cpu(), want), (name, w, "differs from the oracle")
    RAN.add(plan.family)


def test_single_bucket_equals_the_dense_call_and_no_roi(ext):
    f, r = Wk.bench_inputs(R=48, C=64, H=120, W=160, img=640, seed=6, batch=2)
    F, Rr = dev(f), dev(r)
    for path in (ext.PATH_AUTO, ext.PATH_DIRECT, ext.PATH_TILED):
        (idx, crops), = ext.forward_bucketed(F, Rr, 11, [96] * 48, 0.25, path=path)
        assert idx.tolist() == list(range(48))
        assert same_bits(crops, ext.forward(F, Rr, 11, 96, 0.25))
    assert ext.forward_bucketed(F, Rr[:0], 11, [], 0.25) == []
    g = ext.backward_bucketed([], Rr[:0], f.shape, 11, [], 0.25)
    assert g.shape == F.shape and not g.any()
    st = ext._lib.rroi_align_backward_bucketed_hip(None, 0, 0, 0.25, 2, 0, 120, 160, 64, 11, 96, None, g.fill_(1).data_ptr(),
                                                   None, 0, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 1 and not g.any()          # R = 0 through the raw ABI: the zero fill


# ---------------------------------------------------------------- raw ABI: what is written, what is not
NAN_PATTERN = {torch.float32: 0x7FC5A5A5, torch.bfloat16: 0x7FC5, torch.float16: 0x7E55}   # NaNs no finite map produces


def raw_forward(ext, F, Rr, ph, max_w, table_widths, addrs, path, sum_w=None, mult=1, align=None):
    B, C, H, W = F.shape
    R = Rr.shape[0]
    table = ext.crop_table(addrs, table_widths, F.device)
    valid = [w for w in table_widths if 1 <= w <= max_w]
    nbytes = ext._lib.rroi_align_forward_bucketed_workspace_bytes(B, C, H, W, R)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=F.device)
    st = ext._lib.rroi_align_forward_bucketed_hip(
        F.data_ptr(), ext.dtype_code(F.dtype), 0.25, B, R, H, W, C, ph, max_w, sum_w if sum_w is not None else max(sum(valid), R),
        mult, align if align is not None else F.element_size(), Rr.data_ptr(), table.data_ptr(), ws.data_ptr(), nbytes, path,
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def laid_out(F, widths, ph, gap_of, start):
    """One buffer, crop i at element offset start + sum of the crops and gaps before it; returns (buffer as integers,
    element offsets)."""
    C, es = F.shape[1], F.element_size()
    offs, at = [], start
    for i, w in enumerate(widths):
        offs.append(at)
        at += C * ph * w + gap_of(i)
    itype = torch.int32 if es == 4 else torch.int16
    buf = torch.full((at + 64,), NAN_PATTERN[F.dtype], dtype=itype, device=F.device)
    return buf, offs


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", ["patch misaligned", "patch many rois misaligned", "gather aligned gaps"])
def test_nothing_outside_the_crops_is_written(ext, form, dtype):
    rng = np.random.default_rng(9)
    R = 24 if form == "patch misaligned" else 300
    f, r = Wk.bench_inputs(R=R, C=40, H=96, W=128, img=512, seed=8)
    F, Rr = dev(f).to(dtype), dev(r)
    ph, es = 8, F.element_size()
    if form == "gather aligned gaps":
        widths = multiples(rng, R, [32, 64, 96])
        gap = lambda i: (64 // es) * (i % 3)               # whole sectors between the crops, or none
        buf, offs = laid_out(F, widths, ph, gap, 0)
        path, mult, align = ext.PATH_TILED, 32, 64
        fam = ext.PLAN_FWD_TWO_LAUNCH
    else:
        widths = multiples(rng, R, [1, 7, 33, 64, 90])
        gap = lambda i: (1, 0, 3, 5)[i % 4]                # crops an odd number of elements apart: element-aligned only
        buf, offs = laid_out(F, widths, ph, gap, 1)
        path, mult, align = (ext.PATH_DIRECT if R == 24 else ext.PATH_AUTO), 1, es
        fam = ext.PLAN_FWD_DIRECT_K2P
    p = ext._Plan()
    assert ext._lib.rroi_align_forward_bucketed_plan(ext.dtype_code(dtype), 1, R, 96, 128, 40, ph, max(widths), sum(widths),
                                                     mult, align, path, ctypes.byref(p)) == 1 and p.family == fam
    before = buf.clone()
    addrs = [buf.data_ptr() + o * es for o in offs]
    assert raw_forward(ext, F, Rr, ph, max(widths), widths, addrs, path, mult=mult, align=align) == 1
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    for i, (o, w) in enumerate(zip(offs, widths)):
        n = 40 * ph * w
        inside[o:o + n] = True
        crop = buf[o:o + n].view(F.dtype).view(1, 40, ph, w)
        assert same_bits(crop, ext.forward(F, Rr[i:i + 1], ph, w, 0.25)), (form, i, w)
    assert torch.equal(buf[~inside], before[~inside]), "a byte outside the crops was written"
    assert not (buf[inside] == before[inside]).any(), "a crop element was left unwritten"
    RAN.add(fam)


@pytest.mark.parametrize("form", ["patch", "gather"])
def test_rejected_rows_are_skipped_and_neighbours_intact(ext, form):
    """A width of 0, a negative one, one above the stated maximum, a null address -- and, in the gather, a row that breaks
    the form's stated contract (a width with PH * W % 16 != 0, a crop that is not 64-byte aligned): the row is skipped."""
    R = 12 if form == "patch" else 200
    f, r = Wk.bench_inputs(R=R, C=32, H=96, W=128, img=512, seed=10)
    F, Rr = dev(f), dev(r)
    ph, mx = 8, 64
    widths = [32 if i % 2 else 64 for i in range(R)]
    buf, offs = laid_out(F, widths, ph, lambda i: 16, 0)          # (64-byte gaps: every crop stays aligned)
    addrs = [buf.data_ptr() + 4 * o for o in offs]
    table_w, table_a = list(widths), list(addrs)
    bad = {1: 0, 3: 65, 5: -7, 7: 1 << 20}
    for i, w in bad.items():
        table_w[i] = w
    table_a[9] = 0
    skipped = set(bad) | {9}
    if form == "gather":
        table_w[11] = 33                                          # 8 * 33 % 16 != 0
        table_a[13] += 4                                          # element-aligned only
        skipped |= {11, 13}
    before = buf.clone()
    path = ext.PATH_DIRECT if form == "patch" else ext.PATH_TILED
    assert raw_forward(ext, F, Rr, ph, mx, table_w, table_a, path, sum_w=sum(widths), mult=32, align=64) == 1
    for i, (o, w) in enumerate(zip(offs, widths)):
        n = 32 * ph * w
        if i in skipped:
            assert torch.equal(buf[o - 16:o + n + 16], before[o - 16:o + n + 16]), (form, i, "a skipped row was written")
        else:
            crop = buf[o:o + n].view(torch.float32).view(1, 32, ph, w)
            assert same_bits(crop, ext.forward(F, Rr[i:i + 1], ph, w, 0.25)), (form, i)
    # backward: a skipped row contributes nothing -- the ORDERED bits of the dense call with those gradients zeroed
    g = torch.randn(R, 32, ph, mx, device="cuda")
    for i, w in enumerate(widths):
        g[i, :, :, w:] = 0
    crops = [g[i, :, :, :w].contiguous() for i, w in enumerate(widths)]
    tw = list(widths)
    for i, w in bad.items():
        tw[i] = w
    ta = [c.data_ptr() for c in crops]
    ta[9] = 0
    gz = g.clone()
    gz[sorted(set(bad) | {9})] = 0
    table = ext.crop_table(ta, tw, F.device)
    nbytes = ext._lib.rroi_align_backward_bucketed_workspace_bytes(1, 32, 96, 128, R, ph, mx)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(F)
    st = ext._lib.rroi_align_backward_bucketed_hip(table.data_ptr(), 0, 0, 0.25, 1, R, 96, 128, 32, ph, mx, Rr.data_ptr(),
                                                   out.data_ptr(), ws.data_ptr(), nbytes, ext.PATH_DETERMINISTIC,
                                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 1
    assert same_bits(out, ext.backward(gz, Rr, f.shape, 0.25, deterministic=True))


# ---------------------------------------------------------------- backward
def ragged_grads(g_padded, widths, layout, dtype=torch.float32):
    """Per-bucket gradient tensors cut out of a (R, C, PH, W_max) tensor whose columns >= W_i are zero."""
    return [g_padded[idx][:, :, :, :w].to(dtype).contiguous().cuda() for w, idx in layout]


def padded_gradient(rng, R, C, ph, widths):
    g = rng.standard_normal((R, C, ph, max(widths))).astype(np.float32)
    for i, w in enumerate(widths):
        g[i, :, :, w:] = 0
    return g


BACKWARD_SHAPES = {
    # name: (bench_inputs kwargs, PH, width choices)
    "training R=32": (dict(R=32, C=64, H=120, W=160, img=640, seed=21, batch=2), 11, [32, 64, 96]),
    "arbitrary R=150": (dict(R=150, C=48, H=96, W=128, img=512, seed=22), 8, [1, 7, 30, 64, 66]),
    "C=33": (dict(R=40, C=33, H=64, W=96, img=384, seed=23), 8, [5, 32, 64]),
    "C=160": (dict(R=64, C=160, H=64, W=64, img=256, seed=24), 8, [16, 32, 64]),
}


@pytest.mark.parametrize("shape", list(BACKWARD_SHAPES))
def test_backward_deterministic_equals_the_padded_dense_ordered(ext, oracle, shape):
    kw, ph, choices = BACKWARD_SHAPES[shape]
    rng = np.random.default_rng(31)
    f, r0 = Wk.bench_inputs(**kw)
    w0 = multiples(rng, len(r0), choices)
    g0 = padded_gradient(rng, len(r0), f.shape[1], ph, w0)
    # one of test_gpu_deterministic.py's cancelling inputs: the order of every pixel's list is seen
    r, g = sandwich(r0, g0, 2.0 ** 40)
    widths = w0 * 3
    for i, w in enumerate(widths):
        g[i, :, :, w:] = 0
    layout = ext.bucket_layout(widths)
    B, C, H, W = f.shape
    Rr = dev(r)
    want = oracle.backward_c(g, r, f.shape, 0.25, threads=16)
    other = oracle.backward_c(np.ascontiguousarray(g[::-1]), np.ascontiguousarray(r[::-1]), f.shape, 0.25, threads=16)
    assert (other != want).sum() > 100, "the input does not tell the orders apart"
    for dtype in (torch.float32, torch.bfloat16):
        gp = torch.from_numpy(g).to(dtype)   # (bf16: rounded once -- the dense call sees the same rounded values)
        grads = ragged_grads(gp, widths, layout, dtype)
        for cl in ((False, True) if C % 4 == 0 else (False,)):
            plan = ext.backward_bucketed_plan(B, C, H, W, ph, widths, dtype=dtype, bottom_diff_layout=int(cl), deterministic=True)
            assert plan.family == ext.PLAN_BWD_ORDERED
            got = ext.backward_bucketed(grads, Rr, f.shape, ph, widths, 0.25, channels_last_grad=cl, deterministic=True)
            assert got.dtype == dtype and got.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
            dense = ext.backward(gp.cuda(), Rr, f.shape, 0.25, channels_last_grad=cl, deterministic=True)
            assert same_bits(got, dense), (shape, dtype, cl)
            if dtype == torch.float32:
                assert same_bits(got.cpu(), torch.from_numpy(want)), (shape, "differs from the oracle")
    RAN.add(ext.PLAN_BWD_ORDERED)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", list(BACKWARD_SHAPES))
def test_backward_default_paths_within_the_elementwise_bound(ext, oracle, shape, dtype):
    kw, ph, choices = BACKWARD_SHAPES[shape]
    rng = np.random.default_rng(41)
    f, r = Wk.bench_inputs(**kw)
    widths = multiples(rng, len(r), choices)
    g = torch.from_numpy(padded_gradient(rng, len(r), f.shape[1], ph, widths)).to(dtype)
    g_wide = g.float().numpy()
    want = oracle.backward_c(g_wide, r, f.shape, 0.25, threads=16)
    S, n = oracle.backward_bound_c(g_wide, r, f.shape, 0.25, threads=16)
    layout = ext.bucket_layout(widths)
    grads = ragged_grads(g, widths, layout, dtype)
    B, C, H, W = f.shape
    for path, fam in ((ext.PATH_AUTO, None), (ext.PATH_TILED_LISTS, ext.PLAN_BWD_LISTS), (ext.PATH_TILED_BUCKETS, ext.PLAN_BWD_BUCKETS)):
        for cl in ((False, True) if C % 4 == 0 else (False,)):
            plan = ext.backward_bucketed_plan(B, C, H, W, ph, widths, path=path, dtype=dtype, bottom_diff_layout=int(cl))
            assert plan.family in (ext.PLAN_BWD_LISTS, ext.PLAN_BWD_BUCKETS) and (fam is None or plan.family == fam)
            got = ext.backward_bucketed(grads, dev(r), f.shape, ph, widths, 0.25, path=path, channels_last_grad=cl)
            assert got.dtype == dtype and got.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
            what = f"{shape} {dtype} path {path} nhwc {cl}"
            if dtype == torch.float32:
                Wk.check_backward_elementwise(got.cpu().numpy(), want, S, n, what=what)
            else:
                check_half_backward(got, want, S, n, dtype, what)
            RAN.add(plan.family)


# ---------------------------------------------------------------- autograd
def test_module_against_the_dense_module_on_padded_tensors(ext):
    from rroi_align.modules.rroi_align import _RRoiAlign, _RRoiAlignBucketed
    f, r = Wk.bench_inputs(R=40, C=32, H=64, W=96, img=384, seed=51)
    rng = np.random.default_rng(52)
    widths = multiples(rng, 40, [16, 40, 64])
    Rr = dev(r)
    for dtype in DTYPES:
        F1 = dev(f).to(dtype).requires_grad_(True)
        F2 = dev(f).to(dtype).requires_grad_(True)
        buckets = _RRoiAlignBucketed(8, 0.25, deterministic=True)(F1, Rr, widths)
        dense = _RRoiAlign(8, 64, 0.25, deterministic=True)(F2, Rr)
        gd = torch.zeros_like(dense)
        loss = 0
        for k, (idx, crops) in enumerate(buckets):
            w = crops.shape[3]
            assert crops.dtype == dtype and same_bits(crops.detach(), dense.detach()[idx][:, :, :, :w].contiguous())
            gb = torch.randn_like(crops)
            if k == 1:
                gb = gb.transpose(2, 3).contiguous().transpose(2, 3)     # a non-contiguous gradient for one bucket
                assert not gb.is_contiguous()
            gd[idx, :, :, :w] = gb
            loss = loss + (crops * gb).sum()
        loss.backward()
        dense.backward(gd)
        assert F1.grad.dtype == dtype and same_bits(F1.grad, F2.grad), dtype
    # a channels_last backbone gets its gradient back in channels_last storage
    Fc = dev(f).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = _RRoiAlignBucketed(8, 0.25)(Fc, Rr, widths)
    sum(c.sum() for _, c in out).backward()
    assert Fc.grad.is_contiguous(memory_format=torch.channels_last)
    # under autocast the op stays an fp32 operator
    Fh = dev(f).half().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16):
        out = _RRoiAlignBucketed(8, 0.25)(Fh, Rr, widths)
    assert all(c.dtype == torch.float32 for _, c in out)
    sum(c.sum() for _, c in out).backward()
    assert Fh.grad.dtype == torch.float16


def test_a_bucket_without_gradient_contributes_nothing(ext):
    from rroi_align.modules.rroi_align import _RRoiAlignBucketed
    f, r = Wk.bench_inputs(R=30, C=16, H=64, W=96, img=384, seed=53)
    widths = [16, 48, 64] * 10
    F, Rr = dev(f).requires_grad_(True), dev(r)
    buckets = _RRoiAlignBucketed(8, 0.25, deterministic=True)(F, Rr, widths)
    gs = [torch.randn_like(c) for _, c in buckets]
    (buckets[0][1] * gs[0]).sum().add((buckets[2][1] * gs[2]).sum()).backward()     # the 48-wide bucket is unused
    g = torch.zeros(30, 16, 8, 64, device="cuda")
    for k in (0, 2):
        idx, crops = buckets[k]
        g[idx, :, :, :crops.shape[3]] = gs[k]
    assert same_bits(F.grad, ext.backward(g, Rr, f.shape, 0.25, deterministic=True))
    # the same through the binding, and no gradient at all
    got = ext.backward_bucketed([gs[0], None, gs[2]], Rr, f.shape, 8, widths, 0.25, deterministic=True)
    assert same_bits(got, F.grad)
    assert not ext.backward_bucketed([None, None, None], Rr, f.shape, 8, widths, 0.25).any()


def test_use_deterministic_algorithms_selects_ordered(ext):
    from rroi_align.modules.rroi_align import _RRoiAlignBucketed
    f, r0 = Wk.bench_inputs(R=24, C=32, H=64, W=96, img=384, seed=54)
    rng = np.random.default_rng(55)
    w0 = multiples(rng, 24, [16, 40, 64])
    r, g = sandwich(r0, padded_gradient(rng, 24, 32, 8, w0), 2.0 ** 40)
    widths = w0 * 3
    for i, w in enumerate(widths):
        g[i, :, :, w:] = 0
    layout = ext.bucket_layout(widths)
    grads = ragged_grads(torch.from_numpy(g), widths, layout)
    Rr = dev(r)
    want = ext.backward(dev(g), Rr, f.shape, 0.25, deterministic=True)
    assert ext.backward_bucketed_plan(1, 32, 64, 96, 8, widths, deterministic=True).family == ext.PLAN_BWD_ORDERED
    assert ext.backward_bucketed_plan(1, 32, 64, 96, 8, widths).family != ext.PLAN_BWD_ORDERED
    with torch_deterministic(True):
        F = dev(f).requires_grad_(True)
        out = _RRoiAlignBucketed(8, 0.25)(F, Rr, widths)       # deterministic=None: torch's flag, read in the backward
        torch.autograd.backward([c for _, c in out], grads)
        assert same_bits(F.grad, want)
    with torch_deterministic(False):
        F = dev(f).requires_grad_(True)
        out = _RRoiAlignBucketed(8, 0.25, deterministic=True)(F, Rr, widths)
        torch.autograd.backward([c for _, c in out], grads)
        assert same_bits(F.grad, want)


def test_graph_capture_reproduces_the_eager_bits(ext):
    f, r = Wk.bench_inputs(R=96, C=64, H=96, W=128, img=512, seed=56)
    rng = np.random.default_rng(57)
    F, Rr = dev(f), dev(r)
    for widths, path in ((multiples(rng, 96, [32, 64, 96]), ext.PATH_TILED), (multiples(rng, 96, [7, 33, 64]), ext.PATH_AUTO)):
        layout = ext.bucket_layout(widths)
        g = padded_gradient(rng, 96, 64, 8, widths)
        grads = ragged_grads(torch.from_numpy(g), widths, layout)
        eager = ext.forward_bucketed(F, Rr, 8, widths, 0.25, path=path)
        eager_g = ext.backward_bucketed(grads, Rr, f.shape, 8, widths, 0.25, deterministic=True)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                out = ext.forward_bucketed(F, Rr, 8, widths, 0.25, path=path)
                gin = ext.backward_bucketed(grads, Rr, f.shape, 8, widths, 0.25, deterministic=True)
        for _ in range(2):
            for _, c in out:
                c.fill_(float("nan"))
            gin.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert all(same_bits(c, e) for (_, c), (_, e) in zip(out, eager))
            assert same_bits(gin, eager_g)


def test_every_plan_was_reached(ext):
    need = {ext.PLAN_FWD_DIRECT_K2P, ext.PLAN_FWD_TWO_LAUNCH, ext.PLAN_BWD_LISTS, ext.PLAN_BWD_BUCKETS, ext.PLAN_BWD_ORDERED}
    assert need <= RAN, f"plans that no case of this module ran: {sorted(need - RAN)}"
