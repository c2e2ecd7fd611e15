"""GPU (MI355X): the native dense 3x3 convolution against the float64 reference and the derived bound of
conv3x3_cases.py over the whole table, the exact-integer table bit for bit, special values, misaligned views inside a
guarded buffer, degenerate inputs, determinism, graph capture, the switched network on the tensors it really sees, and one
inference chain with all six switches on.

Worst |y - act(ref)| / bound observed over the table on an MI355X: bf16 0.995, fp16 0.988 (profiles/native_conv3x3.md);
with 27 to 1296 terms the bound is dominated by the one rounding to the type, which reaches it at the bottom of a binade."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv3x3_cases as C
from test_gpu_bucketed import NAN_PATTERN

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def same_bits(got, want):
    got, want = got.cpu(), want.cpu()
    both_nan = got.isnan() & want.isnan()
    return got.shape == want.shape and bool(((C.bits(got) == C.bits(want)) | both_nan).all())


# ---------------------------------------------------------------- against the reference
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_the_whole_table_meets_the_bound_and_the_integer_table_every_bit(ext, dtype):
    worst = 0.0
    for case in C.CASES:
        N, Cin, Cout, H, W, s = case
        x, w, ref, S = C.problem(case, dtype)
        p = ext.conv3x3_plan(N, Cin, Cout, H, W, s, dtype=dtype)
        assert (p.tile_m, p.tile_h, p.k_chunks, p.grid_x) == C.plan_of(case)
        xg, wg = x.cuda(), w.cuda()
        for slope in C.SLOPES:
            got = ext.conv3x3(xg, wg, s, slope)
            assert got.shape == ref.shape and got.dtype == dtype and got.is_contiguous()
            got = got.cpu()
            want, lim = C.bound(ref, S, Cin, dtype, slope)
            ok, ratio = C.within(got, want, lim)
            print(f"{C.case_id(case)} slope={slope} tile={p.tile_m}x{p.tile_h}x32: worst error / bound {ratio:.3f}")
            assert bool(got.isfinite().all()) and ok and ratio <= 1.0, (case, slope, ratio)
            worst = max(worst, ratio)
        xe, we, refe = C.exact_problem(case, dtype)
        for slope in (1.0, 0.0):
            got = ext.conv3x3(xe.cuda(), we.cuda(), s, slope).cpu()
            want = C.act64(refe, slope).to(dtype)                  # integers of magnitude <= 252: exact in the type
            assert torch.equal(want.double(), C.act64(refe, slope))
            wrong = int((got.double() != want.double()).sum())     # (-0.0 of a ReLU equals 0.0)
            assert wrong == 0, (case, slope, wrong)
    print(f"worst error / bound over the table: {worst:.4f}")


# ---------------------------------------------------------------- special values
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_non_finite_inputs_poison_their_windows_and_no_other(ext, dtype, stride):
    case = (2, 17, 48, 11, 37, stride)
    x, w = C.random_problem(case, dtype, seed=11)
    w = torch.where(w == 0, torch.ones_like(w), w)                 # no zero weight: every window that holds one is poisoned
    clean = ext.conv3x3(x.cuda(), w.cuda(), stride, 0.01).cpu()
    bad = x.clone()
    spots = ((0, 3, 0, 0, NAN), (0, 16, 5, 20, INF), (1, 0, 10, 36, -INF), (1, 9, 4, 33, NAN))
    for n, c, i, j, v in spots:
        bad[n, c, i, j] = v
    got = ext.conv3x3(bad.cuda(), w.cuda(), stride, 0.01).cpu()
    hit = torch.zeros_like(bad, dtype=torch.float32)
    for n, c, i, j, _ in spots:
        hit[n, :, i, j] = 1.0
    poisoned = F.conv2d(hit, torch.ones(48, 17, 3, 3), stride=stride, padding=1) > 0
    assert poisoned.any() and not poisoned.all()
    assert torch.equal(~got.isfinite(), poisoned)
    ref = C.act64(C.reference(bad, w, stride)[0], 0.01)
    assert torch.equal(got.isnan(), ref.isnan())
    inf_at = got.isinf()
    assert torch.equal(got[inf_at].double(), ref[inf_at])
    assert torch.equal(C.bits(got)[~poisoned], C.bits(clean)[~poisoned])


# ---------------------------------------------------------------- addresses and guards
@pytest.mark.parametrize("case", [(2, 5, 7, 9, 35, 1), (1, 17, 33, 10, 66, 2)], ids=C.case_id)
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_views_and_guards(ext, dtype, case):
    """x, w and y 0 .. 7 elements past a 16-byte boundary, through the raw ABI; y inside a guarded buffer.  Every output
    element is written, no guard byte is, the inputs are unchanged and the bits do not depend on an address."""
    N, Cin, Cout, H, W, s = case
    x, w = C.random_problem(case, dtype, seed=sum(case))
    Ho, Wo = C.out_size(H, W, s)
    n = N * Cout * Ho * Wo
    stream = torch.cuda.current_stream().cuda_stream
    want = ext.conv3x3(x.cuda(), w.cuda(), s, 0.01)

    def shifted(t, off):
        buf = torch.zeros(t.numel() + 16, dtype=dtype, device="cuda")
        view = buf[off:off + t.numel()]
        view.copy_(t.reshape(-1))
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + off * t.element_size()
        return buf, view

    for ox, ow, oy in ((0, 0, 0), (1, 1, 1), (3, 2, 5), (7, 5, 2), (4, 3, 7)):
        (xb, xv), (wb, wv) = shifted(x, ox), shifted(w, ow)
        buf = torch.full((64 + oy + n + 64,), NAN_PATTERN[dtype], dtype=torch.int16, device="cuda")
        before = buf.clone()
        y = buf[64 + oy:64 + oy + n].view(dtype)
        st = ext._lib.rroi_conv3x3_forward_hip(ext.dtype_code(dtype), xv.data_ptr(), wv.data_ptr(), y.data_ptr(), N, Cin, Cout,
                                               H, W, s, 0.01, stream)
        torch.cuda.synchronize()
        assert st == 1
        assert torch.equal(buf[:64 + oy], before[:64 + oy]) and torch.equal(buf[64 + oy + n:], before[64 + oy + n:]), \
            "a byte outside the output was written"
        assert not (buf[64 + oy:64 + oy + n] == before[64 + oy:64 + oy + n]).any(), "an output element was left unwritten"
        assert same_bits(y.view(N, Cout, Ho, Wo), want), (ox, ow, oy)
        for (b, v), t, off in (((xb, xv), x, ox), ((wb, wv), w, ow)):   # the inputs are unchanged
            assert bool((b[:off] == 0).all()) and bool((b[off + t.numel():] == 0).all()) and torch.equal(v.cpu(), t.reshape(-1))


# ---------------------------------------------------------------- degenerate inputs
def test_a_strided_input_is_refused_and_takes_the_stock_path_in_the_module(ext, monkeypatch):
    from fots_e2e.native import DenseConv3x3, conv3x3_ok, use_native_conv3x3
    dtype = torch.bfloat16
    m = nn.Sequential(nn.Conv2d(6, 9, 3, padding=1, bias=False)).cuda().to(dtype).eval()
    assert use_native_conv3x3(m) == (1, 0) and type(m[0]) is DenseConv3x3
    calls = []
    run = ext._conv3x3_run
    monkeypatch.setattr(ext, "_conv3x3_run", lambda *a: calls.append(1) or run(*a))
    base = torch.randn(2, 6, 8, 20, device="cuda").to(dtype)
    view = base[:, :, :, ::2]
    with pytest.raises(ValueError):
        ext.conv3x3(view, m[0].weight.detach())
    with torch.no_grad():
        assert not conv3x3_ok(m[0], view)
        y = m(view)
        assert not calls and y.shape == (2, 9, 8, 10)
        z = m(view.contiguous())
        assert len(calls) == 1
    want, lim = C.bound(*C.reference(view.cpu(), m[0].weight.detach().cpu(), 1), 6, dtype, 1.0)
    assert C.within(z.cpu(), want, lim)[0]


def test_an_empty_batch_returns_without_a_launch(ext, monkeypatch):
    x, w = C.random_problem((1, 4, 6, 5, 7, 1), torch.float16, 1)
    monkeypatch.setattr(ext._lib, "rroi_conv3x3_forward_hip", None)       # calling it would raise
    assert ext.conv3x3(x[:0].cuda(), w.cuda()).shape == (0, 6, 5, 7)
    assert ext.conv3x3(x[:0].cuda(), w.cuda(), stride=2, negative_slope=0.0).shape == (0, 6, 3, 4)


# ---------------------------------------------------------------- determinism, capture
DET_CASES = [(3, 17, 96, 9, 33, 1), (1, 144, 96, 6, 8, 2)]


@pytest.mark.parametrize("case", DET_CASES, ids=C.case_id)
def test_repeated_calls_give_identical_bits(ext, case):
    for dtype in C.DTYPES:
        x, w = (t.cuda() for t in C.problem(case, dtype)[:2])
        first = ext.conv3x3(x, w, case[5], 0.01)
        for _ in range(3):
            assert torch.equal(C.bits(first), C.bits(ext.conv3x3(x, w, case[5], 0.01)))


def test_graph_capture_reproduces_the_eager_bits(ext):
    case, dtype = DET_CASES[0], torch.bfloat16
    x, w = (t.cuda() for t in C.problem(case, dtype)[:2])
    ext.conv3x3(x, w, 1, 0.0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):                # one call on one stream: a linear graph
            out = ext.conv3x3(x, w, 1, 0.0)
    x2, w2 = C.random_problem(case, dtype, seed=77)                # the inputs change in place
    x.copy_(x2), w.copy_(w2)
    out.fill_(NAN)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(C.bits(out), C.bits(ext.conv3x3(x, w, 1, 0.0))) and bool(out.isfinite().all())


# ---------------------------------------------------------------- in the network
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_the_switched_network_runs_the_kernel_on_its_own_tensors(ext, dtype, monkeypatch):
    """FOTSNet on a 64 x 96 image and its recogniser on four crops: hooks collect every switched convolution's real input
    and output; each output meets the bound against the reference of its own input (layer0_1's fused ReLU included), and
    every one of them came from the native call."""
    from fots_e2e.model import FOTSNet
    from fots_e2e import native as nat
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet()).eval().cuda().to(dtype)
    assert nat.use_native_conv3x3(net) == (23, 2)
    monkeypatch.setattr(nat, "_conv3x3_slower", lambda m, x: False)   # every shape class runs the kernel here
    launches = []
    run = ext._conv3x3_run
    monkeypatch.setattr(ext, "_conv3x3_run", lambda *a: launches.append(a[0].shape) or run(*a))
    seen = []
    hooks = [m.register_forward_hook(lambda m, i, o, name=name: seen.append((name, m, i[0].detach(), o.detach())))
             for name, m in net.named_modules() if type(m) is nat.DenseConv3x3]
    assert len(hooks) == 23
    g = torch.Generator().manual_seed(7)
    image = torch.randn(1, 3, 64, 96, generator=g).cuda().to(dtype)
    crops = torch.randn(4, 64, 11, 40, generator=g).cuda().to(dtype)
    with torch.no_grad():
        net(image)
        net.forward_ocr(crops)
    for h in hooks:
        h.remove()
    assert len(seen) == len(launches) == 18 + 8                   # conv6, conv8 and conv9 run twice per pass
    assert len({name for name, *_ in seen}) == 23
    worst = 0.0
    for name, m, x, y in seen:
        slope = 1.0 if m.fused_slope is None else m.fused_slope
        assert (slope == 0.0) == name.startswith("layer0_1.")
        ref, S = C.reference(x.cpu(), m.weight.detach().cpu(), m.stride[0])
        want, lim = C.bound(ref, S, m.in_channels, dtype, slope)
        ok, ratio = C.within(y.cpu(), want, lim)
        print(f"{name} {tuple(x.shape)} -> {tuple(y.shape)}: worst error / bound {ratio:.3f}")
        assert ok and ratio <= 1.0 and bool(y.isfinite().all()), (name, ratio)
        worst = max(worst, ratio)
    print(f"worst error / bound in the network: {worst:.4f}")
    # a gradient is needed: the stock path
    before = len(launches)
    xg = seen[0][2].clone().requires_grad_(True)
    assert not nat.conv3x3_ok(seen[0][1], xg) and seen[0][1](xg).requires_grad and len(launches) == before
    assert nat.use_native_conv3x3(net, False) == (23, 2)


def test_one_inference_chain_with_all_six_switches_returns_as_many_words(ext, monkeypatch):
    """`infer_image` in bfloat16 on a small image with the synthetic detector's maps: with all six switches on the chain
    completes, the native convolution runs in it, and it finds and recognises as many words as the stock chain."""
    from e2e_inputs import synthetic_detector_maps
    from fots_e2e import native as nat
    from fots_e2e.alphabet import ALPHABET
    from fots_e2e.model import FOTSNet
    from fots_e2e.pipeline import infer_image
    from fots_e2e.weights import deterministic_init
    from rroi_align.decode import CTCLabelConverter
    dev = torch.device("cuda", 0)
    net = deterministic_init(FOTSNet(len(ALPHABET) + 1)).eval().to(dev).to(torch.bfloat16)
    conv = CTCLabelConverter(ALPHABET)
    size = (256, 384)
    torch.manual_seed(4)
    im_data = (torch.rand(1, 3, *size, device=dev) * 2 - 1).to(torch.bfloat16)
    maps = tuple(torch.from_numpy(a).to(dev) for a in synthetic_detector_maps(size[0], size[1], 6, seed=7))
    hook = lambda _x: maps  # noqa: E731
    launches = []
    run = ext._conv3x3_run
    monkeypatch.setattr(ext, "_conv3x3_run", lambda *a: launches.append(1) or run(*a))
    with torch.no_grad():
        _, _, (boxes0, out0, _) = infer_image(net, conv, im_data, detector=hook, return_debug=True)
        assert not launches
        assert nat.use_native_depthwise(net) == 22 and nat.use_native_instancenorm(net) == (52, 20)
        assert nat.use_native_heads(net) and nat.use_native_merge(net) and nat.use_native_blocks(net) == (2, 7, 10)
        assert nat.use_native_conv3x3(net) == (23, 2)
        _, _, (boxes1, out1, _) = infer_image(net, conv, im_data, detector=hook, return_debug=True)
    assert launches, "the native convolution did not run"
    assert len(boxes0) >= 3, "the synthetic detector maps must yield boxes"
    assert len(boxes1) == len(boxes0) and len(out1[0]) == len(out0[0]) == len(boxes0)
