"""GPU (MI355X): the native 1x1 convolution with its folded BatchNorm against the float64 reference and the
two bounds of conv1x1_cases.py over the whole table, the exact-integer table bit for bit, special values, misaligned views
inside a guarded buffer, degenerate inputs, determinism, graph capture, the switched network on the tensors it really
sees, and one inference chain with all eight switches on.

Worst |y - want| / bound observed over the table on an MI355X: plain bf16 0.9960, fp16 0.9987; with a norm 0.9957 / 0.9951
(profiles/native_conv1x1.md); both bounds are dominated by the one rounding to the type, which reaches it at the bottom of
a binade."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv1x1_cases as C
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


def on_gpu(norm):
    return None if norm is None else tuple(None if v is None else v.cuda() for v in norm[:4]) + (norm[4],)


# ---------------------------------------------------------------- against the reference
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_the_whole_table_meets_the_bounds_and_the_integer_table_every_bit(ext, dtype):
    worst = {False: 0.0, True: 0.0}
    for case in C.CASES:
        N, Cin, Cout, H, W, s = case
        x, w, ref, A = C.problem(case, dtype)
        p = ext.conv1x1_plan(N, Cin, Cout, H, W, s, dtype=dtype)
        assert (p.tile_m, p.k_chunks, p.grid_x) == C.plan_of(case)
        xg, wg = x.cuda(), w.cuda()
        for norm in (None, C.norm_of(case, dtype)):
            ng = on_gpu(norm)
            for slope in C.SLOPES:
                got = ext.conv1x1(xg, wg, s, slope, ng)
                assert got.shape == ref.shape and got.dtype == dtype and got.is_contiguous()
                got = got.cpu()
                want, lim = C.bound(ref, A, Cin, dtype, slope, norm)
                ok, ratio = C.within(got, want, lim)
                print(f"{C.case_id(case)} slope={slope} norm={norm is not None} tile={p.tile_m}x128: "
                      f"worst error / bound {ratio:.3f}")
                assert bool(got.isfinite().all()) and ok and ratio <= 1.0, (case, slope, norm is not None, ratio)
                worst[norm is not None] = max(worst[norm is not None], ratio)
        xe, we, refe = C.exact_problem(case, dtype)
        for slope in (1.0, 0.0):
            got = ext.conv1x1(xe.cuda(), we.cuda(), s, slope).cpu()
            want = C.act64(refe, slope).to(dtype)                  # integers of magnitude <= 144: exact in the type
            assert torch.equal(want.double(), C.act64(refe, slope))
            wrong = int((got.double() != want.double()).sum())     # (-0.0 of a ReLU equals 0.0)
            assert wrong == 0, (case, slope, wrong)
    print(f"worst error / bound over the table: plain {worst[False]:.4f}, with a norm {worst[True]:.4f}")


def test_a_two_dimensional_weight_and_out_give_the_same_bits(ext):
    case, dtype = (2, 17, 32, 5, 7, 1), torch.float16
    x, w = (t.cuda() for t in C.problem(case, dtype)[:2])
    want = ext.conv1x1(x, w, 1, 0.01)
    out = torch.full_like(want, NAN)
    assert ext.conv1x1(x, w.reshape(32, 17), 1, 0.01, out=out) is out and torch.equal(C.bits(out), C.bits(want))


# ---------------------------------------------------------------- special values
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_non_finite_inputs_poison_their_own_pixel_and_no_other(ext, dtype, stride):
    case = (2, 17, 48, 11, 37, stride)
    x, w = C.random_problem(case, dtype, seed=11)
    w = torch.where(w == 0, torch.ones_like(w), w)                 # no zero weight: every channel of the pixel is poisoned
    clean = ext.conv1x1(x.cuda(), w.cuda(), stride, 0.01).cpu()
    bad = x.clone()
    spots = ((0, 3, 0, 0, NAN), (0, 16, 4, 20, INF), (1, 0, 10, 36, -INF), (1, 9, 6, 32, NAN), (1, 5, 5, 33, NAN))
    for n, c, i, j, v in spots:                                    # (the last one lies on no stride-2 output pixel)
        bad[n, c, i, j] = v
    got = ext.conv1x1(bad.cuda(), w.cuda(), stride, 0.01).cpu()
    hit = torch.zeros_like(bad, dtype=torch.float32)
    for n, c, i, j, _ in spots:
        hit[n, :, i, j] = 1.0
    poisoned = F.conv2d(hit, torch.ones(48, 17, 1, 1), stride=stride) > 0
    assert int(poisoned.sum()) == 48 * (5 if stride == 1 else 4)
    assert torch.equal(~got.isfinite(), poisoned)                  # all Cout of the pixel, nothing else
    ref = C.act64(C.reference(bad, w, stride)[0], 0.01)
    assert torch.equal(got.isnan(), ref.isnan())
    inf_at = got.isinf()
    assert torch.equal(got[inf_at].double(), ref[inf_at])
    assert torch.equal(C.bits(got)[~poisoned], C.bits(clean)[~poisoned])


# ---------------------------------------------------------------- addresses and guards
@pytest.mark.parametrize("case", [(2, 24, 7, 8, 35, 1), (1, 17, 33, 10, 66, 2), (1, 72, 40, 4, 64, 1)], ids=C.case_id)
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_views_and_guards(ext, dtype, case):
    """x, w, y and the four norm vectors 0 .. 7 elements past a 16-byte boundary, through the raw ABI; y inside a guarded
    buffer.  Every output element is written, no guard byte is, the inputs are unchanged and the bits do not depend on an
    address.  (Cin 24 and 72 with planes of 280 and 256 elements: 16-byte loads of x and of w where the address allows.)"""
    N, Cin, Cout, H, W, s = case
    x, w = C.random_problem(case, dtype, seed=sum(case))
    norm = C.random_norm(Cout, dtype, "affine", seed=5)
    Ho, Wo = C.out_size(H, W, s)
    n = N * Cout * Ho * Wo
    stream = torch.cuda.current_stream().cuda_stream
    want = ext.conv1x1(x.cuda(), w.cuda(), s, 0.01, on_gpu(norm))

    def shifted(t, off):
        buf = torch.zeros(t.numel() + 16, dtype=dtype, device="cuda")
        view = buf[off:off + t.numel()]
        view.copy_(t.reshape(-1))
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + off * t.element_size()
        return buf, view

    for ox, ow, oy, ov in ((0, 0, 0, (0, 0, 0, 0)), (1, 1, 1, (1, 2, 3, 4)), (3, 2, 5, (7, 0, 5, 6)), (7, 5, 2, (3, 3, 1, 0)),
                           (4, 3, 7, (2, 6, 4, 7)), (0, 4, 6, (5, 1, 7, 2)), (2, 0, 3, (4, 4, 0, 1)), (5, 6, 4, (6, 7, 2, 3)),
                           (6, 7, 0, (0, 5, 6, 5))):
        pairs = [shifted(x, ox), shifted(w, ow)] + [shifted(v, o) for v, o in zip(norm[:4], ov)]
        buf = torch.full((64 + oy + n + 64,), NAN_PATTERN[dtype], dtype=torch.int16, device="cuda")
        before = buf.clone()
        y = buf[64 + oy:64 + oy + n].view(dtype)
        st = ext._lib.rroi_conv1x1_forward_hip(ext.dtype_code(dtype), pairs[0][1].data_ptr(), pairs[1][1].data_ptr(),
                                               y.data_ptr(), N, Cin, Cout, H, W, s, 0.01, pairs[2][1].data_ptr(),
                                               pairs[3][1].data_ptr(), pairs[4][1].data_ptr(), pairs[5][1].data_ptr(),
                                               norm[4], stream)
        torch.cuda.synchronize()
        assert st == 1
        assert torch.equal(buf[:64 + oy], before[:64 + oy]) and torch.equal(buf[64 + oy + n:], before[64 + oy + n:]), \
            "a byte outside the output was written"
        assert not (buf[64 + oy:64 + oy + n] == before[64 + oy:64 + oy + n]).any(), "an output element was left unwritten"
        assert same_bits(y.view(N, Cout, Ho, Wo), want), (ox, ow, oy, ov)
        for (b, v), t, off in zip(pairs, (x, w) + tuple(norm[:4]), (ox, ow) + ov):   # the inputs are unchanged
            assert bool((b[:off] == 0).all()) and bool((b[off + t.numel():] == 0).all()) and torch.equal(v.cpu(), t.reshape(-1))


# ---------------------------------------------------------------- degenerate inputs
def test_a_strided_input_is_refused_and_takes_the_stock_path_in_the_module(ext, monkeypatch):
    from fots_e2e.native import PointwiseConv1x1, conv1x1_ok, use_native_conv1x1
    dtype = torch.bfloat16
    m = nn.Sequential(nn.Conv2d(6, 9, 1, bias=False)).cuda().to(dtype).eval()
    assert use_native_conv1x1(m) == (1, 0) and type(m[0]) is PointwiseConv1x1
    calls = []
    run = ext._conv1x1_run
    monkeypatch.setattr(ext, "_conv1x1_run", lambda *a: calls.append(1) or run(*a))
    base = torch.randn(2, 6, 8, 20, device="cuda").to(dtype)
    view = base[:, :, :, ::2]
    with pytest.raises(ValueError):
        ext.conv1x1(view, m[0].weight.detach())
    with torch.no_grad():
        assert not conv1x1_ok(m[0], view)
        y = m(view)
        assert not calls and y.shape == (2, 9, 8, 10)
        zc = m(view.contiguous())
        assert len(calls) == 1
    want, lim = C.bound(*C.reference(view.cpu(), m[0].weight.detach().cpu(), 1), 6, dtype, 1.0)
    assert C.within(zc.cpu(), want, lim)[0]


def test_an_empty_batch_returns_without_a_launch(ext, monkeypatch):
    x, w = C.random_problem((1, 4, 6, 5, 7, 1), torch.float16, 1)
    norm = on_gpu(C.random_norm(6, torch.float16, "affine", 1))
    monkeypatch.setattr(ext._lib, "rroi_conv1x1_forward_hip", None)       # calling it would raise
    assert ext.conv1x1(x[:0].cuda(), w.cuda()).shape == (0, 6, 5, 7)
    assert ext.conv1x1(x[:0].cuda(), w.cuda(), stride=2, negative_slope=0.0, norm=norm).shape == (0, 6, 3, 4)


# ---------------------------------------------------------------- determinism, capture
DET_CASES = [(3, 144, 96, 9, 33, 1), (2, 17, 32, 5, 85, 2)]


@pytest.mark.parametrize("case", DET_CASES, ids=C.case_id)
def test_repeated_calls_give_identical_bits(ext, case):
    for dtype in C.DTYPES:
        x, w = (t.cuda() for t in C.problem(case, dtype)[:2])
        norm = on_gpu(C.norm_of(case, dtype))
        first = ext.conv1x1(x, w, case[5], 0.01, norm)
        for _ in range(3):
            assert torch.equal(C.bits(first), C.bits(ext.conv1x1(x, w, case[5], 0.01, norm)))


def test_graph_capture_reproduces_the_eager_bits(ext):
    case, dtype = DET_CASES[0], torch.bfloat16
    x, w = (t.cuda() for t in C.problem(case, dtype)[:2])
    norm = on_gpu(C.norm_of(case, dtype))
    ext.conv1x1(x, w, 1, 0.0, norm)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):                # one call on one stream: a linear graph
            out = ext.conv1x1(x, w, 1, 0.0, norm)
    x2, w2 = C.random_problem(case, dtype, seed=77)                # the inputs change in place
    x.copy_(x2), w.copy_(w2)
    norm[2].mul_(-1.0)
    out.fill_(NAN)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(C.bits(out), C.bits(ext.conv1x1(x, w, 1, 0.0, norm))) and bool(out.isfinite().all())


# ---------------------------------------------------------------- in the network
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_the_switched_network_runs_the_kernel_on_its_own_tensors(ext, dtype, monkeypatch):
    """FOTSNet on a 64 x 96 image: hooks collect the real input and output of every switched convolution that is called as
    a module (26) and of every switched shortcut (3, which call the kernel with their norm folded in); each output meets
    its bound against the reference of its own input, and every one of them came from the native call."""
    from fots_e2e.model import FOTSNet
    from fots_e2e import native as nat
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet()).eval().cuda().to(dtype)
    assert nat.use_native_conv1x1(net) == (29, 3)
    monkeypatch.setattr(nat, "_conv1x1_slower", lambda m, x: False)   # every shape class runs the kernel here
    launches = []
    run = ext._conv1x1_run

    def counted(x, weight, stride, negative_slope=1.0, norm=None, out=None):
        launches.append((weight.data_ptr(), norm is not None))
        return run(x, weight, stride, negative_slope, norm, out)

    monkeypatch.setattr(ext, "_conv1x1_run", counted)
    seen = []
    hooks = [m.register_forward_hook(lambda m, i, o, name=name: seen.append((name, m, i[0].detach(), o.detach())))
             for name, m in net.named_modules() if type(m) in (nat.PointwiseConv1x1, nat.NativeShortcut)]
    assert len(hooks) == 29 + 3
    g = torch.Generator().manual_seed(7)
    image = torch.randn(1, 3, 64, 96, generator=g).cuda().to(dtype)
    with torch.no_grad():
        net(image)
    for h in hooks:
        h.remove()
    assert len(seen) == len(launches) == 29                        # 26 convolutions called as modules + 3 shortcuts
    assert len({ptr for ptr, _ in launches}) == 29                 # 29 distinct convolutions
    assert sum(folded for _, folded in launches) == 3              # three of them with the norm folded in
    worst = 0.0
    for name, m, x, y in seen:
        if type(m) is nat.NativeShortcut:
            conv, bn = m[0], m[1]
            norm = tuple(v.detach().cpu() for v in (bn.weight, bn.bias, bn.running_mean, bn.running_var)) + (bn.eps,)
            assert name.endswith(".downsample") and (conv.weight.data_ptr(), True) in launches
        else:
            conv, norm = m, None
            assert "downsample" not in name and (conv.weight.data_ptr(), False) in launches
        ref, A = C.reference(x.cpu(), conv.weight.detach().cpu(), conv.stride[0])
        want, lim = C.bound(ref, A, conv.in_channels, dtype, 1.0, norm)
        ok, ratio = C.within(y.cpu(), want, lim)
        print(f"{name} {tuple(x.shape)} -> {tuple(y.shape)}: worst error / bound {ratio:.3f}")
        assert ok and ratio <= 1.0 and bool(y.isfinite().all()), (name, ratio)
        worst = max(worst, ratio)
    print(f"worst error / bound in the network: {worst:.4f}")
    # a gradient is needed: the stock path, for a convolution and for a shortcut
    before = len(launches)
    for name, m, x, _ in (seen[0], next(s for s in seen if type(s[1]) is nat.NativeShortcut)):
        xg = x.clone().requires_grad_(True)
        assert m(xg).requires_grad and len(launches) == before, name
    assert nat.use_native_conv1x1(net, False) == (29, 3)


def test_one_inference_chain_with_all_eight_switches_returns_as_many_words(ext, monkeypatch):
    """`infer_image` in bfloat16 on a small image with the synthetic detector's maps: with all eight switches on the chain
    completes, the native 1x1 convolution runs in it, and it finds and recognises as many words as the stock chain."""
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
    run = ext._conv1x1_run
    monkeypatch.setattr(ext, "_conv1x1_run", lambda *a: launches.append(1) or run(*a))
    monkeypatch.setattr(nat, "_conv1x1_slower", lambda m, x: False)
    with torch.no_grad():
        _, _, (boxes0, out0, _) = infer_image(net, conv, im_data, detector=hook, return_debug=True)
        assert not launches
        assert nat.use_native_depthwise(net) == 22 and nat.use_native_instancenorm(net) == (52, 20)
        assert nat.use_native_heads(net) and nat.use_native_merge(net) and nat.use_native_blocks(net) == (2, 7, 10)
        assert nat.use_native_conv3x3(net) == (23, 2) and nat.use_native_recogniser(net)
        assert nat.use_native_conv1x1(net) == (29, 3)
        _, _, (boxes1, out1, _) = infer_image(net, conv, im_data, detector=hook, return_debug=True)
    assert launches, "the native 1x1 convolution did not run"
    assert len(boxes0) >= 3, "the synthetic detector maps must yield boxes"
    assert len(boxes1) == len(boxes0) and len(out1[0]) == len(out0[0]) == len(boxes0)
