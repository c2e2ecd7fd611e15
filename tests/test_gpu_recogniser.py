"""GPU (MI355X): the native recogniser head and the activation + (2,1) max-pool against the references of
recogniser_cases.py: the bound and the bit count of the head's contract over the whole table, saturated logits, poisoned
columns, the pool bit for bit against torch, misaligned views inside guarded buffers, determinism, graph capture, the
switched network on the tensors it really sees, and one inference chain."""
import pytest
import torch
import torch.nn.functional as F

import recogniser_cases as RC
from test_gpu_bucketed import NAN_PATTERN

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def cuda(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def same_bits(got, want):
    d, nan_ok = RC.differing(got.cpu(), want.cpu())
    return d == 0 and nan_ok


# ---------------------------------------------------------------- the head against the reference: conditions (a) and (b)
@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_head_against_the_reference_over_the_whole_table(ext, dtype):
    """Every case: (a) every finite element within recogniser_cases.head_bound of the float64 value, NaN positions equal;
    (b) over the whole table at most 1 element in 10^4, of at least 10^6, differs in bits from the rounded reference."""
    total = differ = 0
    worst_ratio = 0.0
    for case in RC.HEAD_CASES:
        N, C, K, T, _ = case
        x, w, b, want, R = RC.head_problem(case, dtype)
        S, tiles, grid, lds = RC.head_plan_of(N, C, K, T)
        p = ext.ocr_head_plan(N, C, K, T, dtype=dtype)
        assert (p.waves, p.tiles, p.grid_x, p.block, p.lds_bytes) == (S, tiles, grid, 64 * S, lds)
        got = ext.ocr_head(*cuda(x, w, b)).cpu()
        assert got.shape == want.shape == (N, K, T) and got.dtype == dtype
        d, nan_ok = RC.differing(got, want)
        ok, worst = RC.within(got, R.out64, RC.head_bound(R, dtype))
        print(f"{RC.case_id(case)} S={S}: {d} of {got.numel()} differ, worst error / bound {worst:.3f}")
        assert nan_ok and bool(got.isfinite().all()), case
        assert ok and worst <= 1.0, (case, worst)
        total += got.numel()
        differ += d
        worst_ratio = max(worst_ratio, worst)
    print(f"{dtype}: {differ} of {total} elements differ in bits from the reference; worst error / bound {worst_ratio:.4f}")
    assert total >= 10 ** 6 and differ * 10 ** 4 <= total, (differ, total)


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_saturated_logits_a_null_bias_and_a_single_class(ext, dtype):
    """Logits of +-800 through a NULL bias: no NaN, no overflow, the maximum's class at exactly 0 where it stands alone.  A
    one-class head returns exact zeros whatever its logit."""
    zs = torch.tensor([800.0, -800.0, 0.0, 1.0, -1.0, 700.0, 40.0], dtype=dtype)
    x = torch.zeros(2, 2, 1, 5, dtype=dtype)
    x[:, 0, 0] = torch.tensor([1.0, -1.0, 0.5, 0.0, 0.001], dtype=dtype)
    w = torch.stack([zs, torch.zeros_like(zs)], dim=1)            # z[k][t] = zs[k] * x[0][t]
    got = ext.ocr_head(*cuda(x, w), None).cpu()
    want, R = RC.head_reference(x, w, None)
    assert bool(got.isfinite().all()) and RC.differing(got, want)[1]
    assert RC.within(got, R.out64, RC.head_bound(R, dtype))[0]
    g = got.double()
    assert float(g[0, 0, 0]) == 0.0 and float(g[0, 1, 0]) == -1600.0                            # x = 1: 800 stands alone
    assert float(g[0, 1, 1]) == 0.0 and float(g[0, 0, 1]) == -1600.0                            # x = -1: so does -(-800)
    assert bool((g[:, :, 3] == g[0, 0, 3]).all()) and -1.96 < float(g[0, 0, 3]) < -1.93         # x = 0: -log 7 everywhere
    for C, T in ((1, 1), (5, 70), (256, 33)):
        x1, w1, b1 = RC.head_problem_of(3, C, 1, T, dtype, seed=C + T)
        for bias in (b1, None):
            y = ext.ocr_head(*cuda(x1, w1 * 50, bias))
            assert y.shape == (3, 1, T) and bool((RC.bits(y.cpu()) == 0).all())                 # +0.0 exactly


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_poisoned_columns_take_their_own_outputs_and_no_other(ext, dtype):
    """C = 70 is chunks of 32, 32 and 6 channels, K = 43 two waves (rows of 8, 8, 8, 8 and 8, 3, 0, 0 classes), T = 70 five
    tiles.  A NaN, a +inf and a -inf in the first channel, the last channel, either side of the chunk boundaries 31 | 32 and
    63 | 64 and of the lane boundary 15 | 16 of single columns: those columns equal the reference (all NaN), every other
    column keeps the clean run's bits.  A -inf bias either side of the row boundary 7 | 8 and of the wave boundary 31 | 32
    gives -inf in those classes and the reference's bits elsewhere; a +inf bias takes every column."""
    N, C, K, T = 2, 70, 43, 70
    assert RC.head_plan_of(N, C, K, T)[:2] == (2, 5)
    x, w, b = RC.head_problem_of(N, C, K, T, dtype, seed=21)
    clean = ext.ocr_head(*cuda(x, w, b)).cpu()
    assert bool(clean.isfinite().all())
    poisoned = {3: (0, NAN), 10: (69, INF), 20: (31, -INF), 30: (32, NAN), 40: (0, -INF), 50: (69, NAN), 60: (32, INF), 63: (15, INF),
                64: (16, -INF), 66: (31, INF), 67: (63, NAN), 69: (64, -INF)}
    for t, (c, v) in poisoned.items():
        x[t % N, c, 0, t] = v
    got = ext.ocr_head(*cuda(x, w, b)).cpu()
    want, R = RC.head_reference(x, w, b)
    touched = torch.zeros(N, T, dtype=torch.bool)
    for t in poisoned:
        touched[t % N, t] = True
    mask = touched[:, None, :].expand(N, K, T)
    assert same_bits(got[~mask], clean[~mask])
    assert bool(got[mask].isnan().all()) and RC.differing(got, want)[1]
    assert RC.within(got, R.out64, RC.head_bound(R, dtype))[0]
    # the bias: classes 7 | 8, the last of a row of lanes and the first of the next, and 31 | 32, likewise of a wave
    x, w, b = RC.head_problem_of(N, C, K, T, dtype, seed=22)
    b[7] = b[8] = b[31] = b[32] = -INF
    got = ext.ocr_head(*cuda(x, w, b)).cpu()
    want, R = RC.head_reference(x, w, b)
    lost = torch.zeros(K, dtype=torch.bool)
    lost[[7, 8, 31, 32]] = True
    assert bool((got[:, lost] == -INF).all()) and bool(got[:, ~lost].isfinite().all())
    assert RC.differing(got, want)[1] and RC.within(got, R.out64, RC.head_bound(R, dtype))[0]
    assert bool((got.isinf() == want.isinf()).all())
    b[42] = INF
    assert bool(ext.ocr_head(*cuda(x, w, b)).isnan().all())


# ---------------------------------------------------------------- the pool
def equals_stock_on_device(got, x, slope):
    """`got` against torch's expression on x's device, bit for bit -- with one exception that is torch's, not the kernel's.
    In float16 `F.leaky_relu` on the GPU returns +0.0 wherever the rule v < 0 ? v * s : v (and torch's own CPU kernel, and
    its GPU kernel in float32 and bfloat16) gives -0.0: for v = -0.0 at any slope, slope 1.0 included, and for every v < 0
    at slope 0.0 (measured: 9,989 such elements of the (2, 64, 5, 33) case at slope 0.0, 642 at slope 1.0; no element
    differs in anything but that sign).  So in float16 the two may differ where both are zero, and nowhere else; the plain
    pool (slope 1.0) is compared with `F.max_pool2d` alone, which has no such exception in any type."""
    got = got.cpu()
    if slope == 1.0:
        plain = F.max_pool2d(x, (2, 1), stride=(2, 1)).cpu()
        if RC.differing(got, plain) != (0, True):
            return False
    stock = RC.pool_stock(x, slope).cpu()
    d, nan_ok = RC.differing(got, stock)
    if x.dtype != torch.float16:
        return d == 0 and nan_ok
    unequal = (RC.bits(got) != RC.bits(stock)) & ~(got.isnan() & stock.isnan())
    return nan_ok and bool(((got == 0) & (stock == 0))[unequal].all())


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_pool_equals_torch_and_the_cpu_reference_bit_for_bit(ext, dtype):
    for case in RC.POOL_CASES:
        x = RC.pool_problem(case, dtype)
        xg = x.cuda()
        for slope in RC.SLOPES:
            got = ext.act_maxpool2x1(xg, slope)
            assert got.shape == (case[0], case[1], case[2] // 2, case[3]) and got.dtype == dtype
            assert RC.differing(got.cpu(), RC.pool_reference(x, slope)) == (0, True), (case, slope)
            assert equals_stock_on_device(got, xg, slope), (case, slope)
    # the planted pairs: a tie of signed zeros keeps the upper row's element
    x = RC.pool_problem((1, 1, 2, 16), dtype)
    y = ext.act_maxpool2x1(x.cuda(), 1.0).cpu()[0, 0, 0]
    assert float(y[1]) == 0.0 and RC.bits(y[1:2]).item() == 0 and RC.bits(y[4:5]).item() != 0 and float(y[4]) == 0.0
    assert bool(y[2].isnan()) and bool(y[8].isnan()) and float(y[3]) == 1.0 and float(y[12]) == 1.0


# ---------------------------------------------------------------- addresses and guards
@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_head_views_and_guards(ext, dtype):
    """x, w, b and y 0 .. 3 elements past a 16-byte boundary, through the raw ABI, y inside a guard-patterned buffer: every
    output element is written, no guard element is, and the bits do not depend on an address."""
    N, C, K, T = 3, 37, 43, 65
    x, w, b = RC.head_problem_of(N, C, K, T, dtype, seed=5)
    want, R = RC.head_reference(x, w, b)
    lim = RC.head_bound(R, dtype)
    itype = torch.int32 if dtype == torch.float32 else torch.int16
    stream = torch.cuda.current_stream().cuda_stream
    first = None
    for ox, ow, oy in ((0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 0, 3), (0, 3, 1), (2, 1, 0)):
        views = []
        for t, off in ((x, ox), (w, ow), (b, ow ^ 1)):
            buf = torch.zeros(t.numel() + 8, dtype=dtype, device="cuda")
            assert buf.data_ptr() % 16 == 0
            v = buf[off:off + t.numel()]
            v.copy_(t.reshape(-1))
            views.append(v)
        n = N * K * T
        ybuf = torch.full((64 + oy + n + 64,), NAN_PATTERN[dtype], dtype=itype, device="cuda")
        before = ybuf.clone()
        y = ybuf[64 + oy:64 + oy + n].view(dtype)
        st = ext._lib.rroi_ocr_head_forward_hip(ext.dtype_code(dtype), *(v.data_ptr() for v in views), y.data_ptr(), N, C, K, T,
                                                stream)
        torch.cuda.synchronize()
        assert st == 1
        assert torch.equal(ybuf[:64 + oy], before[:64 + oy]) and torch.equal(ybuf[64 + oy + n:], before[64 + oy + n:])
        assert not (ybuf[64 + oy:64 + oy + n] == before[64 + oy:64 + oy + n]).any(), "an output element was left unwritten"
        got = y.cpu().view(N, K, T)
        assert RC.differing(got, want)[1] and RC.within(got, R.out64, lim)[0], (ox, ow, oy)
        first = got if first is None else first
        assert same_bits(got, first), (ox, ow, oy)


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_pool_views_and_guards(ext, dtype):
    itype = torch.int32 if dtype == torch.float32 else torch.int16
    stream = torch.cuda.current_stream().cuda_stream
    for case in ((2, 3, 11, 40), (1, 3, 5, 33), (2, 1, 3, 7)):
        N, C, H, W = case
        x = torch.randn(*case, generator=torch.Generator().manual_seed(9)).to(dtype)
        want = RC.pool_reference(x, 0.01)
        n = want.numel()
        for ox, oy in ((0, 0), (1, 1), (2, 2), (3, 3), (1, 0), (0, 3), (5, 2)):
            xb = torch.zeros(x.numel() + 8, dtype=dtype, device="cuda")
            xv = xb[ox:ox + x.numel()]
            xv.copy_(x.reshape(-1))
            ybuf = torch.full((64 + oy + n + 64,), NAN_PATTERN[dtype], dtype=itype, device="cuda")
            before = ybuf.clone()
            y = ybuf[64 + oy:64 + oy + n].view(dtype)
            st = ext._lib.rroi_act_maxpool2x1_forward_hip(ext.dtype_code(dtype), xv.data_ptr(), y.data_ptr(), N, C, H, W, 0.01,
                                                          stream)
            torch.cuda.synchronize()
            assert st == 1
            assert torch.equal(ybuf[:64 + oy], before[:64 + oy]) and torch.equal(ybuf[64 + oy + n:], before[64 + oy + n:])
            assert not (ybuf[64 + oy:64 + oy + n] == before[64 + oy:64 + oy + n]).any(), "an output element was left unwritten"
            assert same_bits(y.cpu().view(want.shape), want), (case, ox, oy)
            assert torch.equal(xv.cpu(), x.reshape(-1))


# ---------------------------------------------------------------- determinism, capture, the empty batch
def chain_problem(dtype, seed):
    """A pool whose output is the head's input: (3, 256, 2, 65) -> (3, 256, 1, 65) -> (3, 87, 65)."""
    x = torch.randn(3, 256, 2, 65, generator=torch.Generator().manual_seed(seed)).to(dtype)
    _, w, b = RC.head_problem_of(3, 256, 87, 65, dtype, seed)
    return x, w, b


def test_repeated_calls_give_identical_bits(ext):
    for dtype in RC.DTYPES:
        x, w, b = cuda(*chain_problem(dtype, 31))
        first = ext.ocr_head(ext.act_maxpool2x1(x, 0.01), w, b)
        for _ in range(3):
            assert same_bits(ext.ocr_head(ext.act_maxpool2x1(x, 0.01), w, b), first)


def test_graph_capture_of_both_kernels_reproduces_the_eager_bits(ext):
    dtype = torch.bfloat16
    x, w, b = cuda(*chain_problem(dtype, 32))
    ext.ocr_head(ext.act_maxpool2x1(x, 0.01), w, b)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):                # two calls on one stream: a linear graph
            mid = ext.act_maxpool2x1(x, 0.01)
            out = ext.ocr_head(mid, w, b)
    x.copy_(chain_problem(dtype, 77)[0])                          # the input changes in place
    mid.fill_(NAN), out.fill_(NAN)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want_mid = ext.act_maxpool2x1(x, 0.01)
    assert same_bits(mid, want_mid) and same_bits(out, ext.ocr_head(want_mid, w, b)) and bool(out.isfinite().all())


def test_empty_batch_returns_without_a_call(ext, monkeypatch):
    x, w, b = cuda(*RC.head_problem_of(2, 6, 5, 9, torch.float32, 1))
    monkeypatch.setattr(ext._lib, "rroi_ocr_head_forward_hip", None)         # calling it would raise
    monkeypatch.setattr(ext._lib, "rroi_act_maxpool2x1_forward_hip", None)
    assert ext.ocr_head(x[:0], w, b).shape == (0, 5, 9)
    assert ext.act_maxpool2x1(torch.zeros(0, 3, 5, 7, device="cuda"), 0.01).shape == (0, 3, 2, 7)


# ---------------------------------------------------------------- in the network
def all_seven(net):
    from fots_e2e import native as nat
    assert nat.use_native_depthwise(net) == 22 and nat.use_native_instancenorm(net) == (52, 20)
    assert nat.use_native_heads(net) and nat.use_native_merge(net) and nat.use_native_blocks(net) == (2, 7, 10)
    assert nat.use_native_conv3x3(net) == (23, 2) and nat.use_native_recogniser(net)


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_the_switched_network_runs_the_kernels_on_its_own_tensors(ext, dtype, monkeypatch):
    """FOTSNet's recogniser on four crops with all seven switches on and every shape class of the convolution allowed: the
    native calls of one `forward_ocr` are counted with their slopes; each head and pool call meets its contract against the
    reference of its own input; a call that needs a gradient and a network in training mode run none of them."""
    from fots_e2e import native as nat
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet()).eval().cuda().to(dtype)
    all_seven(net)
    assert type(net) is nat.NativeHeadsMergeRecogniserFOTSNet
    monkeypatch.setattr(nat, "_conv3x3_slower", lambda m, x: False)   # every shape class runs its kernel here, the new
    monkeypatch.setattr(nat, "_act_pool_slower", lambda x, slope: False)   # hooks' included: this test is about the wiring
    monkeypatch.setattr(nat, "_ocr_head_slower", lambda m, x: False)
    calls = {"conv": [], "norm": [], "pool": [], "head": [], "leaky": []}
    conv_run, norm_run, pool_run, head_run, leaky = (ext._conv3x3_run, ext._instance_norm_run, ext._act_maxpool2x1_run,
                                                     ext._ocr_head_run, F.leaky_relu)

    def conv(x, w, stride, slope=1.0, out=None):
        calls["conv"].append(slope)
        return conv_run(x, w, stride, slope, out)

    def norm(x, w, b, eps, slope):
        calls["norm"].append(slope)
        return norm_run(x, w, b, eps, slope)

    def pool(x, slope=1.0):
        y = pool_run(x, slope)
        calls["pool"].append((slope, x.detach(), y))
        return y

    def head(x, w, b=None, out=None):
        y = head_run(x, w, b, out)
        calls["head"].append((x.detach(), y))
        return y

    def counted_leaky(*a, **k):
        calls["leaky"].append(1)
        return leaky(*a, **k)
    monkeypatch.setattr(ext, "_conv3x3_run", conv)
    monkeypatch.setattr(ext, "_instance_norm_run", norm)
    monkeypatch.setattr(ext, "_act_maxpool2x1_run", pool)
    monkeypatch.setattr(ext, "_ocr_head_run", head)
    monkeypatch.setattr(F, "leaky_relu", counted_leaky)
    crops = torch.randn(4, 64, 11, 40, generator=torch.Generator().manual_seed(7)).cuda().to(dtype)
    with torch.no_grad():
        out = net.forward_ocr(crops)
    assert out.shape == (4, 87, 40) and out.dtype == dtype and bool(out.isfinite().all())
    if dtype == torch.float32:
        assert calls["conv"] == [] and calls["norm"] == [0.01] * 3 and len(calls["leaky"]) == 4
        assert [s for s, _, _ in calls["pool"]] == [0.01, 0.01]
    else:
        # conv5 and conv7 stand in front of a norm, which takes the activation: slope 1.0 through their modules
        assert calls["conv"] == [1.0, 0.01, 0.01, 1.0, 0.01, 0.01, 0.01, 0.01]
        assert calls["norm"] == [0.01] * 3 and calls["leaky"] == []
        assert [s for s, _, _ in calls["pool"]] == [1.0, 1.0]
    assert [tuple(x.shape) for _, x, _ in calls["pool"]] == [(4, 128, 11, 40), (4, 256, 5, 40)] and len(calls["head"]) == 1
    for slope, x, y in calls["pool"]:
        assert same_bits(y, RC.pool_reference(x.cpu(), slope)) and equals_stock_on_device(y, x, slope)
    x, y = calls["head"][0]
    assert tuple(x.shape) == (4, 256, 1, 40) and y is out
    want, R = RC.head_reference(x.cpu(), net.conv11.weight.detach().cpu(), net.conv11.bias.detach().cpu())
    ok, worst = RC.within(y.cpu(), R.out64, RC.head_bound(R, dtype))
    d, nan_ok = RC.differing(y.cpu(), want)
    print(f"{dtype}: head on its own input: {d} of {y.numel()} differ, worst error / bound {worst:.3f}")
    assert ok and worst <= 1.0 and nan_ok
    # a gradient is needed: every step takes the stock expression
    counts = {k: len(v) for k, v in calls.items() if k != "leaky"}
    with_grad = net.forward_ocr(crops)
    assert with_grad.requires_grad and {k: len(v) for k, v in calls.items() if k != "leaky"} == counts
    # training mode: the stock method; what the module switches do inside it is theirs
    net.train()
    with torch.no_grad():
        net.forward_ocr(crops)
    net.eval()
    assert len(calls["head"]) == 1 and len(calls["pool"]) == 2
    assert nat.use_native_recogniser(net, False) and type(net) is nat.NativeHeadsMergeFOTSNet


def test_one_inference_chain_with_all_seven_switches_returns_as_many_words(ext, monkeypatch):
    """`infer_image` in bfloat16 on a small image with the synthetic detector's maps: with all seven switches on the chain
    completes, the head kernel runs in it, and it finds and recognises as many words as the stock chain."""
    from e2e_inputs import synthetic_detector_maps
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
    launches = {"head": 0, "pool": 0}
    head_run, pool_run = ext._ocr_head_run, ext._act_maxpool2x1_run

    def head(*a):
        launches["head"] += 1
        return head_run(*a)

    def pool(*a):
        launches["pool"] += 1
        return pool_run(*a)
    monkeypatch.setattr(ext, "_ocr_head_run", head)
    monkeypatch.setattr(ext, "_act_maxpool2x1_run", pool)
    with torch.no_grad():
        _, _, (boxes0, out0, _) = infer_image(net, conv, im_data, detector=hook, return_debug=True)
        assert launches == {"head": 0, "pool": 0}
        all_seven(net)
        _, _, (boxes1, out1, _) = infer_image(net, conv, im_data, detector=hook, return_debug=True)
    assert launches["head"] >= 1, "the native head did not run"
    assert len(boxes0) >= 3, "the synthetic detector maps must yield boxes"
    assert len(boxes1) == len(boxes0) and len(out1[0]) == len(out0[0]) == len(boxes0)
