"""CPU: the entry points of the native recogniser head and of the activation + (2,1) max-pool (header section 10, DESIGN
5.16) are exported, declared and host-checked; the plan query equals the mirrored rule; the Python surface refuses what it
says it refuses; `ocr_head_ok` / `act_pool_ok` / `use_native_recogniser` do what fots_e2e.native says, in every order with
`use_native_heads` and `use_native_merge`; the two references of recogniser_cases.py agree with torch.  No kernel is
launched here."""
import ctypes
import itertools

import pytest
import torch
import torch.nn as nn

import recogniser_cases as RC
from test_abi import declared_functions
from test_depthwise_abi import fake_cuda

NAMES = ("rroi_ocr_head_forward_hip", "rroi_ocr_head_plan", "rroi_act_maxpool2x1_forward_hip")
FP32, BF16, FP16 = 0, 1, 2


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


class FakeHuge(torch.Tensor):
    """One element expanded to a huge shape that says it is a contiguous GPU tensor: the size limits of the predicates can
    be asked without allocating 2^31 elements."""
    is_cuda = True

    def is_contiguous(self, *args, **kwargs):
        return True


def huge(*shape, dtype=torch.float32):
    return torch.zeros(1, dtype=dtype).expand(*shape).as_subclass(FakeHuge)


def network(nclass=87):
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    return deterministic_init(FOTSNet(nclass)).eval()


def test_symbols_are_exported_and_declared(ext):
    lib = ctypes.CDLL(ext.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions() and name in ext.EXPORTS and hasattr(lib, name), name
    assert ext.version() == "rroi_align_hip 0.10.0 gfx950"      # the version string stays
    header = open(ext.LIB_PATH.split("fots.pytorch_amd")[0] + "include/rroi_align_hip.h").read()
    assert f"#define RROI_OCR_HEAD_MAX_CLASSES {RC.MAX_CLASSES}" in header and ext.OCR_HEAD_MAX_CLASSES == RC.MAX_CLASSES
    assert "of section 10" in header[header.index("Identification:"):]
    from fots_e2e import native
    assert native._OCR_HEAD_MAX_CLASSES == RC.MAX_CLASSES


def check_plan(ext, N, C, K, T, dtype):
    S, tiles, grid, lds = RC.head_plan_of(N, C, K, T)
    p = ext.ocr_head_plan(N, C, K, T, dtype=dtype)
    assert (p.class_block, p.waves, p.tile_columns, p.tiles, p.grid_x, p.block, p.lds_bytes, p.max_classes) == \
        (RC.CLASS_BLOCK, S, RC.TILE_COLUMNS, tiles, grid, 64 * S, lds, RC.MAX_CLASSES), (N, C, K, T)
    assert p.block <= 256 and p.lds_bytes <= 65536 and RC.CLASS_BLOCK * (S - 1) < K <= RC.CLASS_BLOCK * S
    return S


def test_plan_query_equals_the_mirrored_rule_on_the_table_and_the_network(ext):
    seen = set()
    for N, C, K, T, _ in RC.HEAD_CASES:
        for dtype in RC.DTYPES:
            seen.add(check_plan(ext, N, C, K, T, dtype))
    assert seen == {1, 2, 3, 4}                                   # one wave to the limit
    for shape in RC.NETWORK_HEAD_SHAPES:
        assert check_plan(ext, *shape, torch.bfloat16) == 3
    assert RC.head_plan_of(24, 256, 87, 128) == (3, 8, 192, 87 * 128) and RC.head_plan_of(1, 1, 1, 1) == (1, 1, 1, 512)
    with pytest.raises(ValueError):
        ext.ocr_head_plan(1, 256, RC.MAX_CLASSES + 1, 32)
    with pytest.raises(TypeError):
        ext.ocr_head_plan(1, 256, 87, 32, dtype=torch.float64)


BAD_HEAD = ((0, 4, 4, 8), (1, 0, 4, 8), (1, 4, 0, 8), (1, 4, 4, 0), (-1, 4, 4, 8), (1, 4, 4, -3), (1, 4, RC.MAX_CLASSES + 1, 8),
            (1, 1 << 16, 4, 1 << 15),        # x of 2^31 elements
            (1 << 12, 4, 128, 1 << 12),      # y of 2^31 elements (x is 2^26)
            (0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff))
BAD_POOL = ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 1, 8), (1, 4, 0, 8), (1, 4, 8, 0), (-1, 4, 8, 8), (1, 4, -2, 8),
            (1, 1 << 11, 1 << 10, 1 << 10), (0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff))


def test_refusals_return_zero_before_any_launch(ext):
    head, plan, pool = (getattr(ext._lib, n) for n in NAMES)
    P = 0x7f0000000000   # non-null, never dereferenced: every call below is refused on the host
    ok_head, ok_pool = (2, 4, 5, 8), (2, 4, 8, 8)
    info = ext._OcrHeadPlan()
    for dtype in (3, -1, 7):
        assert head(dtype, P, P, P, P, *ok_head, None) == 0
        assert plan(dtype, *ok_head, ctypes.byref(info)) == 0
        assert pool(dtype, P, P, *ok_pool, 0.01, None) == 0
    for dtype in (FP32, BF16, FP16):
        assert plan(dtype, *ok_head, ctypes.byref(info)) == 1 and info.waves == 1 and info.max_classes == RC.MAX_CLASSES
        assert plan(dtype, 1, 4, RC.MAX_CLASSES, 8, ctypes.byref(info)) == 1 and info.waves == 4
        assert plan(dtype, *ok_head, None) == 0
        for dims in BAD_HEAD:
            assert head(dtype, P, P, P, P, *dims, None) == 0, dims
            assert plan(dtype, *dims, ctypes.byref(info)) == 0, dims
        assert head(dtype, None, P, P, P, *ok_head, None) == 0
        assert head(dtype, P, None, P, P, *ok_head, None) == 0
        assert head(dtype, P, P, P, None, *ok_head, None) == 0
        assert head(dtype, None, None, None, None, *ok_head, None) == 0
        for dims in BAD_POOL:
            assert pool(dtype, P, P, *dims, 1.0, None) == 0, dims
        for slope in (float("nan"), float("inf"), float("-inf")):
            assert pool(dtype, P, P, *ok_pool, slope, None) == 0
        assert pool(dtype, None, P, *ok_pool, 1.0, None) == 0
        assert pool(dtype, P, None, *ok_pool, 0.0, None) == 0


def test_python_surface_refuses_cpu_tensors_and_mismatches(ext):
    x, w, b = torch.zeros(2, 6, 1, 8), torch.zeros(5, 6, 1, 1), torch.zeros(5)
    for dtype in RC.DTYPES:
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.ocr_head(x.to(dtype), w.to(dtype), b.to(dtype))
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.ocr_head(x.to(dtype)[:, :, 0], w.to(dtype)[:, :, 0, 0].contiguous())
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.act_maxpool2x1(torch.zeros(2, 3, 4, 5, dtype=dtype), 0.01)
    with pytest.raises(TypeError):
        ext.ocr_head(fake_cuda(x.double()), fake_cuda(w.double()))
    with pytest.raises(TypeError):
        ext.act_maxpool2x1(fake_cuda(torch.zeros(2, 3, 4, 5, dtype=torch.float64)))
    with pytest.raises(ValueError):
        ext.ocr_head(x, w.half(), b)                              # dtypes differ
    with pytest.raises(ValueError):
        ext.ocr_head(x, w, b.bfloat16())
    with pytest.raises(ValueError):
        ext.ocr_head(x, torch.zeros(5, 7, 1, 1), b)               # channels differ
    with pytest.raises(ValueError):
        ext.ocr_head(x, torch.zeros(5, 6, 1, 3), b)               # not 1x1
    with pytest.raises(ValueError):
        ext.ocr_head(x, w, torch.zeros(4))                        # the bias's length
    with pytest.raises(ValueError):
        ext.ocr_head(torch.zeros(2, 6, 2, 8), w, b)               # more than one row
    with pytest.raises(ValueError):
        ext.ocr_head(x[0, 0], w, b)                               # not 3-D or 4-D
    with pytest.raises(ValueError):
        ext.ocr_head(x, torch.zeros(RC.MAX_CLASSES + 1, 6), None)  # K above the limit
    with pytest.raises(ValueError):
        ext.ocr_head(fake_cuda(torch.zeros(2, 6, 1, 16)[:, :, :, ::2]), fake_cuda(w), fake_cuda(b))   # a strided view
    with pytest.raises(ValueError):
        ext.ocr_head(fake_cuda(x), fake_cuda(w), fake_cuda(b), out=fake_cuda(torch.zeros(2, 5, 9)))
    with pytest.raises(ValueError):
        ext.act_maxpool2x1(torch.zeros(2, 3, 1, 5))               # H < 2
    with pytest.raises(ValueError):
        ext.act_maxpool2x1(torch.zeros(3, 4, 5))                  # not 4-D
    with pytest.raises(ValueError):
        ext.act_maxpool2x1(torch.zeros(2, 3, 4, 5), float("nan"))
    with pytest.raises(ValueError):
        ext.act_maxpool2x1(fake_cuda(torch.zeros(2, 3, 4, 10)[:, :, :, ::2]))


def test_act_pool_ok_declines_each_disqualifying_property(monkeypatch):
    from fots_e2e.native import act_pool_ok
    z = lambda *shape, dtype=torch.float32: fake_cuda(torch.zeros(*shape, dtype=dtype))  # noqa: E731
    with torch.no_grad():
        for dtype in RC.DTYPES:
            assert act_pool_ok(z(2, 4, 11, 8, dtype=dtype)) and act_pool_ok(z(1, 1, 2, 1, dtype=dtype))
        assert not act_pool_ok(torch.zeros(2, 4, 11, 8))          # a CPU tensor
        assert not act_pool_ok(z(4, 11, 8))
        assert not act_pool_ok(z(2, 4, 11, 8, dtype=torch.float64))
        assert not act_pool_ok(fake_cuda(torch.zeros(2, 4, 11, 8).to(memory_format=torch.channels_last)))
        assert not act_pool_ok(fake_cuda(torch.zeros(2, 4, 11, 16)[:, :, :, ::2]))
        assert not act_pool_ok(z(2, 4, 1, 8))                     # a single row
        assert not act_pool_ok(z(0, 4, 11, 8))
        assert act_pool_ok(huge(1, 1 << 10, 1 << 10, 1 << 10))
        assert not act_pool_ok(huge(1, 1 << 11, 1 << 10, 1 << 10))
        with monkeypatch.context() as mp:
            mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
            assert not act_pool_ok(z(2, 4, 11, 8))
        from fots_e2e import native
        with monkeypatch.context() as mp:
            mp.setattr(native, "_act_pool_slower", lambda x, slope: True)
            assert not act_pool_ok(z(2, 4, 11, 8))
        # the measured classes: the pool alone below 3.0e6 elements keeps `F.max_pool2d`; with an activation none is declined
        assert not act_pool_ok(z(24, 128, 11, 64), 1.0) and act_pool_ok(z(24, 128, 11, 64), 0.01) and act_pool_ok(z(24, 128, 11, 64))
        assert act_pool_ok(huge(24, 128, 11, 128), 1.0) and act_pool_ok(huge(24, 256, 5, 128), 1.0)
        assert not act_pool_ok(z(24, 256, 5, 64), 1.0) and act_pool_ok(z(1, 1, 2, 1), 0.0)
    xg = z(2, 4, 11, 8).requires_grad_(True)
    assert not act_pool_ok(xg)
    with torch.no_grad():
        assert act_pool_ok(xg)


def test_ocr_head_ok_declines_each_disqualifying_property(monkeypatch):
    from fots_e2e import native
    from fots_e2e.native import ocr_head_ok
    net = network()
    t = fake_cuda(torch.zeros(3, 256, 1, 40))
    with torch.no_grad():
        assert ocr_head_ok(net, t) and ocr_head_ok(net, fake_cuda(torch.zeros(1, 256, 1, 1)))
        assert not ocr_head_ok(net, torch.zeros(3, 256, 1, 40))   # a CPU tensor
        assert not ocr_head_ok(net, fake_cuda(torch.zeros(3, 256, 40)))
        assert not ocr_head_ok(net, fake_cuda(torch.zeros(3, 256, 2, 40)))                 # more than one row
        assert not ocr_head_ok(net, fake_cuda(torch.zeros(3, 255, 1, 40)))                 # not conv11's channels
        assert not ocr_head_ok(net, fake_cuda(torch.zeros(3, 256, 1, 40, dtype=torch.bfloat16)))   # not the weight's dtype
        assert not ocr_head_ok(net, fake_cuda(torch.zeros(3, 256, 1, 40, dtype=torch.float64)))
        assert not ocr_head_ok(net, fake_cuda(torch.zeros(3, 256, 1, 80)[:, :, :, ::2]))
        assert not ocr_head_ok(net, fake_cuda(torch.zeros(0, 256, 1, 40)))
        assert not ocr_head_ok(net, huge(1 << 11, 256, 1, 1 << 12))    # 2^31 elements in
        with monkeypatch.context() as mp:
            mp.setattr(native, "_ocr_head_slower", lambda m, x: False)
            assert ocr_head_ok(net, huge(1 << 11, 256, 1, 1 << 11))
        # the measured class: more than 4,608 columns keep the stock chain
        assert ocr_head_ok(net, huge(24, 256, 1, 128)) and ocr_head_ok(net, huge(36, 256, 1, 128))
        assert not ocr_head_ok(net, huge(192, 256, 1, 32)) and not ocr_head_ok(net, huge(37, 256, 1, 128))
        for other in (nn.Conv2d(256, 87, 1, stride=2), nn.Conv2d(256, 87, 1, padding=1), nn.Conv2d(256, 87, (1, 3), padding=(0, 1)),
                      nn.Conv2d(256, 88, 1, groups=2), nn.Conv2d(256, 87, 1).double(), nn.Conv2d(256, 87, 1).bfloat16(),
                      nn.Conv2d(256, RC.MAX_CLASSES + 1, 1), nn.Conv2d(128, 87, 1), nn.Identity(),
                      type("Sub", (nn.Conv2d,), {})(256, 87, 1)):
            with monkeypatch.context() as mp:
                mp.setitem(net._modules, "conv11", other)
                assert not ocr_head_ok(net, t), other
        for other in (nn.Conv2d(256, 87, 1, bias=False), nn.Conv2d(256, RC.MAX_CLASSES, 1), nn.Conv2d(256, 1, 1)):
            with monkeypatch.context() as mp:                      # no bias (NULL is +0.0), the limit, one class: qualify
                mp.setitem(net._modules, "conv11", other)
                assert ocr_head_ok(net, t), other
        # 2^31 elements out with fewer in: 2^8 channels in, 2^7 classes out cannot do it; a wide conv11 on few channels can
        with monkeypatch.context() as mp:
            mp.setitem(net._modules, "conv11", nn.Conv2d(1, 128, 1))
            mp.setattr(native, "_ocr_head_slower", lambda m, x: False)
            assert ocr_head_ok(net, huge(1 << 12, 1, 1, 1 << 11))
            assert not ocr_head_ok(net, huge(1 << 12, 1, 1, 1 << 12))
        with monkeypatch.context() as mp:
            mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
            assert not ocr_head_ok(net, t)
        with monkeypatch.context() as mp:
            mp.setattr(native, "_ocr_head_slower", lambda m, x: True)
            assert not ocr_head_ok(net, t)
    assert net.conv11.weight.requires_grad and not ocr_head_ok(net, t)                     # a gradient is needed
    for p in net.parameters():
        p.requires_grad_(False)
    assert ocr_head_ok(net, t)
    tg = fake_cuda(torch.zeros(3, 256, 1, 40)).requires_grad_(True)
    assert not ocr_head_ok(net, tg)
    with torch.no_grad():
        assert ocr_head_ok(net, tg)
    for dtype in (torch.bfloat16, torch.float16):
        half = network().to(dtype)
        with torch.no_grad():
            assert ocr_head_ok(half, fake_cuda(torch.zeros(3, 256, 1, 40, dtype=dtype))) and not ocr_head_ok(half, t)


SWITCHES = ("heads", "merge", "recogniser")


def expected_type(on):
    from fots_e2e import native as nat
    from fots_e2e.model import FOTSNet
    return {(): FOTSNet, ("heads",): nat.NativeHeadsFOTSNet, ("merge",): nat.NativeMergeFOTSNet,
            ("heads", "merge"): nat.NativeHeadsMergeFOTSNet, ("recogniser",): nat.NativeRecogniserFOTSNet,
            ("heads", "recogniser"): nat.NativeHeadsRecogniserFOTSNet, ("merge", "recogniser"): nat.NativeMergeRecogniserFOTSNet,
            ("heads", "merge", "recogniser"): nat.NativeHeadsMergeRecogniserFOTSNet}[tuple(sorted(on))]


def test_the_switch_composes_with_heads_and_merge_in_every_order_and_back():
    from fots_e2e import native as nat
    from fots_e2e.model import FOTSNet
    use = {"heads": nat.use_native_heads, "merge": nat.use_native_merge, "recogniser": nat.use_native_recogniser}
    net = network()
    keys = list(net.state_dict().keys())
    ptrs = {k: p.data_ptr() for k, p in net.named_parameters()}
    for order_on in itertools.permutations(SWITCHES):
        for order_off in itertools.permutations(SWITCHES):
            on = set()
            for name in order_on:
                assert use[name](net) is True
                on.add(name)
                assert type(net) is expected_type(on), (order_on, name)
                assert use[name](net) is False and type(net) is expected_type(on)          # once
            assert isinstance(net, nat.NativeHeadsFOTSNet) and isinstance(net, nat._NativeMerge)
            assert type(net).forward_ocr is nat._NativeRecogniser.forward_ocr
            for name in order_off:
                assert use[name](net, False) is True
                on.discard(name)
                assert type(net) is expected_type(on), (order_off, name)                   # exactly what the others make
                assert use[name](net, False) is False
            assert type(net) is FOTSNet
    assert list(net.state_dict().keys()) == keys and {k: p.data_ptr() for k, p in net.named_parameters()} == ptrs
    # the four classes of the earlier switches keep their names and meaning
    assert nat.NativeHeadsMergeFOTSNet.__mro__[1:3] == (nat._NativeMerge, nat.NativeHeadsFOTSNet)
    assert nat.NativeMergeFOTSNet.forward_ocr is FOTSNet.forward_ocr and nat.NativeHeadsFOTSNet.forward_ocr is FOTSNet.forward_ocr

    class Other(FOTSNet):
        pass
    other = Other()
    assert nat.use_native_recogniser(other) is False and type(other) is Other              # another type is left alone
    seq = nn.Sequential(nn.Conv2d(3, 3, 1))
    assert nat.use_native_recogniser(seq) is False and type(seq) is nn.Sequential
    assert nat.use_native_recogniser(net, False) is False and type(net) is FOTSNet


def all_seven(net, enable=True):
    from fots_e2e import native as nat
    return (nat.use_native_depthwise(net, enable), nat.use_native_instancenorm(net, enable), nat.use_native_heads(net, enable),
            nat.use_native_merge(net, enable), nat.use_native_blocks(net, enable), nat.use_native_conv3x3(net, enable),
            nat.use_native_recogniser(net, enable))


def test_cpu_forward_ocr_of_the_switched_network_keeps_every_bit(monkeypatch):
    """All seven switches on, CPU tensors: every predicate declines, every step takes the stock expression, and the bits are
    those of the stock method -- in eval and in training mode, with and without a gradient, and the binding is never
    asked for."""
    from fots_e2e import native
    from fots_e2e.model import FOTSNet
    net = network()
    crops = torch.randn(2, 64, 11, 24, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = net.forward_ocr(crops)
        want_image = net(torch.zeros(1, 3, 64, 64))
    assert all_seven(net) == (22, (52, 20), True, True, (2, 7, 10), (23, 2), True)

    class Refuse:
        def __getattr__(self, name):
            raise AssertionError(f"the native {name} was called")
    monkeypatch.setattr(native, "_ext", lambda: Refuse())
    with torch.no_grad():
        got = net.forward_ocr(crops)
        got_image = net(torch.zeros(1, 3, 64, 64))
        with pytest.raises(AssertionError, match="the native "):
            net.forward_ocr(fake_cuda(crops))                     # qualifies: a kernel would run
    assert got.shape == (2, 87, 24) and torch.equal(got, want)
    assert all(torch.equal(a, b) for p, q in zip(want_image, got_image) for a, b in zip(p, q))
    with_grad = net.forward_ocr(crops)
    assert with_grad.requires_grad and torch.equal(with_grad, want)
    for dtype in (torch.bfloat16,):
        half = network().to(dtype)
        with torch.no_grad():
            w16 = half.forward_ocr(crops.to(dtype))
            all_seven(half)
            assert torch.equal(half.forward_ocr(crops.to(dtype)), w16)
    net.train()
    torch.manual_seed(5)
    a = net.forward_ocr(fake_cuda(crops))                         # training mode: the stock method, dropout included
    torch.manual_seed(5)
    b = FOTSNet.forward_ocr(net, crops)
    assert torch.equal(a, b)
    net.eval()
    assert all_seven(net, False) == (22, (52, 20), True, True, (2, 7, 10), (23, 2), True) and type(net) is FOTSNet


def test_the_two_head_references_round_to_the_same_bits():
    """The explicit formula (numpy) and torch.log_softmax on float64 logits, each rounded once to the type: over the table at
    most 1 element in 10^4 differs in bits -- the reference alone stays inside the cap of the GPU test's condition (b)."""
    for dtype in RC.DTYPES:
        total = differ = 0
        for case in RC.HEAD_CASES:
            x, w, b, want, R = RC.head_problem(case, dtype)
            N, C, K, T, _ = case
            z = torch.einsum("kc,nct->nkt", w.double().reshape(K, C), x.double().reshape(N, C, T)) + b.double()[None, :, None]
            other = torch.log_softmax(z, dim=1).to(dtype)
            d, nan_ok = RC.differing(other, want)
            assert nan_ok and want.shape == (N, K, T) and want.dtype == dtype
            ok, ratio = RC.within(other, R.out64, RC.head_bound(R, dtype))
            assert ok and ratio <= 1.0, (case, ratio)
            total += want.numel()
            differ += d
        assert total >= 10 ** 6 and differ * 10 ** 4 <= total, (dtype, differ, total)


def test_the_head_bound_is_tight_enough_to_mean_something():
    """The bound is within a few units of the type's rounding: a logit moved by one part in 2^20 breaks it in fp32."""
    case = (1, 256, 87, 65, 6)
    x, w, b, want, R = RC.head_problem(case, torch.float32)
    lim = RC.head_bound(R, torch.float32)
    assert float((lim / R.out64.abs().clamp(min=1e-3)).max()) < 4 * 2.0 ** -24
    assert not RC.within((R.out64 * (1 + 2.0 ** -20)).float(), R.out64, lim)[0]


def test_the_pool_reference_equals_torch_on_the_cpu_ties_and_nans_included():
    for dtype in RC.DTYPES:
        for case in RC.POOL_CASES:
            x = RC.pool_problem(case, dtype)
            for slope in RC.SLOPES:
                want = RC.pool_reference(x, slope)
                try:
                    stock = RC.pool_stock(x, slope)
                except RuntimeError as e:                          # a dtype torch's CPU kernels do not take
                    assert dtype == torch.float16, e
                    continue
                assert want.shape == (case[0], case[1], case[2] // 2, case[3])
                assert RC.differing(want, stock) == (0, True), (case, dtype, slope)
    # the pairs the table plants, read back: a tie of signed zeros keeps the upper row's, a NaN in either row wins
    x = RC.pool_problem((1, 1, 2, 16), torch.float32)
    y = RC.pool_reference(x, 1.0)[0, 0, 0]
    up, low = x[0, 0, 0], x[0, 0, 1]
    for j in range(16):
        if up[j].isnan() or low[j].isnan():
            assert y[j].isnan()
        elif up[j] == low[j]:
            assert RC.bits(y[j:j + 1]).item() == RC.bits(up[j:j + 1].contiguous()).item()
    assert RC.bits(y[1:2]).item() == 0 and RC.bits(y[4:5]).item() == RC.bits(torch.tensor([-0.0])).item()   # (+0,-0), (-0,+0)
