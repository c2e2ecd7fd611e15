"""CPU: the gated merge's entry points are exported, declared and host-checked; the plan query equals the mirrored rule;
the Python surface refuses CPU tensors and mismatched arguments; `merge_ok` / `use_native_merge` do what fots_e2e.native
says; the float64 reference is pinned against torch's own chain.  No kernel is launched here."""
import ctypes

import pytest
import torch
import torch.nn as nn

import merge_cases as MC
from test_abi import declared_functions
from test_depthwise_abi import fake_cuda

NAMES = ("rroi_merge_forward_hip", "rroi_merge_plan")


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def test_symbols_are_exported_and_declared(ext):
    lib = ctypes.CDLL(ext.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions() and name in ext.EXPORTS and hasattr(lib, name), name
    assert not hasattr(lib, "rroi_merge_forward_forced_hip")     # the measurement build's alone
    assert ext.version() == "rroi_align_hip 0.10.0 gfx950"      # the version string stays


def test_plan_query_equals_the_mirrored_rule_on_the_whole_table(ext):
    seen = set()
    network = tuple(((n, 256, 704 // s, 1280 // s), a, (704 // (2 * s), 1280 // (2 * s)))
                    for n in (1, 8) for s, a in ((16, (22, 40)), (8, (88, 160)), (4, (176, 320))))
    for case in MC.CASES + network:
        (N, C, H, W), a_size, g_size = case
        for dtype in MC.DTYPES:
            V, K = MC.plan_of(case[0], a_size, dtype)
            tiles = -(-H * W // (256 * V))
            for gate_size in (g_size, None):
                p = ext.merge_plan(N, C, H, W, a_size, gate_size, dtype=dtype)
                assert (p.vector_elems, p.channel_groups, p.tiles, p.grid_x, p.block, p.channel_block) == \
                    (V, K, tiles, N * K * tiles, 256, -(-C // K)), case
                assert (K - 1) * p.channel_block < C                 # no block is empty
                assert p.resize_a == int(tuple(a_size) != (H, W))
                assert p.resize_gate == int(gate_size is not None and tuple(gate_size) != (H, W))
                assert p.a_scale_y == (0.0 if H == 1 else (a_size[0] - 1) / (H - 1))
                assert p.a_scale_x == (0.0 if W == 1 else (a_size[1] - 1) / (W - 1))
                if gate_size is not None:
                    assert p.gate_scale_y == (0.0 if H == 1 else (g_size[0] - 1) / (H - 1))
                    assert p.gate_scale_x == (0.0 if W == 1 else (g_size[1] - 1) / (W - 1))
            if case in MC.CASES:
                seen.add((V, K))
    # every form the table is meant to reach: both pixel counts per lane, one block, equal blocks, unequal blocks
    assert seen == {(4, 1), (2, 1), (2, 32), (2, 2), (4, 2), (4, 8)}
    f32, b16 = torch.float32, torch.bfloat16
    assert MC.plan_of((1, 256, 176, 320), (176, 320), f32) == (4, 32) and MC.plan_of((1, 256, 176, 320), (176, 320), b16) == (4, 32)
    assert MC.plan_of((8, 256, 176, 320), (176, 320), f32) == (4, 4) and MC.plan_of((8, 256, 176, 320), (176, 320), b16) == (4, 4)
    assert MC.plan_of((1, 256, 44, 80), (22, 40), f32) == (2, 32) and MC.plan_of((1, 256, 44, 80), (22, 40), b16) == (2, 32)


BAD_DIMS = ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (-1, 4, 8, 8), (1, 4, 8, -3))
TOO_LARGE = ((1, 1 << 11, 1 << 10, 1 << 10), (1 << 16, 1 << 15, 1, 1), (2, 2, 1 << 15, 1 << 14),
             (0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff))


def test_refusals_return_zero_before_any_launch(ext):
    merge, plan = (getattr(ext._lib, n) for n in NAMES)
    P = 0x7f0000000000   # non-null, never dereferenced: every call below is refused on the host
    ok = (1, 4, 8, 8)
    info = ext._MergePlan()
    call = lambda dtype, a, ah, aw, g, gh, gw, f, y, dims: merge(dtype, a, ah, aw, g, gh, gw, f, y, *dims, None)  # noqa: E731
    for dtype in (3, -1):                                         # an unknown dtype
        assert call(dtype, P, 4, 4, P, 4, 4, P, P, ok) == 0
        assert plan(dtype, *ok, 4, 4, 4, 4, 1, ctypes.byref(info)) == 0
    for dtype in (0, 1, 2):
        for dims in BAD_DIMS + TOO_LARGE:                         # a dimension of f below 1, N * C * H * W >= 2^31
            assert call(dtype, P, 4, 4, P, 4, 4, P, P, dims) == 0, dims
            assert call(dtype, P, 4, 4, None, 4, 4, P, P, dims) == 0, dims
            for gated in (0, 1):
                assert plan(dtype, *dims, 4, 4, 4, 4, gated, ctypes.byref(info)) == 0, dims
        for ah, aw in ((0, 4), (4, 0), (-1, 4), (4, -2)):         # a dimension of a below 1
            assert call(dtype, P, ah, aw, P, 4, 4, P, P, ok) == 0
            assert plan(dtype, *ok, ah, aw, 4, 4, 1, ctypes.byref(info)) == 0
        for gh, gw in ((0, 4), (4, 0), (-1, 4), (4, -2)):         # a dimension of the gate below 1 -- with a gate
            assert call(dtype, P, 4, 4, P, gh, gw, P, P, ok) == 0
            assert plan(dtype, *ok, 4, 4, gh, gw, 1, ctypes.byref(info)) == 0
            assert plan(dtype, *ok, 4, 4, gh, gw, 0, ctypes.byref(info)) == 1
        # N * C * a_h * a_w >= 2^31 with a small f; N * g_h * g_w >= 2^31
        assert call(dtype, P, 1 << 15, 1 << 14, P, 4, 4, P, P, ok) == 0
        assert plan(dtype, *ok, 1 << 15, 1 << 14, 4, 4, 1, ctypes.byref(info)) == 0
        assert plan(dtype, *ok, 1 << 15, (1 << 14) - 1, 4, 4, 1, ctypes.byref(info)) == 1     # 4 * (2^29 - 2^15) < 2^31
        assert call(dtype, P, 4, 4, P, 1 << 16, 1 << 15, P, P, ok) == 0
        for k in (0, 2, 3):                                       # a NULL a, f or y (a NULL gate is the ungated call)
            args = [P, P, P, P]
            args[k] = None
            assert call(dtype, args[0], 4, 4, args[1], 4, 4, args[2], args[3], ok) == 0, k
        for gated in (2, -1):
            assert plan(dtype, *ok, 4, 4, 4, 4, gated, ctypes.byref(info)) == 0
        assert plan(dtype, *ok, 4, 4, 4, 4, 1, None) == 0
        assert plan(dtype, *ok, 4, 4, 4, 4, 1, ctypes.byref(info)) == 1
    with pytest.raises(ValueError):
        ext.merge_plan(1, 4, 8, 8, (0, 4), (4, 4))


def test_python_surface_refuses_cpu_tensors_and_mismatches(ext):
    a, f, g = torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 8, 8), torch.zeros(2, 1, 4, 4)
    for dtype in MC.DTYPES:
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.gated_merge(a.to(dtype), f.to(dtype), g.to(dtype))
        with pytest.raises(RuntimeError, match="GPU only"):
            ext.gated_merge(a.to(dtype), f.to(dtype))
    with pytest.raises(ValueError):
        ext.gated_merge(a.half(), f, g)                            # dtypes differ
    with pytest.raises(ValueError):
        ext.gated_merge(a, f.bfloat16(), g)
    with pytest.raises(ValueError):
        ext.gated_merge(a, f, g.double())
    with pytest.raises(ValueError):
        ext.gated_merge(torch.zeros(1, 3, 4, 4), f, g)             # batch sizes differ
    with pytest.raises(ValueError):
        ext.gated_merge(torch.zeros(2, 4, 4, 4), f, g)             # channels differ
    with pytest.raises(ValueError):
        ext.gated_merge(a, f, torch.zeros(1, 1, 4, 4))             # the gate's batch size
    with pytest.raises(ValueError):
        ext.gated_merge(a, f, torch.zeros(2, 3, 4, 4))             # a gate that is not one channel
    with pytest.raises(ValueError):
        ext.gated_merge(a[0], f, g)                                # not 4-D
    with pytest.raises(ValueError):
        ext.gated_merge(a, f[0], g)
    with pytest.raises(ValueError):
        ext.gated_merge(a, f, g[0])


# ---------------------------------------------------------------- merge_ok, use_native_merge
def test_merge_ok_declines_each_disqualifying_property(monkeypatch):
    from fots_e2e.native import merge_ok
    z = lambda *shape, **kw: fake_cuda(torch.zeros(*shape, **kw))  # noqa: E731
    a, f, g = z(1, 256, 2, 3), z(1, 256, 4, 6), z(1, 1, 2, 3)
    with torch.no_grad():
        assert merge_ok(a, f, g) and merge_ok(a, f) and merge_ok(z(1, 256, 4, 6), f, g) and merge_ok(a, f, z(1, 1, 4, 6))
        for dtype in (torch.bfloat16, torch.float16):
            assert merge_ok(z(1, 8, 2, 3, dtype=dtype), z(1, 8, 4, 6, dtype=dtype), z(1, 1, 2, 3, dtype=dtype))
        for k in range(3):                                        # each tensor in turn
            stock = (torch.zeros(1, 256, 2, 3), torch.zeros(1, 256, 4, 6), torch.zeros(1, 1, 2, 3))

            def swapped(t):
                args = [a, f, g]
                args[k] = t
                return merge_ok(*args)
            assert not swapped(stock[k])                                                          # a CPU tensor
            assert not swapped(fake_cuda(stock[k][0]))                                            # not 4-D
            assert not swapped(fake_cuda(stock[k].repeat(1, 1, 1, 2)[:, :, :, ::2]))              # a strided view
            assert not swapped(fake_cuda(stock[k].double()))                                      # float64
            assert not swapped(fake_cuda(stock[k].bfloat16()))                                    # not the others' dtype
            assert not swapped(fake_cuda(torch.zeros(stock[k].shape, device="meta")))             # another device
            assert not swapped(fake_cuda(stock[k][:0]))                                           # empty
        assert not merge_ok(fake_cuda(torch.zeros(1, 256, 4, 6).to(memory_format=torch.channels_last)), f, g)
        assert not merge_ok(z(2, 256, 2, 3), f, g) and not merge_ok(z(1, 128, 2, 3), f, g)       # N, C of a
        assert not merge_ok(a, f, z(2, 1, 2, 3)) and not merge_ok(a, f, z(1, 2, 2, 3))           # N of the gate, two channels
        big = fake_cuda(torch.zeros(1).expand(1, 256, 1 << 12, 1 << 11))                         # 2^31 elements
        assert not merge_ok(big, f, g) and not merge_ok(a, big, g)
        assert not merge_ok(a, f, fake_cuda(torch.zeros(1).expand(1, 1, 1 << 16, 1 << 15)))
        assert not merge_ok(None, f, g) and not merge_ok(a, None, g)
        with monkeypatch.context() as mp:                          # under autocast the stock chain is left to autocast
            mp.setattr(torch, "is_autocast_enabled", lambda *x: True)
            assert not merge_ok(a, f, g) and not merge_ok(a, f)
    # a gradient is needed: of any of the three
    for k in range(3):
        args = [z(1, 256, 2, 3), z(1, 256, 4, 6), z(1, 1, 2, 3)]
        args[k].requires_grad_(True)
        assert not merge_ok(*args)
        with torch.no_grad():
            assert merge_ok(*args)
    assert merge_ok(a, f, g)                                       # grad mode on, nothing requires one


@pytest.fixture(scope="module")
def net():
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    return deterministic_init(FOTSNet()).eval()


def same(before, after):
    for p, q in zip(before, after):
        for s, t in zip(p, q):
            if not (torch.equal(s, t) or bool((s.isnan() == t.isnan()).all() and torch.equal(s.nan_to_num(), t.nan_to_num()))):
                return False
    return True


def test_use_native_merge_switches_by_exact_type_and_composes(net):
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import (NativeHeadsFOTSNet, NativeHeadsMergeFOTSNet, NativeMergeFOTSNet, use_native_blocks,
                                 use_native_depthwise, use_native_heads, use_native_instancenorm, use_native_merge)
    keys = list(net.state_dict().keys())
    ptrs = {k: p.data_ptr() for k, p in net.named_parameters()}
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        before = net(x)
    assert use_native_merge(net) is True and type(net) is NativeMergeFOTSNet
    assert use_native_merge(net) is False and type(net) is NativeMergeFOTSNet           # once
    assert isinstance(net, FOTSNet)
    assert list(net.state_dict().keys()) == keys and {k: p.data_ptr() for k, p in net.named_parameters()} == ptrs
    with torch.no_grad():
        assert same(before, net(x))                               # CPU tensors: the stock expression, the same bits
    # merge first, then heads, and back in both orders
    assert use_native_heads(net) is True and type(net) is NativeHeadsMergeFOTSNet
    assert isinstance(net, NativeHeadsFOTSNet)
    assert use_native_heads(net) is False and use_native_merge(net) is False
    with torch.no_grad():
        assert same(before, net(x))
    assert use_native_merge(net, False) is True and type(net) is NativeHeadsFOTSNet
    assert use_native_merge(net, False) is False
    assert use_native_merge(net) is True and type(net) is NativeHeadsMergeFOTSNet       # heads first, then merge
    assert use_native_heads(net, False) is True and type(net) is NativeMergeFOTSNet
    assert use_native_heads(net, False) is False
    assert use_native_merge(net, False) is True and type(net) is FOTSNet
    assert use_native_merge(net, False) is False and use_native_heads(net, False) is False
    # what use_native_heads does to a plain FOTSNet is unchanged
    assert use_native_heads(net) is True and type(net) is NativeHeadsFOTSNet
    assert use_native_heads(net, False) is True and type(net) is FOTSNet
    # with the three module switches, in any order
    assert use_native_depthwise(net) == 22 and use_native_merge(net) is True
    assert use_native_instancenorm(net) == (52, 20) and use_native_heads(net) is True and use_native_blocks(net) == (2, 7, 10)
    assert type(net) is NativeHeadsMergeFOTSNet and list(net.state_dict().keys()) == keys
    with torch.no_grad():
        assert same(before, net(x))
    assert use_native_merge(net, False) is True and use_native_blocks(net, False) == (2, 7, 10)
    assert use_native_depthwise(net, False) == 22 and use_native_heads(net, False) is True
    assert use_native_instancenorm(net, False) == (52, 20)
    assert type(net) is FOTSNet and list(net.state_dict().keys()) == keys
    assert {k: p.data_ptr() for k, p in net.named_parameters()} == ptrs

    class Other(FOTSNet):
        pass
    other = Other()
    assert use_native_merge(other) is False and type(other) is Other                   # another type is left alone
    assert use_native_merge(other, False) is False and use_native_heads(other) is False and type(other) is Other
    seq = nn.Sequential(nn.Conv2d(3, 3, 1))
    assert use_native_merge(seq) is False and type(seq) is nn.Sequential


def test_the_network_without_attention_and_training_mode_take_the_stock_bits():
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import use_native_merge
    from fots_e2e.weights import deterministic_init
    plain = deterministic_init(FOTSNet(attention=False)).eval()
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        before = plain(x)
        assert use_native_merge(plain)
        assert same(before, plain(x))
    f = [torch.randn(1, 256, 64 >> s, 64 >> s, generator=torch.Generator().manual_seed(s)) for s in (2, 3, 4, 5)]
    plain.train()                                                 # training: FOTSNet._merge itself
    calls = []
    plain._merge_one = lambda *a: calls.append(a)
    m1, m2 = plain._merge(*f)
    assert not calls and m1.requires_grad and m1.shape == f[0].shape and m2.shape == f[1].shape


def test_qualifying_merges_call_the_kernel_and_declined_ones_do_not(net, monkeypatch):
    """With tensors that say they are on the GPU each of the three merges asks for `_gated_merge_run`; a `requires_grad`
    input takes the stock expression, and its result is the stock method's."""
    from fots_e2e import native
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import use_native_merge

    class Refuse:
        def __getattr__(self, name):
            raise AssertionError(f"the native {name} was called")
    monkeypatch.setattr(native, "_ext", lambda: Refuse())
    g = torch.Generator().manual_seed(11)
    f1, f2, f3, f4 = (torch.randn(1, 256, 32 >> s, 48 >> s, generator=g) for s in range(4))
    assert use_native_merge(net)
    try:
        with torch.no_grad():
            want = FOTSNet._merge(net, f1, f2, f3, f4)
            with pytest.raises(AssertionError, match="native _gated_merge_run"):
                net._merge(*(fake_cuda(t) for t in (f1, f2, f3, f4)))
            got = net._merge(f1, f2, f3, f4)                       # CPU tensors
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        for p in net.parameters():
            p.requires_grad_(False)
        got = net._merge(*(fake_cuda(t.clone()).requires_grad_(True) for t in (f1, f2, f3, f4)))
        assert got[0].requires_grad and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    finally:
        for p in net.parameters():
            p.requires_grad_(True)
        assert use_native_merge(net, False)


# ---------------------------------------------------------------- the reference, pinned against torch
@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_stock_chain_lies_inside_the_stock_bound(dtype):
    """Over the table, on CPU tensors, with and without the gate: every element of torch's own chain in T is within
    merge_cases.stock_bound of the float64 reference rounded to T."""
    worst = 0.0
    for case in MC.CASES:
        a, f, gate, gated, ungated = MC.problem(case, dtype)
        for g, (want, R) in ((gate, gated), (None, ungated)):
            got = MC.stock(a, f, g)
            assert got.dtype == dtype and not bool(got.isnan().any())
            ok, ratio = MC.within(got, want, MC.stock_bound(a, f, g, R))
            assert ok, (case, g is not None, ratio)
            worst = max(worst, ratio)
    print(f"{dtype}: worst stock error / stock bound {worst:.3f}")
    assert worst > 0.05                                           # the bound is not vacuous


def test_reference_reads_an_equal_sized_source_as_it_is_and_keeps_special_values():
    a = torch.tensor([[[[1.0, float("inf")], [2.0, 3.0]]]])
    f = torch.ones(1, 1, 2, 2)
    y, _ = MC.reference(a, f, None)
    assert torch.equal(y, torch.tensor([[[[2.0, float("inf")], [3.0, 4.0]]]]))
    y, _ = MC.reference(a, torch.ones(1, 1, 3, 3), None)          # l1 == 0 next to an inf: 0 * inf = NaN
    assert bool(y.isnan()[0, 0, 0, 0]) and float(y[0, 0, 2, 0]) == 3.0 and float(y[0, 0, 2, 2]) == 4.0
