"""GPU (MI355X): the network with ten switches on -- the eight of fots_e2e.native and the two of
fots_e2e.native_remainder -- in bfloat16 and float16.

With every `_*_slower` hook forced off (the six of network_cases.slower_hooks() and the two new ones) one `forward` and one
`forward_ocr` run NO ATen operator that computes anything; the teacher-forced stages of network_cases.stages stay within
the project's two caps, RATIO_CAP and NEG_CAP, unchanged; the whole network gives the same bits twice WITHOUT
`torch.backends.cudnn.deterministic`; and switching the two off restores the eight-switch network's bits."""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

import network_cases as C
from test_gpu_network import (BOOKKEEPING, Ledger, expected_native_calls, inputs, name_of, repeatable_stock_convolutions,
                              run_all, same_bits)

pytestmark = pytest.mark.gpu

DTYPE_PARAMS = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
NEW_HOOKS = ("_conv2x3_slower", "_up_depthwise_slower")


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


@pytest.fixture(scope="module")
def rem():
    from rroi_align._ext.rroi_align import remainder
    return remainder


def all_ten(net):
    import fots_e2e.native_remainder as rm
    C.all_eight(net)
    assert rm.use_native_conv2x3(net) == 1 and rm.use_native_upconv(net) == 2
    return net


@functools.lru_cache(maxsize=None)
def trio(dtype):
    """(ten-switch network, unswitched copy on the same GPU, float64 twin on the CPU), left as they are by every test."""
    return all_ten(C.network(dtype).cuda()), C.network(dtype).cuda(), C.twin(C.network(dtype))


def force_every_kernel(monkeypatch):
    import fots_e2e.native_remainder as rm
    from fots_e2e import native as nat
    for hook in C.slower_hooks():
        monkeypatch.setattr(nat, hook, lambda *a, **k: False)
    assert sorted(k for k in vars(rm) if k.startswith("_") and k.endswith("_slower")) == sorted(NEW_HOOKS)
    for hook in NEW_HOOKS:
        monkeypatch.setattr(rm, hook, lambda *a, **k: False)


# ---------------------------------------------------------------- the ledger
@DTYPE_PARAMS
def test_the_ledger_runs_no_stock_operator_that_computes(ext, rem, dtype, monkeypatch):
    native, _, _ = trio(dtype)
    force_every_kernel(monkeypatch)
    want = expected_native_calls(native)
    assert want["_depthwise3x3_run"] == 22
    want["_depthwise3x3_run"] = 20                                 # the two of upconv1 / upconv2 run inside the fused call
    want.update(run_conv2x3=1, run_up_depthwise3x3=2)
    calls = collections.Counter()

    def counted(name, run):
        def call(*a, **k):
            calls[name] += 1
            return run(*a, **k)
        return call

    for name in want:
        mod = rem if name.startswith("run_") else ext
        monkeypatch.setattr(mod, name, counted(name, getattr(mod, name)))
    functional = collections.Counter()
    for name in ("leaky_relu", "relu", "interpolate"):
        fn = getattr(F, name)
        monkeypatch.setattr(F, name, lambda *a, _n=name, _f=fn, **k: functional.update([_n]) or _f(*a, **k))
    image, crops = inputs(dtype, 0)
    with torch.no_grad(), Ledger() as ledger:
        native(image)
        native.forward_ocr(crops)
    torch.cuda.synchronize()
    print(dict(calls), dict(ledger.ops))
    assert dict(calls) == want
    assert not functional, functional
    stock = {k: v for k, v in ledger.ops.items() if k not in BOOKKEEPING}
    assert stock == {}, stock                                      # none


# ---------------------------------------------------------------- teacher-forced stages
def teacher_forced(dtype, mode):
    native, stock, tw = trio(dtype)
    table = C.stages(stock)
    rows, broken = [], []
    for which, (image_key, _) in enumerate(C.INPUTS):
        def step(st, xs):
            with torch.no_grad():
                ys = C.as_tuple(st.on_net(native, *xs))
                stocks = C.as_tuple(st.on_net(stock, *xs))
                refs = C.as_tuple(st.on_twin(tw, *(x.double().cpu() for x in xs)))
            for out, y, s, ref in zip(st.makes, ys, stocks, refs):
                assert y.dtype == s.dtype == dtype and y.shape == s.shape == ref.shape, (st.name, out)
                rel_native, rel_stock = C.rel(y, ref), C.rel(s, ref)
                ratio = rel_native / rel_stock if rel_stock > 0 else float("inf")
                rel_neg = C.rel_neg(y, ref) if st.leaky else None
                rows.append((st.name, out, ratio, rel_neg))
                if st.name in ("_merge", "forward_ocr"):
                    print(f"{name_of(dtype)} {mode} {st.name:12s} {out:4s} {image_key:9s} rel native {rel_native:.3e} "
                          f"stock {rel_stock:.3e} ratio {ratio:5.2f}")
                if not rel_native <= C.RATIO_CAP * rel_stock:
                    broken.append((st.name, out, image_key, "ratio", ratio))
                if st.leaky and not rel_neg <= C.NEG_CAP:
                    broken.append((st.name, out, image_key, "rel_neg", rel_neg))
            return ys
        C.drive(table, *inputs(dtype, which), step)
    assert len(rows) == 2 * (len(table) + 1 + 2 + 2)
    print(f"{name_of(dtype)} {mode}: worst ratio {max(r[2] for r in rows):.3f}, "
          f"worst rel_neg {max(r[3] for r in rows if r[3] is not None):.4f}")
    return broken


@pytest.mark.parametrize("forced", (True, False), ids=("forced", "shipped"))
@DTYPE_PARAMS
def test_every_stage_of_the_ten_switch_network_is_within_both_caps(dtype, forced, monkeypatch):
    if forced:
        force_every_kernel(monkeypatch)
    broken = teacher_forced(dtype, "forced" if forced else "shipped")
    assert not broken, broken


# ---------------------------------------------------------------- repeatability, switching off
@DTYPE_PARAMS
def test_the_forced_network_gives_the_same_bits_twice_without_the_deterministic_flag(dtype, monkeypatch):
    assert not torch.backends.cudnn.deterministic
    force_every_kernel(monkeypatch)
    native, _, _ = trio(dtype)
    first = run_all(native, dtype)
    assert len(first) == 2 * 9 and all(bool(t.isfinite().all()) for t in first)
    for _ in range(2):
        assert all(same_bits(a, b) for a, b in zip(run_all(native, dtype), first))


@DTYPE_PARAMS
def test_switching_the_two_off_restores_the_eight_switch_bits(dtype):
    import fots_e2e.native_remainder as rm
    eight = C.all_eight(C.network(dtype).cuda())
    ten = all_ten(C.network(dtype).cuda())
    with repeatable_stock_convolutions():
        want = run_all(eight, dtype)
        assert all(same_bits(a, b) for a, b in zip(run_all(eight, dtype), want))        # the stock remainder is repeatable now
        got = run_all(ten, dtype)
        assert not all(same_bits(a, b) for a, b in zip(got, want))                      # conv10_s sums in another order
        assert rm.use_native_upconv(ten, False) == 2 and rm.use_native_conv2x3(ten, False) == 1
        assert [type(m) for m in ten.modules()] == [type(m) for m in eight.modules()] and type(ten) is type(eight)
        assert all(same_bits(a, b) for a, b in zip(run_all(ten, dtype), want))
