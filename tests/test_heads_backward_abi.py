"""CPU: the ABI of the heads' and the gate's training forward and backward (header section 7b) -- the symbols,
the plan and workspace queries against the mirror of heads_backward_cases.py, every host refusal, the reference against
torch's float64 autograd of the network's own expressions, the negative controls of the check, and what
fots_e2e.native_train_heads says about its predicate and its switch.  No kernel is launched here."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import heads_backward_cases as B
import heads_cases as HC
from test_abi import declared_functions
from test_depthwise_abi import fake_cuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rroi_heads_forward_train_hip", "rroi_gate_forward_train_hip", "rroi_heads_backward_hip", "rroi_gate_backward_hip",
         "rroi_heads_backward_workspace_bytes", "rroi_heads_backward_plan")
NETWORK_MAPS = ((256, 176, 320), (256, 88, 160), (256, 44, 80), (256, 22, 40))     # of a 704 x 1280 image


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def test_symbols_are_exported_and_declared(ext):
    lib = ctypes.CDLL(ext.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions() and name in ext.EXPORTS and hasattr(lib, name), name
    assert ext.version() == "rroi_align_hip 0.10.0 gfx950"      # the version string stays


def test_plan_and_workspace_queries_agree_with_the_mirror(ext):
    shapes = list(B.CASES) + [(n, c, h, w) for n in (1, 8) for c, h, w in NETWORK_MAPS]
    for N, C, Hh, W in shapes:
        want = B.plan_of(N, C, Hh, W)
        for outputs in (7, 1):
            for dtype in HC.DTYPES:
                p = ext.heads_backward_plan(N, C, Hh, W, outputs=outputs, dtype=dtype)
                assert (p.vector_elems, p.grid_x, p.partial_rows, p.tiles_per_workgroup) == \
                    (want["V"], want["rows"], want["rows"], want["tpw"]), (N, C, Hh, W)
                assert p.block == 256 and p.launches == 2 and p.pixels_per_workgroup == want["tpw"] * 64 * want["V"]
                assert p.lds_bytes == 4 * (min(want["cb"], B.PASS_BLOCK) // 8) * 64 * 8 <= 32768
                assert p.workspace_bytes == want["rows"] * outputs * (C + 1) * 8 == B.workspace_bytes(N, C, Hh, W, outputs)
            assert ext.heads_backward_workspace_bytes(N, C, Hh, W, outputs) == B.workspace_bytes(N, C, Hh, W, outputs)
    # what the table is there for
    assert B.plan_of(1, 1, 1, 1)["rows"] == 1 and B.plan_of(1, 64, 5, 13)["rows"] == 2 and B.plan_of(3, 5, 8, 8)["rows"] == 3
    crossing = B.plan_of(3, 3, 181, 242)
    assert crossing["tpw"] == 2 and crossing["tiles"] % 2 == 1 and crossing["rows"] == 515 and B.plan_of(2, 515, 3, 5)["passes"] == 2
    # the grid cap: the rows, and with them the workspace, stop growing once it is reached
    sizes = [ext.heads_backward_workspace_bytes(n, 1, 176, 320) for n in (1, 2, 3, 64, 1024, 2048, 16384)]
    cap = 4 * B.CUS * 7 * 2 * 8
    assert 0 < sizes[0] < sizes[1] and all(0 < s <= cap for s in sizes) and sizes[-3:] == [cap] * 3
    assert ext.heads_backward_plan(16384, 1, 176, 320).partial_rows == 4 * B.CUS
    assert all(ext.heads_backward_workspace_bytes(n, 256, 176, 320) <= 4 * B.CUS * 7 * 257 * 8 for n in (1, 2, 3, 8, 16))
    with pytest.raises(ValueError):
        ext.heads_backward_plan(1, 256, 0, 8)
    assert ext.heads_backward_workspace_bytes(1, 256, 0, 8) == 0 and ext.heads_backward_workspace_bytes(1, 4, 8, 8, outputs=3) == 0


BAD_DIMS = ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (-1, 4, 8, 8), (1, 4, 8, -3))
TOO_LARGE = ((1, 1 << 11, 1 << 10, 1 << 10), (1 << 16, 1 << 15, 1, 1), (0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff),
             (1, 0x7ffffff0, 1, 1))                           # the last: 7 (C + 1) entries of a row do not fit 31 bits


def test_refusals_return_zero_before_any_launch(ext):
    ftrain, gtrain, hbwd, gbwd, wsb, plan = (getattr(ext._lib, n) for n in NAMES)
    P = 0x7f0000000000      # non-null, 256-aligned, never dereferenced: every call below is refused on the host
    at = lambda k: P + (k << 32)  # noqa: E731   (disjoint ranges)
    ok = (1, 4, 8, 8)
    BIG = 1 << 30
    info = ext._HeadsBwdPlan()
    heads_args = lambda: [at(k) for k in range(15)]  # noqa: E731   dscore drbox dangle x z w*3 dx (dw db)*3
    gate_args = lambda: [at(k) for k in range(7)]    # noqa: E731   dy x z w dx dw db

    def heads(args, dims=ok, dtype=0, scale=128.0, ws=at(20), nbytes=BIG):
        return hbwd(dtype, *args, *dims, scale, ws, nbytes, None)

    def gate(args, dims=ok, dtype=0, ws=at(20), nbytes=BIG):
        return gbwd(dtype, *args, *dims, ws, nbytes, None)
    # section 7's refusals: an unknown dtype, a dimension below 1, too many elements, an rbox_scale that is not finite
    for dtype in (3, -1):
        assert ftrain(dtype, *[P] * 11, *ok, 128.0, None) == 0 and gtrain(dtype, *[P] * 5, *ok, None) == 0
        assert heads(heads_args(), dtype=dtype) == 0 and gate(gate_args(), dtype=dtype) == 0
        assert plan(dtype, 7, *ok, ctypes.byref(info)) == 0
    for dims in BAD_DIMS + TOO_LARGE:
        tiny = dims == TOO_LARGE[-1]                           # (fewer than 2^31 elements: the forward takes it)
        assert tiny or (ftrain(0, *[P] * 11, *dims, 128.0, None) == 0 and gtrain(0, *[P] * 5, *dims, None) == 0), dims
        assert heads(heads_args(), dims=dims) == 0 and (tiny or gate(gate_args(), dims=dims) == 0), dims
        assert plan(0, 7, *dims, ctypes.byref(info)) == 0 and wsb(7, *dims) == 0, dims
    for outputs in (0, 2, 8):
        assert plan(0, outputs, *ok, ctypes.byref(info)) == 0 and wsb(outputs, *ok) == 0
    for scale in (float("nan"), float("inf"), float("-inf")):
        assert ftrain(0, *[P] * 11, *ok, scale, None) == 0 and heads(heads_args(), scale=scale) == 0
    for dtype in (0, 1, 2):
        # the training forward: a NULL x, weight, output or z (biases may be NULL)
        for k in (0, 1, 3, 5, 7, 8, 9, 10):
            args = [P] * 11
            args[k] = None
            assert ftrain(dtype, *args, *ok, 128.0, None) == 0, k
        for k in (0, 1, 3, 4):
            args = [P] * 5
            args[k] = None
            assert gtrain(dtype, *args, *ok, None) == 0, k
        # the backward: a NULL x or z
        for k in (3, 4):
            args = heads_args()
            args[k] = None
            assert heads(args, dtype=dtype) == 0, k
        for k in (1, 2):
            args = gate_args()
            args[k] = None
            assert gate(args, dtype=dtype) == 0, k
        # a NULL weight while dx is wanted
        for k in (5, 6, 7):
            args = heads_args()
            args[k] = None
            assert heads(args, dtype=dtype) == 0, k
        args = gate_args()
        args[3] = None
        assert gate(args, dtype=dtype) == 0
        # no output gradient given; no output wanted
        assert heads([None] * 3 + heads_args()[3:], dtype=dtype) == 0 and gate([None] + gate_args()[1:], dtype=dtype) == 0
        assert heads(heads_args()[:8] + [None] * 7, dtype=dtype) == 0 and gate(gate_args()[:4] + [None] * 3, dtype=dtype) == 0
        # a workspace that is NULL, misaligned or too small while a parameter gradient is wanted
        need = wsb(7, *ok)
        assert need == 7 * 5 * 8 and wsb(1, *ok) == 5 * 8
        for ws, nbytes in ((None, BIG), (at(20) + 8, BIG), (at(20), need - 1), (at(20), 0)):
            assert heads(heads_args(), dtype=dtype, ws=ws, nbytes=nbytes) == 0
            assert gate(gate_args(), dtype=dtype, ws=ws, nbytes=wsb(1, *ok) - 1 if nbytes == need - 1 else nbytes) == 0
        # an output overlapping an input, another output or the workspace
        for out in range(8, 15):
            for other in list(range(8)) + [o for o in range(8, 15) if o != out]:
                args = heads_args()
                args[out] = args[other]
                assert heads(args, dtype=dtype) == 0, (out, other)
            args = heads_args()
            args[out] = at(20)
            assert heads(args, dtype=dtype) == 0, out
        for out in (4, 5, 6):
            for other in (0, 1, 2, 3):
                args = gate_args()
                args[out] = args[other]
                assert gate(args, dtype=dtype) == 0, (out, other)
        esize = 4 if dtype == 0 else 2
        args = heads_args()
        args[8] = args[3] + (1 * 4 * 8 * 8 - 1) * esize              # dx begins in x's last element
        assert heads(args, dtype=dtype) == 0


def test_python_surface_raises_what_it_documents(ext):
    x, z = torch.zeros(2, 3, 8, 8), torch.zeros(2, 7, 8, 8, dtype=torch.float64)
    ws, wr, wa = torch.zeros(1, 3), torch.zeros(4, 3, 1, 1), torch.zeros(2, 3)
    g = (torch.zeros(2, 1, 8, 8), torch.zeros(2, 4, 8, 8), torch.zeros(2, 2, 8, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        ext.heads_backward(*g, x, z, ws, wr, wa)
    with pytest.raises(RuntimeError, match="GPU only"):
        ext.heads_train(x, ws, None, wr, None, wa, None)
    with pytest.raises(RuntimeError, match="GPU only"):
        ext.gate_train(x, ws, None)
    c = fake_cuda
    with pytest.raises(ValueError, match="float64"):
        ext.heads_backward(*map(c, g), c(x), c(z.float()), c(ws), c(wr), c(wa))
    with pytest.raises(ValueError, match="float64"):
        ext.gate_backward(c(g[0]), c(x), c(z), c(ws))                              # seven planes of z for the gate
    with pytest.raises(ValueError, match="no output gradient"):
        ext.heads_backward(None, None, None, c(x), c(z), c(ws), c(wr), c(wa))
    with pytest.raises(ValueError, match="drbox"):
        ext.heads_backward(c(g[0]), c(g[0]), c(g[2]), c(x), c(z), c(ws), c(wr), c(wa))
    with pytest.raises(ValueError, match="dangle"):
        ext.heads_backward(c(g[0]), c(g[1]), c(g[2].half()), c(x), c(z), c(ws), c(wr), c(wa))
    with pytest.raises(ValueError, match="rbox"):
        ext.heads_backward(*map(c, g), c(x), c(z), c(ws), c(wa), c(wa))
    with pytest.raises(ValueError, match="no gradient"):
        ext.heads_backward(*map(c, g), c(x), c(z), c(ws), c(wr), c(wa), need_dx=False, need_dweight=False, need_dbias=False)
    with pytest.raises(ValueError, match="rbox_scale"):
        ext.heads_backward(*map(c, g), c(x), c(z), c(ws), c(wr), c(wa), rbox_scale=float("inf"))
    with pytest.raises(TypeError):
        ext.gate_backward(c(g[0]), c(x), None, c(ws))


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("shape", ((2, 3, 7, 9), (3, 5, 8, 8), (1, 64, 5, 13), (2, 255, 11, 23)), ids=B.case_id)
def test_the_reference_is_torchs_float64_autograd_of_the_networks_expressions(shape):
    """`FOTSNet._heads` and the convolution and sigmoid of `FOTSNet._gate`, on a network whose head convolutions carry the
    case's parameters, in float64 under torch's autograd, against the longdouble restatement: 1e-12 relative."""
    from fots_e2e.model import FOTSNet
    x, hp, gp, hg, gg = B.problem(shape, torch.float32)
    C = shape[1]
    net = FOTSNet().double()
    for name, (w, b) in zip(("act", "rbox", "angle", "conv_attenton"), (hp[0:2], hp[2:4], hp[4:6], gp)):
        conv = torch.nn.Conv2d(C, w.size(0), 1).double()
        with torch.no_grad():
            conv.weight.copy_(w.double().reshape(-1, C, 1, 1))
            conv.bias.copy_(b.double())
        setattr(net, name, conv)
    Rh, Rg = B.reference(shape, torch.float32)
    close = lambda got, ref: float((got.reshape(ref.shape) - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))  # noqa: E731
    x64 = x.double().requires_grad_(True)
    torch.autograd.backward(net._heads(x64), [t.double() for t in hg])
    assert close(x64.grad, Rh.dx)
    assert close(torch.cat([m.weight.grad.reshape(-1, C) for m in (net.act, net.rbox, net.angle)]), Rh.dw)
    assert close(torch.cat([m.bias.grad for m in (net.act, net.rbox, net.angle)]), Rh.db)
    x64 = x.double().requires_grad_(True)
    y = net._gate(x64, x64)                                                       # `like` of its own size: the resize is the identity
    y.backward(gg[0].double())
    assert close(x64.grad, Rg.dx) and close(net.conv_attenton.weight.grad, Rg.dw) and close(net.conv_attenton.bias.grad, Rg.db)
    with torch.no_grad():
        z = torch.cat([m(x.double()) for m in (net.act, net.rbox, net.angle)], dim=1)
    assert close(z, Rh.z)


def test_the_check_holds_the_rounded_reference_and_rejects_what_is_wrong():
    """The reference rounded once to the dtype is inside its bound; one element moved by 4 ulps of the dtype is outside it,
    and so is a reference with two weight rows swapped."""
    for shape in ((2, 255, 11, 23), (1, 64, 5, 13)):
        for dtype in HC.DTYPES:
            Rh, Rg = B.reference(shape, dtype)
            x, _, gp, _, gg = B.problem(shape, dtype)
            # the gate's gradients are below 2^-4, where 2^-25, the bound's absolute term, is 8 ulps of float32: the control
            # also runs on the gate with dy scaled by 2^10 (exact in every dtype), whose results are normal numbers near 2^6
            for R in (Rh, Rg, B.Reference(x, gp, (gg[0] * 1024,))):
                dx, dw, db = R.dx.to(dtype), R.dw.to(dtype), R.db.to(dtype)
                ok, worst = B.check_all(R, dx, dw, db)
                # (within half of it where the results are normal numbers; a float16 subnormal may be half a subnormal off)
                assert ok and (dtype == torch.float16 or max(worst.values()) <= 0.5 + 1e-6), (shape, dtype, worst)
                if R is Rg and dtype == torch.float32:
                    continue      # (the scaled gate behind it stands for this one)
                for name, t in (("dx", dx), ("dw", dw), ("db", db)):
                    flat = t.clone().reshape(-1)
                    # the element whose bound is the tightest in ulps, among the normal numbers of every dtype: at another
                    # one the allowance for the double sums (c mag) may itself be several ulps of float32
                    ref, lim = getattr(R, name).reshape(-1), getattr(R, name + "_lim").reshape(-1)
                    k = int(torch.where(ref.abs() > 2.0 ** -14, lim / ref.abs(), torch.full_like(lim, float("inf"))).argmin())
                    as_int = flat.view(torch.int32 if dtype == torch.float32 else torch.int16)
                    as_int[k] += 4
                    moved = {"dx": dx, "dw": dw, "db": db}
                    moved[name] = flat.reshape(t.shape)
                    ok, worst = B.check_all(R, moved["dx"], moved["dw"], moved["db"])
                    assert not ok and worst[name] > 1, (shape, dtype, name, worst)
            swapped = Rh.dw.to(dtype)[[0, 2, 1, 3, 4, 5, 6]]
            assert not B.check(swapped, Rh.dw, Rh.dw_lim)[0]
            assert not B.check(Rh.dx.to(dtype).roll(1, 1), Rh.dx, Rh.dx_lim)[0]
    # a NaN where the reference has none, and none where it has one
    Rh, _ = B.reference((2, 255, 11, 23), torch.float32)
    bad = Rh.db.float().clone()
    bad[3] = float("nan")
    assert not B.check(bad, Rh.db, Rh.db_lim)[0]
    # a float16 sum that leaves the range: the infinity of its sign is the correct rounding, the other one is not
    ref, lim = torch.tensor([70000.0, -70000.0, 100.0]), torch.tensor([1.0, 1.0, 1.0])
    inf = float("inf")
    assert B.check(torch.tensor([inf, -inf, 100.0], dtype=torch.float16), ref, lim)[0]
    assert not B.check(torch.tensor([-inf, -inf, 100.0], dtype=torch.float16), ref, lim)[0]
    assert not B.check(torch.tensor([inf, -inf, inf], dtype=torch.float16), ref, lim)[0]
    assert B.overflow_threshold(torch.float16) == 65520.0


# ---------------------------------------------------------------- the predicate and the switch
ASK_THE_PREDICATE = """
import sys, torch
from fots_e2e import native_train_heads as TH
from fots_e2e.model import FOTSNet
net = FOTSNet().train()
x = torch.zeros(1, 256, 4, 4, requires_grad=True)
assert not TH.trainable_heads_ok(net, x) and not TH.trainable_heads_ok(net, x, gate=True)
assert TH.use_trainable_heads(net) is False
loaded = sorted(m for m in sys.modules if m == "rroi_align" or m.startswith("rroi_align."))
assert not loaded, loaded
print("asked")
"""


def test_asking_the_predicate_needs_neither_library_nor_gpu():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "fots.pytorch_amd")] + sys.path))
    p = subprocess.run([sys.executable, "-c", ASK_THE_PREDICATE], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "asked", p.stderr[-2000:]


def test_trainable_heads_ok_is_heads_ok_without_its_gradient_clauses(monkeypatch):
    from fots_e2e import native_train_heads as TH
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import heads_ok
    net = FOTSNet().train()
    x = fake_cuda(torch.zeros(2, 256, 4, 4))
    xg = fake_cuda(torch.zeros(2, 256, 4, 4)).requires_grad_(True)
    for gate in (False, True):
        assert not heads_ok(net, x, gate) and not heads_ok(net, xg, gate)          # the weights need gradients
        assert TH.trainable_heads_ok(net, x, gate) and TH.trainable_heads_ok(net, xg, gate)
    assert torch.is_grad_enabled()                                                 # asking leaves grad mode as it was
    for bad in (torch.zeros(2, 256, 4, 4), fake_cuda(torch.zeros(2, 256, 4, 4).to(memory_format=torch.channels_last)),
                fake_cuda(torch.zeros(2, 256, 4, 4, dtype=torch.bfloat16)), fake_cuda(torch.zeros(2, 255, 4, 4)),
                fake_cuda(torch.zeros(0, 256, 4, 4)), fake_cuda(torch.zeros(256, 4, 4))):
        assert not TH.trainable_heads_ok(net, bad) and not TH.trainable_heads_ok(net, bad, gate=True)
    with monkeypatch.context() as mp:
        mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert not TH.trainable_heads_ok(net, x)
    with monkeypatch.context() as mp:                                              # this module's own hook declines a shape
        seen = []
        mp.setattr(TH, "_heads_backward_slower", lambda t, gate: (seen.append(gate), True)[1])
        assert not TH.trainable_heads_ok(net, x) and not TH.trainable_heads_ok(net, x, gate=True) and seen == [False, True]
        torch.use_deterministic_algorithms(True)                                   # asked there as well: the stock leg does not raise
        try:
            assert not TH.trainable_heads_ok(net, x) and len(seen) == 3
        finally:
            torch.use_deterministic_algorithms(False)


def test_switch_algebra():
    """All six classes are reached; on last, off first; out of order a toggle returns False and leaves the type alone;
    no key of the state_dict moves; the tables of native and native_train are what they were."""
    from fots_e2e import native as nat
    from fots_e2e import native_train as T
    from fots_e2e import native_train_heads as TH
    from fots_e2e.model import FOTSNet
    assert len(nat._NETS) == 8 and len(T._NETS) == 8 and len(TH._NETS) == 12 and len(TH._TRAINABLE) == 6
    assert not any(issubclass(c, TH._TrainableHeads) for c in list(nat._NETS.values()) + list(T._NETS.values()))
    bases = [c.__bases__[1] for c in TH._TRAINABLE]
    assert all(c.__bases__[0] is TH._TrainableHeads and issubclass(c, nat.NativeHeadsFOTSNet) for c in TH._TRAINABLE)
    assert sorted(b.__name__ for b in bases) == sorted(
        c.__name__ for c in set(nat._NETS.values()) | set(T._NETS.values()) if issubclass(c, nat.NativeHeadsFOTSNet))
    net = FOTSNet()
    keys, params = list(net.state_dict().keys()), [id(p) for p in net.parameters()]
    others = (nat.use_native_heads, nat.use_native_merge, nat.use_native_recogniser, T.use_trainable_merge)
    reached = set()
    for base in bases:
        net.__class__ = base
        assert TH.use_trainable_heads(net, False) is False and type(net) is base
        assert TH.use_trainable_heads(net) is True and type(net) in TH._TRAINABLE and type(net).__bases__[1] is base
        reached.add(type(net))
        cls = type(net)
        for switch in others:                                                      # on last: the others find no class of theirs
            assert switch(net) is False and switch(net, False) is False and type(net) is cls
        assert TH.use_trainable_heads(net) is False and type(net) is cls
        assert list(net.state_dict().keys()) == keys and [id(p) for p in net.parameters()] == params
        assert TH.use_trainable_heads(net, False) is True and type(net) is base     # off first
    assert reached == set(TH._TRAINABLE)
    for cls in (FOTSNet, nat.NativeMergeFOTSNet, nat.NativeRecogniserFOTSNet, T.TrainableMergeFOTSNet):   # no native heads
        net.__class__ = cls
        assert TH.use_trainable_heads(net) is False and type(net) is cls
    # the documented order, through the switches themselves
    net.__class__ = FOTSNet
    assert nat.use_native_heads(net) and nat.use_native_merge(net) and nat.use_native_recogniser(net) and T.use_trainable_merge(net)
    assert TH.use_trainable_heads(net) and type(net).__name__ == "TrainableHeadsTrainableHeadsMergeRecogniserFOTSNet"
    assert getattr(TH, type(net).__name__) is type(net)
    assert T.use_trainable_merge(net, False) is False and nat.use_native_heads(net, False) is False
    assert TH.use_trainable_heads(net, False) and T.use_trainable_merge(net, False) and nat.use_native_recogniser(net, False)
    assert nat.use_native_merge(net, False) and nat.use_native_heads(net, False) and type(net) is FOTSNet


def test_on_the_cpu_the_switched_network_computes_what_it_did():
    """`_train_gate` is the expression `_train_merge_one` held; with the heads switch off `_train_merge_one` computes what it
    did; with it on, on the CPU, every method falls through to its parent: float64, bit for bit."""
    from fots_e2e import native as nat
    from fots_e2e import native_train as T
    from fots_e2e import native_train_heads as TH
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet()).double().train()
    g = torch.Generator().manual_seed(5)
    a, f, t = (torch.randn(1, 256, h, w, generator=g, dtype=torch.float64, requires_grad=True) for h, w in ((2, 3), (4, 6), (2, 3)))
    assert nat.use_native_heads(net) and nat.use_native_merge(net) and T.use_trainable_merge(net)
    gate = torch.sigmoid(net.conv_attenton(t))
    assert torch.equal(net._train_gate(t), gate)
    want = net._up(a, f) + f * net._up(gate, f)
    assert torch.equal(net._train_merge_one(a, f, t), want)
    heads_want, gate_want = net._heads(f), net._gate(t, f)
    assert TH.use_trainable_heads(net)
    assert torch.equal(net._train_gate(t), gate) and torch.equal(net._train_merge_one(a, f, t), want)
    assert all(torch.equal(x, y) for x, y in zip(net._heads(f), heads_want)) and torch.equal(net._gate(t, f), gate_want)
    net._train_merge_one(a, f, t).sum().backward()
    assert all(p.grad is not None for p in net.conv_attenton.parameters()) and t.grad is not None
    assert np.isfinite(float(t.grad.abs().sum()))
