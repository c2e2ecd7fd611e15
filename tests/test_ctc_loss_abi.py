"""CPU: the native CTC loss -- the entry points are exported, declared and host-checked; the plan query is pure
and consistent; the Python surface refuses CPU tensors and bad arguments; `recognition_loss` defaults to the stock loss; the
float64 restatement the GPU tests measure against equals `F.ctc_loss` on the CPU in float64 (loss and autograd gradient)
on every finite and feasible case, and its gradient is the true derivative of a `torch.logsumexp` statement of the
recursion.  No kernel is launched here."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_loss_cases as CC
from test_abi import declared_functions

NAMES = ("rroi_ctc_loss_forward_hip", "rroi_ctc_loss_plan", "rroi_ctc_loss_workspace_bytes")
FP32, BF16, FP16 = 0, 1, 2
P = 0x7f0000000000   # non-null, 8-byte aligned, never dereferenced: every call it is passed to is refused on the host


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


@pytest.fixture(scope="module")
def cl():
    from rroi_align._ext.rroi_align import ctc_loss
    return ctc_loss


def test_symbols_are_exported_and_declared(ext, cl):
    lib = ctypes.CDLL(ext.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions() and name in ext.EXPORTS and hasattr(lib, name), name
    assert ext.version() == "rroi_align_hip 0.10.0 gfx950"      # the version string stays
    # the package's `_*_run` callables stay the closed list the network's ledger reads
    assert not any(k.startswith("_") and k.endswith("_run") for k in vars(cl))
    assert callable(cl.run_ctc_loss) and callable(cl.ctc_loss_plan) and callable(cl.ctc_loss_workspace_bytes)


SHAPES = [(c["N"], c["K"], c["T"], c["targets"].shape[1]) for c in CC.CASES] + [(32, 87, 96, 9), (512, 87, 128, 9), (1, 1, 0, 0),
                                                                                  (4, 3000, 50, 20), (2, 87, 400, 150)]


def test_plan_query_is_pure_and_consistent(cl):
    for (n, k, t, lmax) in SHAPES:
        for dtype in CC.DTYPES:
            for want in (True, False):
                for (st, sk) in ((n * k, 1), (1, t)):
                    p = cl.ctc_loss_plan(n, k, t, lmax, st, sk, want, dtype)
                    assert cl.ctc_loss_plan(n, k, t, lmax, st, sk, want, dtype) == p                      # pure
                    assert p.grid_x == n and p.block == 256                                               # no empty workgroup
                    assert 0 < p.lds_bytes <= p.lds_limit == 65536
                    assert p.positions == 2 * min(lmax, t) + 1
                    assert p.chunk_steps in (1, 2, 4, 8, 16)
                    assert p.stage_along_t == int(st == 1 and sk != 1)
                    # the LDS the kernel carves: four rows and three int arrays of S_max, a flag, the chunk's three arrays, the alpha and beta rows
                    base = p.positions * (4 * 8 + 3 * 4) + 4 + p.chunk_steps * (2 * p.positions + k) * 8
                    alpha = 2 * t * p.positions * 8
                    ws = cl.ctc_loss_workspace_bytes(n, k, t, lmax, want)
                    if not want:
                        assert p.lds_bytes == base and ws == 0 and not p.alpha_in_workspace
                    elif p.alpha_in_workspace:
                        assert p.lds_bytes == base and base + alpha > p.lds_limit and ws == n * alpha
                    else:
                        assert p.lds_bytes == base + alpha and ws == 0
                    assert p.chunk_steps == 16 or 2 * p.chunk_steps * (2 * p.positions + k) * 8 > p.lds_limit // 2
    # the training shape keeps everything in LDS, sixteen steps at a time; the long-target case goes to the workspace
    assert cl.ctc_loss_plan(32, 87, 96, 9)[:6] == (32, 256, 46024, 65536, 19, 16)
    assert cl.ctc_loss_plan(3, 130, 160, 64).alpha_in_workspace == 1 and cl.ctc_loss_plan(3, 130, 160, 64).chunk_steps == 8
    assert {cl.ctc_loss_plan(c["N"], c["K"], c["T"], c["targets"].shape[1]).alpha_in_workspace for c in CC.CASES} == {0, 1}


def _call(ext, dtype=FP32, lp=P, strides=(15, 5, 1), dims=(3, 5, 33), tg=P, lmax=4, il=P, tl=P, blank=0, nll=P, grad=P,
          gstrides=(15, 5, 1), ws=None, ws_bytes=0):
    return ext._lib.rroi_ctc_loss_forward_hip(dtype, lp, *strides, *dims, tg, lmax, il, tl, blank, 0, nll, grad, *gstrides, ws,
                                              ws_bytes, None)


def test_refusals_return_zero_before_any_launch(ext, cl):
    plan, info = ext._lib.rroi_ctc_loss_plan, cl._CtcLossPlan()
    for dtype in (3, -1):
        assert _call(ext, dtype=dtype) == 0
        assert plan(dtype, 3, 5, 33, 4, 15, 1, 1, ctypes.byref(info)) == 0
    for dtype in (FP32, BF16, FP16):
        assert plan(dtype, 3, 5, 33, 4, 15, 1, 1, ctypes.byref(info)) == 1
        assert plan(dtype, 3, 5, 33, 4, 15, 1, 1, None) == 0
        for dims, lmax in (((-1, 5, 33), 4), ((3, 0, 33), 4), ((3, -5, 33), 4), ((3, 5, -1), 4), ((3, 5, 33), -1),
                           ((3, 9000, 33), 4), ((3, 5, 5000), 2500)):              # the last two: no room in LDS
            assert _call(ext, dtype=dtype, dims=dims, lmax=lmax) == 0, (dims, lmax)
            assert plan(dtype, *dims, lmax, 15, 1, 1, ctypes.byref(info)) == 0, (dims, lmax)
            assert cl.ctc_loss_workspace_bytes(*dims, lmax) == 0
        for blank in (-1, 5, 1 << 20):
            assert _call(ext, dtype=dtype, blank=blank) == 0
        for null in ("lp", "tg", "il", "tl", "nll"):                                # a NULL pointer with N > 0
            assert _call(ext, dtype=dtype, **{null: None}) == 0, null
        # N == 0 is a no-op whatever the pointers; without targets (L_max == 0) their pointer may be NULL
        assert _call(ext, dtype=dtype, dims=(0, 5, 33), lp=None, tg=None, il=None, tl=None, nll=None, grad=None) == 1
        # a shape whose alpha rows live in the workspace: NULL, short and misaligned are refused; without a gradient none is needed
        big = dict(dtype=dtype, strides=(390, 130, 1), gstrides=(390, 130, 1), dims=(3, 130, 160), lmax=64)
        need = cl.ctc_loss_workspace_bytes(3, 130, 160, 64)
        assert need == 3 * 2 * 160 * 129 * 8
        assert _call(ext, ws=None, ws_bytes=need, **big) == 0
        assert _call(ext, ws=P, ws_bytes=need - 1, **big) == 0
        assert _call(ext, ws=P + 4, ws_bytes=need, **big) == 0
        assert cl.ctc_loss_workspace_bytes(3, 130, 160, 64, want_grad=False) == 0
    with pytest.raises(ValueError):
        cl.ctc_loss_plan(3, 0, 33, 4)
    with pytest.raises(TypeError):
        cl.ctc_loss_plan(3, 5, 33, 4, dtype=torch.float64)


def test_surface_refuses_cpu_tensors_and_bad_arguments():
    from rroi_align.ctc import CTCLoss, ctc_loss
    lp = torch.zeros(4, 2, 5).log_softmax(2)
    tg = torch.ones(2, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU only"):
        ctc_loss(lp, tg, [4, 4], [2, 2])
    with pytest.raises(RuntimeError, match="GPU only"):
        CTCLoss()(lp, tg, [4, 4], [2, 2])
    with pytest.raises(TypeError):
        ctc_loss(lp.numpy(), tg, [4, 4], [2, 2])
    with pytest.raises(ValueError):
        ctc_loss(lp, tg, [4, 4], [2, 2], reduction="median")
    with pytest.raises(ValueError):
        CTCLoss(reduction="median")
    assert list(inspect.signature(ctc_loss).parameters) == list(inspect.signature(F.ctc_loss).parameters)
    for name, p in inspect.signature(F.ctc_loss).parameters.items():
        assert inspect.signature(ctc_loss).parameters[name].default == p.default, name
    # the length arguments, whose checks need no device
    from rroi_align import ctc
    with pytest.raises(ValueError):
        ctc._lengths([4], "input_lengths", 2, lp.device)
    with pytest.raises(ValueError):
        ctc._lengths(torch.zeros(2), "input_lengths", 2, lp.device)
    with pytest.raises(ValueError):
        ctc._lengths(3, "input_lengths", 2, lp.device)
    assert ctc._lengths(torch.tensor([4, 3]), "input_lengths", 2, lp.device) == (None, [4, 3])
    assert ctc._lengths((4, 3), "input_lengths", 2, lp.device) == (None, [4, 3])


def test_recognition_loss_defaults_to_the_stock_loss():
    from fots_e2e.train import recognition_loss
    params = inspect.signature(recognition_loss).parameters
    assert list(params) == ["net", "features", "rois", "targets", "target_lengths", "native_ctc", "return_debug"]
    assert params["native_ctc"].default is False and params["return_debug"].default is False


def _close(got, want):
    """1e-12 relative, with a floor of one unit: |got - want| <= 1e-12 * max(1, |want|) -- the quantities are log-domain
    sums of up to ~1000 in magnitude (the losses) and differences of probabilities (the gradients)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all())


@pytest.mark.parametrize("name", CC.FINITE_FEASIBLE)
def test_restatement_equals_torch_on_the_cpu_in_float64(name):
    c = CC.CASE[name]
    for dtype in (torch.float32, torch.bfloat16):          # the values the GPU tests feed: both roundings of the case
        lp, (nll, grad, M) = CC.materialise(c, dtype)
        assert np.isfinite(nll).all() and np.isfinite(lp.float().numpy()).all()
        x = lp.double().requires_grad_(True)
        loss = F.ctc_loss(x, torch.from_numpy(c["targets"]), c["in_len"], c["tgt_len"], blank=c["blank"], reduction="none")
        loss.sum().backward()
        print("%s %s: loss %.3e grad %.3e" % (name, dtype, np.abs(loss.detach().numpy() - nll).max(), np.abs(x.grad.numpy() - grad).max()))
        assert _close(nll, loss.detach().numpy())
        assert _close(grad, x.grad.numpy())


def _nll_by_logsumexp(lp, target, Tn, blank):
    """The forward recursion of one sequence in differentiable torch: lp (T, K) double -> nll."""
    ext = [blank] * (2 * len(target) + 1)
    ext[1::2] = target
    S, ninf = len(ext), torch.tensor(-np.inf, dtype=torch.float64)
    a = [lp[0, ext[s]] if s < 2 else ninf for s in range(S)]
    for t in range(1, Tn):
        nxt = []
        for s in range(S):
            terms = [a[s]] + ([a[s - 1]] if s >= 1 else []) + \
                ([a[s - 2]] if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2] else [])
            terms = [v for v in terms if v.item() != -np.inf]
            nxt.append(lp[t, ext[s]] + torch.logsumexp(torch.stack(terms), 0) if terms else ninf)
        a = nxt
    return -torch.logsumexp(torch.stack([v for v in a[max(S - 2, 0):] if v.item() != -np.inf]), 0)


def test_convention_gradient_is_the_derivative_with_respect_to_the_logits():
    """The 'torch convention' gradient is not d nll / d lp of free variables (which has no exp(lp) term) but what
    log_softmax's backward turns into the true derivative with respect to the logits: g - softmax * sum_k g."""
    c = CC.CASE["t33_ragged"]
    rng = np.random.default_rng(5)
    T, N, K = c["T"], c["N"], c["K"]
    z = torch.from_numpy(rng.standard_normal((T, N, K)) * 2.0).requires_grad_(True)
    lp = z.log_softmax(2)
    total = sum(_nll_by_logsumexp(lp[:, n], [int(v) for v in c["targets"][n, :c["tgt_len"][n]]], c["in_len"][n], c["blank"])
                for n in range(N))
    want, = torch.autograd.grad(total, z)
    nll, g, _ = CC.ref64(lp.detach().numpy(), c["targets"], c["in_len"], c["tgt_len"], c["blank"])
    p = lp.detach().exp().numpy()
    through = g - p * g.sum(2, keepdims=True)
    assert _close(through, want.numpy())
    assert (want.numpy()[c["in_len"][1]:, 1] == 0).all() and (g[c["in_len"][1]:, 1] == 0).all()     # nothing past T_n


def test_restatement_defines_the_cases_torch_leaves_open():
    for name in ("t1", "t2_k2", "repeats", "holes", "bad_label", "bad_lengths"):
        c = CC.CASE[name]
        lp, (nll, grad, M) = CC.materialise(c)
        assert not np.isnan(nll).any() and not np.isnan(grad).any(), name
        assert (grad[:, np.isinf(nll)] == 0).all(), name
        nll0 = CC.ref64(lp.double().numpy(), c["targets"], c["in_len"], c["tgt_len"], c["blank"], zero_infinity=True)[0]
        assert (nll0[np.isinf(nll)] == 0).all() and np.array_equal(nll0[~np.isinf(nll)], nll[~np.isinf(nll)]), name
    assert np.isinf(CC.materialise(CC.CASE["t1"])[1][0]).tolist() == [False, False, True]           # T_n = 0 with a target
    assert np.isinf(CC.materialise(CC.CASE["t2_k2"])[1][0]).tolist() == [False, True, False]        # 'aa' needs three steps
    assert np.isinf(CC.materialise(CC.CASE["repeats"])[1][0]).tolist() == [False, False, True]      # exactly feasible; one short
    assert np.isinf(CC.materialise(CC.CASE["bad_label"])[1][0]).tolist() == [False, True, True]
    assert np.isinf(CC.materialise(CC.CASE["bad_lengths"])[1][0]).tolist() == [False, True, True]
    lp, (nll, grad, _) = CC.materialise(CC.CASE["holes"])
    assert np.isinf(lp.numpy()).any() and np.isfinite(nll).sum() >= 2 and (grad[np.isinf(lp.numpy())] == 0).all()
    # near-certain inputs: the loss all but vanishes and the gradient is a difference of nearly equal numbers
    lp, (nll, grad, _) = CC.materialise(CC.CASE["certain"])
    assert (nll < 1e-6).all() and np.abs(grad).max() < 1e-6 and np.exp(lp.numpy().max(2)).min() > 1 - 1e-6
    # the ulp helper: spacing at 1, below 1, and of the subnormals
    assert CC.ulp(1.0, torch.float32) == 2.0 ** -23 and CC.ulp(0.75, torch.bfloat16) == 2.0 ** -8
    assert CC.ulp(0.0, torch.float16) == 2.0 ** -24 and CC.ulp(1e-30, torch.float16) == 2.0 ** -24
