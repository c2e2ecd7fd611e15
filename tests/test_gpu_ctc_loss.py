"""GPU: the native CTC loss against the float64 restatement of tests/ctc_loss_cases.py, whose bound is derived
there: |grad - ref| <= ulp_out(ref) + 4 E, |nll - ref| <= ulp_fp32(ref) + 2 E, E = 8 (T + 1) M 2^-53.  Every test asserts
ratio <= 1 and prints the ratio it met."""
import numpy as np
import pytest
import torch

import ctc_loss_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = [c["name"] for c in CC.CASES]


def _ctc():
    from rroi_align import ctc
    return ctc


def _forms(case, i):
    """The case's targets and lengths in one of the accepted forms, by index: padded / flat, int64 / int32, lengths as host
    lists / device tensors.  A target length beyond the padded width has no flat form and stays padded."""
    tg = torch.from_numpy(case["targets"])
    flat_ok = all(0 <= L <= tg.shape[1] for L in case["tgt_len"])
    if i & 1 and flat_ok:
        tg = torch.cat([tg[n, :L] for n, L in enumerate(case["tgt_len"])])
    tg = tg.to(torch.int32 if i & 2 else torch.int64).to(DEV)
    if i & 4:
        return tg, torch.tensor(case["in_len"], dtype=torch.int64, device=DEV), torch.tensor(case["tgt_len"], dtype=torch.int32, device=DEV)
    return tg, list(case["in_len"]), tuple(case["tgt_len"])


def _run(lp_dev, case, form=0, **kw):
    """nll (N) and the autograd gradient for grad_output = 1, through the public surface."""
    tg, il, tl = _forms(case, form)
    x = lp_dev.detach().requires_grad_(True)
    nll = _ctc().ctc_loss(x, tg, il, tl, blank=case["blank"], reduction="none", **kw)
    g, = torch.autograd.grad(nll, x, torch.ones_like(nll))
    return nll.detach(), g


def _check(nll, g, case, dtype, what):
    lp, (rn, rg, M) = CC.materialise(case, dtype)
    assert nll.dtype == torch.float32 and g.dtype == dtype and g.shape == lp.shape
    assert not torch.isnan(nll).any() and not torch.isnan(g).any(), what
    rl, rgr = CC.nll_ratio(nll, rn, case["T"], M), CC.grad_ratio(g, rg, dtype, case["T"], M)
    print("%s: nll ratio %.3f, grad ratio %.3f (E = %.2e)" % (what, rl, rgr, CC.E_of(case["T"], M)))
    assert rl <= 1.0 and rgr <= 1.0, (what, rl, rgr)
    return rl, rgr


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", NAMES)
def test_every_case_meets_the_bound_and_repeats_bit_for_bit(name, dtype):
    case = CC.CASE[name]
    lp, (rn, rg, M) = CC.materialise(case, dtype)
    x = lp.to(DEV)
    form = NAMES.index(name) + 3 * CC.DTYPES.index(dtype)
    nll, g = _run(x, case, form)
    _check(nll, g, case, dtype, "%s %s form %d" % (name, dtype, form % 8))
    nll2, g2 = _run(x, case, form)
    assert torch.equal(nll, nll2) and torch.equal(g.view(torch.uint8), g2.view(torch.uint8))
    # infinite losses: exactly where the restatement has them, with a zero gradient; 0 with zero_infinity, the rest unchanged
    inf = torch.from_numpy(np.isinf(rn)).to(DEV)
    assert torch.equal(torch.isinf(nll), inf) and (nll[inf] > 0).all() and not g[:, inf].any()
    nll0, g0 = _run(x, case, form, zero_infinity=True)
    assert not nll0[inf].any() and torch.equal(nll0[~inf], nll[~inf]) and torch.equal(g0.view(torch.uint8), g.view(torch.uint8))
    # no gradient wanted: the same losses from the alpha pass alone
    tg, il, tl = _forms(case, form)
    with torch.no_grad():
        assert torch.equal(_ctc().ctc_loss(x, tg, il, tl, blank=case["blank"], reduction="none"), nll)
    assert torch.equal(_ctc().ctc_loss(x, tg, il, tl, blank=case["blank"], reduction="none"), nll)


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", ["t33_ragged", "l31_l32", "l64_ws", "holes"])
def test_layouts_are_read_in_place_and_a_third_takes_the_copy(name, dtype):
    case = CC.CASE[name]
    lp = CC.materialise(case, dtype)[0]
    base, _ = _run(lp.to(DEV), case)                                   # torch's contiguous (T, N, K)
    # the recogniser's (N, K, T) viewed as (T, N, K): read where it lies, the gradient with the same strides
    x = lp.permute(1, 2, 0).contiguous().to(DEV).permute(2, 0, 1)
    assert x.stride(0) == 1 and not x.is_contiguous()
    nll, g = _run(x, case)
    assert g.stride() == x.stride()
    _check(nll, g, case, dtype, "%s %s (N, K, T)" % (name, dtype))
    assert torch.equal(nll, base)                                      # the same arithmetic whatever the layout
    x = lp.to(DEV)
    nll, g = _run(x, case)
    assert g.stride() == x.stride() and g.is_contiguous()
    # neither stride is 1: (K, T, N) viewed as (T, N, K) takes one contiguous copy
    x = lp.permute(2, 0, 1).contiguous().to(DEV).permute(1, 2, 0)
    assert x.stride(0) != 1 and x.stride(2) != 1
    nll, g = _run(x, case)
    assert g.shape == x.shape
    _check(nll, g, case, dtype, "%s %s copied" % (name, dtype))
    assert torch.equal(nll, base)


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=["fp32", "bf16", "fp16"])
def test_reductions_and_a_non_uniform_grad_output(dtype):
    """grad_output w_n scales sequence n's gradient: the stored gradient (within ulp_out + 4 E of the reference) times w in
    float32, rounded once more to the dtype: |got - w ref| <= |w| (ulp_out(ref) + 4 E) + ulp_out(w ref) + 2^-22 |w ref|, the
    last term for a w that torch itself evaluates in float32 ('mean': 1 / (N max(L, 1)))."""
    case = CC.CASE["t33_ragged"]
    lp, (rn, rg, M) = CC.materialise(case, dtype)
    tg, il, tl = _forms(case, 0)
    T, N = case["T"], case["N"]
    E = CC.E_of(T, M)

    def ratio(g, w):
        ref = rg * w[None, :, None]
        tol = np.abs(w)[None, :, None] * (CC.ulp(rg, dtype) + 4 * E) + CC.ulp(ref, dtype) + 2.0 ** -22 * np.abs(ref)
        return float((np.abs(g.double().cpu().numpy() - ref) / tol).max())

    w = np.array([0.5, -1.25, 3.0])
    x = lp.to(DEV).requires_grad_(True)
    nll = _ctc().ctc_loss(x, tg, il, tl, blank=case["blank"], reduction="none")
    g, = torch.autograd.grad(nll, x, torch.from_numpy(w).float().to(DEV))
    r_none = ratio(g, w)
    # mean: each loss over its target length (at least 1), then the average; sum: the plain sum
    x = lp.to(DEV).requires_grad_(True)
    loss = _ctc().CTCLoss(blank=case["blank"])(x, tg, il, tl)
    loss.backward()
    wm = 1.0 / (N * np.maximum(np.array(case["tgt_len"]), 1.0))
    r_mean = ratio(x.grad, wm)
    want = float((rn * wm).sum())
    tol = float(((CC.ulp(rn, torch.float32) + 2 * E) * wm).sum() + (N + 2) * 2.0 ** -23 * np.abs(rn * wm).sum())
    r_loss = abs(float(loss.detach()) - want) / tol
    total = _ctc().ctc_loss(lp.to(DEV), tg, il, tl, blank=case["blank"], reduction="sum")
    tol = float((CC.ulp(rn, torch.float32) + 2 * E).sum() + (N + 1) * 2.0 ** -23 * np.abs(rn).sum())
    r_sum = abs(float(total) - float(rn.sum())) / tol
    print("%s: none %.3f mean %.3f (loss %.3f) sum %.3f" % (dtype, r_none, r_mean, r_loss, r_sum))
    assert max(r_none, r_mean, r_loss, r_sum) <= 1.0
    assert loss.dtype == torch.float32 and loss.dim() == 0 and x.grad.dtype == dtype


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=["fp32", "bf16", "fp16"])
def test_gradient_into_a_view_leaves_its_surroundings_untouched(dtype):
    from rroi_align._ext.rroi_align.ctc_loss import run_ctc_loss
    case = CC.CASE["t33_ragged"]
    lp, (rn, rg, M) = CC.materialise(case, dtype)
    T, N, K = lp.shape
    tg = torch.from_numpy(case["targets"]).to(torch.int32).to(DEV)
    il = torch.tensor(case["in_len"], dtype=torch.int32, device=DEV)
    tl = torch.tensor(case["tgt_len"], dtype=torch.int32, device=DEV)
    for permuted in (False, True):
        buf = torch.full((T * N * K + 2,), 7.0, dtype=dtype, device=DEV)
        g = buf[1:-1].view(N, K, T).permute(2, 0, 1) if permuted else buf[1:-1].view(T, N, K)
        nll, out = run_ctc_loss(lp.to(DEV), tg, il, tl, case["blank"], False, True, grad=g)
        assert out is g and out.data_ptr() == buf.data_ptr() + buf.element_size()
        assert float(buf[0]) == 7.0 and float(buf[-1]) == 7.0
        assert not (g == 7.0).any()                        # no gradient is 7: every element was written
        _check(nll, g, case, dtype, "%s into a view, permuted %s" % (dtype, permuted))


def test_forward_and_backward_run_in_deterministic_mode():
    case = CC.CASE["t33_ragged"]
    lp = CC.materialise(case)[0]
    torch.use_deterministic_algorithms(True)
    try:
        for form in (0, 5):                                # host lists; flat targets with device lengths
            nll, g = _run(lp.to(DEV), case, form)
            torch.cuda.synchronize()
            _check(nll, g, case, torch.float32, "deterministic mode, form %d" % form)
    finally:
        torch.use_deterministic_algorithms(False)


@pytest.mark.parametrize("name", ["repeats", "bad_label", "bad_lengths", "t1", "t2_k2"])
def test_infeasible_sequences_are_infinite_with_a_zero_gradient(name):
    case = CC.CASE[name]
    lp, (rn, rg, M) = CC.materialise(case)
    assert np.isinf(rn).any()
    for form in (0, 6):
        nll, g = _run(lp.to(DEV), case, form)
        inf = np.isinf(rn)
        assert np.array_equal(torch.isinf(nll).cpu().numpy(), inf) and (nll.cpu().numpy()[inf] > 0).all()
        assert not g.cpu().numpy()[:, inf].any() and not torch.isnan(g).any()
        nll0, g0 = _run(lp.to(DEV), case, form, zero_infinity=True)
        assert not nll0.cpu().numpy()[inf].any() and not g0.cpu().numpy()[:, inf].any()
        assert not torch.isnan(nll0).any() and not torch.isnan(g0).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_recognition_loss_native(dtype):
    from fots_e2e.model import FOTSNet
    from fots_e2e.train import recognition_loss
    from fots_e2e.weights import deterministic_init
    rng = np.random.default_rng(11)
    net = deterministic_init(FOTSNet(87)).to(DEV).to(dtype).train()
    fmap = torch.from_numpy(rng.standard_normal((2, 64, 32, 32)).astype(np.float32)).to(DEV).to(dtype).requires_grad_(True)
    rois = torch.tensor([[0, 40, 40, 16, 50, 10], [1, 64, 64, 20, 64, -20], [0, 80, 50, 12, 30, 0], [1, 50, 90, 24, 60, 35]],
                        dtype=torch.float32, device=DEV)
    lens = [3, 4, 2, 5]
    targets = torch.from_numpy(rng.integers(1, 87, sum(lens))).to(DEV)
    loss, crops, preds = recognition_loss(net, [None, fmap], rois, targets, lens, native_ctc=True, return_debug=True)
    assert crops.shape[:3] == (4, 64, 11) and crops.size(3) == int(np.ceil(11 * 3.2)) and preds.shape[:2] == (4, 87)
    assert preds.dtype == dtype and loss.dtype == torch.float32
    T = preds.size(2)
    padded = np.zeros((4, 5), dtype=np.int64)
    flat = targets.cpu().numpy()
    for n, L in enumerate(lens):
        padded[n, :L] = flat[sum(lens[:n]):sum(lens[:n]) + L]
    rn, _, M = CC.ref64(preds.detach().permute(2, 0, 1).double().cpu().numpy(), padded, [T] * 4, lens)
    assert np.isfinite(rn).all()
    tol = ((CC.ulp(rn, torch.float32) + 2 * CC.E_of(T, M)).sum() + 5 * CC.ulp(rn.sum(), torch.float32)) / 4
    r = abs(float(loss.detach()) - rn.sum() / 4) / tol
    print("%s: recognition loss %.6f, ratio %.3f" % (dtype, float(loss.detach()), r))
    assert r <= 1.0
    loss.backward()
    assert fmap.grad is not None and torch.isfinite(fmap.grad).all() and fmap.grad.abs().sum() > 0
    # two calls on the same log-probabilities: the same bits, and the bits recognition_loss returned
    from rroi_align.ctc import ctc_loss
    a = ctc_loss(preds.detach().permute(2, 0, 1), targets, [T] * 4, lens, reduction="sum") / 4
    b = ctc_loss(preds.detach().permute(2, 0, 1), targets, [T] * 4, lens, reduction="sum") / 4
    assert torch.equal(a, b) and torch.equal(a, loss.detach())
