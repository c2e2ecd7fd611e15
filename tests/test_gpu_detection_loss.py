"""GPU: the native detection loss against the float64 restatement of tests/detection_loss_cases.py, whose bound
is derived there: a term within ulp_fp32(ref) + 2 d of the reference, a gradient element within ulp_out(|ref| + 2 e) / 2 + 2 e,
d and e the propagated double-precision errors.  Every test asserts ratio <= 1 and prints the ratio it met."""
import numpy as np
import pytest
import torch

import detection_loss_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = ["fp32", "bf16", "fp16"]


def _det():
    from rroi_align import detection
    return detection


def _flat(lists, case):
    return [lists[k][s] for s in range(1 + case["multi"]) for k in range(3)]


def _run(case, dtype, fn=None, **kw):
    """terms (4) and the gradients of g . terms in the order s4, a4, r4, s8, a8, r8, through the public surface."""
    fn = fn or _det().detection_loss
    lists, gt = DC.tensors(case, dtype, DEV)
    terms = fn(lists[0], gt[0], gt[1], lists[1], gt[2], lists[2], gt[3], multi_scale=case["multi"], return_terms=True, **kw)
    g = torch.tensor(case["g"], dtype=terms.dtype, device=DEV)
    grads = torch.autograd.grad(terms, _flat(lists, case), g, allow_unused=True)
    return terms.detach(), grads


def _check(terms, grads, case, dtype, what):
    preds, ref = DC.materialise(case, dtype)
    assert terms.dtype == torch.float32 and terms.shape == (4,)
    flat = [p[k] for p in preds for k in range(3)]
    assert len(grads) == len(flat) and all(g.dtype == dtype and g.shape == p.shape for g, p in zip(grads, flat))
    rt, rg = DC.terms_ratio(terms, ref), DC.grads_ratio(grads, ref, dtype)
    print("%s: terms ratio %.3f, gradient ratio %.3f (d = %.2e, e = %.2e)" %
          (what, rt, rg, ref["d_terms"].max(), max(float(e.max()) for e in ref["e_grads"])))
    assert rt <= 1.0 and rg <= 1.0, (what, rt, rg)
    return rt, rg


def _bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("dtype", DC.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", DC.NAMES)
def test_every_case_meets_the_bound_and_repeats_bit_for_bit(name, dtype):
    case = DC.CASE[name]
    terms, grads = _run(case, dtype)
    _check(terms, grads, case, dtype, "%s %s" % (name, dtype))
    terms2, grads2 = _run(case, dtype)
    assert torch.equal(_bits(terms), _bits(terms2))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads, grads2))
    # no gradient wanted: the same terms, nothing saved; the scalar form is terms[3]
    lists, gt = DC.tensors(case, dtype, DEV)
    args = (lists[0], gt[0], gt[1], lists[1], gt[2], lists[2], gt[3])
    with torch.no_grad():
        t = _det().detection_loss(*args, multi_scale=case["multi"], return_terms=True)
        assert torch.equal(_bits(t), _bits(terms)) and not t.requires_grad and t.grad_fn is None
    lists, gt = DC.tensors(case, dtype, DEV, requires_grad=False)
    args = (lists[0], gt[0], gt[1], lists[1], gt[2], lists[2], gt[3])
    t = _det().detection_loss(*args, multi_scale=case["multi"], return_terms=True)
    assert torch.equal(_bits(t), _bits(terms)) and t.grad_fn is None
    total = _det().DetectionLoss(multi_scale=case["multi"])(*args)
    assert total.dim() == 0 and torch.equal(total, terms[3])


def test_the_cases_reach_both_plans_and_the_documented_zeros():
    from rroi_align._ext.rroi_align.detection_loss import detection_loss_plan
    c = DC.CASE["multiblock"]
    p = detection_loss_plan(c["N"], c["H"], c["W"], c["H8"], c["W8"])
    assert p.grid_x > 1 and p.items_per_thread > 1 and p.blocks_eighth > 1
    assert {detection_loss_plan(c["N"], c["H"], c["W"], c["H8"], c["W8"]).items_per_thread for c in DC.CASES} == {1, 4}
    # empty: the angle and box terms are 0 with zero gradients, the dice term is not
    terms, grads = _run(DC.CASE["empty"], torch.float32)
    assert float(terms[1]) == 0 and float(terms[2]) == 0 and float(terms[0]) < 0 and torch.equal(terms[3], terms[0])
    assert not any(bool(g.any()) for g in (grads[1], grads[2], grads[4], grads[5])) and grads[0].any() and grads[3].any()
    # an empty left / right selection: no NaN, that side's gradient is zero, the rest is not
    for name, side in (("no_left", 2), ("no_right", 3)):
        terms, grads = _run(DC.CASE[name], torch.float32)
        assert torch.isfinite(terms).all() and float(terms[2]) > 0
        for g in (grads[2], grads[5]):
            assert torch.isfinite(g).all() and not g[:, side].any() and g[:, 5 - side].any() and g[:, 0].any()


@pytest.mark.parametrize("dtype", DC.DTYPES, ids=IDS)
def test_every_gradient_element_is_written(dtype):
    """Through the binding: buffers full of NaN, with a guard element on either side, come back with no NaN inside, exact
    zeros off the mask, and the guards untouched."""
    from rroi_align._ext.rroi_align.detection_loss import run_detection_loss, run_detection_loss_backward
    for name in ("odd", "single_scale", "multiblock"):
        case = DC.CASE[name]
        lists, gt = DC.tensors(case, dtype, DEV, requires_grad=False)
        preds = [tuple(lists[k][s] for k in range(3)) for s in range(1 + case["multi"])]
        preds8 = preds[1] if case["multi"] else None
        terms, state = run_detection_loss(preds[0], preds8, tuple(gt))
        assert state.dtype == torch.float64 and state.numel() == 20
        bufs = [[torch.full((t.numel() + 2,), float("nan"), dtype=dtype, device=DEV) for t in p] for p in preds]
        views = [tuple(b[1:-1].view(t.shape) for b, t in zip(bs, p)) for bs, p in zip(bufs, preds)]
        g = torch.tensor(case["g"], dtype=torch.float32, device=DEV)
        g4, g8 = run_detection_loss_backward(preds[0], preds8, tuple(gt), state, g, views[0], views[1] if case["multi"] else None)
        assert all(a is b for a, b in zip(g4, views[0])) and (g8 is None) == (not case["multi"])
        for bs in bufs:
            for b in bs:
                assert torch.isnan(b[0]) and torch.isnan(b[-1]) and not torch.isnan(b[1:-1]).any()
        _check(terms, [v for vs in views for v in vs], case, dtype, "%s %s into NaN-filled buffers" % (name, dtype))
        for s, vs in enumerate(views):
            mask = torch.from_numpy(DC.truth_of_scale(case["gt"], preds[s][0].shape[2:] if s else None)[0] > 0.5).to(DEV)
            off = ~mask[:, None]
            assert not vs[1][off.expand_as(vs[1])].any() and not vs[2][off.expand_as(vs[2])].any()
            assert vs[1][mask[:, None].expand_as(vs[1])].any()


def test_no_host_synchronisation_forward_and_backward():
    """The native call under torch's synchronisation check set to raise.  (The stock restatement indexes with boolean masks
    and branches on `.sum() > 0`, each a synchronisation, as a reading of fots_e2e/train.py shows; it is not run here.)"""
    case = DC.CASE["square"]
    results = []
    for dtype in (torch.float32, torch.bfloat16):
        lists, gt = DC.tensors(case, dtype, DEV)
        g = torch.tensor(case["g"], dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            terms = _det().detection_loss(lists[0], gt[0], gt[1], lists[1], gt[2], lists[2], gt[3], return_terms=True)
            grads = torch.autograd.grad(terms, _flat(lists, case), g)
            total = _det().detection_loss(lists[0], gt[0], gt[1], lists[1], gt[2], lists[2], gt[3])
            total.backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        results.append((dtype, terms.detach(), grads, total.detach(), lists))
    for dtype, terms, grads, total, lists in results:
        _check(terms, grads, case, dtype, "no synchronisation, %s" % dtype)
        assert torch.equal(total, terms[3])
        assert all(torch.equal(_bits(t.grad), _bits(g)) for t, g in zip(_flat(lists, case), grads))     # g = [0, 0, 0, 1] both ways


def test_forward_and_backward_are_graph_capturable():
    """The three launches on one stream, captured and replayed into cleared buffers: the same bits."""
    from rroi_align._ext import rroi_align as ext
    from rroi_align._ext.rroi_align.detection_loss import detection_loss_workspace_bytes
    case, dtype = DC.CASE["multiblock"], torch.bfloat16
    lists, gt = DC.tensors(case, dtype, DEV, requires_grad=False)
    preds = _flat(lists, case)
    dims = (case["N"], case["H"], case["W"], case["H8"], case["W8"])
    nbytes = detection_loss_workspace_bytes(*dims)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    terms = torch.empty(4, dtype=torch.float32, device=DEV)
    grads = [torch.empty_like(p) for p in preds]
    g = torch.tensor(case["g"], dtype=torch.float32, device=DEV)
    ptr = [t.data_ptr() for t in gt]

    def calls():
        st = torch.cuda.current_stream().cuda_stream
        assert ext._lib.rroi_detection_loss_forward_hip(1, *(p.data_ptr() for p in preds), *ptr, *dims, terms.data_ptr(),
                                                        ws.data_ptr(), nbytes, st) == 1
        assert ext._lib.rroi_detection_loss_backward_hip(1, preds[1].data_ptr(), preds[2].data_ptr(), preds[4].data_ptr(),
                                                         preds[5].data_ptr(), *ptr, *dims, ws[-20:].data_ptr(), g.data_ptr(),
                                                         *(t.data_ptr() for t in grads), st) == 1
    calls()
    torch.cuda.synchronize()
    want_terms, want_grads = terms.clone(), [t.clone() for t in grads]
    _check(want_terms, want_grads, case, dtype, "through the C calls")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls()
    for t in [terms, ws] + grads:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(terms), _bits(want_terms))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads, want_grads))


def test_train_detection_loss_native_against_stock():
    """fots_e2e.train.detection_loss on `square` in float32: the stock path (float32 sums, float32 resize) within the
    float32-accumulation tolerance of the float64 restatement, the native path within its own bound."""
    from fots_e2e.train import detection_loss
    case = DC.CASE["square"]
    ref = DC.materialise(case, torch.float32)[1]
    n = DC.items(case)
    terms, grads = _run(case, torch.float32, detection_loss, native=True)
    _check(terms, grads, case, torch.float32, "train.detection_loss(native=True)")
    sterms, sgrads = _run(case, torch.float32, detection_loss, native=False)
    rt, rg = DC.f32_terms_ratio(sterms, ref["terms"], n), DC.f32_grads_ratio(sgrads, ref["grads"], n)
    print("stock float32 against the restatement: terms ratio %.4f, gradient ratio %.4f (n = %d)" % (rt, rg, n))
    assert rt <= 1.0 and rg <= 1.0
    lists, gt = DC.tensors(case, torch.float32, DEV)
    total = detection_loss(lists[0], gt[0], gt[1], lists[1], gt[2], lists[2], gt[3], native=True)
    assert total.dim() == 0 and torch.equal(total, terms[3])
