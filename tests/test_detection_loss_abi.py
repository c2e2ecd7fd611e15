"""CPU: the native detection loss -- the entry points are exported, declared and host-checked; the plan query is
pure and depends on the shape alone; the workspace size follows from the plan; the Python surface refuses CPU tensors,
mixed dtypes and bad shapes; `fots_e2e.train.detection_loss` defaults to the stock restatement, which reproduces the
reference's own numbers (tests/golden/detection_loss.npz) in float32; the float64 restatement the GPU tests measure against
equals the stock restatement run in float64 (terms and autograd gradients) on every case without an empty selection, and
gives zeros where the stock path gives NaN.  No kernel is launched here."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import detection_loss_cases as DC
from test_abi import declared_functions

NAMES = ("rroi_detection_loss_forward_hip", "rroi_detection_loss_backward_hip", "rroi_detection_loss_plan",
         "rroi_detection_loss_workspace_bytes")
FP32, BF16, FP16 = 0, 1, 2
P = 0x7f0000000000   # non-null, 16-byte aligned, never dereferenced: every call it is passed to is refused on the host
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detection_loss.npz")


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


@pytest.fixture(scope="module")
def dl():
    from rroi_align._ext.rroi_align import detection_loss
    return detection_loss


def test_symbols_are_exported_and_declared(ext, dl):
    lib = ctypes.CDLL(ext.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions() and name in ext.EXPORTS and hasattr(lib, name), name
    assert ext.version() == "rroi_align_hip 0.10.0 gfx950"      # the version string stays
    # the package's `_*_run` callables stay the closed list the network's ledger reads
    assert not any(k.startswith("_") and k.endswith("_run") for k in vars(dl))
    for name in ("run_detection_loss", "run_detection_loss_backward", "detection_loss_plan", "detection_loss_workspace_bytes"):
        assert callable(getattr(dl, name)), name


SHAPES = [(c["N"], c["H"], c["W"], c["H8"], c["W8"]) for c in DC.CASES] + [
    (2, 128, 128, 64, 64), (8, 128, 128, 64, 64), (16, 128, 128, 64, 64), (8, 176, 320, 88, 160), (1, 1, 1, 0, 0), (1, 64, 64, 0, 0),
    (1, 64, 64, 1, 1), (2, 32, 32, 31, 33)]


def _ipt(items):
    return 1 if items <= 4096 else 2 if items <= 16384 else 4 if items <= 262144 else 8


def test_plan_query_is_pure_and_depends_on_the_shape_alone(dl):
    for (n, h, w, h8, w8) in SHAPES:
        plans = [dl.detection_loss_plan(n, h, w, h8, w8, dtype) for dtype in DC.DTYPES]
        assert plans[0] == plans[1] == plans[2] == dl.detection_loss_plan(n, h, w, h8, w8)            # pure; no dtype in it
        p = plans[0]
        i4, i8 = n * h * w, n * h8 * w8
        per = 256 * _ipt(i4 + i8)
        assert p.block == 256 and p.items_per_thread == _ipt(i4 + i8)
        assert p.blocks_quarter == -(-i4 // per) and p.blocks_eighth == -(-i8 // per)                 # no empty workgroup
        assert p.grid_x == p.blocks_quarter + p.blocks_eighth
        assert (p.slot_doubles, p.state_doubles, p.finish_block) == (10, 20, 64)
        assert dl.detection_loss_workspace_bytes(n, h, w, h8, w8) == (p.grid_x * p.slot_doubles + p.state_doubles) * 8
    # the reference's training shape: 40 workgroups of four items a thread; the test cases: one workgroup, and several
    assert dl.detection_loss_plan(2, 128, 128, 64, 64)[:5] == (40, 256, 4, 32, 8)
    c = DC.CASE["multiblock"]
    p = dl.detection_loss_plan(c["N"], c["H"], c["W"], c["H8"], c["W8"])
    assert p.grid_x > 1 and p.items_per_thread > 1
    assert dl.detection_loss_plan(1, 2, 2, 1, 1).grid_x == 2 and dl.detection_loss_plan(1, 13, 19).grid_x == 1
    # nothing in the source of the plan asks the device for anything
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "fots.pytorch_amd", "csrc", "rroi_detection_loss_host.h")).read()
    assert "hipGetDevice" not in src and "hipDeviceGetAttribute" not in src and "multiProcessorCount" not in src


def _forward(ext, dtype=FP32, preds4=(P, P, P), preds8=(P, P, P), gt=(P, P, P, P), dims=(2, 13, 21, 7, 11), terms=P, ws=P,
             ws_bytes=1 << 20):
    return ext._lib.rroi_detection_loss_forward_hip(dtype, *preds4, *preds8, *gt, *dims, terms, ws, ws_bytes, None)


def _backward(ext, dtype=FP32, preds4=(P, P), preds8=(P, P), gt=(P, P, P, P), dims=(2, 13, 21, 7, 11), state=P, g=P,
              grads4=(P, P, P), grads8=(P, P, P)):
    return ext._lib.rroi_detection_loss_backward_hip(dtype, *preds4, *preds8, *gt, *dims, state, g, *grads4, *grads8, None)


def _with(seq, i, v):
    return tuple(v if k == i else x for k, x in enumerate(seq))


def test_refusals_return_zero_before_any_launch(ext, dl):
    plan, info = ext._lib.rroi_detection_loss_plan, dl._DetectionLossPlan()
    good = (2, 13, 21, 7, 11)
    for dtype in (3, -1):
        assert _forward(ext, dtype=dtype) == 0 and _backward(ext, dtype=dtype) == 0
        assert plan(dtype, *good, ctypes.byref(info)) == 0
    need = dl.detection_loss_workspace_bytes(*good)
    assert need == ((3 + 1) * 10 + 20) * 8
    for dtype in (FP32, BF16, FP16):
        assert plan(dtype, *good, ctypes.byref(info)) == 1
        assert plan(dtype, *good, None) == 0
        for dims in ((0, 13, 21, 7, 11), (2, 0, 21, 7, 11), (2, 13, -1, 7, 11), (2, 13, 21, 0, 11), (2, 13, 21, 7, 0),
                     (2, 13, 21, -7, -11), (4, 1 << 15, 1 << 15, 0, 0), (1, 8, 8, 1 << 16, 1 << 15)):     # the last two: too many pixels
            assert _forward(ext, dtype=dtype, dims=dims) == 0, dims
            assert _backward(ext, dtype=dtype, dims=dims) == 0, dims
            assert plan(dtype, *dims, ctypes.byref(info)) == 0, dims
            assert dl.detection_loss_workspace_bytes(*dims) == 0
        # a NULL tensor that the shape needs
        for i in range(3):
            assert _forward(ext, dtype=dtype, preds4=_with((P, P, P), i, None)) == 0
            assert _forward(ext, dtype=dtype, preds8=_with((P, P, P), i, None)) == 0
            assert _backward(ext, dtype=dtype, grads4=_with((P, P, P), i, None)) == 0
            assert _backward(ext, dtype=dtype, grads8=_with((P, P, P), i, None)) == 0
        for i in range(2):
            assert _backward(ext, dtype=dtype, preds4=_with((P, P), i, None)) == 0
            assert _backward(ext, dtype=dtype, preds8=_with((P, P), i, None)) == 0
        for i in range(4):
            assert _forward(ext, dtype=dtype, gt=_with((P, P, P, P), i, None)) == 0
            assert _backward(ext, dtype=dtype, gt=_with((P, P, P, P), i, None)) == 0
        assert _forward(ext, dtype=dtype, terms=None) == 0
        assert _backward(ext, dtype=dtype, state=None) == 0 and _backward(ext, dtype=dtype, g=None) == 0
        # roi_gt is read four channels at a time; the state is doubles, the weights floats
        assert _forward(ext, dtype=dtype, gt=(P, P, P, P + 8)) == 0 and _backward(ext, dtype=dtype, gt=(P, P, P, P + 4)) == 0
        assert _backward(ext, dtype=dtype, state=P + 4) == 0 and _backward(ext, dtype=dtype, g=P + 2) == 0
        # the workspace: NULL, short and misaligned
        assert _forward(ext, dtype=dtype, ws=None, ws_bytes=need) == 0
        assert _forward(ext, dtype=dtype, ws=P, ws_bytes=need - 1) == 0
        assert _forward(ext, dtype=dtype, ws=P + 4, ws_bytes=need) == 0
    with pytest.raises(ValueError):
        dl.detection_loss_plan(2, 13, 21, 7, 0)
    with pytest.raises(TypeError):
        dl.detection_loss_plan(2, 13, 21, 7, 11, dtype=torch.float64)


def _cpu_arguments(name="odd", dtype=torch.float32):
    lists, gt = DC.tensors(DC.CASE[name], dtype, "cpu", requires_grad=False)
    return lists, gt


def _call(fn, lists, gt, **kw):
    return fn(lists[0], gt[0], gt[1], lists[1], gt[2], lists[2], gt[3], **kw)


def test_surface_refuses_cpu_tensors_mixed_dtypes_and_bad_shapes():
    from rroi_align.detection import DetectionLoss, detection_loss
    lists, gt = _cpu_arguments()
    with pytest.raises(RuntimeError, match="GPU only"):
        _call(detection_loss, lists, gt)
    with pytest.raises(RuntimeError, match="GPU only"):
        _call(DetectionLoss(), lists, gt)
    with pytest.raises(RuntimeError, match="GPU only"):
        _call(detection_loss, lists, gt, multi_scale=False)
    # dtypes: TypeError, before the device is looked at
    for k in range(3):
        for s in range(2):
            mixed = [list(v) for v in lists]
            mixed[k][s] = mixed[k][s].to(torch.bfloat16)
            with pytest.raises(TypeError):
                _call(detection_loss, mixed, gt)
    with pytest.raises(TypeError):
        _call(detection_loss, [[t.double() for t in v] for v in lists], gt)
    with pytest.raises(TypeError):
        _call(detection_loss, lists, _with(gt, 0, gt[0].to(torch.bfloat16)))
    with pytest.raises(TypeError):
        _call(detection_loss, lists, _with(gt, 3, gt[3].numpy()))
    # shapes: ValueError
    s4, a4, r4 = lists[0][0], lists[1][0], lists[2][0]
    bad = [
        ([[s4[:, 0], lists[0][1]], lists[1], lists[2]], gt),                       # (N, H, W) scores
        ([lists[0], [a4[:, :1], lists[1][1]], lists[2]], gt),                      # one angle channel
        ([lists[0], lists[1], [r4[:, :3], lists[2][1]]], gt),                      # three box channels
        ([lists[0], [a4[:1], lists[1][1]], lists[2]], gt),                         # another batch size
        ([lists[0], lists[1], [r4[..., :-1], lists[2][1]]], gt),                   # another width on 1/4
        ([lists[0], lists[1], [r4, lists[2][1][..., :-1]]], gt),                   # r8 against s8
        ([lists[0][:1], lists[1], lists[2]], gt),                                  # no 1/8 score with multi_scale
        (lists, _with(gt, 0, gt[0][:, :-1])),
        (lists, _with(gt, 3, gt[3][..., :3])),
        (lists, _with(gt, 2, gt[2].unsqueeze(1))),
    ]
    for args, g in bad:
        with pytest.raises(ValueError):
            _call(detection_loss, args, g)
    # a single scale does not look at the 1/8 entries: the bad r8 passes the checks and the device refuses
    with pytest.raises(RuntimeError, match="GPU only"):
        _call(detection_loss, [lists[0][:1], lists[1][:1], lists[2][:1]], gt, multi_scale=False)


def test_train_detection_loss_defaults_to_the_stock_path():
    from fots_e2e.train import detection_loss
    params = inspect.signature(detection_loss).parameters
    assert list(params) == ["segm_preds", "segm_gt", "iou_mask", "angle_preds", "angle_gt", "roi_preds", "roi_gt", "multi_scale",
                            "native", "return_terms"]
    assert params["multi_scale"].default is True and params["native"].default is False and params["return_terms"].default is False
    lists, gt = _cpu_arguments()
    total = _call(detection_loss, lists, gt)                                        # the stock path runs on the CPU
    terms = _call(detection_loss, lists, gt, return_terms=True)
    assert total.dim() == 0 and terms.shape == (4,) and terms.dtype == torch.float32 and torch.equal(terms[3], total)
    with pytest.raises(RuntimeError, match="GPU only"):                            # native=True reaches the native surface
        _call(detection_loss, lists, gt, native=True)
    from rroi_align.detection import detection_loss as native
    assert list(inspect.signature(native).parameters) == [p for p in params if p != "native"]


def _stock(case, dtype, preds=None):
    """The stock restatement on the CPU in `dtype`: the terms and the gradients of g . terms (None -> zeros)."""
    from fots_e2e.train import detection_loss
    preds = DC.materialise(case, torch.float32)[0] if preds is None else preds
    lists = [[p[k].detach().to(dtype, copy=True).requires_grad_(True) for p in preds] for k in range(3)]
    gt = [torch.from_numpy(v).to(dtype) for v in case["gt"]]
    terms = _call(detection_loss, lists, gt, multi_scale=case["multi"], return_terms=True)
    flat = [lists[k][s] for s in range(len(preds)) for k in range(3)]
    grads = torch.autograd.grad(terms, flat, torch.tensor(case["g"], dtype=terms.dtype), allow_unused=True)
    return terms.detach(), [torch.zeros_like(t) if g is None else g for g, t in zip(grads, flat)]


@pytest.mark.parametrize("name", DC.GOLDEN)
def test_stock_restatement_reproduces_the_reference_in_float32(name):
    """The stock restatement against the numbers the reference's own function gave for the same float32 inputs: both are
    float32 evaluations of the same expressions, so each lies within DC.f32_tol of the exact value -- (3 n + 16) 2^-24 of
    the magnitude, n the case's pixels on both scales -- and they differ by at most twice that."""
    case, gold = DC.CASE[name], np.load(GOLDEN)
    for s, p in enumerate(case["preds"]):                                           # the fixture holds the case's inputs
        for k, tag in enumerate(("segm", "angle", "roi")):
            assert np.array_equal(gold["%s.%s%d" % (name, tag, 4 << s)], p[k])
    for tag, v in zip(("segm_gt", "iou_mask", "angle_gt", "roi_gt"), case["gt"]):
        assert np.array_equal(gold["%s.%s" % (name, tag)], v)
    assert case["g"] == DC.G_TOTAL
    terms, grads = _stock(case, torch.float32)
    n = DC.items(case)
    want = [gold["%s.grad_%s%d" % (name, tag, 4 << s)].astype(np.float64) for s in range(len(case["preds"]))
            for tag in ("segm", "angle", "roi")]
    rt = DC.f32_terms_ratio(terms, gold[name + ".terms"].astype(np.float64), n) / 2
    rg = DC.f32_grads_ratio(grads, want, n) / 2
    print("%s: n = %d, terms ratio %.4f, gradient ratio %.4f" % (name, n, rt, rg))
    assert rt <= 1.0 and rg <= 1.0
    # and the reference's float32 numbers lie within the same tolerance of the float64 restatement
    ref = DC.materialise(case, torch.float32)[1]
    r64 = max(DC.f32_terms_ratio(gold[name + ".terms"], ref["terms"], n), DC.f32_grads_ratio(want, ref["grads"], n))
    print("%s: the reference against the float64 restatement, ratio %.4f" % (name, r64))
    assert r64 <= 1.0


@pytest.mark.parametrize("name", DC.NO_EMPTY_SELECTION)
def test_restatement_equals_the_stock_path_in_float64(name):
    case = DC.CASE[name]
    for dtype in (torch.float32, torch.bfloat16):          # the values the GPU tests feed: both roundings of the case
        preds, ref = DC.materialise(case, dtype)
        terms, grads = _stock(case, torch.float64, preds)
        assert np.isfinite(terms.numpy()).all()
        dt = np.abs(terms.numpy() - ref["terms"]).max()
        dg = max(np.abs(g.numpy() - r).max() for g, r in zip(grads, ref["grads"]))
        print("%s %s: terms %.3e gradients %.3e" % (name, dtype, dt, dg))
        assert dt <= 1e-12 and dg <= 1e-12
        assert len(grads) == len(ref["grads"]) and all(g.shape == r.shape for g, r in zip(grads, ref["grads"]))


def test_restatement_gives_zeros_where_the_stock_path_gives_nan():
    for name, nan_terms in (("no_left", True), ("no_right", True), ("empty", False)):
        case = DC.CASE[name]
        preds, ref = DC.materialise(case)
        terms, grads = _stock(case, torch.float64, preds)
        # the reference: NaN for an empty left or right selection; with no pixel above 0.5 its `if` skips both terms
        assert bool(torch.isnan(terms[2])) == nan_terms and bool(torch.isnan(terms[3])) == nan_terms, name
        assert np.isfinite(ref["terms"]).all() and all(np.isfinite(g).all() for g in ref["grads"]), name
        assert abs(float(terms[0]) - ref["terms"][0]) <= 1e-12 and abs(float(terms[1]) - ref["terms"][1]) <= 1e-12
    e = DC.materialise(DC.CASE["empty"])[1]
    assert e["terms"][1] == 0 and e["terms"][2] == 0 and e["terms"][0] < 0 and e["terms"][3] == e["terms"][0]
    assert not any(g.any() for g in e["grads"][1:3] + e["grads"][4:6]) and e["grads"][0].any() and e["grads"][3].any()
    for name, side in (("no_left", 2), ("no_right", 3)):
        r = DC.materialise(DC.CASE[name])[1]
        assert r["terms"][2] > 0                                                    # the other half still counts
        for g in (r["grads"][2], r["grads"][5]):
            assert not g[:, side].any() and g[:, 5 - side].any() and g[:, 0].any()
    # the tie case splits min's gradient: the restatement's shares hold a half
    c = DC.CASE["tie"]
    r4 = DC.materialise(c)[0][0][2].double().numpy()
    assert (r4 == np.moveaxis(c["gt"][3].astype(np.float64), -1, 1)).sum() > 10
    # the ulp helper: spacing at 1, below 1, and of the subnormals
    assert DC.ulp(1.0, torch.float32) == 2.0 ** -23 and DC.ulp(0.75, torch.bfloat16) == 2.0 ** -8
    assert DC.ulp(0.0, torch.float16) == 2.0 ** -24 and DC.ulp(1e-30, torch.float16) == 2.0 ** -24
