"""GPU (MI355X): native preprocessing against its float64 restatement rounded once -- 0 elements differ,
for every case of preprocess_cases.py in three dtypes, on two runs; a result written into a view one element into a larger
buffer (the element-store form) leaves its surroundings untouched; fp32 equals the stock `preprocess` bit for bit where
nothing is resized and is no farther from the float64 value than the stock chain where something is; the workload's own
720 x 1280 > 704 x 1280 and a shape whose threads own four rows; `infer_batch` / `infer_image` / `infer_stream` with
`native_preprocess=True` give the default path's results, also where the predicate declines."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import preprocess_cases as PC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def pp():
    from rroi_align._ext.rroi_align import preprocess
    return preprocess


@pytest.fixture(scope="module")
def refs():
    """case index -> (images, packed bytes and table on the device, float64 reference): computed once, never written."""
    out = {}
    for k, case in enumerate(PC.CASES):
        ims = PC.images_of(case, seed=100 + k)
        src, table = PC.pack(ims)
        out[k] = (ims, torch.from_numpy(src).to(DEV), torch.from_numpy(table).to(DEV), PC.ref_batch(ims, case[1]))
    return out


def differing(got, ref, dtype):
    want = PC.rounded(ref, dtype)
    assert got.shape == want.shape and got.dtype == dtype
    return int((PC.bits(got.cpu()) != PC.bits(want)).sum())


@pytest.mark.parametrize("dtype", PC.DTYPES, ids=("fp32", "bf16", "fp16"))
@pytest.mark.parametrize("k", range(len(PC.CASES)))
def test_no_element_differs_from_the_restatement_and_runs_repeat(pp, refs, k, dtype):
    ims, src, table, ref = refs[k]
    size = PC.CASES[k][1]
    got = pp.preprocess_images(src, table, size, dtype)
    again = pp.preprocess_images(src, table, size, dtype)
    assert tuple(got.shape) == (len(ims), 3) + tuple(size)
    assert differing(got, ref, dtype) == 0
    assert torch.equal(PC.bits(got), PC.bits(again))


@pytest.mark.parametrize("dtype", PC.DTYPES, ids=("fp32", "bf16", "fp16"))
@pytest.mark.parametrize("k", (0, 1, 6, 8))
def test_view_one_element_into_a_buffer_is_written_and_nothing_around_it(pp, refs, k, dtype):
    ims, src, table, ref = refs[k]
    size = PC.CASES[k][1]
    n = len(ims) * 3 * size[0] * size[1]
    big = torch.full((n + 64,), 77.0, dtype=dtype, device=DEV)
    out = big[1:1 + n].view(len(ims), 3, *size)
    assert out.data_ptr() % 16 != 0
    got = pp.preprocess_images(src, table, size, dtype, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert differing(got, ref, dtype) == 0
    assert float(big[0]) == 77.0 and bool((big[1 + n:] == 77.0).all())


def test_fp32_equals_the_stock_preprocess_bit_for_bit_where_nothing_is_resized(pp, refs):
    from fots_e2e.pipeline import preprocess, preprocess_batch
    for k in (0, 12):
        ims, src, table, _ = refs[k]
        assert PC.CASES[k][0] == (PC.CASES[k][1],)
        stock = preprocess(ims[0], DEV)
        assert torch.equal(PC.bits(pp.preprocess_images(src, table, PC.CASES[k][1], torch.float32)), PC.bits(stock))
        assert torch.equal(PC.bits(preprocess_batch(ims, DEV)), PC.bits(stock))


def stock_chain(im, size):
    """The stock front's operators (`fots_e2e.pipeline.preprocess`) with the target size given."""
    t = torch.as_tensor(im).to(device=DEV).to(torch.float32).permute(2, 0, 1).unsqueeze(0)
    t = F.interpolate(t, size=size, mode="bilinear", align_corners=False)
    return t / 128 - 1


@pytest.mark.parametrize("k", [i for i, c in enumerate(PC.CASES) if c in PC.RESIZING])
def test_native_is_no_farther_from_float64_than_the_stock_chain(pp, refs, k):
    ims, src, table, ref = refs[k]
    size = PC.CASES[k][1]
    native = pp.preprocess_images(src, table, size, torch.float32).cpu().numpy().astype(np.float64)
    stock = torch.cat([stock_chain(im, size) for im in ims]).cpu().numpy().astype(np.float64)
    err_native, err_stock = float(np.abs(native - ref).max()), float(np.abs(stock - ref).max())
    print("case %d %s -> %s: native %.3e stock %.3e" % (k, PC.CASES[k][0], size, err_native, err_stock))
    assert err_native <= 2.0 ** -24
    assert err_native <= err_stock


def test_the_workloads_size_in_bf16(pp):
    from fots_e2e.pipeline import preprocess_batch, preprocess_ok, resize_rule
    ims = [PC.image(720, 1280, "random", 40 + k) for k in range(2)]
    assert resize_rule(720, 1280) == (704, 1280) and preprocess_ok(ims, DEV, torch.bfloat16)
    assert pp.preprocess_plan(2, 704, 1280, torch.bfloat16).rows_per_thread == 2
    ref = PC.ref_batch(ims, (704, 1280))
    got = preprocess_batch(ims, DEV, torch.bfloat16)
    assert differing(got, ref, torch.bfloat16) == 0


def test_threads_that_own_four_rows(pp):
    size = (512, 1024)
    assert pp.preprocess_plan(2, *size, torch.float32).rows_per_thread == 4
    ims = [PC.image(40, 50, "random", 50), PC.image(41, 49, "checker", 0)]
    src, table = PC.pack(ims)
    got = pp.preprocess_images(torch.from_numpy(src).to(DEV), torch.from_numpy(table).to(DEV), size, torch.float32)
    assert differing(got, PC.ref_batch(ims, size), torch.float32) == 0


def test_preprocess_batch_of_different_sources(pp):
    from fots_e2e.pipeline import preprocess_batch, resize_rule
    ims = [PC.image(70, 101, "random", 60), PC.image(65, 127, "random", 61), PC.image(64, 96, "random", 62)]
    assert {resize_rule(*im.shape[:2]) for im in ims} == {(64, 96)}
    ref = PC.ref_batch(ims, (64, 96))
    for dtype in PC.DTYPES:
        assert differing(preprocess_batch(ims, DEV, dtype), ref, dtype) == 0
    assert differing(preprocess_batch([np.asfortranarray(ims[0])], DEV), ref[:1], torch.float32) == 0   # made contiguous
    # the same sizes again with other bytes (the kept table), then in another order (another table)
    other = [PC.image(*im.shape[:2], "random", 63 + k) for k, im in enumerate(ims)]
    assert differing(preprocess_batch(other, DEV), PC.ref_batch(other, (64, 96)), torch.float32) == 0
    assert differing(preprocess_batch(other[::-1], DEV), PC.ref_batch(other[::-1], (64, 96)), torch.float32) == 0


# ---------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def setup():
    from fots_e2e.alphabet import ALPHABET
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    from rroi_align.decode import CTCLabelConverter
    net = deterministic_init(FOTSNet(len(ALPHABET) + 1)).eval().to(DEV)
    return net, CTCLabelConverter(ALPHABET)


def _hook(size, nwords, seed, batch):
    from e2e_inputs import synthetic_detector_maps
    per = [synthetic_detector_maps(size[0], size[1], nwords, seed=seed + k) for k in range(batch)]
    maps = tuple(torch.from_numpy(np.stack([p[j] for p in per])).to(DEV) for j in range(3))
    return lambda im_data: maps


def _assert_same_results(a, b):
    """Two runs of `infer_batch(return_debug=True)` on the same input bits: the same boxes always (the detector's maps are
    injected); the same crops bit for bit and the same texts where the two passes through the backbone gave the same
    feature bits (the stock backbone picks its kernels per call and need not repeat itself: tests/test_gpu_bucketed_e2e.py)."""
    (res_a, (per_a, dbg_a, feats_a)), (res_b, (per_b, dbg_b, feats_b)) = a, b
    assert len(per_a) == len(per_b) and all(np.array_equal(x, y) for x, y in zip(per_a, per_b))
    assert len(dbg_a[1]) == len(dbg_b[1]) and all(x.shape == y.shape for x, y in zip(dbg_a[1], dbg_b[1]))
    same_feats = all(torch.equal(x, y) for x, y in zip(feats_a, feats_b))
    if same_feats:
        assert all(torch.equal(PC.bits(x), PC.bits(y)) for x, y in zip(dbg_a[1], dbg_b[1]))
        assert dbg_a[0] == dbg_b[0]
        for (ba, ta), (bb, tb) in zip(res_a, res_b):
            assert np.array_equal(ba, bb) and ta == tb
    return same_feats


def test_infer_batch_native_preprocess_equals_the_default(setup):
    from fots_e2e.pipeline import _front_input, infer_batch, infer_image, preprocess_ok
    net, conv = setup
    size = (256, 384)
    ims = [PC.image(size[0], size[1], "random", 70 + k) for k in range(3)]
    hook = _hook(size, 6, 11, 3)
    assert preprocess_ok(ims, DEV)
    with torch.no_grad():
        # the network's input is the same bits
        assert torch.equal(PC.bits(_front_input(ims, DEV, torch.float32, True)), PC.bits(_front_input(ims, DEV, torch.float32, False)))
        want = infer_batch(net, conv, ims, detector=hook, return_debug=True)
        got = infer_batch(net, conv, ims, detector=hook, return_debug=True, native_preprocess=True)
        again = infer_batch(net, conv, ims, detector=hook, return_debug=True)
        assert sum(len(b) for b in want[1][0]) >= 6
        # where the default path repeats itself, the native front must give exactly its results
        repeats = _assert_same_results(want, again)
        assert _assert_same_results(want, got) or not repeats
        h1 = lambda im_data: tuple(m[0] for m in hook(im_data))
        ba, ta = infer_image(net, conv, ims[0], detector=h1)
        bb, tb = infer_image(net, conv, ims[0], detector=h1, native_preprocess=True)
        assert ba.shape == bb.shape and len(ta) == len(tb)
        if repeats:
            assert np.array_equal(ba, bb) and ta == tb


def test_keyword_on_and_a_declined_input_runs_the_stock_path(setup, monkeypatch):
    import fots_e2e.pipeline as pl
    net, conv = setup
    size = (256, 384)
    ims = [PC.image(size[0], 2 * size[1], "random", 80 + k)[:, ::2] for k in range(2)]      # non-contiguous: declined
    hook = _hook(size, 6, 13, 2)
    assert not pl.preprocess_ok(ims, DEV)
    called = []
    monkeypatch.setattr(pl, "preprocess_batch", lambda *a, **k: called.append(1))
    with torch.no_grad():
        assert torch.equal(pl._front_input(ims, DEV, torch.float32, True), pl._front_input(ims, DEV, torch.float32, False))
        want = pl.infer_batch(net, conv, ims, detector=hook, return_debug=True)
        got = pl.infer_batch(net, conv, ims, detector=hook, return_debug=True, native_preprocess=True)
        again = pl.infer_batch(net, conv, ims, detector=hook, return_debug=True)
        repeats = _assert_same_results(want, again)
        assert _assert_same_results(want, got) or not repeats
    assert not called


def test_infer_stream_native_preprocess(setup):
    from fots_e2e.pipeline import infer_batch, infer_stream
    net, conv = setup
    size = (256, 384)
    batches = [[PC.image(size[0], size[1], "random", 90 + 2 * k + j) for j in range(2)] for k in range(3)]
    hooks = [_hook(size, 6, 20 + k, 2) for k in range(3)]
    with torch.no_grad():
        got = list(infer_stream(net, conv, batches, detector=lambda k, x: hooks[k](x), native_preprocess=True))
        want = [infer_batch(net, conv, b, detector=hooks[k]) for k, b in enumerate(batches)]
    assert len(got) == 3
    for g, w in zip(got, want):
        assert len(g) == len(w) == 2
        for (bg, tg), (bw, tw) in zip(g, w):
            assert len(bg) == len(tg) and bg.shape[1:] == bw.shape[1:]
    assert sum(len(t) for g in got for _, t in g) > 0
