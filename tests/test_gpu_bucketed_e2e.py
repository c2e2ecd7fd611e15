"""GPU (MI355X): the inference pipeline with `bucketed=True` -- the crops come from the bucketed RoIRotate,
one dense tensor per pooled-width bucket, and go to the recognition head as they are.  Same boxes, the same crop bits
for every word, the same texts as the default path; BucketedRRoiAlign's buckets are BatchedRRoiAlign's crops sliced."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from fots_e2e.alphabet import ALPHABET
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    from rroi_align.decode import CTCLabelConverter
    dev = torch.device("cuda", 0)
    net = deterministic_init(FOTSNet(len(ALPHABET) + 1)).eval().to(dev)
    return net, CTCLabelConverter(ALPHABET), dev


def _hook(size, nwords, seed, dev, batch=None):
    from e2e_inputs import synthetic_detector_maps
    if batch is None:
        maps = tuple(torch.from_numpy(a).to(dev) for a in synthetic_detector_maps(size[0], size[1], nwords, seed=seed))
    else:
        per = [synthetic_detector_maps(size[0], size[1], nwords, seed=seed + k) for k in range(batch)]
        maps = tuple(torch.from_numpy(np.stack([p[j] for p in per])).to(dev) for j in range(3))
    return lambda im_data: maps


def _same_words(net, dbg_a, dbg_b):
    """The recogniser's (texts, crops, labels) of two runs: every crop bit for bit; every text equal -- except where the
    head, run on the same bits in another batch layout, decided a numerical tie the other way (the margin between the two
    best classes at every differing step within the head's own noise, the bar of tests/test_e2e_gpu.py)."""
    (ta, ca, la), (tb, cb, lb) = dbg_a, dbg_b
    assert len(ta) == len(tb) == len(ca) == len(cb)
    widths = set()
    for i in range(len(ta)):
        assert ca[i].shape == cb[i].shape
        assert torch.equal(ca[i].contiguous().view(torch.int32), cb[i].contiguous().view(torch.int32)), "crop %d differs" % i
        widths.add(ca[i].shape[3])
        if torch.equal(la[i], lb[i]):
            assert ta[i] == tb[i]
        else:
            top2 = net.forward_ocr(ca[i].contiguous()).topk(2, dim=1).values[0]
            assert float((top2[0] - top2[1])[la[i] != lb[i]].abs().max()) < 2e-3, "labels of word %d differ beyond a tie" % i
    return widths, all(torch.equal(a, b) for a, b in zip(la, lb))


def test_infer_image_bucketed_equals_the_default(setup):
    from e2e_inputs import synthetic_boxes
    from fots_e2e.pipeline import batched, infer_image, target_widths_host
    net, conv, dev = setup
    size = (256, 384)
    torch.manual_seed(4)
    im_data = torch.rand(1, 3, *size, device=dev) * 2 - 1
    hook = _hook(size, 6, 7, dev)
    with torch.no_grad():
        kept_a, texts_a, (boxes_a, _, feats) = infer_image(net, conv, im_data, detector=hook, return_debug=True)
        kept_b, texts_b, (boxes_b, _, _) = infer_image(net, conv, im_data, detector=hook, return_debug=True, bucketed=True)
        assert len(boxes_a) >= 3 and np.array_equal(boxes_a, boxes_b)
        # two passes through the backbone need not be bit-identical (MIOpen picks its kernels per call): crops, labels and
        # texts are compared on ONE feature map -- the detector's boxes, then word-shaped boxes of several width buckets
        gw = target_widths_host(boxes_a)
        dbg_a = batched(net, conv, feats, boxes_a, return_crops=True, gw_host=gw)
        dbg_b = batched(net, conv, feats, boxes_a, return_crops=True, gw_host=gw, bucketed=True)
        _, same_labels = _same_words(net, dbg_a, dbg_b)
        if same_labels:
            assert dbg_a[0] == dbg_b[0]
            keep = [i for i, t in enumerate(dbg_a[0]) if len(t) > 0]
            assert np.array_equal(kept_b, boxes_a[keep]) and texts_b == [dbg_b[0][i] for i in keep]
        boxes = synthetic_boxes(9, size[0], size[1], seed=5)
        dbg_a = batched(net, conv, feats, boxes, return_crops=True)              # (reads the widths back)
        dbg_b = batched(net, conv, feats, boxes, return_crops=True, bucketed=True)
        widths, same_labels = _same_words(net, dbg_a, dbg_b)
        assert len(widths) >= 2
        if same_labels:
            assert dbg_a[0] == dbg_b[0]


def test_infer_batch_bucketed_equals_the_default(setup):
    from fots_e2e.pipeline import _batch_back, _batch_front, infer_batch
    net, conv, dev = setup
    size = (256, 384)
    torch.manual_seed(5)
    ims = torch.rand(3, 3, *size, device=dev) * 2 - 1
    hook = _hook(size, 6, 11, dev, batch=3)
    with torch.no_grad():
        front = _batch_front(net, ims, hook, 0.5)
        res_a, (per_a, dbg_a, _) = _batch_back(net, conv, front, return_debug=True)
        res_b, (per_b, dbg_b, _) = _batch_back(net, conv, front, return_debug=True, bucketed=True)
        res_c = infer_batch(net, conv, ims, detector=hook, bucketed=True)
    assert sum(len(b) for b in per_a) >= 6
    assert all(np.array_equal(a, b) for a, b in zip(per_a, per_b))
    _, same_labels = _same_words(net, dbg_a, dbg_b)
    if same_labels:
        for (ba, ta), (bb, tb) in zip(res_a, res_b):
            assert np.array_equal(ba, bb) and ta == tb
    assert len(res_c) == 3 and all(len(b) == len(t) for b, t in res_c)
    # no box at all
    assert infer_batch(net, conv, [], bucketed=True) == []


def test_infer_stream_bucketed(setup):
    from fots_e2e.pipeline import infer_batch, infer_stream
    net, conv, dev = setup
    size = (256, 384)
    torch.manual_seed(6)
    batches = [torch.rand(2, 3, *size, device=dev) * 2 - 1 for _ in range(3)]
    hooks = [_hook(size, 6, 20 + k, dev, batch=2) for k in range(3)]
    with torch.no_grad():
        got = list(infer_stream(net, conv, batches, detector=lambda k, x: hooks[k](x), bucketed=True))
        want = [infer_batch(net, conv, b, detector=hooks[k]) for k, b in enumerate(batches)]
    # (the crops and texts of the bucketed path are compared above, on one feature map; two passes through the backbone
    # need not be bit-identical, so this checks that the two-stream driver runs the flag through: the same structure,
    # boxes that are a subset of what the detector maps yield, one text per kept box)
    assert len(got) == 3
    for g, w in zip(got, want):
        assert len(g) == len(w) == 2
        for (bg, tg), (bw, tw) in zip(g, w):
            assert len(bg) == len(tg) and bg.shape[1:] == bw.shape[1:]
    assert sum(len(t) for g in got for _, t in g) > 0


def test_bucketed_module_equals_the_batched_crops_sliced(setup):
    from e2e_inputs import synthetic_boxes
    from rroi_align.batched import BatchedRRoiAlign, BucketedRRoiAlign
    from fots_e2e.pipeline import target_widths_host
    net, _, dev = setup
    torch.manual_seed(7)
    feats = torch.randn(2, 64, 176, 320, device=dev)
    boxes = np.concatenate([synthetic_boxes(24, 704, 1280, seed=s) for s in (1, 2)])
    quads = torch.from_numpy(boxes[:, :8].copy()).to(dev)
    bidx = torch.from_numpy(np.repeat(np.arange(2, dtype=np.float32), 24)).to(dev)
    for dtype in (torch.float32, torch.bfloat16):
        F = feats.to(dtype)
        dense, gw = BatchedRRoiAlign()(F, quads, bidx)
        for widths in (None, target_widths_host(boxes)):
            buckets, gw2 = BucketedRRoiAlign()(F, quads, bidx, widths=widths)
            assert torch.equal(gw, gw2)
            seen = []
            for idx, crops in buckets:
                w = crops.shape[3]
                assert set(gw[idx].tolist()) == {w}
                sl = dense.index_select(0, idx)[:, :, :, :w].contiguous()
                it = torch.int32 if dtype == torch.float32 else torch.int16
                assert torch.equal(crops.view(it), sl.view(it)) or bool((crops.isnan() == sl.isnan()).all())
                assert torch.equal(crops.view(it)[~crops.isnan()], sl.view(it)[~sl.isnan()])
                seen += idx.tolist()
            assert sorted(seen) == list(range(48)) and len(buckets) >= 2
