"""The inference pipeline end to end in bfloat16 / float16 on the GPU: the callers' kernels on 16-bit data against the
fp32 entry points on the widened data (byte for byte) and against the CPU oracles, and the pipeline around them.

The contract: a 16-bit element is widened exactly where it is loaded and everything after the load is the
fp32 kernel's arithmetic, so nothing here needs a tolerance.  The pipeline checks record what the pipeline itself
computed (the head's log-probabilities, the feature maps) and never compare two passes through MIOpen with each other."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HALF = (torch.bfloat16, torch.float16)
ids = lambda d: str(d).replace("torch.", "")   # noqa: E731


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as E
    return E


# ---------------------------------------------------------------------------------------------------- RBOX decode
def _raw_decode(ext, maps, thr, cap):
    """One call of the entry point that belongs to the maps' dtype with a buffer of exactly `cap` records (+ one guard
    record that must stay untouched) -> (count, records (cap, 64) uint8 on the host)."""
    s, r, a = (m.contiguous() for m in maps)
    h, w = s.shape
    rec = torch.full((cap + 1, 64), 0xCD, dtype=torch.uint8, device=s.device)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=s.device)
    tail = (s.data_ptr(), r.data_ptr(), a.data_ptr(), h, w, float(thr), rec.data_ptr(), cap, cnt.data_ptr(), ext._stream())
    if s.dtype == torch.float32:
        st = ext._lib.rroi_rbox_decode_hip(*tail)
    else:
        st = ext._lib.rroi_rbox_decode_typed_hip(ext._DTYPES[s.dtype], *tail)
    assert st == 1
    torch.cuda.synchronize()
    host = rec.cpu()
    assert bool((host[cap] == 0xCD).all()), "a record was written beyond the capacity"
    return int(cnt.item()), host[:cap]


def _full_capacity(h, w):
    slabs = (h * w + 1023) // 1024
    return h * w + ((slabs * 4 + 63) // 64 if slabs > 256 else 0)


def _widen(maps):
    return tuple(m.float() for m in maps)


def _check_against_fp32(ext, maps16, thr=0.5, caps=None):
    """Typed decode of 16-bit maps == the fp32 entry point on the widened maps: count and records, per capacity."""
    h, w = maps16[0].shape
    n_first = None
    for cap in caps or (_full_capacity(h, w),):
        n16, rec16 = _raw_decode(ext, maps16, thr, cap)
        n32, rec32 = _raw_decode(ext, _widen(maps16), thr, cap)
        assert n16 == n32
        assert n_first in (None, n16), "the count must not depend on the capacity"
        n_first = n16
        k = min(n16, cap, h * w)
        assert torch.equal(rec16[:k], rec32[:k]), "records differ (capacity %d)" % cap
    return n_first


def _check_against_oracle(maps16, thr=0.5):
    """`rroi_align.nms.decode` of 16-bit maps against oracle/nms_oracle.decode on the widened maps, field by field."""
    from oracle import nms_oracle as NO
    from rroi_align.nms import CANDIDATE, decode
    rec, cnt = decode(*maps16, thr)
    n = int(cnt.item())
    got = rec[:n].cpu().numpy().view(CANDIDATE).reshape(-1)
    s, r, a = (m.float().cpu().numpy() for m in maps16)
    want = NO.decode(s, r.transpose(1, 2, 0), a.transpose(1, 2, 0), thr)
    assert n == len(want)
    for g, p in zip(got, want):
        assert g["quad"].tolist() == np.asarray(p["poly"], np.int64).reshape(8).tolist()
        assert g["score"] == p["score"] and g["rdist"].tolist() == [float(v) for v in p["rdist"]]
        assert (int(g["x"]), int(g["y"])) == (p["x"], p["y"]) and int(g["pad"]) == 0
    return n


def _random_maps(h, w, seed, dev, dtype, lead=()):
    """About half of the pixels pass 0.5; distances and directions of a plausible size."""
    g = torch.Generator().manual_seed(seed)
    s = torch.rand(*lead, h, w, generator=g)
    r = torch.rand(*lead, 4, h, w, generator=g) * 40
    ang = torch.rand(*lead, h, w, generator=g) - 0.5
    a = torch.stack([torch.sin(ang), torch.cos(ang)], dim=len(lead))
    return tuple(t.to(dev).to(dtype) for t in (s, r, a))


@pytest.mark.parametrize("dtype", HALF, ids=ids)
@pytest.mark.parametrize("size,nwords", [((256, 384), 6), ((704, 1280), 24)])
def test_decode_of_synthetic_detector_maps(ext, dev, dtype, size, nwords):
    from e2e_inputs import synthetic_detector_maps
    from rroi_align.nms import get_boxes
    maps = tuple(torch.from_numpy(a).to(dev).to(dtype) for a in synthetic_detector_maps(size[0], size[1], nwords, seed=1))
    n = _check_against_fp32(ext, maps)
    assert n > 0
    if size == (256, 384):
        assert _check_against_oracle(maps) == n
    boxes = get_boxes(*maps)
    assert len(boxes) >= nwords // 2, "the synthetic detector maps must yield boxes"
    assert np.array_equal(boxes, get_boxes(*_widen(maps)))


@pytest.mark.parametrize("dtype", HALF, ids=ids)
def test_decode_of_a_random_map_and_of_unaligned_batch_images(ext, dev, dtype):
    """45 x 67 = 3015 pixels, an odd number: images 1 and 2 of a batch start on 2-byte boundaries."""
    from rroi_align.nms import decode, decode_batch, get_boxes, get_boxes_batch
    maps = _random_maps(45, 67, 3, dev, dtype)
    n = _check_against_fp32(ext, maps)
    assert 0.35 * 3015 < n < 0.65 * 3015
    assert _check_against_oracle(maps) == n
    batch = _random_maps(45, 67, 4, dev, dtype, lead=(3,))
    assert batch[0][1].data_ptr() % 4 == 2, "image 1 must start on a 2-byte boundary for this case to mean anything"
    pending, hw = decode_batch(*batch)
    assert hw == (45, 67) and len(pending) == 3
    per_image = get_boxes_batch(*batch)
    for i in range(3):
        one = tuple(m[i] for m in batch)
        rec, cnt = pending[i]
        rec32, cnt32 = decode(*_widen(one))
        k = int(cnt.item())
        assert k == int(cnt32.item()) and 0.35 * 3015 < k < 0.65 * 3015
        assert torch.equal(rec[:k], rec32[:k])
        assert _check_against_oracle(one) == k
        assert np.array_equal(per_image[i], get_boxes(*_widen(one)))
        assert np.array_equal(get_boxes(*one), per_image[i])
    # a larger odd map: the workgroups past the first 8192 pixels count with the 16-byte loads on image 0 and take the
    # scalar loop on image 1, whose base is not 16-byte aligned
    big = _random_maps(125, 163, 5, dev, dtype, lead=(2,))
    assert big[0][1].data_ptr() % 16 != 0
    for i in range(2):
        one = tuple(m[i] for m in big)
        k = _check_against_fp32(ext, one, caps=(125 * 163, 300))
        rec, cnt = decode(*one)
        rec32, _ = decode(*_widen(one))
        assert int(cnt.item()) == k and torch.equal(rec[:k], rec32[:k])


@pytest.mark.parametrize("dtype", HALF, ids=ids)
def test_decode_beyond_262144_pixels_in_both_launch_forms(ext, dev, dtype):
    """520 x 520 = 270,400 pixels: count + decode launches with the full capacity, the one-launch form with exactly
    h * w records and with a buffer that overflows (`count` still reports the total)."""
    h = w = 520
    maps = _random_maps(h, w, 6, dev, dtype)
    full = _full_capacity(h, w)
    assert full > h * w
    n = _check_against_fp32(ext, maps, caps=(full, h * w, 1000))
    assert 0.4 * h * w < n < 0.6 * h * w and n > 1000
    from rroi_align.nms import decode
    rec, cnt = decode(*maps)
    rec32, _ = decode(*_widen(maps))
    assert int(cnt.item()) == n and torch.equal(rec[:n], rec32[:n])


@pytest.mark.parametrize("dtype", HALF, ids=ids)
def test_decode_of_more_than_1024_slabs_in_both_launch_forms(ext, dev, dtype):
    """1030 x 1024 pixels = 1030 slabs (the map of test_nms.py's ordered-decode case, rounded to 16 bits): in the
    two-launch form the workgroups of slabs 1025 .. 1029 sum the counts of the slabs before theirs in two trips.  The
    full capacity takes that form, h * w and 1000 records the one-launch form; the count is the same in all three."""
    from test_nms import many_workgroup_maps, passing_on_both_sides_of_slab_1024
    h, w = 1030, 1024
    _, segm, geo, ang = many_workgroup_maps(h, w)
    maps = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype) for a in (segm, geo.transpose(2, 0, 1), ang))
    mask = (maps[0].float() > 0.5).cpu().numpy()
    assert passing_on_both_sides_of_slab_1024(mask)
    full = _full_capacity(h, w)
    assert full > h * w
    n = _check_against_fp32(ext, maps, caps=(full, h * w, 1000))
    assert n == int(mask.sum()) and 0.03 * h * w < n < 0.05 * h * w


@pytest.mark.parametrize("dtype", HALF, ids=ids)
def test_decode_special_scores_and_tiny_maps(ext, dev, dtype):
    """NaN and a score exactly equal to the threshold do not pass, +inf does, -inf does not: decided on the widened value."""
    from rroi_align.nms import CANDIDATE, decode
    s, r, a = _random_maps(45, 67, 8, dev, dtype)
    s = s.clone()
    special = [float("nan"), float("inf"), float("-inf"), 0.5, 0.75, 0.25]
    flat = s.view(-1)
    for k, v in enumerate(special):
        flat[100 * k + 7] = v
    assert float(flat[307].float()) == 0.5      # 0.5 is exact in both 16-bit types
    n = _check_against_fp32(ext, (s, r, a))
    assert _check_against_oracle((s, r, a)) == n
    rec, cnt = decode(s, r, a, 0.5)
    got = rec[:int(cnt.item())].cpu().numpy().view(CANDIDATE).reshape(-1)
    passed = set((got["y"] * 67 + got["x"]).tolist())
    assert [(100 * k + 7) in passed for k in range(6)] == [False, True, False, False, True, False]
    for hh, ww in ((1, 1), (1, 1025), (25, 41)):   # h * w of 1, of 1025 (one pixel in the second slab), of 1025 again
        m = _random_maps(hh, ww, 9 + ww, dev, dtype)
        m[0].view(-1)[-1] = 0.875              # the last pixel passes
        k = _check_against_fp32(ext, m, caps=(hh * ww, max(1, hh * ww // 3), 0))
        assert k >= 1 and _check_against_oracle(m) == k


def test_decode_refuses_mixed_and_unknown_dtypes_before_any_launch(dev):
    from rroi_align.nms import decode, decode_batch, get_boxes
    s, r, a = _random_maps(16, 24, 1, dev, torch.float32)
    for bad in ((s.bfloat16(), r, a), (s, r.half(), a), (s.half(), r.half(), a.bfloat16()), (s.bfloat16(), r.bfloat16(), a)):
        with pytest.raises(TypeError, match="score, rbox and angle"):
            decode(*bad)
        with pytest.raises(TypeError):
            get_boxes(*bad)
        with pytest.raises(TypeError):
            decode_batch(*(m[None] for m in bad))
    with pytest.raises(TypeError):
        decode(s.double(), r.double(), a.double())
    with pytest.raises(TypeError):
        decode(s, r, a.double())


# ---------------------------------------------------------------------------------------------------- greedy CTC
VALUES = torch.tensor([-3.0, -1.5, -0.75, 0.0, 0.25, 1.0, 2.5, 6.0])   # exact in bfloat16 and float16


def _tied_logits(n, k, t, seed, dev, dtype):
    g = torch.Generator().manual_seed(seed)
    x = VALUES[torch.randint(0, 8, (n, k, t), generator=g)]
    return x.to(dev).to(dtype)


def _check_ctc(logits, lengths):
    from oracle import ctc_decode_oracle as CO
    from rroi_align.decode import ctc_greedy_decode
    dec, dlen, lab = ctc_greedy_decode(logits, lengths, return_labels=True)
    dec32, dlen32, lab32 = ctc_greedy_decode(logits.float(), lengths, return_labels=True)
    assert torch.equal(lab, lab32) and torch.equal(dec, dec32) and torch.equal(dlen, dlen32)
    want_lab = CO.argmax_labels(logits.float().cpu().numpy())
    want_dec, want_len = CO.collapse(want_lab, None if lengths is None else np.asarray(lengths))
    assert np.array_equal(lab.cpu().numpy(), want_lab)
    assert np.array_equal(dec.cpu().numpy(), want_dec) and np.array_equal(dlen.cpu().numpy(), want_len)
    d2, l2 = ctc_greedy_decode(logits, lengths)          # without the labels
    assert torch.equal(d2, dec) and torch.equal(l2, dlen)


@pytest.mark.parametrize("dtype", HALF, ids=ids)
@pytest.mark.parametrize("K", [1, 2, 87])
def test_ctc_of_tied_logits(dev, dtype, K):
    for T in (1, 63, 64, 65, 129, 200):
        N = 5
        x = _tied_logits(N, K, T, 100 * K + T, dev, dtype)
        if K == 87:
            # the case shows nothing unless the arg-max tie rule decides most steps
            xf = x.float()
            tied = (xf == xf.max(dim=1, keepdim=True).values).sum(dim=1) > 1
            assert float(tied.float().mean()) > 0.5
        _check_ctc(x, None)
        _check_ctc(x, [T, 0, T // 2, T + 5, -3])


@pytest.mark.parametrize("dtype", HALF, ids=ids)
def test_ctc_special_values_and_shapes(dev, dtype):
    from rroi_align.decode import CTCLabelConverter, ctc_greedy_decode
    N, K, T = 4, 87, 65          # odd T: rows start on 2-byte boundaries
    x = _tied_logits(N, K, T, 7, dev, dtype)
    x[0, 5, 3] = float("nan")                   # NaN counts as largest ...
    x[0, 9, 3] = float("inf")                   # ... also beside +inf, whichever comes first
    x[0, 2, 4] = float("inf")
    x[0, 7, 4] = float("nan")                   # (here the NaN comes second and still wins)
    x[1, :, 10] = float("-inf")                 # all -inf: the first class
    x[1, :, 11] = float("nan")                  # all NaN: the first class
    x[2, 40, :] = float("inf")                  # a whole row of one label: collapses to one
    x[3, 0, ::2] = float("inf")                 # blanks between repeated labels
    x[3, 86, 1::2] = float("inf")
    _check_ctc(x, None)
    _check_ctc(x, [65, 12, 1, 64])
    lab = ctc_greedy_decode(x, None, return_labels=True)[2].cpu()
    assert lab[0, 3] == 5 and lab[0, 4] == 7 and lab[1, 10] == 0 and lab[1, 11] == 0
    assert int(ctc_greedy_decode(x)[1][2]) == 1 and int(ctc_greedy_decode(x)[1][3]) == 32
    # a non-contiguous view, N = 0, T = 0
    y = _tied_logits(3, 129, 87, 8, dev, dtype).transpose(1, 2)
    assert not y.is_contiguous()
    _check_ctc(y, None)
    d, n = ctc_greedy_decode(torch.empty(0, K, T, device=dev, dtype=dtype))
    assert d.shape == (0, T) and n.shape == (0,)
    d, n = ctc_greedy_decode(torch.empty(3, K, 0, device=dev, dtype=dtype))
    assert d.shape == (3, 0) and n.cpu().tolist() == [0, 0, 0]
    conv = CTCLabelConverter("abcdefghijklmnopqrstuvwxyz")
    z = _tied_logits(6, 27, 40, 9, dev, dtype)
    assert conv.decode_logits(z) == conv.decode_logits(z.float())
    with pytest.raises(TypeError):
        ctc_greedy_decode(z.double())


# ---------------------------------------------------------------------------------------------------- the pipeline
class _Recorder(object):
    """Keeps every log-probability tensor `net.forward_ocr` returns (wrapped on the instance)."""

    def __init__(self, net):
        self.net, self.logs = net, []
        orig = net.forward_ocr

        def wrapped(x):
            out = orig(x)
            self.logs.append(out)
            return out
        net.forward_ocr = wrapped

    def close(self):
        del self.net.forward_ocr


def _make_net(dev, dtype, channels_last=False):
    from fots_e2e.alphabet import ALPHABET
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet(len(ALPHABET) + 1)).eval().to(dev).to(dtype)
    return net.to(memory_format=torch.channels_last) if channels_last else net


@pytest.fixture(scope="module")
def conv():
    from fots_e2e.alphabet import ALPHABET
    from rroi_align.decode import CTCLabelConverter
    return CTCLabelConverter(ALPHABET)


def _maps(size, nwords, seed, dev, dtype):
    from e2e_inputs import synthetic_detector_maps
    return tuple(torch.from_numpy(a).to(dev).to(dtype) for a in synthetic_detector_maps(size[0], size[1], nwords, seed=seed))


def _image(size, seed):
    return np.random.default_rng(seed).integers(0, 256, (size[0], size[1], 3), dtype=np.uint8)


def _expected_from_records(conv, logs, boxes):
    """What the fp32 CTC entry point and the converter make of the RECORDED log-probabilities, widened: one tensor per
    pooled-width bucket, in ascending width (the order `batched` runs the head in) -> (labels, texts) per box."""
    from fots_e2e.pipeline import target_widths_host
    from rroi_align.decode import ctc_greedy_decode
    gw = target_widths_host(boxes) if len(boxes) else []
    widths = sorted(set(gw))
    assert len(logs) == len(widths)
    labels, texts = [None] * len(gw), [None] * len(gw)
    for wdt, logp in zip(widths, logs):
        idx = [i for i, v in enumerate(gw) if v == wdt]
        assert logp.shape[0] == len(idx)
        dec, dlen, lab = ctc_greedy_decode(logp.float(), None, return_labels=True)
        words = conv.to_texts(dec, dlen)
        for j, i in enumerate(idx):
            labels[i], texts[i] = lab[j].to(torch.int64), words[j]
    return labels, texts


def _check_crops(focr, boxes, crops, dtype, batch_index=None):
    from fots_e2e.pipeline import target_widths_host
    from rroi_align.batched import rois_from_quads
    from rroi_align.modules.rroi_align import _RRoiAlign
    gw = target_widths_host(boxes)
    quads = torch.from_numpy(np.ascontiguousarray(boxes[:, :8])).to(focr.device)
    bidx = None if batch_index is None else torch.as_tensor(batch_index, dtype=torch.float32, device=focr.device)
    rois, _ = rois_from_quads(quads, bidx, False, 11)
    op = _RRoiAlign(11, max(gw), 1.0 / 4)
    ref = op(focr, rois)
    ref32 = op(focr.float(), rois).to(dtype)
    assert ref.dtype == dtype and focr.dtype == dtype
    for i, c in enumerate(crops):
        assert c.dtype == dtype and c.shape == (1, focr.shape[1], 11, gw[i])
        assert torch.equal(c, ref[i:i + 1, :, :, :gw[i]]), "crop %d differs from the op's own" % i
        assert torch.equal(c, ref32[i:i + 1, :, :, :gw[i]]), "crop %d differs from the rounded fp32 crop" % i


def _check_image_chain(net, conv, dev, dtype, size, nwords, map_dtype=None):
    from fots_e2e.pipeline import infer_image
    from rroi_align.nms import get_boxes
    maps = _maps(size, nwords, 7, dev, map_dtype or dtype)
    rec = _Recorder(net)
    try:
        with torch.no_grad():
            kept, texts, (boxes, (all_t, crops, labels), feats) = infer_image(net, conv, _image(size, 3), detector=lambda _x: maps,
                                                                             return_debug=True)
            logs = list(rec.logs)
    finally:
        rec.close()
    assert len(boxes) >= nwords // 2, "the synthetic detector maps must yield boxes"
    assert np.array_equal(boxes, get_boxes(*maps)) and np.array_equal(boxes, get_boxes(*_widen(maps)))
    assert all(f.dtype == dtype for f in feats) and all(l.dtype == dtype for l in logs)
    with torch.no_grad():
        _check_crops(feats[1], boxes, crops, dtype)
    want_lab, want_txt = _expected_from_records(conv, logs, boxes)
    assert len(all_t) == len(boxes) == len(labels)
    for i in range(len(boxes)):
        assert torch.equal(labels[i], want_lab[i]), "labels of word %d" % i
    assert all_t == want_txt
    keep = [i for i, t in enumerate(want_txt) if len(t) > 0]
    assert texts == [want_txt[i] for i in keep] and np.array_equal(kept, boxes[keep])


@pytest.mark.parametrize("dtype", HALF, ids=ids)
@pytest.mark.parametrize("size,nwords", [((256, 384), 6), ((704, 1280), 24)])
def test_infer_image_in_16_bits(dev, conv, dtype, size, nwords):
    _check_image_chain(_make_net(dev, dtype), conv, dev, dtype, size, nwords)


def test_infer_image_channels_last_bfloat16(dev, conv):
    _check_image_chain(_make_net(dev, torch.bfloat16, channels_last=True), conv, dev, torch.bfloat16, (256, 384), 6)


def test_detector_maps_may_have_another_dtype_than_the_network(dev, conv):
    _check_image_chain(_make_net(dev, torch.bfloat16), conv, dev, torch.bfloat16, (256, 384), 6, map_dtype=torch.float32)
    _check_image_chain(_make_net(dev, torch.float32), conv, dev, torch.float32, (256, 384), 6, map_dtype=torch.float16)


@pytest.mark.parametrize("dtype", HALF, ids=ids)
def test_infer_batch_and_infer_stream_in_16_bits(dev, conv, dtype):
    from fots_e2e.pipeline import batched, infer_batch, infer_stream
    from rroi_align.nms import get_boxes
    net = _make_net(dev, dtype)
    size, nimg = (256, 384), 3
    maps = [_maps(size, 5 + 3 * i, 11 + i, dev, dtype) for i in range(nimg)]
    stacked = tuple(torch.stack([m[j] for m in maps]) for j in range(3))
    ims = [_image(size, 20 + i) for i in range(nimg)]
    rec = _Recorder(net)
    try:
        with torch.no_grad():
            res, (per_image, (all_t, c_bat, l_bat), feats) = infer_batch(net, conv, ims, detector=lambda _x: stacked, return_debug=True)
            logs = list(rec.logs)
            assert len(res) == len(per_image) == nimg and feats[1].shape[0] == nimg and feats[1].dtype == dtype
            boxes_all = np.concatenate(per_image, 0)
            bidx = np.repeat(np.arange(nimg), [len(b) for b in per_image])
            _check_crops(feats[1], boxes_all, c_bat, dtype, batch_index=bidx)
            want_lab, want_txt = _expected_from_records(conv, logs, boxes_all)
            assert all_t == want_txt and all(torch.equal(a, b) for a, b in zip(l_bat, want_lab))
            at = 0
            for b in range(nimg):
                boxes_b = get_boxes(*maps[b], 0.5)
                assert len(boxes_b) >= 2 and np.array_equal(boxes_b, per_image[b])
                assert np.array_equal(boxes_b, get_boxes(*_widen(maps[b]), 0.5))
                # every crop bit-identical to the one `batched` cuts from that image's slice of the same feature maps
                _, c1, _ = batched(net, conv, [f[b:b + 1].contiguous() for f in feats], boxes_b, return_crops=True)
                for i in range(len(boxes_b)):
                    assert c1[i].shape == c_bat[at + i].shape and torch.equal(c1[i], c_bat[at + i]), "image %d crop %d" % (b, i)
                t = want_txt[at:at + len(boxes_b)]
                keep = [i for i, x in enumerate(t) if len(x) > 0]
                assert res[b][1] == [t[i] for i in keep] and np.array_equal(res[b][0], boxes_b[keep])
                at += len(boxes_b)
            assert at == len(all_t)
            # the stream: two such batches in flight; batch k's head runs before batch k + 1's, so the records are in order
            del rec.logs[:]
            maps2 = [_maps(size, 4 + 2 * i, 31 + i, dev, dtype) for i in range(nimg)]
            stacked2 = tuple(torch.stack([m[j] for m in maps2]) for j in range(3))
            ims2 = [_image(size, 40 + i) for i in range(nimg)]
            seq = list(infer_stream(net, conv, [ims, ims2], detector=lambda k, _x: (stacked, stacked2)[k]))
            logs = list(rec.logs)
    finally:
        rec.close()
    assert len(seq) == 2
    at_log = 0
    from fots_e2e.pipeline import target_widths_host
    for k, mk in enumerate((maps, maps2)):
        per_image = [get_boxes(*m, 0.5) for m in mk]
        boxes_all = np.concatenate(per_image, 0)
        nb = len(set(target_widths_host(boxes_all)))
        _, want_txt = _expected_from_records(conv, logs[at_log:at_log + nb], boxes_all)
        at_log += nb
        at = 0
        assert len(seq[k]) == nimg
        for b in range(nimg):
            t = want_txt[at:at + len(per_image[b])]
            keep = [i for i, x in enumerate(t) if len(x) > 0]
            assert seq[k][b][1] == [t[i] for i in keep] and np.array_equal(seq[k][b][0], per_image[b][keep])
            at += len(per_image[b])
    assert at_log == len(logs)


def test_preprocess_rounds_once(dev):
    from fots_e2e.pipeline import preprocess
    for shape in ((256, 384, 3), (300, 500, 3)):       # the second one is resized (288 x 480)
        im = np.random.default_rng(5).integers(0, 256, shape, dtype=np.uint8)
        base = preprocess(im, dev)
        assert base.dtype == torch.float32 and torch.equal(base, preprocess(im, dev, torch.float32))
        for dtype in HALF:
            got = preprocess(im, dev, dtype)
            assert got.dtype == dtype and torch.equal(got, base.to(dtype))


def test_a_16_bit_chain_synchronises_as_often_as_the_fp32_one(dev, conv):
    import warnings
    from fots_e2e.pipeline import infer_image, target_widths_host
    size = (256, 384)
    counts = {}
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        net = _make_net(dev, dtype)
        maps = _maps(size, 6, 9, dev, torch.float32)     # the same maps for all three: the same boxes and buckets
        torch.manual_seed(5)
        im_data = (torch.rand(1, 3, *size, device=dev) * 2 - 1).to(dtype)
        with torch.no_grad():
            all_boxes = infer_image(net, conv, im_data, detector=lambda _x: maps, return_debug=True)[2][0]   # warm-up
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("warn")
            try:
                with warnings.catch_warnings(record=True) as w:
                    warnings.simplefilter("always")
                    infer_image(net, conv, im_data, detector=lambda _x: maps)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        syncs = [str(x.message) for x in w if "synchroniz" in str(x.message).lower()]
        nbuckets = len(set(target_widths_host(all_boxes)))
        assert 2 <= len(syncs) <= 2 + 3 * nbuckets, (dtype, syncs, nbuckets)
        counts[dtype] = (len(syncs), nbuckets)
    assert counts[torch.bfloat16] == counts[torch.float32] == counts[torch.float16], counts
