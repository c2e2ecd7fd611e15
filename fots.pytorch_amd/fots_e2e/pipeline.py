"""The inference driver around RoIRotate, restated on PyTorch-ROCm (`test.py:44-127`).

    im (H0, W0, 3) uint8 BGR --resize_rule/preprocess--> im_data (1, 3, H, W) in [-1, 1)
      --net--> score, rbox, angle maps (1/4) and features [merged 256 ch, focr 64 ch]
      --boxes--> (N, 9) quads + score   (`nms.get_boxes`; rroi_align.nms here, or a seeded synthetic
                                          set while the detection heads carry random weights)
      --recognise--> N strings

  batched   ROI rows of all boxes built on the device (`rroi_align_quads_to_rois_hip`), ONE RoIRotate
            launch per image at the widest pooled width, `forward_ocr` once per width BUCKET on the
            crops' own first target_gw columns (InstanceNorm statistics are per sample and per
            width, so a word must see exactly the columns the per-box call gives it), one batched
            greedy-CTC launch per bucket: per IMAGE a handful of launches and one read-back.

The reference's own structure (`tools/ocr_utils.py:131-199`: per WORD a host-built ROI, an upload, an R = 1
launch, the head, `max(1)`, a Python decode) is not part of this package: it lives with the checkers
(`oracle/e2e_loop_oracle.py`), where the tests compare the two and `bench_e2e.py` times it as the baseline.
"""

import collections
import threading

import numpy as np
import torch
import torch.nn.functional as F

from rroi_align.batched import _crops_channels_last, rois_from_quads
from rroi_align.decode import ctc_greedy_decode
from rroi_align.modules.rroi_align import _RRoiAlign, _RRoiAlignBucketed

TARGET_H = 11           # tools/ocr_utils.py:147
SPATIAL_SCALE = 1.0 / 4  # :151, features[1] is the 1/4-resolution map


def resize_rule(h0, w0, max_size=1585152, scale_up=False):
    """(resize_h, resize_w) of `resize_image` (test.py:25-41): multiples of 32, area capped."""
    f = 3 if scale_up else 1
    size = [w0 * f // 32 * 32, h0 * f // 32 * 32]
    while size[0] * size[1] > max_size:
        size[0] /= 1.2
        size[1] /= 1.2
        size[0] = int(size[0] // 32) * 32
        size[1] = int(size[1] // 32) * 32
    return int(size[1]), int(size[0])


def preprocess(im_u8, device, dtype=torch.float32):
    """(H0, W0, 3) uint8 -> (1, 3, H, W) = resized / 128 - 1 (test.py:77-83).  The resize is
    half-pixel bilinear like cv2.resize's default, done on the device.  `dtype`: of the network that takes the image
    (float32, bfloat16, float16): resize and scaling run in fp32 whatever it is, and the result is rounded ONCE."""
    # the BYTES go up (a quarter of the fp32 image) and are widened on the device: `.to(device, dtype)` in one step converts
    # on the host first -- a parallel region of torch's intra-op pool per image, whose spinning workers are what a
    # CPU-quota'd container gets throttled for (hostcpus.py; round 6: batches of images took 36 or 70 ms at random)
    t = torch.as_tensor(im_u8).to(device=device).to(torch.float32).permute(2, 0, 1).unsqueeze(0)
    h, w = resize_rule(t.shape[2], t.shape[3])
    if (h, w) != tuple(t.shape[2:]):
        t = F.interpolate(t, size=(h, w), mode="bilinear", align_corners=False)
    t = t / 128 - 1
    return t if dtype == torch.float32 else t.to(dtype)


def _one_size(ims):
    """The one (H, W) that `resize_rule` maps every image of a batch to; ValueError where they differ."""
    sizes = {resize_rule(im.shape[0], im.shape[1]) for im in ims}
    if len(sizes) != 1:
        raise ValueError("infer_batch: the images must resize to one size, got %s (group them by size)" % sorted(sizes))
    return sizes.pop()


def preprocess_ok(ims, device, dtype=torch.float32) -> bool:
    """Whether `preprocess_batch` can stand in for `preprocess` on these images (a pure predicate: no GPU, no library):
    a non-empty list of C-contiguous uint8 (H, W, 3) arrays that `resize_rule` maps to ONE size of at least one pixel, a
    CUDA device, one of the three dtypes, fewer than 2^31 bytes to upload and fewer than 2^31 elements to write, and not
    one of the classes that measured slower (`_preprocess_slower`)."""
    if not isinstance(ims, (list, tuple)) or len(ims) == 0:
        return False
    try:
        if torch.device(device).type != "cuda":
            return False
    except (TypeError, RuntimeError):
        return False
    if dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return False
    for im in ims:
        if not (isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3
                and im.flags["C_CONTIGUOUS"] and im.shape[0] >= 1 and im.shape[1] >= 1):
            return False
    sizes = {resize_rule(im.shape[0], im.shape[1]) for im in ims}
    if len(sizes) != 1:
        return False
    h, w = next(iter(sizes))
    if h < 1 or w < 1:
        return False
    if sum(im.size for im in ims) >= (1 << 31) or len(ims) * 3 * h * w >= (1 << 31):
        return False
    return not _preprocess_slower(len(ims), (h, w), dtype)


def _preprocess_slower(n_images, size, dtype) -> bool:
    """The classes in which the native call's median was not below the stock chain's (profiles/native_preprocess.md,
    tools/preprocess_bench.py; per call, 720 x 1280 > 704 x 1280, microseconds, native / stock, fp32 | bf16 | fp16): none.
    All 12 rows win.  Between device events, the bytes already uploaded: one image 9.3 / 33.2 | 9.4 / 37.6 | 9.6 / 37.4,
    eight 24.3 / 300.5 | 28.5 / 330.8 | 28.5 / 329.1.  By the host clock, upload included, as the pipeline calls it: one
    image 94.8 / 112.5 | 99.1 / 118.3 | 98.8 / 125.7 (the closest rows: the minimum of the stock arm, 112.3, is below the
    maximum of the native one, 114.6), eight 568.4 / 912.3 | 561.8 / 957.0 | 608.5 / 983.3."""
    return False


_PP_TABLES = collections.OrderedDict()      # (device index, the images' sizes) -> (device table, byte offsets, total bytes)
_PP_TABLES_MAX = 32
_pp_tables_lock = threading.Lock()


def _preprocess_table(ims, device):
    """The kernel's table {byte offset, H0, W0, 0} for images of these sizes laid back to back, on `device`: built and
    uploaded on first use and kept (a stream of images has a handful of sizes -- ICDAR 2015 has one -- so the table of a
    batch is the table of the batch before it).  A kept table is written once, by a synchronous upload, before it is
    returned, so a launch on any stream may read it; `preprocess_batch` records the stream that does (record_stream), so
    that a table that ages out -- at most _PP_TABLES_MAX are kept, least recently used first out -- is not handed out again
    under a launch that still reads it."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index,) + tuple(im.shape[:2] for im in ims)
    with _pp_tables_lock:
        ent = _PP_TABLES.get(key)
        if ent is not None:
            _PP_TABLES.move_to_end(key)
            return ent
    table = np.zeros((len(ims), 4), np.int32)
    at = 0
    for k, im in enumerate(ims):
        table[k] = (at, im.shape[0], im.shape[1], 0)
        at += im.size
    ent = (torch.from_numpy(table).to(device), table[:, 0].tolist(), at)
    with _pp_tables_lock:
        _PP_TABLES[key] = ent
        while len(_PP_TABLES) > _PP_TABLES_MAX:
            _PP_TABLES.popitem(last=False)
    return ent


def preprocess_batch(ims, device, dtype=torch.float32):
    """N images, each (H0, W0, 3) uint8, -> (N, 3, H, W) in `dtype`: what `torch.cat([preprocess(im, device, dtype) ...])`
    computes, by ONE launch (rroi_align._ext.rroi_align.preprocess).  Every image's bytes go up as they are,
    straight from its array into its place in one device buffer -- the images back to back, at whatever address that is --
    and the kernel reads them there, resizes (half-pixel bilinear, like `preprocess`), scales and rounds ONCE from double;
    the table that tells it where each image lies is kept on the device per set of sizes (`_preprocess_table`).  Per call:
    N uploads and one launch, against N uploads and 5 to 6 launches per image plus a `torch.cat`.  (Packing the images and
    the table into one host buffer first, for ONE upload, was measured and is not done: copying eight 720 x 1280 images
    on the host takes the 0.38 ms that the single upload saves twice over -- profiles/native_preprocess.md.)
    Where no resize is needed the float32 result is `preprocess`'s bit for bit; where one is, it is the closer of the two
    to the exact value (`preprocess` resizes in fp32).  The source sizes may differ as long as `resize_rule` maps them to
    one size (the ValueError of `infer_batch` otherwise).  The buffer and the result are allocated, written and read on the
    current stream."""
    from rroi_align._ext.rroi_align import preprocess as _pp
    if len(ims) == 0:
        raise ValueError("preprocess_batch: no images")
    ims = [np.ascontiguousarray(im) for im in ims]
    for im in ims:
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise TypeError("preprocess_batch: every image must be an (H, W, 3) uint8 array, got %s %s" % (im.dtype, im.shape))
    size = _one_size(ims)
    if sum(im.size for im in ims) >= (1 << 31):
        raise ValueError("preprocess_batch: the batch must be smaller than 2^31 bytes")
    device = torch.device(device)
    table, offsets, total = _preprocess_table(ims, device)
    if len(ims) == 1:
        src = torch.from_numpy(ims[0].reshape(-1)).to(device)
    else:
        src = torch.empty(total, dtype=torch.uint8, device=device)
        for at, im in zip(offsets, ims):
            src[at:at + im.size].copy_(torch.from_numpy(im.reshape(-1)))
    out = _pp.preprocess_images(src, table, size, dtype)
    table.record_stream(torch.cuda.current_stream(device))
    return out


def _front_input(ims, device, dtype, native_preprocess):
    """The network's input for a list of images: `preprocess_batch` where it was asked for and `preprocess_ok` holds, the
    stock expression otherwise."""
    if native_preprocess and preprocess_ok(ims, device, dtype):
        return preprocess_batch(ims, device, dtype)
    _one_size(ims)
    return torch.cat([preprocess(im, device, dtype) for im in ims], 0)


def _net_device_dtype(net):
    """Where the network lives and the dtype it runs in (`net.to(torch.bfloat16)`): its first parameter's."""
    p = next(net.parameters())
    return p.device, p.dtype


def target_widths_host(boxes):
    """The callers' pooled-width rule (tools/ocr_utils.py:146-150) for boxes that are already on the host:
    target_gw = int(w * (11 / max(1, h))) + 11 rounded down to a multiple of 32, at least 64 -- w, h from the fp32
    corner differences, square root in double.  The same numbers the device kernel
    (`rroi_align_quads_to_rois_hip`, mode 0) writes next to its ROI rows (asserted equal in
    tests/test_e2e_gpu.py); having them here saves `infer_image` a read-back before the head."""
    b = np.asarray(boxes, np.float32)[:, :8].reshape(-1, 4, 2)
    dw, dh = b[:, 2] - b[:, 1], b[:, 1] - b[:, 0]
    w = np.sqrt((dw[:, 0] * dw[:, 0] + dw[:, 1] * dw[:, 1]).astype(np.float64))
    h = np.sqrt((dh[:, 0] * dh[:, 0] + dh[:, 1] * dh[:, 1]).astype(np.float64))
    gw = (w * (TARGET_H / np.maximum(1.0, h))).astype(np.int64) + TARGET_H
    return (np.maximum(2, gw // 32) * 32).tolist()


def batched(net, converter, features, boxes, return_crops=False, gw_host=None, batch_index=None, bucketed=False):
    """All words of an image at once.  `boxes`: (N, >= 8) tensor on the device (or array).
    `gw_host`: the boxes' pooled widths when the caller already has them on the host (`infer_image`:
    the boxes come out of the host-side merge: `target_widths_host`) -- then nothing is
    read back before the head.
    A network in bfloat16 / float16 hands 16-bit features over: the op cuts 16-bit crops natively (each element the fp32
    crop's, rounded once), the head runs in 16 bits and the greedy CTC reads its 16-bit log-probabilities as they are --
    no widening copy anywhere on the path.  Quads, ROI rows and widths are float32 / int32: they carry geometry.
    `batch_index` (N,): the image each box belongs to when `features` hold SEVERAL images (`infer_batch`) -- the op's
    own first ROI column (`tools/ocr_utils.py:151` writes 0 there: one image per call); still ONE RoIRotate launch.
    `bucketed` (opt-in): the crops come from the bucketed op (`_RRoiAlignBucketed`) -- every word pooled at its own
    bucket's width, each bucket a dense tensor the head takes as it is: no crop tensor at the widest width, no
    index_select, no slice.  The same crops bit for bit, hence the same texts."""
    focr = features[1]
    quads = torch.as_tensor(boxes, dtype=torch.float32, device=focr.device)[:, :8].contiguous()
    n = quads.shape[0]
    if n == 0:
        return ([], [], []) if return_crops else []
    if batch_index is not None:
        batch_index = torch.as_tensor(batch_index, dtype=torch.float32).to(focr.device).contiguous()
    rois, gw = rois_from_quads(quads, batch_index, False, TARGET_H)
    if gw_host is None:
        gw_host = gw.cpu()                              # the one read-back before the head
    else:
        gw_host = torch.as_tensor(gw_host, dtype=torch.int32)
        if gw_host.numel() != n:
            raise ValueError("gw_host must have one width per box")
    widths = sorted(set(int(v) for v in gw_host))
    texts = [None] * n
    crops, labels = [None] * n, [None] * n
    # every bucket's head and decode are enqueued before anything is read back: one wait for the image,
    # not two per bucket (the buckets' index lists come from the widths that are on the host already)
    pending = []
    gw_list = gw_host.tolist()
    if bucketed:
        for idx_dev, x in _RRoiAlignBucketed(TARGET_H, SPATIAL_SCALE)(focr, rois, gw_list):
            logp = net.forward_ocr(x)
            decoded, dlen, lab = ctc_greedy_decode(logp, None, return_labels=True)
            pending.append(([i for i, v in enumerate(gw_list) if int(v) == x.shape[3]], decoded, dlen, x, lab))
        widths = []
    else:
        # (the crops follow the features' layout: a channels_last network gets channels_last crops, no relayout on either side)
        crops_all = _RRoiAlign(TARGET_H, widths[-1], SPATIAL_SCALE, _crops_channels_last(focr, None))(focr, rois)
    for wdt in widths:                                  # buckets are multiples of 32: a handful
        idx = [i for i, v in enumerate(gw_list) if int(v) == wdt]
        idx_dev = torch.tensor(idx, dtype=torch.int64).to(focr.device, non_blocking=True)
        x = crops_all.index_select(0, idx_dev)[:, :, :, :wdt]
        logp = net.forward_ocr(x)
        decoded, dlen, lab = ctc_greedy_decode(logp, None, return_labels=True)
        pending.append((idx, decoded, dlen, x, lab))
    for idx, decoded, dlen, x, lab in pending:
        words = converter.to_texts(decoded, dlen)       # the first of these waits for the whole image
        for j, i in enumerate(idx):
            texts[i] = words[j]
            if return_crops:
                crops[i], labels[i] = x[j:j + 1], lab[j].to(torch.int64)
    return (texts, crops, labels) if return_crops else texts


def infer_image(net, converter, im, detector=None, segm_thresh=0.5, return_debug=False, bucketed=False,
                native_preprocess=False):
    """One image through the whole chain of `test.py:75-116`: preprocess -> net -> `get_boxes` on the maps
    where the network wrote them -> RoIRotate + recognition head + greedy CTC for every box ->
    (boxes (n, 9) numpy, texts); like the reference's loop, boxes whose text is empty are dropped
    (test.py:109-110).  `return_debug` appends (all boxes, the recogniser's (texts, crops, labels), the features).

    `detector`: optional hook `im_data -> (score (h, w), rbox (4, h, w), angle (2, h, w))` device tensors
    that stand in for the three head outputs -- random weights pass no box (or a hundred thousand)
    through the NMS, so tests and the benchmark inject the maps of `tests/e2e_inputs.py: synthetic_detector_maps` here.

    Host synchronisations per image: ONE before the head (`get_boxes` reads the number of passing pixels
    and their records: the merge is sequential host code) and the final read-back of the decoded labels.
    The pooled-width buckets need no second one: the boxes are on the host after the merge and the width
    rule is plain arithmetic (`target_widths_host`).

    The image is preprocessed into the dtype of the network's parameters (float32, bfloat16, float16), so
    `infer_image(net.to(torch.bfloat16), ...)` runs the whole chain in 16 bits with the same synchronisations; a tensor
    passed instead of an image is used as it is.  The `detector` hook's maps may have any of the three dtypes.
    `bucketed`: see `batched` (opt-in; same boxes, texts and crops).
    `native_preprocess` (opt-in): the image goes through `preprocess_batch` -- one upload, one launch -- where
    `preprocess_ok` holds, through `preprocess` otherwise; the same input bit for bit in float32 where no resize is needed."""
    from rroi_align.nms import get_boxes
    device, dtype = _net_device_dtype(net)
    if isinstance(im, torch.Tensor):
        im_data = im
    elif native_preprocess and preprocess_ok([im], device, dtype):
        im_data = preprocess_batch([im], device, dtype)
    else:
        im_data = preprocess(im, device, dtype)
    score, rbox, angle, feats = net(im_data)
    if detector is not None:
        s, r, a = detector(im_data)
    else:
        s, r, a = score[0][0, 0], rbox[0][0], angle[0][0]
    boxes = get_boxes(s, r, a, segm_thresh)
    out = batched(net, converter, feats, boxes, return_crops=return_debug, gw_host=target_widths_host(boxes),
                  bucketed=bucketed)
    texts = out[0] if return_debug else out
    keep = [i for i, t in enumerate(texts) if len(t) > 0]
    res = (boxes[keep], [texts[i] for i in keep])
    return res + ((boxes, out, feats),) if return_debug else res


def _batch_front(net, ims, detector, segm_thresh, native_preprocess=False):
    """The first half of `infer_batch`, ENQUEUED on the current stream and nothing read back: preprocessing, one pass of the
    network, one decode launch per image."""
    from rroi_align.nms import decode_batch
    device, dtype = _net_device_dtype(net)
    if isinstance(ims, torch.Tensor):
        im_data = ims
    else:
        im_data = _front_input(ims, device, dtype, native_preprocess)
    score, rbox, angle, feats = net(im_data)
    if detector is not None:
        s, r, a = detector(im_data)
    else:
        s, r, a = score[0][:, 0], rbox[0], angle[0]
    return im_data.shape[0], feats, decode_batch(s, r, a, segm_thresh)


def _batch_back(net, converter, front, return_debug=False, bucketed=False):
    """The second half, on the current stream: the boxes of every image (`merge_decoded`: two synchronisations, host merges),
    ONE RoIRotate launch for all their words, the head per pooled-width bucket, the strings."""
    from rroi_align.nms import merge_decoded
    nimg, feats, decoded = front
    per_image = merge_decoded(decoded)
    counts = [len(b) for b in per_image]
    boxes = np.concatenate(per_image, 0) if nimg else np.zeros((0, 9), np.float32)
    bidx = np.repeat(np.arange(nimg, dtype=np.float32), counts)
    out = batched(net, converter, feats, boxes, return_crops=return_debug, gw_host=target_widths_host(boxes) if len(boxes) else [],
                  batch_index=bidx, bucketed=bucketed)
    texts = out[0] if return_debug else out
    res, at = [], 0
    for b in range(nimg):
        t = texts[at:at + counts[b]]
        keep = [i for i, x in enumerate(t) if len(x) > 0]
        res.append((per_image[b][keep], [t[i] for i in keep]))
        at += counts[b]
    return (res, (per_image, out, feats)) if return_debug else res


def infer_batch(net, converter, ims, detector=None, segm_thresh=0.5, return_debug=False, bucketed=False,
                native_preprocess=False):
    """SEVERAL images of one size through the chain of `test.py:75-116` at once (round 6; the reference's loop takes one
    image per pass, `test.py:62-75` -- its test set, ICDAR 2015, is 1280 x 720 throughout): ONE pass through the network
    for the batch, `get_boxes` per image (every image's device decode is enqueued before the first read-back: one wait
    for the batch), ONE RoIRotate launch for the words of ALL images (the op's batch index, `kernel.cu:46`), the
    recognition head once per pooled-width bucket across the images, one read-back of the decoded labels.
    -> a list of `infer_image`'s (boxes (n, 9) numpy, texts) per image, in order.  A word's crop is bit-identical to the
    one the per-image chain cuts out of the same feature map (`tests/test_e2e_gpu.py`).

    `ims`: a list of (H0, W0, 3) uint8 arrays that `resize_rule` maps to ONE size, or an (N, 3, H, W) tensor that is
    already preprocessed.  `detector`: as in `infer_image`, for the whole batch: `im_data -> (score (N, h, w),
    rbox (N, 4, h, w), angle (N, 2, h, w))`.  `native_preprocess` (opt-in): the whole batch goes through ONE
    `preprocess_batch` -- one upload, one launch, no `torch.cat` -- where `preprocess_ok` holds (see `infer_image`)."""
    if len(ims) == 0:
        return ([], ([], ([], [], []), None)) if return_debug else []
    return _batch_back(net, converter, _batch_front(net, ims, detector, segm_thresh, native_preprocess), return_debug, bucketed)


def infer_stream(net, converter, batches, detector=None, segm_thresh=0.5, bucketed=False, native_preprocess=False):
    """`infer_batch` over a SEQUENCE of batches with two batches in flight (a generator: one list of (boxes, texts) per
    batch, in order): the network pass of batch k + 1 is enqueued on the caller's stream BEFORE batch k's boxes are read
    back, and batch k's second half -- read-backs, host merges, RoIRotate, head, strings -- runs on a second stream
    beside it.  The device never waits for the host's merges and string building, the host never waits for a network
    pass it does not need yet; results are those of `infer_batch` (same kernels on the same data).  `detector`: a callable
    `(k, im_data) -> maps` (the batch's index first), or None.  `bucketed`: see `batched`; everything the bucketed op
    allocates (crops, tables, scratch) is allocated on the side stream that uses it, so the invariant below covers it.
    `native_preprocess`: see `infer_batch`; the packed upload and the input tensor are allocated, written and read on the
    caller's stream alone (the side stream reads neither), so the invariant needs nothing more."""
    device = next(net.parameters()).device
    side = torch.cuda.Stream(device=device)

    def back(front, ready):
        # INVARIANT: everything `side` reads was allocated on the caller's stream -- the feature maps and each image's
        # (records, count).  `ready` orders the reads after their producers; record_stream tells the caching allocator
        # that `side` uses the blocks too, so that a tensor the caller's stream frees (the generator drops `front`
        # while batch k + 1's network pass is being enqueued) is not handed out again before `side` is done with it.
        _, feats, (pending, _) = front
        for t in feats:
            t.record_stream(side)
        for rec, cnt in pending:
            rec.record_stream(side)
            cnt.record_stream(side)
        with torch.cuda.stream(side):
            side.wait_event(ready)
            res = _batch_back(net, converter, front, bucketed=bucketed)      # its read-backs synchronise `side` only
        return res
    prev = None
    for k, ims in enumerate(batches):
        if len(ims) == 0:
            if prev is not None:
                yield back(*prev)
                prev = None
            yield []
            continue
        front = _batch_front(net, ims, None if detector is None else (lambda x, k=k: detector(k, x)), segm_thresh,
                             native_preprocess)
        ready = torch.cuda.Event()
        ready.record()
        if prev is not None:
            yield back(*prev)
        prev = (front, ready)
    if prev is not None:
        yield back(*prev)
