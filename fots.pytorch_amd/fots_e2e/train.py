"""fots_e2e.train -- the training caller's recognition branch (the reference's src/ocr_process.py:259-301): RoIRotate on the
64-channel 1/4 map -> forward_ocr -> CTC, the loss summed over the words and divided by their number.

The reference's loss is warpctc (`ctc_loss(preds, text, preds_size, label_length) / preds.size(1)`); the stock stand-in here
is `F.ctc_loss(..., reduction="sum")`, as bench_legs.train_step uses it.  `native_ctc=True` switches to
rroi_align.ctc.ctc_loss -- deterministic, 16-bit log-probabilities read as they are, the head's (N, K, T) output read where
it lies.  Opt-in and off by default, like every switch of this package."""
import math

import torch
import torch.nn.functional as F

from rroi_align.modules.rroi_align import _RRoiAlign

POOLED_HEIGHT = 11        # src/ocr_process.py:260
SPATIAL_SCALE = 1.0 / 4   # :266


def recognition_loss(net, features, rois, targets, target_lengths, native_ctc=False, return_debug=False):
    """features: what `net(x)` returns last, [merged map, the 64-channel 1/4 map] -- features[1] is cropped (:267); rois (R, 6)
    {batch index, cx, cy, h, w, angle}; targets flat (sum L,) or padded (R, L_max) labels, 0 the blank; target_lengths R
    lengths.  -> the loss (a scalar: the sum over the words / R); with return_debug also the crops and the head's
    log-probabilities (R, K, T)."""
    rois = rois.view(-1, 6)
    pooled_width = math.ceil(POOLED_HEIGHT * (rois[:, 4] / rois[:, 3]).max().item())       # :261-263
    crops = _RRoiAlign(POOLED_HEIGHT, pooled_width, SPATIAL_SCALE)(features[1], rois)       # :266-267
    preds = net.forward_ocr(crops)                                                          # :295
    log_probs = preds.permute(2, 0, 1)                                                      # :296, (T, R, K)
    T, R = log_probs.size(0), log_probs.size(1)
    if native_ctc:
        from rroi_align.ctc import ctc_loss
        loss = ctc_loss(log_probs, targets, [T] * R, target_lengths, blank=0, reduction="sum") / R
    else:
        loss = F.ctc_loss(log_probs, targets, [T] * R, target_lengths, blank=0, reduction="sum") / R   # :300-301
    return (loss, crops, preds) if return_debug else loss
