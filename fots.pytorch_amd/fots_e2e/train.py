"""fots_e2e.train -- the training caller's recognition branch (the reference's src/ocr_process.py:259-301): RoIRotate on the
64-channel 1/4 map -> forward_ocr -> CTC, the loss summed over the words and divided by their number.

The reference's loss is warpctc (`ctc_loss(preds, text, preds_size, label_length) / preds.size(1)`); the stock stand-in here
is `F.ctc_loss(..., reduction="sum")`, as bench_legs.train_step uses it.  `native_ctc=True` switches to
rroi_align.ctc.ctc_loss -- deterministic, 16-bit log-probabilities read as they are, the head's (N, K, T) output read where
it lies.  Opt-in and off by default, like every switch of this package.

`detection_loss` is the other half of the reference's step: `ModelResNetSep2.loss` (tools/models.py:459-505, with `dice_loss`
:105-113 and `iou_loss` :197-235) restated in torch, its operations in its order; `native=True` switches to rroi_align.detection.detection_loss
-- two launches forward and one backward, no host synchronisation, deterministic.  Off by default as well."""
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


def _dice(pred, truth):
    """-(2 sum(pred truth) + 1) / (sum pred + sum truth + 1) over all pixels: models.py:105-113, its smoothing constant 1."""
    pred, truth = pred.reshape(-1), truth.reshape(-1)
    overlap = (pred * truth).sum()
    return -((2. * overlap + 1.) / (pred.sum() + truth.sum() + 1.))


def _box_half(top_gt, bottom_gt, side_gt, top, bottom, side):
    """The IoU term of one half of the boxes -- the part left of each pixel (:216-225) or right of it (:227-235) -- as the
    mean of -log((intersection + 1) / (union + 1)) over the selected pixels; the mean of nothing is NaN, as there."""
    area_gt = (top_gt + bottom_gt) * side_gt
    area = (top + bottom) * side
    overlap = torch.min(side_gt, side) * (torch.min(top_gt, top) + torch.min(bottom_gt, bottom))
    union = area_gt + area - overlap
    return torch.mean(-torch.log((overlap + 1.0) / (union + 1.0)))


def _text_terms(text, angle_gt, angles, distances_gt, distances):
    """[sin, cos, left, right] of one scale over the pixels of the boolean map `text`: the two angle errors (:478-482) and
    the two box halves (`iou_loss`, :197-235).  distances_gt (N, h, w, 4) and distances (N, 4, h, w) hold
    {top, bottom, left, right}; a half counts the pixels whose ground-truth distance to that side is positive (:203-206)."""
    theta = angle_gt[text]
    terms = [F.mse_loss(angles[:, 0][text], torch.sin(theta)), F.mse_loss(angles[:, 1][text], torch.cos(theta))]
    gt = [distances_gt[..., k][text] for k in range(4)]
    pred = [distances[:, k][text] for k in range(4)]
    for side in (2, 3):
        has = gt[side] > 0
        terms.append(_box_half(gt[0][has], gt[1][has], gt[side][has], pred[0][has], pred[1][has], pred[side][has]))
    return terms


def _resize(x, size):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=True)


def detection_loss(segm_preds, segm_gt, iou_mask, angle_preds, angle_gt, roi_preds, roi_gt, multi_scale=True, native=False,
                   return_terms=False):
    """The reference's detection loss, `net.loss(...)` of tools/models.py:459-505 with its argument order.
    segm_preds = [s4 (N, 1, H, W), s8 (N, 1, H8, W8)], angle_preds = [a4 (N, 2, H, W), a8], roi_preds = [r4 (N, 4, H, W), r8], as
    `net(x)` returns them; segm_gt, iou_mask, angle_gt (N, H, W) and roi_gt (N, H, W, 4) {top, bottom, left, right} float32, as
    the reference's data generator makes them.  -> total = segm + 2 angle + 0.5 box; with return_terms the tensor
    [segm, angle, box, total] (what the reference keeps as `net.segm_loss_value` ... for its log line), float32 for every
    dtype the reference runs in (the dtype the arithmetic ran in: float64 for float64 arguments).
    native=False is the stock restatement: the reference's operations in the reference's order, so its float32 results
    bit for bit (tests/golden/detection_loss.npz), its behaviour included -- NaN where the selection of the left or right
    box half is empty, a host synchronisation at every boolean index and at both `if`s.  native=True is
    rroi_align.detection.detection_loss, which defines those cases as 0 and synchronises nowhere."""
    if native:
        from rroi_align.detection import detection_loss as native_loss
        return native_loss(segm_preds, segm_gt, iou_mask, angle_preds, angle_gt, roi_preds, roi_gt, multi_scale, return_terms)
    segm = _dice(segm_preds[0].squeeze(1) * iou_mask, segm_gt * iou_mask)                   # :464-466
    if multi_scale:                                                                         # :469-472
        size = tuple(segm_preds[1].shape[2:])
        segm_gt8 = _resize(segm_gt.unsqueeze(1), size).squeeze(1)
        iou_mask8 = _resize(iou_mask.unsqueeze(1), size).squeeze(1)
        segm = segm + _dice(segm_preds[1].squeeze(1) * iou_mask8, segm_gt8 * iou_mask8)
    angle, box = segm_gt.new_zeros(()), segm_gt.new_zeros(())                               # :461-462
    scales = [(segm_gt > 0.5, angle_gt, angle_preds[0], roi_gt, roi_preds[0])]              # :474
    if multi_scale:
        # the 1/8 scale: text where the resized score map is above 0.5 (:490), the geometry resized and halved (:493, :501-502)
        scales.append((segm_gt8 > 0.5, None, angle_preds[1], None, roi_preds[1]))
    for k, (text, theta, angles, distances_gt, distances) in enumerate(scales):
        if not text.sum() > 0:                                                              # :476, :491 -- the second inside the first
            break
        if k == 1:
            theta = _resize(angle_gt.unsqueeze(1), size).squeeze(1)
            distances_gt = (_resize(roi_gt.permute(0, 3, 1, 2), size) / 2).permute(0, 2, 3, 1)
        sin_term, cos_term, left, right = _text_terms(text, theta, angles, distances_gt, distances)
        angle = angle + sin_term + cos_term                                                 # :484-485, :498-499
        box = box + left + right                                                            # :487, :503
    total = segm + angle * 2 + 0.5 * box                                                    # :505
    if return_terms:
        return torch.stack([v.to(total.dtype) for v in (segm, angle, box, total)])
    return total
