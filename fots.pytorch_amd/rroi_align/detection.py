"""rroi_align.detection -- the training-time twin of the native detection heads: the reference's detection loss
(`ModelResNetSep2.loss`, tools/models.py:459-505 with `dice_loss` :105 and `iou_loss` :197) as native HIP.

What it adds to the stock restatement (`fots_e2e.train.detection_loss`): no host synchronisation -- the stock form indexes
with a boolean mask some thirty times and branches twice on a sum, each a device-to-host round trip --, so the call can be
captured into a graph; two launches forward and one backward instead of a hundred small kernels each way; float32 / bfloat16
/ float16 predictions read as they are; the 1/8 ground truth resized inside the kernel and never stored; and a
DETERMINISTIC result: everything is evaluated in double, every sum in a fixed order that depends on the shape alone, no
atomic, so a second run gives the same bits (include/rroi_align_hip.h section 16 is the arithmetic contract).  The four
terms come out in float32, the gradients in the predictions' dtype, rounded once from double.

Where it differs from the reference on purpose: a term whose selection is empty -- no pixel with segm_gt above 0.5, or none
of those with a left (roi_gt[..., 2]) or right (roi_gt[..., 3]) distance above 0 -- contributes 0 and a zero gradient; the
reference takes `torch.mean` of nothing there and returns NaN for the last two.  Nothing read from the ground truth is used
as an index, so no contents of it can take a kernel out of bounds.  There is no gradient for the ground truth.  GPU only, as
the rest of the package."""
import torch
from torch.autograd.function import once_differentiable

from ._ext.rroi_align import _IO_DTYPES, _require_cuda_f32
from ._ext.rroi_align.detection_loss import run_detection_loss, run_detection_loss_backward

_CHANNELS = (("segm_preds", 1), ("angle_preds", 2), ("roi_preds", 4))


def _tensor(t, name, dtypes):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, got {t.dtype}")


def _scale(preds, k, N, hw, dtype):
    """The three predictions of scale k (0: 1/4, 1: 1/8), their types and shapes checked; -> the tensors."""
    out = []
    for (name, channels), p in zip(_CHANNELS, preds):
        if not isinstance(p, (list, tuple)) or len(p) <= k:
            raise ValueError(f"{name} must be a list of the 1/4 and the 1/8 prediction")
        t = p[k]
        _tensor(t, f"{name}[{k}]", _IO_DTYPES)
        if t.dtype != dtype:
            raise TypeError(f"all six predictions share one dtype: {name}[{k}] is {t.dtype}, segm_preds[0] {dtype}")
        if t.dim() != 4 or t.size(0) != N or t.size(1) != channels or (hw is not None and tuple(t.shape[2:]) != hw):
            want = f"({N}, {channels}, {hw[0]}, {hw[1]})" if hw is not None else f"({N}, {channels}, h, w)"
            raise ValueError(f"{name}[{k}] must be {want}, got {tuple(t.shape)}")
        if min(t.shape) < 1:
            raise ValueError(f"{name}[{k}] is empty: {tuple(t.shape)}")
        hw = tuple(t.shape[2:])
        out.append(t)
    return tuple(out)


def _prepare(segm_preds, segm_gt, iou_mask, angle_preds, angle_gt, roi_preds, roi_gt, multi_scale):
    """Checked arguments -> (preds4, preds8 or None, truth) as the binding takes them.  Types first, then shapes, then
    devices, all on the host before any launch."""
    if not isinstance(segm_preds, (list, tuple)) or not segm_preds:
        raise ValueError("segm_preds must be a list of the 1/4 and the 1/8 prediction")
    first = segm_preds[0]
    _tensor(first, "segm_preds[0]", _IO_DTYPES)
    if first.dim() != 4:
        raise ValueError(f"segm_preds[0] must be (N, 1, H, W), got {tuple(first.shape)}")
    N, H, W = first.size(0), first.size(2), first.size(3)
    preds = (segm_preds, angle_preds, roi_preds)
    preds4 = _scale(preds, 0, N, (H, W), first.dtype)
    preds8 = _scale(preds, 1, N, None, first.dtype) if multi_scale else None
    truth = (("segm_gt", segm_gt, (N, H, W)), ("iou_mask", iou_mask, (N, H, W)), ("angle_gt", angle_gt, (N, H, W)),
             ("roi_gt", roi_gt, (N, H, W, 4)))
    for name, t, shape in truth:
        _tensor(t, name, (torch.float32,))
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    named = [(f"{n}[{k}]", t) for k, ps in enumerate((preds4, preds8 or ())) for (n, _), t in zip(_CHANNELS, ps)]
    for name, t in named + [(n, t) for n, t, _ in truth]:
        _require_cuda_f32(t, name, (t.dtype,))
        if t.device != first.device:
            raise ValueError(f"{name} is on {t.device}, segm_preds[0] on {first.device}")
    gts = [t.detach().contiguous() for _, t, _ in truth]
    if gts[3].data_ptr() % 16:
        gts[3] = gts[3].clone()                                       # roi_gt is read four channels at a time
    return tuple(t.contiguous() for t in preds4), (tuple(t.contiguous() for t in preds8) if preds8 else None), tuple(gts)


class _DetectionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, want, multi, truth, *preds):
        preds4, preds8 = preds[:3], (preds[3:] if multi else None)
        terms, state = run_detection_loss(preds4, preds8, truth)
        if want:
            ctx.multi = multi
            ctx.save_for_backward(state, *truth, *preds)
        return terms

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        state, truth, preds = ctx.saved_tensors[0], ctx.saved_tensors[1:5], ctx.saved_tensors[5:]
        g = g.to(torch.float32).contiguous()
        grads4, grads8 = run_detection_loss_backward(preds[:3], preds[3:] if ctx.multi else None, truth, state, g)
        return (None, None, None) + tuple(grads4) + (tuple(grads8) if ctx.multi else ())


def detection_loss(segm_preds, segm_gt, iou_mask, angle_preds, angle_gt, roi_preds, roi_gt, multi_scale=True, return_terms=False):
    """The reference's detection loss on the GPU, native and deterministic, with the reference's argument order.
    segm_preds = [s4 (N, 1, H, W), s8 (N, 1, H8, W8)], angle_preds = [a4 (N, 2, H, W), a8], roi_preds = [r4 (N, 4, H, W), r8]:
    all six of one dtype, float32, bfloat16 or float16 (a non-contiguous one takes one `.contiguous()`); H8, W8 come from
    the 1/8 predictions and need not be H / 2, W / 2; with multi_scale=False the 1/8 entries are not looked at.  segm_gt,
    iou_mask, angle_gt: (N, H, W) float32; roi_gt: (N, H, W, 4) float32, {top, bottom, left, right}.
    Returns the total `segm + 2 angle + 0.5 box` (a float32 scalar), or with return_terms the float32 tensor
    [segm, angle, box, total], every entry differentiable.  A term whose selection is empty is 0 with a zero gradient (the
    reference: NaN for an empty left or right selection).  No host synchronisation; the same bits on every run.
    RuntimeError for CPU tensors, TypeError for other or mixed dtypes, ValueError for bad shapes, all before any launch."""
    preds4, preds8, truth = _prepare(segm_preds, segm_gt, iou_mask, angle_preds, angle_gt, roi_preds, roi_gt, multi_scale)
    preds = preds4 + (preds8 or ())
    want = torch.is_grad_enabled() and any(t.requires_grad for t in preds)      # else nothing is saved
    terms = _DetectionLoss.apply(want, bool(multi_scale), truth, *preds)
    return terms if return_terms else terms[3]


class DetectionLoss(torch.nn.Module):
    """`detection_loss` above as a module, the reference's `net.loss(...)` call: the same seven arguments in forward."""

    def __init__(self, multi_scale=True, return_terms=False):
        super().__init__()
        self.multi_scale, self.return_terms = multi_scale, return_terms

    def forward(self, segm_preds, segm_gt, iou_mask, angle_preds, angle_gt, roi_preds, roi_gt):
        return detection_loss(segm_preds, segm_gt, iou_mask, angle_preds, angle_gt, roi_preds, roi_gt, self.multi_scale,
                              self.return_terms)
