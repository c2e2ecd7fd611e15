"""rroi_align._ext.rroi_align.detection_loss -- the binding of the native detection loss (header section 16):
the dice, angle and IoU terms of both scales in two launches, their gradient with respect to the six predictions in one, no
host synchronisation, deterministic, for float32 / bfloat16 / float16 predictions.

A module of the binding like the package's own (`csrc/rroi_detection_loss_host.h`), loaded on first use by
`rroi_align.detection`: the package's `_*_run` callables are a closed list that the network's ledger test reads, so the hot
calls here are `run_detection_loss` and `run_detection_loss_backward`.  The public surface (argument forms, checks,
autograd) is rroi_align.detection."""
import collections
import ctypes

import torch

from ._core import _DTYPES, DTYPE_FP32, _bind, _check, _i, _lib, _stream, _sz, _vp, dtype_code


class _DetectionLossPlan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("grid_x", "block", "items_per_thread", "blocks_quarter", "blocks_eighth", "slot_doubles",
                                  "state_doubles", "finish_block")]


_bind("rroi_detection_loss_forward_hip", [_i] + [_vp] * 10 + [_i] * 5 + [_vp, _vp, _sz, _vp])
_bind("rroi_detection_loss_backward_hip", [_i] + [_vp] * 8 + [_i] * 5 + [_vp] * 9)
_bind("rroi_detection_loss_plan", [_i] * 6 + [ctypes.POINTER(_DetectionLossPlan)])
_bind("rroi_detection_loss_workspace_bytes", [_i] * 5, _sz)

DetectionLossPlan = collections.namedtuple("DetectionLossPlan", [n for n, _ in _DetectionLossPlan._fields_])


def detection_loss_plan(batch_size, height, width, height8=0, width8=0, dtype=DTYPE_FP32) -> DetectionLossPlan:
    """What the calls launch for (batch_size, height, width) maps at 1/4 and (height8, width8) at 1/8 (both 0: a single
    scale) -- host only, no GPU needed, a pure function of the shape: the grid, the block, the items per thread, the
    workgroups of each scale, the doubles per slot and of the state, the finishing workgroup's threads.  ValueError where the
    calls would refuse the arguments."""
    p = _DetectionLossPlan()
    if _lib.rroi_detection_loss_plan(dtype_code(dtype), int(batch_size), int(height), int(width), int(height8), int(width8),
                                     ctypes.byref(p)) != 1:
        raise ValueError("rroi_detection_loss_plan: the calls would refuse these arguments")
    return DetectionLossPlan(*(getattr(p, n) for n in DetectionLossPlan._fields))


def detection_loss_workspace_bytes(batch_size, height, width, height8=0, width8=0) -> int:
    """Bytes of workspace the forward call needs: the slots of partial sums, then the state (0: refused arguments)."""
    return int(_lib.rroi_detection_loss_workspace_bytes(int(batch_size), int(height), int(width), int(height8), int(width8)))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _dims(preds4, preds8):
    N, _, H, W = preds4[0].shape
    H8, W8 = (preds8[0].shape[2:] if preds8 is not None else (0, 0))
    return N, H, W, H8, W8


def run_detection_loss(preds4, preds8, truth):
    """The forward call, for arguments already checked (rroi_align.detection): preds4 = (segm, angle, roi) of the 1/4
    scale, contiguous NCHW of one dtype on one GPU; preds8 likewise or None; truth = (segm_gt, iou_mask, angle_gt, roi_gt)
    contiguous float32.  Returns (terms, state): terms 4 float32 {segm, angle, box, total}; state the 20 doubles the backward
    call reads -- a view of the workspace allocated here, which lives as long as the view does."""
    dev = preds4[0].device
    if dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev.index):
            return run_detection_loss(preds4, preds8, truth)
    dims = _dims(preds4, preds8)
    nbytes = _lib.rroi_detection_loss_workspace_bytes(*dims)
    if not nbytes:
        raise ValueError("rroi_detection_loss_forward_hip: invalid argument (shape)")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)        # per call: the state outlives it
    terms = torch.empty(4, dtype=torch.float32, device=dev)
    p8 = preds8 if preds8 is not None else (None, None, None)
    st = _lib.rroi_detection_loss_forward_hip(_DTYPES[preds4[0].dtype], *(_ptr(t) for t in preds4), *(_ptr(t) for t in p8),
                                              *(_ptr(t) for t in truth), *dims, terms.data_ptr(), ws.data_ptr(), nbytes, _stream())
    if st != 1:
        _check(st, "rroi_detection_loss_forward_hip")
    return terms, ws[-20:]


def run_detection_loss_backward(preds4, preds8, truth, state, grad_terms, grads4=None, grads8=None):
    """The backward call: grad_terms 4 float32 on the device (read by the kernel, never by the host), state from
    run_detection_loss.  Returns (grads4, grads8): gradients shaped and typed like the predictions (grads8 None for a single
    scale), into the given buffers where given.  Every element is written by the launch: no memset."""
    dev = preds4[0].device
    if dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev.index):
            return run_detection_loss_backward(preds4, preds8, truth, state, grad_terms, grads4, grads8)
    if grads4 is None:
        grads4 = tuple(torch.empty_like(t) for t in preds4)
    if grads8 is None and preds8 is not None:
        grads8 = tuple(torch.empty_like(t) for t in preds8)
    p8 = preds8 if preds8 is not None else (None, None, None)
    g8 = grads8 if preds8 is not None else (None, None, None)
    st = _lib.rroi_detection_loss_backward_hip(_DTYPES[preds4[0].dtype], _ptr(preds4[1]), _ptr(preds4[2]), _ptr(p8[1]), _ptr(p8[2]),
                                               *(_ptr(t) for t in truth), *_dims(preds4, preds8), state.data_ptr(),
                                               grad_terms.data_ptr(), *(_ptr(t) for t in grads4), *(_ptr(t) for t in g8), _stream())
    if st != 1:
        _check(st, "rroi_detection_loss_backward_hip")
    return grads4, (grads8 if preds8 is not None else None)
