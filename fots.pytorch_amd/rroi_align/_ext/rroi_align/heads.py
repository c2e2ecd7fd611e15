"""rroi_align._ext.rroi_align.heads -- the binding of the network's detection heads and attention gate (header section 7,
DESIGN 5.12; `csrc/rroi_heads_host.h`)."""
import collections
import ctypes

import torch

from ._core import (_DTYPES, _IO_DTYPES, DTYPE_FP32, _bind, _check, _d, _finite, _i, _lib, _plan_query, _require_cuda_f32, _stream, _vp,
                    dtype_code)


class _HeadsPlan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("vector_elems", "channel_splits", "tiles", "grid_x", "block", "lds_bytes", "channel_block",
                                  "reserved")]


_bind("rroi_heads_forward_hip", [_i] + [_vp] * 10 + [_i] * 4 + [_d, _vp])
_bind("rroi_gate_forward_hip", [_i] + [_vp] * 4 + [_i] * 4 + [_vp])
_bind("rroi_heads_plan", [_i] * 6 + [ctypes.POINTER(_HeadsPlan)])

HeadsPlan = collections.namedtuple("HeadsPlan", [n for n, _ in _HeadsPlan._fields_[:-1]])


def heads_plan(batch_size, channels, height, width, outputs=7, dtype=DTYPE_FP32) -> HeadsPlan:
    """What `heads` (outputs=7) or `gate` (outputs=1) launches for a map of this shape (host only, no GPU needed: 256 CUs
    are assumed without one): pixels per lane V, channel splits S, tiles per image, grid, block, LDS bytes, channels per
    wave.  ValueError where the call would refuse the arguments."""
    return _plan_query(_lib.rroi_heads_plan, _HeadsPlan, HeadsPlan, "rroi_heads_plan",
                       (dtype_code(dtype), outputs, batch_size, channels, height, width))


def _require_pointwise(x, pairs):
    """The checks `heads` and `gate` share: x (N,C,H,W); every (name, weight, bias, k): weight (k,C) or (k,C,1,1), bias
    (k,) or None, of x's dtype and device.  Returns the contiguous (weight, bias) pairs."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,C,H,W), got {tuple(x.shape)}")
    C = x.size(1)
    for name, w, b, k in pairs:
        if not isinstance(w, torch.Tensor) or not (b is None or isinstance(b, torch.Tensor)):
            raise TypeError(f"{name}: weight must be a torch.Tensor, bias a torch.Tensor or None")
        if tuple(w.shape) not in ((k, C), (k, C, 1, 1)):
            raise ValueError(f"{name}: weight must be {(k, C)} or {(k, C, 1, 1)} for x {tuple(x.shape)}, got {tuple(w.shape)}")
        if b is not None and tuple(b.shape) != (k,):
            raise ValueError(f"{name}: bias must be {(k,)}, got {tuple(b.shape)}")
        for t in (w, b):
            if t is not None and t.dtype != x.dtype:
                raise ValueError(f"{name}: x and the parameters must have one dtype, got {x.dtype} and {t.dtype}")
    _require_cuda_f32(x, "x", _IO_DTYPES)
    out = []
    for name, w, b, k in pairs:
        for t in (w, b):
            if t is not None:
                _require_cuda_f32(t, name, _IO_DTYPES)
                if t.device != x.device:
                    raise ValueError(f"{name}: x and the parameters must be on the same device")
        out.append((w.contiguous(), None if b is None else b.contiguous()))
    if C < 1 or x.size(2) < 1 or x.size(3) < 1:
        raise ValueError(f"x must have at least one channel, row and column, got {tuple(x.shape)}")
    return out


def heads(x: torch.Tensor, w_score, b_score, w_rbox, b_rbox, w_angle, b_angle, rbox_scale: float = 128.0):
    """The three detection heads of (N,C,H,W) `x` in one launch: 1x1 convolutions to 1 / 4 / 2 channels
    (weights (k,C) or (k,C,1,1), biases (k,) or None), sigmoid, then score = s, rbox = rbox_scale * s, angle = (2 s - 1)
    normalised to unit length.  -> (score (N,1,H,W), rbox (N,4,H,W), angle (N,2,H,W)) of x's dtype (float32, bfloat16 or
    float16).  x is made NCHW-contiguous.  Sums and epilogue in double in a fixed order, one rounding to fp32 and one to
    the tensor's type: the same bits on every run.  Forward only (no autograd).  ValueError for mismatched shapes or
    dtypes, RuntimeError for CPU tensors."""
    rbox_scale = _finite(rbox_scale, "rbox_scale")
    (ws, bs), (wr, br), (wa, ba) = _require_pointwise(x, (("score", w_score, b_score, 1), ("rbox", w_rbox, b_rbox, 4),
                                                         ("angle", w_angle, b_angle, 2)))
    return _heads_run(x.contiguous(), ws, bs, wr, br, wa, ba, rbox_scale)


def _heads_run(x, w_score, b_score, w_rbox, b_rbox, w_angle, b_angle, rbox_scale: float = 128.0):
    """The call itself, for arguments already checked (heads above; fots_e2e.native after heads_ok): x is a contiguous CUDA
    (N,C,H,W) tensor, the parameters contiguous, of its dtype and device, a bias or None."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _heads_run(x, w_score, b_score, w_rbox, b_rbox, w_angle, b_angle, rbox_scale)
    N, C, H, W = x.shape
    score = torch.empty((N, 1, H, W), dtype=x.dtype, device=x.device)
    rbox = torch.empty((N, 4, H, W), dtype=x.dtype, device=x.device)
    angle = torch.empty((N, 2, H, W), dtype=x.dtype, device=x.device)
    if N == 0:
        return score, rbox, angle
    st = _lib.rroi_heads_forward_hip(_DTYPES[x.dtype], x.data_ptr(), w_score.data_ptr(),
                                     None if b_score is None else b_score.data_ptr(), w_rbox.data_ptr(),
                                     None if b_rbox is None else b_rbox.data_ptr(), w_angle.data_ptr(),
                                     None if b_angle is None else b_angle.data_ptr(), score.data_ptr(), rbox.data_ptr(),
                                     angle.data_ptr(), N, C, H, W, rbox_scale, _stream())
    if st != 1:
        _check(st, "rroi_heads_forward_hip")
    return score, rbox, angle


def gate(x: torch.Tensor, w, b) -> torch.Tensor:
    """sigmoid of a 1x1 convolution of (N,C,H,W) `x` to one channel, in one launch: w (1,C) or (1,C,1,1), b
    (1,) or None -> (N,1,H,W).  The terms of `heads`."""
    ((w, b),) = _require_pointwise(x, (("gate", w, b, 1),))
    return _gate_run(x.contiguous(), w, b)


def _gate_run(x, w, b):
    """The call itself, for arguments already checked (gate above; fots_e2e.native after heads_ok)."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _gate_run(x, w, b)
    N, C, H, W = x.shape
    y = torch.empty((N, 1, H, W), dtype=x.dtype, device=x.device)
    if N == 0:
        return y
    st = _lib.rroi_gate_forward_hip(_DTYPES[x.dtype], x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(),
                                    y.data_ptr(), N, C, H, W, _stream())
    if st != 1:
        _check(st, "rroi_gate_forward_hip")
    return y
