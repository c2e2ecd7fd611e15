"""rroi_align._ext.rroi_align.heads -- the binding of the network's detection heads and attention gate (header section 7,
DESIGN 5.12; `csrc/rroi_heads_host.h`) and of their training forward and backward (section 7b, DESIGN 5.27;
`csrc/rroi_heads_backward_host.h`)."""
import collections
import ctypes

import torch

from ._core import (_DTYPES, _IO_DTYPES, DTYPE_FP32, _bind, _check, _d, _finite, _i, _lib, _ll, _plan_query, _require_cuda_f32,
                    _stream, _sz, _vp, _workspace, dtype_code)


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


# --------------------------------------------------------------------------- training forward and backward (header section 7b)
class _HeadsBwdPlan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("vector_elems", "grid_x", "partial_rows", "tiles_per_workgroup", "block", "lds_bytes",
                                  "launches", "reserved")] + [("pixels_per_workgroup", _ll), ("workspace_bytes", _ll)]


_bind("rroi_heads_forward_train_hip", [_i] + [_vp] * 11 + [_i] * 4 + [_d, _vp])
_bind("rroi_gate_forward_train_hip", [_i] + [_vp] * 5 + [_i] * 4 + [_vp])
_bind("rroi_heads_backward_hip", [_i] + [_vp] * 15 + [_i] * 4 + [_d, _vp, _sz, _vp])
_bind("rroi_gate_backward_hip", [_i] + [_vp] * 7 + [_i] * 4 + [_vp, _sz, _vp])
_bind("rroi_heads_backward_workspace_bytes", [_i] * 5, _sz)
_bind("rroi_heads_backward_plan", [_i] * 6 + [ctypes.POINTER(_HeadsBwdPlan)])

HeadsBackwardPlan = collections.namedtuple("HeadsBackwardPlan", [n for n, _ in _HeadsBwdPlan._fields_ if n != "reserved"])


def heads_backward_plan(batch_size, channels, height, width, outputs=7, dtype=DTYPE_FP32) -> HeadsBackwardPlan:
    """What `heads_backward` (outputs=7) or `gate_backward` (outputs=1) launches for an x of this shape (host only, no GPU
    needed: 256 CUs are assumed without one): pixels per lane, workgroups, partial rows of the workspace, tiles and pixels
    per workgroup, block, LDS bytes, the launches of a call that wants a parameter gradient, the workspace's bytes.
    ValueError where the call would refuse the arguments."""
    return _plan_query(_lib.rroi_heads_backward_plan, _HeadsBwdPlan, HeadsBackwardPlan, "rroi_heads_backward_plan",
                       (dtype_code(dtype), outputs, batch_size, channels, height, width))


def heads_backward_workspace_bytes(batch_size, channels, height, width, outputs=7) -> int:
    """Bytes of workspace the backward needs for a parameter gradient at this shape (one row of outputs * (C + 1) doubles
    per workgroup); 0 for a shape the call would refuse."""
    return int(_lib.rroi_heads_backward_workspace_bytes(int(outputs), int(batch_size), int(channels), int(height), int(width)))


def _ptr(t):
    return None if t is None else t.data_ptr()


def heads_train(x: torch.Tensor, w_score, b_score, w_rbox, b_rbox, w_angle, b_angle, rbox_scale: float = 128.0):
    """`heads` with one more result: -> (score, rbox, angle, z), z (N,7,H,W) float64, the pre-activation sums as the
    kernel forms them, which `heads_backward` takes.  score, rbox and angle have the bits `heads` gives."""
    rbox_scale = _finite(rbox_scale, "rbox_scale")
    (ws, bs), (wr, br), (wa, ba) = _require_pointwise(x, (("score", w_score, b_score, 1), ("rbox", w_rbox, b_rbox, 4),
                                                         ("angle", w_angle, b_angle, 2)))
    return run_heads_train(x.contiguous(), ws, bs, wr, br, wa, ba, rbox_scale)


def run_heads_train(x, w_score, b_score, w_rbox, b_rbox, w_angle, b_angle, rbox_scale: float = 128.0):
    """The call itself, for arguments already checked (heads_train above; rroi_align.heads): as `_heads_run`."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_heads_train(x, w_score, b_score, w_rbox, b_rbox, w_angle, b_angle, rbox_scale)
    N, C, H, W = x.shape
    score = torch.empty((N, 1, H, W), dtype=x.dtype, device=x.device)
    rbox = torch.empty((N, 4, H, W), dtype=x.dtype, device=x.device)
    angle = torch.empty((N, 2, H, W), dtype=x.dtype, device=x.device)
    z = torch.empty((N, 7, H, W), dtype=torch.float64, device=x.device)
    if N == 0:
        return score, rbox, angle, z
    st = _lib.rroi_heads_forward_train_hip(_DTYPES[x.dtype], x.data_ptr(), w_score.data_ptr(), _ptr(b_score), w_rbox.data_ptr(),
                                           _ptr(b_rbox), w_angle.data_ptr(), _ptr(b_angle), score.data_ptr(), rbox.data_ptr(),
                                           angle.data_ptr(), z.data_ptr(), N, C, H, W, rbox_scale, _stream())
    if st != 1:
        _check(st, "rroi_heads_forward_train_hip")
    return score, rbox, angle, z


def gate_train(x: torch.Tensor, w, b):
    """`gate` with one more result: -> (y, z), z (N,1,H,W) float64, which `gate_backward` takes."""
    ((w, b),) = _require_pointwise(x, (("gate", w, b, 1),))
    return run_gate_train(x.contiguous(), w, b)


def run_gate_train(x, w, b):
    """The call itself, for arguments already checked (gate_train above; rroi_align.heads): as `_gate_run`."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_gate_train(x, w, b)
    N, C, H, W = x.shape
    y = torch.empty((N, 1, H, W), dtype=x.dtype, device=x.device)
    z = torch.empty((N, 1, H, W), dtype=torch.float64, device=x.device)
    if N == 0:
        return y, z
    st = _lib.rroi_gate_forward_train_hip(_DTYPES[x.dtype], x.data_ptr(), w.data_ptr(), _ptr(b), y.data_ptr(), z.data_ptr(), N, C,
                                          H, W, _stream())
    if st != 1:
        _check(st, "rroi_gate_forward_train_hip")
    return y, z


def _require_backward(x, z, grads, weights):
    """The checks `heads_backward` and `gate_backward` share.  grads: (name, tensor or None, k); weights: (name, tensor, k).
    -> the contiguous (x, z, grads, weights)."""
    if not isinstance(x, torch.Tensor) or not isinstance(z, torch.Tensor):
        raise TypeError("x and z must be torch.Tensors")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,C,H,W), got {tuple(x.shape)}")
    N, C, H, W = x.shape
    _require_cuda_f32(x, "x", _IO_DTYPES)
    k_all = sum(k for _, _, k in weights)
    if z.dtype != torch.float64 or tuple(z.shape) != (N, k_all, H, W) or z.device != x.device:
        raise ValueError(f"z must be a float64 {(N, k_all, H, W)} tensor on x's device")
    if all(g is None for _, g, _ in grads):
        raise ValueError("no output gradient is given")
    out_g, out_w = [], []
    for name, g, k in grads:
        if g is not None:
            if not isinstance(g, torch.Tensor):
                raise TypeError(f"{name} must be a torch.Tensor or None")
            if tuple(g.shape) != (N, k, H, W) or g.dtype != x.dtype or g.device != x.device:
                raise ValueError(f"{name} must be {(N, k, H, W)} of x's dtype and device, got {tuple(g.shape)} {g.dtype}")
            g = g.contiguous()
        out_g.append(g)
    for name, w, k in weights:
        if not isinstance(w, torch.Tensor):
            raise TypeError(f"{name}: weight must be a torch.Tensor")
        if tuple(w.shape) not in ((k, C), (k, C, 1, 1)) or w.dtype != x.dtype or w.device != x.device:
            raise ValueError(f"{name}: weight must be {(k, C)} or {(k, C, 1, 1)} of x's dtype and device, got {tuple(w.shape)}")
        out_w.append(w.contiguous())
    if C < 1 or H < 1 or W < 1:
        raise ValueError(f"x must have at least one channel, row and column, got {tuple(x.shape)}")
    return x.contiguous(), z.contiguous(), out_g, out_w


def _need(need_dx, need_dweight, need_dbias):
    need = bool(need_dx), bool(need_dweight), bool(need_dbias)
    if not any(need):
        raise ValueError("no gradient is asked for")
    return need


def heads_backward(dscore, drbox, dangle, x, z, w_score, w_rbox, w_angle, rbox_scale: float = 128.0, need_dx: bool = True,
                   need_dweight: bool = True, need_dbias: bool = True):
    """The backward of `heads_train` -- DESIGN 5.27: -> (dx, (dw_score, dw_rbox, dw_angle), (db_score, db_rbox, db_angle)),
    dx None and the tuples of Nones where they were not asked for.  dscore / drbox / dangle: the gradients of the three
    outputs, each or None (zero), not all None; z: what `heads_train` returned.  Every sum in double in a fixed order
    without atomics, one rounding: the same bits on every run.  ValueError for mismatched shapes, dtypes or devices and
    for a call that asks for no gradient."""
    rbox_scale = _finite(rbox_scale, "rbox_scale")
    x, z, g, w = _require_backward(x, z, (("dscore", dscore, 1), ("drbox", drbox, 4), ("dangle", dangle, 2)),
                                   (("score", w_score, 1), ("rbox", w_rbox, 4), ("angle", w_angle, 2)))
    return run_heads_backward(*g, x, z, *w, rbox_scale, *_need(need_dx, need_dweight, need_dbias))


def run_heads_backward(dscore, drbox, dangle, x, z, w_score, w_rbox, w_angle, rbox_scale, need_dx, need_dweight, need_dbias):
    """The call itself, for arguments already checked (heads_backward above; rroi_align.heads): contiguous CUDA tensors
    of one dtype and device (z float64), at least one gradient given and one flag set.  The workspace comes from the
    per-stream scratch (`_core._workspace`)."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_heads_backward(dscore, drbox, dangle, x, z, w_score, w_rbox, w_angle, rbox_scale, need_dx, need_dweight,
                                      need_dbias)
    N, C, H, W = x.shape
    new = lambda *shape: torch.empty(shape, dtype=x.dtype, device=x.device)  # noqa: E731
    dx = torch.empty_like(x) if need_dx else None
    dw = tuple(torch.empty_like(w) for w in (w_score, w_rbox, w_angle)) if need_dweight else (None,) * 3
    db = (new(1), new(4), new(2)) if need_dbias else (None,) * 3
    if N == 0:
        for t in dw + db:
            if t is not None:
                t.zero_()
        return dx, dw, db
    ws, nbytes = None, 0
    if need_dweight or need_dbias:
        nbytes = _lib.rroi_heads_backward_workspace_bytes(7, N, C, H, W)
        ws = _workspace(x.device, nbytes)
    st = _lib.rroi_heads_backward_hip(_DTYPES[x.dtype], _ptr(dscore), _ptr(drbox), _ptr(dangle), x.data_ptr(), z.data_ptr(),
                                      w_score.data_ptr(), w_rbox.data_ptr(), w_angle.data_ptr(), _ptr(dx), _ptr(dw[0]),
                                      _ptr(db[0]), _ptr(dw[1]), _ptr(db[1]), _ptr(dw[2]), _ptr(db[2]), N, C, H, W, rbox_scale,
                                      _ptr(ws), nbytes, _stream())
    if st != 1:
        _check(st, "rroi_heads_backward_hip")
    return dx, dw, db


def gate_backward(dy, x, z, w, need_dx: bool = True, need_dweight: bool = True, need_dbias: bool = True):
    """The backward of `gate_train`: -> (dx, dw, db), each None where it was not asked for.  The terms of `heads_backward`."""
    x, z, (dy,), (w,) = _require_backward(x, z, (("dy", dy, 1),), (("gate", w, 1),))
    return run_gate_backward(dy, x, z, w, *_need(need_dx, need_dweight, need_dbias))


def run_gate_backward(dy, x, z, w, need_dx, need_dweight, need_dbias):
    """The call itself, for arguments already checked (gate_backward above; rroi_align.heads)."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_gate_backward(dy, x, z, w, need_dx, need_dweight, need_dbias)
    N, C, H, W = x.shape
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(w) if need_dweight else None
    db = torch.empty((1,), dtype=x.dtype, device=x.device) if need_dbias else None
    if N == 0:
        for t in (dw, db):
            if t is not None:
                t.zero_()
        return dx, dw, db
    ws, nbytes = None, 0
    if need_dweight or need_dbias:
        nbytes = _lib.rroi_heads_backward_workspace_bytes(1, N, C, H, W)
        ws = _workspace(x.device, nbytes)
    st = _lib.rroi_gate_backward_hip(_DTYPES[x.dtype], dy.data_ptr(), x.data_ptr(), z.data_ptr(), w.data_ptr(), _ptr(dx), _ptr(dw),
                                     _ptr(db), N, C, H, W, _ptr(ws), nbytes, _stream())
    if st != 1:
        _check(st, "rroi_gate_backward_hip")
    return dx, dw, db
