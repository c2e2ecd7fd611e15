"""rroi_align._ext.rroi_align.merge -- the binding of the gated merge of the network's feature merge (header section 8,
DESIGN 5.14; `csrc/rroi_merge_host.h`), and of its backward, the stand-alone resize and the resize's backward (section 8b,
DESIGN 5.26; `csrc/rroi_merge_backward_host.h`)."""
import collections
import ctypes

import torch

from ._core import (_DTYPES, _IO_DTYPES, DTYPE_FP32, _bind, _check, _d, _i, _lib, _ll, _plan_query, _require_cuda_f32,
                    _require_map, _size2, _stream, _sz, _vp, _workspace, dtype_code)


class _MergePlan(ctypes.Structure):
    _fields_ = ([(n, _i) for n in ("vector_elems", "channel_groups", "tiles", "grid_x", "block", "channel_block", "resize_a",
                                   "resize_gate")]
                + [(n, _d) for n in ("a_scale_y", "a_scale_x", "gate_scale_y", "gate_scale_x")])


_bind("rroi_merge_forward_hip", [_i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp])
_bind("rroi_merge_plan", [_i] * 10 + [ctypes.POINTER(_MergePlan)])

MergePlan = collections.namedtuple("MergePlan", [n for n, _ in _MergePlan._fields_])


def merge_plan(batch_size, channels, height, width, a_size=None, gate_size=None, dtype=DTYPE_FP32) -> MergePlan:
    """What `gated_merge` launches for an `f` of this shape, an `a` of spatial size `a_size` (None: f's) and a gate of
    `gate_size` (None: no gate) (host only, no GPU needed: 256 CUs are assumed without one): pixels per lane V, channel
    groups K, tiles per image, grid, block, channels per group, whether each source is resized, and the four scales.
    ValueError where the call would refuse the arguments."""
    a_h, a_w = (height, width) if a_size is None else a_size
    g_h, g_w = (1, 1) if gate_size is None else gate_size
    return _plan_query(_lib.rroi_merge_plan, _MergePlan, MergePlan, "rroi_merge_plan",
                       (dtype_code(dtype), batch_size, channels, height, width, a_h, a_w, g_h, g_w,
                        0 if gate_size is None else 1))


def gated_merge(a: torch.Tensor, f: torch.Tensor, gate=None) -> torch.Tensor:
    """y = A + f * G in one launch: `a` (N,C,a_h,a_w) and the one-channel `gate` (N,1,g_h,g_w) are resized
    to f's (H,W) -- bilinear, align_corners=True, in double -- and a source of f's size is read as it is; gate=None:
    y = A + f.  -> (N,C,H,W) of f's dtype (float32, bfloat16 or float16).  The tensors are made NCHW-contiguous.  Every
    operation rounds once to double in a fixed order, one rounding to fp32 and one to the tensor's type: a float64
    restatement gives the same bits.  Forward only (no autograd).  ValueError for mismatched shapes or dtypes, RuntimeError
    for CPU tensors."""
    for name, t in (("a", a), ("f", f)) + ((("gate", gate),) if gate is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dim() != 4:
            raise ValueError(f"{name} must be 4-D (N,C,H,W), got {tuple(t.shape)}")
        if t.dtype != f.dtype:
            raise ValueError(f"a, f and the gate must have one dtype, got {f.dtype} and {t.dtype} ({name})")
    if a.shape[:2] != f.shape[:2]:
        raise ValueError(f"a and f must agree in batch size and channels, got {tuple(a.shape)} and {tuple(f.shape)}")
    if gate is not None and (gate.size(0) != f.size(0) or gate.size(1) != 1):
        raise ValueError(f"the gate must be (N,1,h,w) with f's batch size, got {tuple(gate.shape)} for f {tuple(f.shape)}")
    for name, t in (("f", f), ("a", a)) + ((("gate", gate),) if gate is not None else ()):
        _require_cuda_f32(t, name, _IO_DTYPES)
        if t.device != f.device:
            raise ValueError(f"{name}: a, f and the gate must be on the same device")
    if f.size(0) > 0 and min(f.shape[1:] + a.shape[2:] + (gate.shape[2:] if gate is not None else ())) < 1:
        raise ValueError("every tensor must have at least one channel, row and column")
    return _gated_merge_run(a.contiguous(), f.contiguous(), None if gate is None else gate.contiguous())


def _gated_merge_run(a, f, gate=None):
    """The call itself, for arguments already checked (gated_merge above; fots_e2e.native after merge_ok): contiguous CUDA
    tensors of one dtype and device, a (N,C,a_h,a_w), f (N,C,H,W), gate (N,1,g_h,g_w) or None."""
    index = f.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _gated_merge_run(a, f, gate)
    N, C, H, W = f.shape
    y = torch.empty((N, C, H, W), dtype=f.dtype, device=f.device)
    if N == 0:
        return y
    g_h, g_w = (1, 1) if gate is None else gate.shape[2:]
    st = _lib.rroi_merge_forward_hip(_DTYPES[f.dtype], a.data_ptr(), a.size(2), a.size(3),
                                     None if gate is None else gate.data_ptr(), g_h, g_w, f.data_ptr(), y.data_ptr(),
                                     N, C, H, W, _stream())
    if st != 1:
        _check(st, "rroi_merge_forward_hip")
    return y


# --------------------------------------------------------------------------- backward (header section 8b)
class _ResizeBwdPlan(ctypes.Structure):
    _fields_ = ([(n, _i) for n in ("vector_elems", "channel_groups", "tiles", "grid_x", "block", "channel_block", "identity",
                                   "max_rows", "max_cols")]
                + [(n, _d) for n in ("scale_y", "scale_x")])


class _MergeBwdPlan(ctypes.Structure):
    _fields_ = ([(n, _i) for n in ("vector_elems", "channel_groups", "tiles", "grid_x", "block", "channel_block", "gate_tiles",
                                   "gate_grid_x", "resize_gate", "launches")]
                + [("workspace_bytes", _ll)] + [(n, _d) for n in ("gate_scale_y", "gate_scale_x")])


_bind("rroi_resize_forward_hip", [_i, _vp, _vp] + [_i] * 6 + [_vp])
_bind("rroi_resize_backward_hip", [_i, _vp, _vp] + [_i] * 6 + [_vp])
_bind("rroi_resize_footprint", [_i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)])
_bind("rroi_resize_backward_plan", [_i] * 7 + [ctypes.POINTER(_ResizeBwdPlan)])
_bind("rroi_merge_backward_hip", [_i, _vp, _vp, _vp, _vp, _vp] + [_i] * 6 + [_vp, _sz, _vp])
_bind("rroi_merge_backward_workspace_bytes", [_i] * 7, _sz)
_bind("rroi_merge_backward_plan", [_i] * 8 + [ctypes.POINTER(_MergeBwdPlan)])

ResizeBackwardPlan = collections.namedtuple("ResizeBackwardPlan", [n for n, _ in _ResizeBwdPlan._fields_])
MergeBackwardPlan = collections.namedtuple("MergeBackwardPlan", [n for n, _ in _MergeBwdPlan._fields_])


def resize_footprint(n_in: int, n_out: int, i: int):
    """(lo, hi): the output indices lo .. hi - 1 of an axis resized from `n_in` to `n_out` elements (bilinear,
    align_corners=True, header section 8) whose taps reach source index `i` -- the rows `resize_bilinear_backward` sums for
    it.  Host only.  ValueError for a size below 1 or an `i` outside the source."""
    lo, hi = _i(), _i()
    if _lib.rroi_resize_footprint(int(n_in), int(n_out), int(i), ctypes.byref(lo), ctypes.byref(hi)) != 1:
        raise ValueError(f"rroi_resize_footprint: invalid argument ({n_in}, {n_out}, {i})")
    return lo.value, hi.value


def resize_backward_plan(batch_size, channels, in_size, size, dtype=DTYPE_FP32) -> ResizeBackwardPlan:
    """What `resize_bilinear_backward` launches for a dy of (N,C,*size) and a dx of (N,C,*in_size) (host only, no GPU
    needed: 256 CUs are assumed without one).  ValueError where the call would refuse the arguments."""
    return _plan_query(_lib.rroi_resize_backward_plan, _ResizeBwdPlan, ResizeBackwardPlan, "rroi_resize_backward_plan",
                       (dtype_code(dtype), batch_size, channels, in_size[0], in_size[1], size[0], size[1]))


def merge_backward_plan(batch_size, channels, height, width, gate_size=None, dtype=DTYPE_FP32) -> MergeBackwardPlan:
    """What `gated_merge_backward` launches for an `f` of this shape and a gate of `gate_size` (None: no gate, df only)
    (host only, no GPU needed; the same on every device).  ValueError where the call would refuse the arguments."""
    g_h, g_w = (1, 1) if gate_size is None else gate_size
    return _plan_query(_lib.rroi_merge_backward_plan, _MergeBwdPlan, MergeBackwardPlan, "rroi_merge_backward_plan",
                       (dtype_code(dtype), batch_size, channels, height, width, g_h, g_w, 0 if gate_size is None else 1))


def merge_backward_workspace_bytes(batch_size, channels, height, width, gate_size, dtype=DTYPE_FP32) -> int:
    """Bytes of workspace `rroi_merge_backward_hip` needs for dgate at this shape; 0 for a shape the call would refuse."""
    return int(_lib.rroi_merge_backward_workspace_bytes(dtype_code(dtype), int(batch_size), int(channels), int(height),
                                                        int(width), int(gate_size[0]), int(gate_size[1])))


def resize_bilinear(x: torch.Tensor, size) -> torch.Tensor:
    """(N,C,h,w) -> (N,C,*size): the resize of `gated_merge` on its own (bilinear, align_corners=True, in double, rounded to
    fp32 once and then to x's type): bit for bit what `gated_merge` adds as `a`.  An x of that size is copied.  x is made
    NCHW-contiguous.  Forward only (no autograd: `rroi_align.merge.bilinear_resize`).  ValueError for a bad shape or size,
    TypeError / RuntimeError as `gated_merge`."""
    _require_map(x, "x")
    return run_resize_bilinear(x.contiguous(), *_size2(size, "size"))


def run_resize_bilinear(x, H: int, W: int):
    """The call itself, for arguments already checked: x a contiguous CUDA (N,C,h,w) tensor, H, W >= 1."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_resize_bilinear(x, H, W)
    N, C, h, w = x.shape
    y = torch.empty((N, C, H, W), dtype=x.dtype, device=x.device)
    if N == 0:
        return y
    st = _lib.rroi_resize_forward_hip(_DTYPES[x.dtype], x.data_ptr(), y.data_ptr(), N, C, h, w, H, W, _stream())
    if st != 1:
        _check(st, "rroi_resize_forward_hip")
    return y


def resize_bilinear_backward(dy: torch.Tensor, in_size) -> torch.Tensor:
    """The backward of `resize_bilinear` -- DESIGN 5.26: dy (N,C,H,W) -> dx (N,C,*in_size), the transpose of the resize as
    a gather: every element the double sum of its taps in a fixed order (rows ascending, columns ascending within a row),
    rounded once; no atomic, the same bits on every run.  dy is made NCHW-contiguous.  ValueError for a bad shape or size
    (a resize in which more than 4096 output rows or columns meet in one source element is refused), TypeError /
    RuntimeError as `gated_merge`."""
    _require_map(dy, "dy")
    return run_resize_bilinear_backward(dy.contiguous(), *_size2(in_size, "in_size"))


def run_resize_bilinear_backward(dy, h: int, w: int):
    """The call itself, for arguments already checked: dy a contiguous CUDA (N,C,H,W) tensor, h, w >= 1."""
    index = dy.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_resize_bilinear_backward(dy, h, w)
    N, C, H, W = dy.shape
    dx = torch.empty((N, C, h, w), dtype=dy.dtype, device=dy.device)
    if N == 0:
        return dx
    st = _lib.rroi_resize_backward_hip(_DTYPES[dy.dtype], dy.data_ptr(), dx.data_ptr(), N, C, h, w, H, W, _stream())
    if st != 1:
        _check(st, "rroi_resize_backward_hip")
    return dx


def gated_merge_backward(dy: torch.Tensor, f: torch.Tensor, gate=None, need_df: bool = True, need_dgate: bool = True):
    """The backward of `gated_merge` in f and the gate -- DESIGN 5.26: -> (df, dgate), each None where it was not asked
    for.  dy and f are (N,C,H,W), the gate (N,1,g_h,g_w) or None (then dgate is not computed and df is dy's values).
    df = dy * G with G recomputed as the forward computes it, bit for bit a float64 restatement; dgate is the transposed
    resize of the per-pixel double sum of dy * f over the channels, summed in an order the shape alone fixes, no atomic,
    rounded once: the same bits on every run and device.  (da is dy, or `resize_bilinear_backward(dy, a's size)`.)  The
    tensors are made NCHW-contiguous.  ValueError for mismatched shapes, dtypes or devices and for a call that asks for no
    gradient, TypeError / RuntimeError as `gated_merge`."""
    _require_map(f, "f")
    _require_map(dy, "dy", f, "f")
    if dy.shape != f.shape:
        raise ValueError(f"dy and f must have one shape, got {tuple(dy.shape)} and {tuple(f.shape)}")
    if gate is not None:
        _require_map(gate, "gate", f, "f")
        if gate.size(0) != f.size(0) or gate.size(1) != 1:
            raise ValueError(f"the gate must be (N,1,h,w) with f's batch size, got {tuple(gate.shape)} for f {tuple(f.shape)}")
    need_df, need_dgate = bool(need_df), bool(need_dgate) and gate is not None
    if not need_df and not need_dgate:
        raise ValueError("no gradient is asked for")
    return run_gated_merge_backward(dy.contiguous(), f.contiguous(), None if gate is None else gate.contiguous(), need_df,
                                    need_dgate)


def run_gated_merge_backward(dy, f, gate, need_df: bool, need_dgate: bool):
    """The call itself, for arguments already checked (gated_merge_backward above; rroi_align.merge): contiguous CUDA
    tensors of one dtype and device, dy and f (N,C,H,W), gate (N,1,g_h,g_w) or None (then need_dgate is False), at least one
    of the two flags.  The workspace comes from the per-stream scratch (`_core._workspace`)."""
    index = f.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_gated_merge_backward(dy, f, gate, need_df, need_dgate)
    N, C, H, W = f.shape
    df = torch.empty_like(f) if need_df else None
    dg = torch.empty_like(gate) if need_dgate else None
    if N == 0:
        return df, dg
    g_h, g_w = (1, 1) if gate is None else gate.shape[2:]
    ws, nbytes = None, 0
    if need_dgate:
        nbytes = _lib.rroi_merge_backward_workspace_bytes(_DTYPES[f.dtype], N, C, H, W, g_h, g_w)
        ws = _workspace(f.device, nbytes)
    st = _lib.rroi_merge_backward_hip(_DTYPES[f.dtype], dy.data_ptr(), f.data_ptr(), None if gate is None else gate.data_ptr(),
                                      None if df is None else df.data_ptr(), None if dg is None else dg.data_ptr(), N, C, H, W,
                                      g_h, g_w, None if ws is None else ws.data_ptr(), nbytes, _stream())
    if st != 1:
        _check(st, "rroi_merge_backward_hip")
    return df, dg
