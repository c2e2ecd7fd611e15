"""rroi_align._ext.rroi_align.merge -- the binding of the gated merge of the network's feature merge (header section 8,
DESIGN 5.14; `csrc/rroi_merge_host.h`)."""
import collections
import ctypes

import torch

from ._core import (_DTYPES, _IO_DTYPES, DTYPE_FP32, _bind, _check, _d, _i, _lib, _plan_query, _require_cuda_f32, _stream, _vp,
                    dtype_code)


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
