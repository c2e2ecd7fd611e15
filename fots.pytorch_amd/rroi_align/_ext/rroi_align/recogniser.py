"""rroi_align._ext.rroi_align.recogniser -- the binding of the recogniser's head (1x1 convolution + log-softmax) and of its
activation + (2,1) max pool (header section 10; `csrc/rroi_recogniser_host.h`)."""
import collections
import ctypes

import torch

from ._core import (_DTYPES, _IO_DTYPES, DTYPE_FP32, _bind, _check, _f, _finite, _i, _lib, _plan_query, _require_cuda_f32, _require_out,
                    _stream, _vp, dtype_code)


class _OcrHeadPlan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("class_block", "waves", "tile_columns", "tiles", "grid_x", "block", "lds_bytes", "max_classes")]


_bind("rroi_ocr_head_forward_hip", [_i, _vp, _vp, _vp, _vp] + [_i] * 4 + [_vp])
_bind("rroi_ocr_head_plan", [_i] * 5 + [ctypes.POINTER(_OcrHeadPlan)])
_bind("rroi_act_maxpool2x1_forward_hip", [_i, _vp, _vp] + [_i] * 4 + [_f, _vp])
OCR_HEAD_MAX_CLASSES = 128

OcrHeadPlan = collections.namedtuple("OcrHeadPlan", [n for n, _ in _OcrHeadPlan._fields_])


def ocr_head_plan(batch_size, channels, classes, steps, dtype=DTYPE_FP32) -> OcrHeadPlan:
    """What `ocr_head` launches for an x of (batch_size, channels, steps) and `classes` rows of weights (host only, no GPU
    needed): classes per wave, waves per workgroup, columns per tile, tiles per crop, grid, block, LDS bytes and the limit on
    `classes`.  ValueError where the call would refuse the arguments (more classes than the limit among them)."""
    return _plan_query(_lib.rroi_ocr_head_plan, _OcrHeadPlan, OcrHeadPlan, "rroi_ocr_head_plan",
                       (dtype_code(dtype), batch_size, channels, classes, steps))


def ocr_head(x: torch.Tensor, weight: torch.Tensor, bias=None, out=None) -> torch.Tensor:
    """(N,C,T) or (N,C,1,T) x, (K,C) or (K,C,1,1) weight, (K,) bias or None -> (N,K,T):
    log_softmax(conv1x1(x) + bias, dim=1) in one launch.  float32, bfloat16 or float16, all tensors alike and
    contiguous (a non-contiguous tensor is refused, not copied); K <= OCR_HEAD_MAX_CLASSES.  Logits, maximum, sum and
    logarithm in double in a fixed order, one rounding to fp32 and one to the tensors' type: the same bits on every run.
    out: a contiguous (N,K,T) tensor of x's dtype and device to write into.  Forward only (no autograd).  ValueError for
    mismatched shapes, dtypes or layouts, RuntimeError for CPU tensors."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor) or not (bias is None or isinstance(bias, torch.Tensor)):
        raise TypeError("x and weight must be torch.Tensors, bias a torch.Tensor or None")
    if x.dim() not in (3, 4) or (x.dim() == 4 and x.size(2) != 1):
        raise ValueError(f"x must be (N,C,T) or (N,C,1,T), got {tuple(x.shape)}")
    N, C, T = x.size(0), x.size(1), x.size(-1)
    K = weight.size(0) if weight.dim() > 0 else 0
    if tuple(weight.shape) not in ((K, C), (K, C, 1, 1)):
        raise ValueError(f"weight must be (K, {C}) or (K, {C}, 1, 1) for x {tuple(x.shape)}, got {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (K,):
        raise ValueError(f"bias must be {(K,)}, got {tuple(bias.shape)}")
    for t in (weight, bias):
        if t is not None and t.dtype != x.dtype:
            raise ValueError(f"x and the parameters must have one dtype, got {x.dtype} and {t.dtype}")
    if not 1 <= K <= OCR_HEAD_MAX_CLASSES:
        raise ValueError(f"the head takes 1 to {OCR_HEAD_MAX_CLASSES} classes, got {K}")
    _require_cuda_f32(x, "x", _IO_DTYPES)
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None:
            _require_cuda_f32(t, name, _IO_DTYPES)
            if t.device != x.device:
                raise ValueError(f"{name}: x and the parameters must be on the same device")
    if C < 1 or T < 1:
        raise ValueError(f"x must have at least one channel and column, got {tuple(x.shape)}")
    if not x.is_contiguous() or not weight.is_contiguous() or not (bias is None or bias.is_contiguous()):
        raise ValueError("x, weight and bias must be contiguous")
    if out is not None:
        _require_out(out, (N, K, T), x)
    return _ocr_head_run(x, weight, bias, out)


def _ocr_head_run(x: torch.Tensor, weight: torch.Tensor, bias=None, out=None) -> torch.Tensor:
    """The call itself, for arguments already checked (ocr_head above; fots_e2e.native after ocr_head_ok): contiguous CUDA
    tensors of one dtype and device, x (N,C,T) or (N,C,1,T), weight (K,C) or (K,C,1,1), bias (K,) or None."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _ocr_head_run(x, weight, bias, out)
    N, C, T = x.size(0), x.size(1), x.size(-1)
    K = weight.size(0)
    if out is None:
        out = torch.empty((N, K, T), dtype=x.dtype, device=x.device)
    if N == 0:
        return out
    st = _lib.rroi_ocr_head_forward_hip(_DTYPES[x.dtype], x.data_ptr(), weight.data_ptr(),
                                        None if bias is None else bias.data_ptr(), out.data_ptr(), N, C, K, T, _stream())
    if st != 1:
        _check(st, "rroi_ocr_head_forward_hip")
    return out


def act_maxpool2x1(x: torch.Tensor, negative_slope: float = 1.0) -> torch.Tensor:
    """(N,C,H,W) -> (N,C,H//2,W): `F.max_pool2d(F.leaky_relu(x, negative_slope), (2, 1), stride=(2, 1))` in one launch, bit
    for bit; negative_slope = 1.0 is the plain pool.  float32, bfloat16 or float16, NCHW-contiguous (a
    non-contiguous tensor is refused, not copied), H >= 2; an odd last row is dropped.  Forward only (no autograd).
    ValueError for a wrong shape or layout, RuntimeError for CPU tensors."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,C,H,W), got {tuple(x.shape)}")
    negative_slope = _finite(negative_slope, "negative_slope")
    if x.size(2) < 2:
        raise ValueError(f"x must have at least two rows, got {tuple(x.shape)}")
    _require_cuda_f32(x, "x", _IO_DTYPES)
    if x.size(1) < 1 or x.size(3) < 1:
        raise ValueError(f"x must have at least one channel and column, got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError("x must be NCHW-contiguous")
    return _act_maxpool2x1_run(x, negative_slope)


def _act_maxpool2x1_run(x: torch.Tensor, negative_slope: float = 1.0) -> torch.Tensor:
    """The call itself, for arguments already checked (act_maxpool2x1 above; fots_e2e.native after act_pool_ok): a contiguous
    CUDA (N,C,H,W) tensor with H >= 2."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _act_maxpool2x1_run(x, negative_slope)
    N, C, H, W = x.shape
    out = torch.empty((N, C, H // 2, W), dtype=x.dtype, device=x.device)
    if N == 0:
        return out
    st = _lib.rroi_act_maxpool2x1_forward_hip(_DTYPES[x.dtype], x.data_ptr(), out.data_ptr(), N, C, H, W, negative_slope,
                                              _stream())
    if st != 1:
        _check(st, "rroi_act_maxpool2x1_forward_hip")
    return out
