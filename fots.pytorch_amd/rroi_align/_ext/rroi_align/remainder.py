"""rroi_align._ext.rroi_align.remainder -- the bindings of the two kernels that take the last stock operators out of a
16-bit pass of FOTSNet: the recogniser's (2,3) convolution on the matrix cores (header section 12) and the
bilinear resize fused with the depthwise 3x3 behind it (header section 13).

A submodule of its own: the package's `_*_run` callables are a closed list that the network's ledger test reads, so the
hot calls here are `run_conv2x3` and `run_up_depthwise3x3`.  It shares the package's library handle, status check, stream
and dtype table."""
import collections
import ctypes

import torch

from . import _check, _lib, _stream, dtype_code, DTYPE_BF16, _CONV_DTYPES, _DTYPES, _IO_DTYPES, _require_cuda_f32

_i, _f, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p


class _Conv2x3Plan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("tile_m", "tile_w", "wave_items", "k_chunk", "k_chunks", "m_tiles", "x_tiles", "items",
                                  "grid_x", "block", "lds_bytes", "out_h", "out_w", "reserved")]


_lib.rroi_conv2x3_forward_hip.restype = _i
_lib.rroi_conv2x3_forward_hip.argtypes = [_i, _vp, _vp, _vp] + [_i] * 5 + [_f, _vp]
_lib.rroi_conv2x3_plan.restype = _i
_lib.rroi_conv2x3_plan.argtypes = [_i] * 6 + [ctypes.POINTER(_Conv2x3Plan)]
_lib.rroi_up_depthwise3x3_forward_hip.restype = _i
_lib.rroi_up_depthwise3x3_forward_hip.argtypes = [_i, _vp, _vp, _vp] + [_i] * 6 + [_vp]

# --------------------------------------------------------------------------- the (2,3) convolution (header section 12)
Conv2x3Plan = collections.namedtuple("Conv2x3Plan", [n for n, _ in _Conv2x3Plan._fields_[:-1]])


def conv2x3_plan(batch_size, in_channels, out_channels, height, width, dtype=DTYPE_BF16) -> Conv2x3Plan:
    """What `conv2x3` launches for an x of (batch_size, in_channels, height, width) and `out_channels` filters (host only,
    no GPU needed): the tile (output channels, columns), the items per workgroup, the K chunk and their number, the tiles
    along Cout and W, the item count, grid, block, LDS bytes and the output's size.  ValueError where the call would
    refuse the arguments (float32 and height < 2 among them)."""
    p = _Conv2x3Plan()
    if _lib.rroi_conv2x3_plan(dtype_code(dtype), int(batch_size), int(in_channels), int(out_channels), int(height), int(width),
                              ctypes.byref(p)) != 1:
        raise ValueError("rroi_conv2x3_plan: the call would refuse these arguments")
    return Conv2x3Plan(*(getattr(p, n) for n in Conv2x3Plan._fields))


def conv2x3(x: torch.Tensor, weight: torch.Tensor, negative_slope: float = 1.0, out=None) -> torch.Tensor:
    """(N,Cin,H,W) x (Cout,Cin,2,3) -> (N,Cout,H-1,W): act(conv2d(x, weight, stride=1, padding=(0,1))) on the matrix cores
    in one launch.  bfloat16 or float16, x and weight alike, both NCHW-contiguous (a non-contiguous tensor is
    refused, not copied); no bias; H >= 2.  act is a leaky ReLU of `negative_slope`: 1.0 none, 0.0 a ReLU.  fp32
    accumulation in a fixed order (the same bits on every run), one rounding to the tensors' type after the activation.
    out: a contiguous tensor of the result's shape, dtype and device to write into.  Forward only (no autograd).
    ValueError for mismatched shapes, dtypes or layouts, TypeError for float32, RuntimeError for CPU tensors."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor):
        raise TypeError("x and weight must be torch.Tensors")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,Cin,H,W), got {tuple(x.shape)}")
    N, C, H, W = x.shape
    if weight.dim() != 4 or weight.size(1) != C or tuple(weight.shape[2:]) != (2, 3):
        raise ValueError(f"weight must be (Cout, {C}, 2, 3) for x {tuple(x.shape)}, got {tuple(weight.shape)}")
    if weight.dtype != x.dtype:
        raise ValueError(f"x and weight must have one dtype, got {x.dtype} and {weight.dtype}")
    negative_slope = float(negative_slope)
    if negative_slope != negative_slope or negative_slope in (float("inf"), float("-inf")):
        raise ValueError(f"negative_slope must be finite, got {negative_slope!r}")
    _require_cuda_f32(x, "x", _CONV_DTYPES)
    _require_cuda_f32(weight, "weight", _CONV_DTYPES)
    if weight.device != x.device:
        raise ValueError("x and weight must be on the same device")
    if C < 1 or H < 2 or W < 1 or weight.size(0) < 1:
        raise ValueError(f"x must have at least one channel, two rows and one column, got {tuple(x.shape)}, {tuple(weight.shape)}")
    if not x.is_contiguous() or not weight.is_contiguous():
        raise ValueError("x and weight must be NCHW-contiguous")
    if out is not None:
        shape = (N, weight.size(0), H - 1, W)
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != x.dtype or out.device != x.device
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous {shape} tensor of x's dtype and device")
    return run_conv2x3(x, weight, negative_slope, out)


def run_conv2x3(x: torch.Tensor, weight: torch.Tensor, negative_slope: float = 1.0, out=None) -> torch.Tensor:
    """The call itself, for arguments already checked (conv2x3 above; fots_e2e.native_remainder after conv2x3_ok):
    contiguous CUDA tensors of one 16-bit dtype and device, x (N,Cin,H,W) with H >= 2, weight (Cout,Cin,2,3)."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_conv2x3(x, weight, negative_slope, out)
    N, C, H, W = x.shape
    K = weight.size(0)
    if out is None:
        out = torch.empty((N, K, H - 1, W), dtype=x.dtype, device=x.device)
    if N == 0:
        return out
    st = _lib.rroi_conv2x3_forward_hip(_DTYPES[x.dtype], x.data_ptr(), weight.data_ptr(), out.data_ptr(), N, C, K, H, W,
                                       negative_slope, _stream())
    if st != 1:
        _check(st, "rroi_conv2x3_forward_hip")
    return out


# --------------------------------------------------------------------------- resize + depthwise 3x3 (header section 13)
def up_depthwise3x3(a: torch.Tensor, weight: torch.Tensor, size) -> torch.Tensor:
    """(N,C,h,w) x (C,1,3,3) -> (N,C,Ho,Wo), size = (Ho, Wo): the depthwise 3x3 convolution (padding 1, stride 1, no bias)
    of `a` resized to `size` -- bilinear, align_corners=True, in double, rounded to the tensors' type -- in one launch; the
    resized map is never stored.  float32, bfloat16 or float16, a and weight alike; a is made
    NCHW-contiguous.  Bit for bit what `depthwise3x3` gives on that rounded resized map; a source of the target's size is
    read as it is.  Forward only (no autograd).  ValueError for mismatched shapes or dtypes, RuntimeError for CPU tensors."""
    if not isinstance(a, torch.Tensor) or not isinstance(weight, torch.Tensor):
        raise TypeError("a and weight must be torch.Tensors")
    if a.dim() != 4:
        raise ValueError(f"a must be (N,C,h,w), got {tuple(a.shape)}")
    N, C, h, w = a.shape
    if tuple(weight.shape) != (C, 1, 3, 3):
        raise ValueError(f"weight must be {(C, 1, 3, 3)} for a {tuple(a.shape)}, got {tuple(weight.shape)}")
    if weight.dtype != a.dtype:
        raise ValueError(f"a and weight must have one dtype, got {a.dtype} and {weight.dtype}")
    try:
        Ho, Wo = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (Ho, Wo), got {size!r}") from None
    if Ho < 1 or Wo < 1:
        raise ValueError(f"size must be at least (1, 1), got {size!r}")
    _require_cuda_f32(a, "a", _IO_DTYPES)
    _require_cuda_f32(weight, "weight", _IO_DTYPES)
    if weight.device != a.device:
        raise ValueError("a and weight must be on the same device")
    if C < 1 or h < 1 or w < 1:
        raise ValueError(f"a must have at least one channel, row and column, got {tuple(a.shape)}")
    if max(a.numel(), N * C * Ho * Wo) >= (1 << 31):
        raise ValueError("a and the result must each have fewer than 2^31 elements")
    return run_up_depthwise3x3(a.contiguous(), weight, (Ho, Wo))


def run_up_depthwise3x3(a: torch.Tensor, weight: torch.Tensor, size) -> torch.Tensor:
    """The call itself, for arguments already checked (up_depthwise3x3 above; fots_e2e.native_remainder after
    up_depthwise_ok): a is a contiguous CUDA (N,C,h,w) tensor, weight (C,1,3,3) of its dtype and device, size (Ho, Wo)."""
    N, C, h, w = a.shape
    weight = weight.contiguous()
    index = a.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_up_depthwise3x3(a, weight, size)
    Ho, Wo = size
    out = torch.empty((N, C, Ho, Wo), dtype=a.dtype, device=a.device)
    if N == 0:
        return out
    st = _lib.rroi_up_depthwise3x3_forward_hip(_DTYPES[a.dtype], a.data_ptr(), weight.data_ptr(), out.data_ptr(), N, C, h, w,
                                               Ho, Wo, _stream())
    if st != 1:
        _check(st, "rroi_up_depthwise3x3_forward_hip")
    return out
