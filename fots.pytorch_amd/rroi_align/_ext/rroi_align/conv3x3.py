"""rroi_align._ext.rroi_align.conv3x3 -- the binding of the network's dense 3x3 convolution on the matrix cores (header
section 9; `csrc/rroi_conv3x3_host.h`)."""
import collections
import ctypes

import torch

from ._core import (_CONV_DTYPES, _DTYPES, DTYPE_BF16, _bind, _check, _f, _finite, _i, _lib, _plan_query, _require_cuda_f32, _require_out,
                    _stream, _vp, dtype_code)


class _ConvPlan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("tile_m", "tile_h", "tile_w", "k_chunk", "k_chunks", "m_tiles", "y_tiles", "x_tiles",
                                  "grid_x", "block", "lds_bytes", "out_h", "out_w", "reserved")]


_bind("rroi_conv3x3_forward_hip", [_i, _vp, _vp, _vp] + [_i] * 6 + [_f, _vp])
_bind("rroi_conv3x3_plan", [_i] * 7 + [ctypes.POINTER(_ConvPlan)])

Conv3x3Plan = collections.namedtuple("Conv3x3Plan", [n for n, _ in _ConvPlan._fields_[:-1]])


def conv3x3_plan(batch_size, in_channels, out_channels, height, width, stride=1, dtype=DTYPE_BF16) -> Conv3x3Plan:
    """What `conv3x3` launches for an x of (batch_size, in_channels, height, width) and `out_channels` filters (host only,
    no GPU needed): the tile (output channels, rows, columns), the K chunk and their
    number, tiles per image along each axis, grid, block, LDS bytes and the output's size.  ValueError where the call
    would refuse the arguments (float32 among them)."""
    return _plan_query(_lib.rroi_conv3x3_plan, _ConvPlan, Conv3x3Plan, "rroi_conv3x3_plan",
                       (dtype_code(dtype), batch_size, in_channels, out_channels, height, width, stride))


def conv3x3(x: torch.Tensor, weight: torch.Tensor, stride: int = 1, negative_slope: float = 1.0, out=None) -> torch.Tensor:
    """(N,Cin,H,W) x (Cout,Cin,3,3) -> (N,Cout,Ho,Wo): act(conv2d(x, weight, stride=stride, padding=1)) on the matrix cores
    in one launch.  bfloat16 or float16, x and weight alike, both NCHW-contiguous (a non-contiguous tensor is
    refused, not copied); no bias; stride 1 or 2.  act is a leaky ReLU of `negative_slope`: 1.0 none, 0.0 a ReLU.  fp32
    accumulation in a fixed order (the same bits on every run), one rounding to the tensors' type after the activation.
    out: a contiguous tensor of the result's shape, dtype and device to write into.  Forward only (no autograd).
    ValueError for mismatched shapes, dtypes or layouts, TypeError for float32, RuntimeError for CPU tensors."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor):
        raise TypeError("x and weight must be torch.Tensors")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,Cin,H,W), got {tuple(x.shape)}")
    N, C, H, W = x.shape
    if weight.dim() != 4 or weight.size(1) != C or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f"weight must be (Cout, {C}, 3, 3) for x {tuple(x.shape)}, got {tuple(weight.shape)}")
    if weight.dtype != x.dtype:
        raise ValueError(f"x and weight must have one dtype, got {x.dtype} and {weight.dtype}")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2, got {stride!r}")
    negative_slope = _finite(negative_slope, "negative_slope")
    _require_cuda_f32(x, "x", _CONV_DTYPES)
    _require_cuda_f32(weight, "weight", _CONV_DTYPES)
    if weight.device != x.device:
        raise ValueError("x and weight must be on the same device")
    if C < 1 or H < 1 or W < 1 or weight.size(0) < 1:
        raise ValueError(f"x and weight must have at least one channel, row and column, got {tuple(x.shape)}, {tuple(weight.shape)}")
    if not x.is_contiguous() or not weight.is_contiguous():
        raise ValueError("x and weight must be NCHW-contiguous")
    if out is not None:
        _require_out(out, (N, weight.size(0), (H - 1) // stride + 1, (W - 1) // stride + 1), x)
    return _conv3x3_run(x, weight, int(stride), negative_slope, out)


def _conv3x3_run(x: torch.Tensor, weight: torch.Tensor, stride: int, negative_slope: float = 1.0, out=None) -> torch.Tensor:
    """The call itself, for arguments already checked (conv3x3 above; fots_e2e.native after conv3x3_ok): contiguous CUDA
    tensors of one 16-bit dtype and device, x (N,Cin,H,W), weight (Cout,Cin,3,3), stride 1 or 2."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _conv3x3_run(x, weight, stride, negative_slope, out)
    N, C, H, W = x.shape
    K = weight.size(0)
    if out is None:
        out = torch.empty((N, K, (H - 1) // stride + 1, (W - 1) // stride + 1), dtype=x.dtype, device=x.device)
    if N == 0:
        return out
    st = _lib.rroi_conv3x3_forward_hip(_DTYPES[x.dtype], x.data_ptr(), weight.data_ptr(), out.data_ptr(), N, C, K, H, W,
                                       stride, negative_slope, _stream())
    if st != 1:
        _check(st, "rroi_conv3x3_forward_hip")
    return out
