"""rroi_align._ext.rroi_align.remainder -- the bindings of the two kernels that take the last stock operators out of a
16-bit pass of FOTSNet: the recogniser's (2,3) convolution on the matrix cores (header section 12) and the
bilinear resize fused with the depthwise 3x3 behind it (header section 13).

A module of the binding like the package's own (`csrc/rroi_conv2x3_host.h`, `rroi_updw_host.h`), loaded on first use by
`fots_e2e`: the package's `_*_run` callables are a closed list that the network's ledger test reads, so the hot calls here
are `run_conv2x3` and `run_up_depthwise3x3`."""
import collections
import ctypes

import torch

from ._core import (_CONV_DTYPES, _DTYPES, DTYPE_BF16, _bind, _check, _f, _finite, _i, _lib, _plan_query, _require_cuda_f32,
                    _require_depthwise_device, _require_depthwise_shapes, _require_out, _stream, _vp, dtype_code)


class _Conv2x3Plan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("tile_m", "tile_w", "wave_items", "k_chunk", "k_chunks", "m_tiles", "x_tiles", "items",
                                  "grid_x", "block", "lds_bytes", "out_h", "out_w", "reserved")]


_bind("rroi_conv2x3_forward_hip", [_i, _vp, _vp, _vp] + [_i] * 5 + [_f, _vp])
_bind("rroi_conv2x3_plan", [_i] * 6 + [ctypes.POINTER(_Conv2x3Plan)])
_bind("rroi_up_depthwise3x3_forward_hip", [_i, _vp, _vp, _vp] + [_i] * 6 + [_vp])

# --------------------------------------------------------------------------- the (2,3) convolution (header section 12)
Conv2x3Plan = collections.namedtuple("Conv2x3Plan", [n for n, _ in _Conv2x3Plan._fields_[:-1]])


def conv2x3_plan(batch_size, in_channels, out_channels, height, width, dtype=DTYPE_BF16) -> Conv2x3Plan:
    """What `conv2x3` launches for an x of (batch_size, in_channels, height, width) and `out_channels` filters (host only,
    no GPU needed): the tile (output channels, columns), the items per workgroup, the K chunk and their number, the tiles
    along Cout and W, the item count, grid, block, LDS bytes and the output's size.  ValueError where the call would
    refuse the arguments (float32 and height < 2 among them)."""
    return _plan_query(_lib.rroi_conv2x3_plan, _Conv2x3Plan, Conv2x3Plan, "rroi_conv2x3_plan",
                       (dtype_code(dtype), batch_size, in_channels, out_channels, height, width))


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
    negative_slope = _finite(negative_slope, "negative_slope")
    _require_cuda_f32(x, "x", _CONV_DTYPES)
    _require_cuda_f32(weight, "weight", _CONV_DTYPES)
    if weight.device != x.device:
        raise ValueError("x and weight must be on the same device")
    if C < 1 or H < 2 or W < 1 or weight.size(0) < 1:
        raise ValueError(f"x must have at least one channel, two rows and one column, got {tuple(x.shape)}, {tuple(weight.shape)}")
    if not x.is_contiguous() or not weight.is_contiguous():
        raise ValueError("x and weight must be NCHW-contiguous")
    if out is not None:
        _require_out(out, (N, weight.size(0), H - 1, W), x)
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
    _require_depthwise_shapes(a, weight, "a", "(N,C,h,w)")
    try:
        Ho, Wo = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (Ho, Wo), got {size!r}") from None
    if Ho < 1 or Wo < 1:
        raise ValueError(f"size must be at least (1, 1), got {size!r}")
    _require_depthwise_device(a, weight, "a")
    if max(a.numel(), a.size(0) * a.size(1) * Ho * Wo) >= (1 << 31):
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
