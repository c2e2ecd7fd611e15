"""rroi_align._ext.rroi_align.conv1x1 -- the binding of the network's 1x1 convolution on the matrix cores with a shortcut's
BatchNorm folded in (header section 11; `csrc/rroi_conv1x1_host.h`)."""
import collections
import ctypes

import torch

from ._core import (_CONV_DTYPES, _DTYPES, DTYPE_BF16, _bind, _check, _d, _f, _finite, _i, _lib, _plan_query, _require_cuda_f32,
                    _require_out, _stream, _vp, dtype_code)


class _Conv1x1Plan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("tile_m", "tile_p", "k_chunk", "k_chunks", "m_tiles", "p_tiles", "grid_x", "block",
                                  "lds_bytes", "out_h", "out_w", "reserved")]


_bind("rroi_conv1x1_forward_hip", [_i, _vp, _vp, _vp] + [_i] * 6 + [_f] + [_vp] * 4 + [_d, _vp])
_bind("rroi_conv1x1_plan", [_i] * 7 + [ctypes.POINTER(_Conv1x1Plan)])

Conv1x1Plan = collections.namedtuple("Conv1x1Plan", [n for n, _ in _Conv1x1Plan._fields_[:-1]])


def conv1x1_plan(batch_size, in_channels, out_channels, height, width, stride=1, dtype=DTYPE_BF16) -> Conv1x1Plan:
    """What `conv1x1` launches for an x of (batch_size, in_channels, height, width) and `out_channels` filters (host only,
    no GPU needed): the tile (output channels, output pixels), the K chunk and their number, tiles per image along each
    axis, grid, block, LDS bytes and the output's size.  ValueError where the call would refuse the arguments (float32
    among them)."""
    return _plan_query(_lib.rroi_conv1x1_plan, _Conv1x1Plan, Conv1x1Plan, "rroi_conv1x1_plan",
                       (dtype_code(dtype), batch_size, in_channels, out_channels, height, width, stride))


def conv1x1(x: torch.Tensor, weight: torch.Tensor, stride: int = 1, negative_slope: float = 1.0, norm=None,
            out=None) -> torch.Tensor:
    """(N,Cin,H,W) x (Cout,Cin,1,1) or (Cout,Cin) -> (N,Cout,Ho,Wo): act(s * conv2d(x, weight, stride=stride) + t) on the
    matrix cores in one launch.  bfloat16 or float16, x and weight alike, both contiguous (a non-contiguous
    tensor is refused, not copied); no bias; stride 1 or 2.  norm: None, or an eval-mode BatchNorm as
    (weight or None, bias or None, running_mean, running_var, eps) -- vectors of Cout elements of x's dtype and device,
    weight and bias both given or both None -- folded in as s = weight / sqrt(var + eps), t = bias - mean * s, computed in
    fp32 inside the launch.  act is a leaky ReLU of `negative_slope`: 1.0 none, 0.0 a ReLU.  fp32 accumulation in a fixed
    order (the same bits on every run), one rounding to the tensors' type after the activation.  out: a contiguous tensor
    of the result's shape, dtype and device to write into.  Forward only (no autograd).
    ValueError for mismatched shapes, dtypes or layouts, TypeError for float32, RuntimeError for CPU tensors."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor):
        raise TypeError("x and weight must be torch.Tensors")
    if x.dim() != 4:
        raise ValueError(f"x must be (N,Cin,H,W), got {tuple(x.shape)}")
    N, C, H, W = x.shape
    if not ((weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1)) or weight.dim() == 2) or weight.size(1) != C:
        raise ValueError(f"weight must be (Cout, {C}, 1, 1) or (Cout, {C}) for x {tuple(x.shape)}, got {tuple(weight.shape)}")
    if weight.dtype != x.dtype:
        raise ValueError(f"x and weight must have one dtype, got {x.dtype} and {weight.dtype}")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2, got {stride!r}")
    negative_slope = _finite(negative_slope, "negative_slope")
    K = weight.size(0)
    if norm is not None:
        if not isinstance(norm, (tuple, list)) or len(norm) != 5:
            raise ValueError("norm must be (weight or None, bias or None, running_mean, running_var, eps)")
        g, b, mean, var, eps = norm
        if (g is None) != (b is None):
            raise ValueError("norm: weight and bias must both be given or both be None")
        if mean is None or var is None:
            raise ValueError("norm: running_mean and running_var must be given")
        for name, v in (("weight", g), ("bias", b), ("running_mean", mean), ("running_var", var)):
            if v is not None and (not isinstance(v, torch.Tensor) or tuple(v.shape) != (K,) or v.dtype != x.dtype
                                  or v.device != x.device or not v.is_contiguous()):
                raise ValueError(f"norm: {name} must be a contiguous ({K},) tensor of x's dtype and device")
        eps = float(eps)
        if not (0.0 <= eps < float("inf")):
            raise ValueError(f"norm: eps must be finite and not negative, got {eps!r}")
        norm = (g, b, mean, var, eps)
    _require_cuda_f32(x, "x", _CONV_DTYPES)
    _require_cuda_f32(weight, "weight", _CONV_DTYPES)
    if weight.device != x.device:
        raise ValueError("x and weight must be on the same device")
    if C < 1 or H < 1 or W < 1 or K < 1:
        raise ValueError(f"x and weight must have at least one channel, row and column, got {tuple(x.shape)}, {tuple(weight.shape)}")
    if not x.is_contiguous() or not weight.is_contiguous():
        raise ValueError("x and weight must be contiguous")
    if out is not None:
        _require_out(out, (N, K, (H - 1) // stride + 1, (W - 1) // stride + 1), x)
    return _conv1x1_run(x, weight, int(stride), negative_slope, norm, out)


def _conv1x1_run(x: torch.Tensor, weight: torch.Tensor, stride: int, negative_slope: float = 1.0, norm=None,
                 out=None) -> torch.Tensor:
    """The call itself, for arguments already checked (conv1x1 above; fots_e2e.native after conv1x1_ok / shortcut_ok):
    contiguous CUDA tensors of one 16-bit dtype and device, x (N,Cin,H,W), weight (Cout,Cin[,1,1]), stride 1 or 2, norm
    None or (weight or None, bias or None, running_mean, running_var, eps)."""
    index = x.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return _conv1x1_run(x, weight, stride, negative_slope, norm, out)
    N, C, H, W = x.shape
    K = weight.size(0)
    if out is None:
        out = torch.empty((N, K, (H - 1) // stride + 1, (W - 1) // stride + 1), dtype=x.dtype, device=x.device)
    if N == 0:
        return out
    if norm is None:
        g = b = mean = var = None
        eps = 0.0
    else:
        g, b, mean, var, eps = norm
        g, b = (None, None) if g is None else (g.data_ptr(), b.data_ptr())
        mean, var = mean.data_ptr(), var.data_ptr()
    st = _lib.rroi_conv1x1_forward_hip(_DTYPES[x.dtype], x.data_ptr(), weight.data_ptr(), out.data_ptr(), N, C, K, H, W,
                                       stride, negative_slope, g, b, mean, var, eps, _stream())
    if st != 1:
        _check(st, "rroi_conv1x1_forward_hip")
    return out
