"""rroi_align._ext.rroi_align.preprocess -- the binding of native preprocessing (header section 14): the
uploaded bytes of a whole batch of uint8 images to the network's (N, 3, H, W) input tensor in one launch.

A module of the binding like the package's own (`csrc/rroi_preprocess_host.h`), loaded on first use by `fots_e2e`: the
package's `_*_run` callables are a closed list that the network's ledger test reads, so the hot call here is
`run_preprocess_images`."""
import collections
import ctypes

import torch

from ._core import _DTYPES, _IO_DTYPES, DTYPE_FP32, _bind, _check, _i, _lib, _plan_query, _require_cuda_f32, _stream, _vp, dtype_code


class _PreprocessPlan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("grid_x", "block", "columns_per_thread", "rows_per_thread", "strips", "bands", "items",
                                  "wide_store")]


_bind("rroi_preprocess_forward_hip", [_i, _vp, _vp, _vp, _i, _i, _i, _vp])
_bind("rroi_preprocess_plan", [_i] * 4 + [ctypes.POINTER(_PreprocessPlan)])

PreprocessPlan = collections.namedtuple("PreprocessPlan", [n for n, _ in _PreprocessPlan._fields_])


def preprocess_plan(batch_size, height, width, dtype=DTYPE_FP32) -> PreprocessPlan:
    """What `preprocess_images` launches for a result of (batch_size, 3, height, width) (host only, no GPU needed): grid,
    block, the columns and rows of one thread's item, the strips and bands, the item count and whether the 16-byte store
    form applies (it then runs where the result is 16-byte aligned).  ValueError where the call would refuse the
    arguments."""
    return _plan_query(_lib.rroi_preprocess_plan, _PreprocessPlan, PreprocessPlan, "rroi_preprocess_plan",
                       (dtype_code(dtype), batch_size, height, width))


def preprocess_images(src_u8: torch.Tensor, table: torch.Tensor, size, dtype=torch.float32, out=None) -> torch.Tensor:
    """bytes of N images -> (N, 3, H, W) of `dtype`, size = (H, W): every image resized (half-pixel bilinear,
    align_corners=False) to `size`, `/ 128 - 1`, evaluated in double and rounded once to `dtype`, in one launch
    (DESIGN 5.21).  src_u8: a 1-D contiguous uint8 tensor holding the images back to back, each (H0, W0, 3) interleaved.
    table: (N, 4) contiguous int32 on the same device, rows {byte offset in src_u8, H0, W0, 0}; offsets need no alignment
    and the sizes may differ.  The rows are not checked against src_u8 (the call trusts them, as it trusts ROI rows).
    dtype: float32, bfloat16 or float16.  out: a tensor of the result's shape, dtype and device to write into, contiguous
    but at any element-aligned address (a view into a larger buffer).  Where an image already has the target's size the
    float32 result is bit for bit `fots_e2e.pipeline.preprocess`'s.  Forward only.
    ValueError for mismatched shapes or layouts, TypeError for other dtypes, RuntimeError for CPU tensors."""
    if not isinstance(dtype, torch.dtype) or dtype not in _IO_DTYPES:
        raise TypeError(f"dtype must be float32, bfloat16 or float16, got {dtype!r}")
    _require_cuda_f32(src_u8, "src_u8", (torch.uint8,))
    _require_cuda_f32(table, "table", (torch.int32,))
    if table.device != src_u8.device:
        raise ValueError("src_u8 and table must be on the same device")
    if src_u8.dim() != 1 or not src_u8.is_contiguous():
        raise ValueError(f"src_u8 must be a contiguous 1-D tensor of bytes, got {tuple(src_u8.shape)}")
    if table.dim() != 2 or table.size(1) != 4 or not table.is_contiguous():
        raise ValueError(f"table must be a contiguous (N, 4) tensor, got {tuple(table.shape)}")
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (H, W), got {size!r}") from None
    if H < 1 or W < 1:
        raise ValueError(f"size must be at least (1, 1), got {size!r}")
    N = table.size(0)
    if N * 3 * H * W >= (1 << 31) or src_u8.numel() >= (1 << 31):
        raise ValueError("the result must have fewer than 2^31 elements and src_u8 fewer than 2^31 bytes")
    if N > 0 and src_u8.numel() == 0:
        raise ValueError("src_u8 is empty")
    if out is not None:
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != (N, 3, H, W) or out.dtype != dtype
                or out.device != src_u8.device or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous {(N, 3, H, W)} tensor of {dtype} on src_u8's device")
    return run_preprocess_images(src_u8, table, (H, W), dtype, out)


def run_preprocess_images(src_u8: torch.Tensor, table: torch.Tensor, size, dtype=torch.float32, out=None) -> torch.Tensor:
    """The call itself, for arguments already checked (preprocess_images above; fots_e2e.pipeline.preprocess_batch, which
    builds both tensors itself): contiguous CUDA tensors on one device, src_u8 uint8, table (N, 4) int32, size (H, W)."""
    index = src_u8.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_preprocess_images(src_u8, table, size, dtype, out)
    H, W = size
    N = table.size(0)
    if out is None:
        out = torch.empty((N, 3, H, W), dtype=dtype, device=src_u8.device)
    if N == 0:
        return out
    st = _lib.rroi_preprocess_forward_hip(_DTYPES[dtype], src_u8.data_ptr(), table.data_ptr(), out.data_ptr(), N, H, W, _stream())
    if st != 1:
        _check(st, "rroi_preprocess_forward_hip")
    return out
