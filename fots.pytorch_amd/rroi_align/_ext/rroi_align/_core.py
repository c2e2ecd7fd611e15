"""rroi_align._ext.rroi_align._core -- what every module of the binding shares: the library handle, the ctypes aliases, the
dtype codes, the status check, the stream, the per-stream scratch cache and the checks that more than one operator makes.
Each operator's module binds the functions of one `csrc/rroi_*_host.h` and imports from here, never from the package."""
from __future__ import annotations

import collections
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librroi_align_hip.so")

# element types of the features / crops (forward) and grad_output / gradient (backward), 0.10.0: the `dtype` argument of
# the typed entry points.  rois are float32 in every case.
DTYPE_FP32, DTYPE_BF16, DTYPE_FP16 = 0, 1, 2
_DTYPES = {torch.float32: DTYPE_FP32, torch.bfloat16: DTYPE_BF16, torch.float16: DTYPE_FP16}
_IO_DTYPES = (torch.float32, torch.bfloat16, torch.float16)   # features / crops, grad_output / gradient
_CONV_DTYPES = (torch.bfloat16, torch.float16)                # the matrix-core convolutions

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C fots.pytorch_amd/csrc` "
        "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
        "rroi_align has no CPU or PyTorch fallback.")

# torch must be imported first so that libamdhip64.so.7 resolves to the runtime
# torch already loaded (same SONAME) and streams/pointers are interchangeable.
_lib = ctypes.CDLL(LIB_PATH)

_vp, _f, _i, _sz, _ll, _d = (ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_size_t, ctypes.c_longlong,
                             ctypes.c_double)


def _bind(name, argtypes, restype=_i) -> None:
    """Give `_lib.<name>` its prototype of include/rroi_align_hip.h: a wrong count or kind does not raise at the call, it
    shifts or truncates the arguments of a launch (tests/test_binding_prototypes.py holds every one to the header)."""
    fn = getattr(_lib, name)
    fn.restype, fn.argtypes = restype, argtypes


_lib.rroi_align_hip_version.restype = ctypes.c_char_p
_bind("rroi_align_release_launcher_scratch", [])
_bind("rroi_align_launcher_scratch_stats", [_vp, _vp, _vp, _vp])


def version() -> str:
    return _lib.rroi_align_hip_version().decode()


def dtype_code(dtype) -> int:
    """DTYPE_* of a torch dtype (float32, bfloat16, float16) or of a DTYPE_* value; TypeError for anything else."""
    if isinstance(dtype, torch.dtype):
        if dtype not in _DTYPES:
            raise TypeError(f"rroi_align takes float32, bfloat16 or float16 tensors, got {dtype}")
        return _DTYPES[dtype]
    return int(dtype)


def _check(status: int, what: str) -> None:
    if status == 1:
        return
    if status == 0:
        raise ValueError(f"{what}: invalid argument (shape/layout/workspace)")
    raise RuntimeError(f"{what}: HIP error {-status}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# Scratch for the tiled paths, one buffer per (device, stream), grown on demand and reused: calls on
# one stream are ordered, so the next call may overwrite what the previous one left (the contents
# are dead after a call); another stream gets its own buffer.  Saves the allocator round trip per call.
# What is kept is bounded: a request above _SCRATCH_KEEP_BYTES (the backward of a 4096-ROI problem asks
# for 2.4 GB) is served by a plain allocation that goes back to torch's caching allocator with the call,
# at most _SCRATCH_MAX_STREAMS buffers are kept (least recently used first out; a buffer whose stream
# has been destroyed ages out this way), and the table is guarded by a lock.
_SCRATCH_KEEP_BYTES = 512 << 20
_SCRATCH_MAX_STREAMS = 8
_scratch = collections.OrderedDict()
_scratch_lock = threading.Lock()


def _workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    if nbytes > _SCRATCH_KEEP_BYTES or torch.cuda.is_current_stream_capturing():
        # too large to pin, or a graph owns its memory: nothing of it is cached
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    with _scratch_lock:
        buf = _scratch.get(key)
        if buf is not None and buf.numel() >= nbytes:
            _scratch.move_to_end(key)
            return buf
        buf = None
        _scratch.pop(key, None)           # release the smaller buffer before asking for the larger one
        while len(_scratch) >= _SCRATCH_MAX_STREAMS:
            _scratch.popitem(last=False)
        buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        _scratch[key] = buf
        return buf


def release_workspaces() -> None:
    """Drop the cached scratch buffers -- the Python surface's and the library's own (the per-stream
    scratch of the reference-ABI launchers); all of them are re-created on demand."""
    with _scratch_lock:
        _scratch.clear()
    _check(_lib.rroi_align_release_launcher_scratch(), "rroi_align_release_launcher_scratch")


def launcher_scratch_stats() -> dict:
    """State of the library's scratch table for the reference-ABI launchers (see the header)."""
    u, p, c, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_ulonglong()
    _lib.rroi_align_launcher_scratch_stats(ctypes.byref(u), ctypes.byref(p), ctypes.byref(c), ctypes.byref(t))
    return {"in_use": u.value, "pinned": p.value, "capacity": c.value, "transient_calls": t.value}


def _require_cuda_f32(t: torch.Tensor, name: str, dtypes=(torch.float32,)) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on {t.device}: rroi_align runs on the GPU only (the reference's CPU "
            "branch, functions/rroi_align.py:22-25, is dead code and is not reproduced)")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, got {t.dtype}")


# --------------------------------------------------------------------------- checks that more than one operator makes
def _plan_query(fn, struct_type, tuple_type, what, args):
    """A plan query of the library: `fn(*args, &plan)` -> the namedtuple `tuple_type` of the struct's fields of that name
    (host only, no GPU needed); ValueError where the call these arguments describe would refuse them."""
    p = struct_type()
    if fn(*(int(a) for a in args), ctypes.byref(p)) != 1:
        raise ValueError(f"{what}: the call would refuse these arguments")
    return tuple_type(*(getattr(p, n) for n in tuple_type._fields))


def _finite(value, name) -> float:
    """float(value); ValueError for a NaN or an infinity (a slope or a scale that becomes a kernel argument)."""
    value = float(value)
    if value != value or value in (float("inf"), float("-inf")):
        raise ValueError(f"{name} must be finite, got {value!r}")
    return value


def _require_out(out, shape, like) -> None:
    """What the calls with an `out=` ask of it: a contiguous tensor of `shape`, of the dtype and device of `like` (x)."""
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != like.dtype or out.device != like.device
            or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {shape} tensor of x's dtype and device")


def _require_depthwise_shapes(x, weight, name: str, dims: str):
    """The first checks of a depthwise 3x3 call on `x` (called `name`, laid out as `dims`): tensors, x 4-D, weight
    (C,1,3,3) of x's dtype.  The call's own arguments are checked between this and `_require_depthwise_device`."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor):
        raise TypeError(f"{name} and weight must be torch.Tensors")
    if x.dim() != 4:
        raise ValueError(f"{name} must be {dims}, got {tuple(x.shape)}")
    C = x.size(1)
    if tuple(weight.shape) != (C, 1, 3, 3):
        raise ValueError(f"weight must be {(C, 1, 3, 3)} for {name} {tuple(x.shape)}, got {tuple(weight.shape)}")
    if weight.dtype != x.dtype:
        raise ValueError(f"{name} and weight must have one dtype, got {x.dtype} and {weight.dtype}")


def _require_depthwise_device(x, weight, name: str) -> None:
    """... and the last: both on one GPU, float32 / bfloat16 / float16, x with at least one channel, row and column."""
    _require_cuda_f32(x, name, _IO_DTYPES)
    _require_cuda_f32(weight, "weight", _IO_DTYPES)
    if weight.device != x.device:
        raise ValueError(f"{name} and weight must be on the same device")
    if x.size(1) < 1 or x.size(2) < 1 or x.size(3) < 1:
        raise ValueError(f"{name} must have at least one channel, row and column, got {tuple(x.shape)}")


def _require_map(t, name: str, like=None, like_name: str = "") -> None:
    """What the resize and merge-backward calls ask of every tensor: a 4-D (N,C,H,W) tensor with at least one channel, row
    and column, on the GPU, float32 / bfloat16 / float16 -- and, given `like`, of its dtype and device."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dim() != 4:
        raise ValueError(f"{name} must be 4-D (N,C,H,W), got {tuple(t.shape)}")
    if like is not None and t.dtype != like.dtype:
        raise ValueError(f"{name} and {like_name} must have one dtype, got {t.dtype} and {like.dtype}")
    _require_cuda_f32(t, name, _IO_DTYPES)
    if like is not None and t.device != like.device:
        raise ValueError(f"{name} and {like_name} must be on the same device")
    if min(t.shape[1:]) < 1:
        raise ValueError(f"{name} must have at least one channel, row and column, got {tuple(t.shape)}")


def _size2(size, name: str):
    """(h, w) of a `size` argument: two positive integers."""
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be two integers (h, w), got {size!r}") from None
    if h < 1 or w < 1:
        raise ValueError(f"{name} must be positive, got {size!r}")
    return h, w
