"""rroi_align._ext.rroi_align.bucketed -- the binding of bucketed RoIRotate (header section 2b; planned and
launched by the ROI core's `csrc/rroi_host_plan.h` and `rroi_host_launch.h`): one pooled width per ROI in one launch
chain, the device tables a width list needs (built once, cached) and the two plan queries."""
import collections
import ctypes

import torch

from ._core import (_DTYPES, _IO_DTYPES, DTYPE_FP32, _bind, _check, _f, _i, _lib, _ll, _require_cuda_f32, _scratch_lock, _stream, _sz,
                    _vp, _workspace, dtype_code)
from .roi import (LAYOUT_NCHW, LAYOUT_NHWC, PATH_AUTO, PATH_DIRECT, TRIG_DOUBLE, Plan, _path_word, _plan, _Plan,
                  _require_features_rois)

_bind("rroi_align_forward_bucketed_workspace_bytes", [_i] * 5, _sz)
_bind("rroi_align_backward_bucketed_workspace_bytes", [_i] * 7, _sz)
_bind("rroi_align_forward_bucketed_hip", [_vp, _i, _f, _i, _i, _i, _i, _i, _i, _i, _ll, _i, _i, _vp, _vp, _vp, _sz, _i, _vp])
_bind("rroi_align_backward_bucketed_hip", [_vp, _i, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp])
_bind("rroi_align_forward_bucketed_plan", [_i] * 8 + [_ll] + [_i] * 3 + [ctypes.POINTER(_Plan)])
_bind("rroi_align_backward_bucketed_plan", [_i] * 10 + [ctypes.POINTER(_Plan)])


def bucket_layout(widths):
    """Pure host: the ROIs 0 .. R-1 split by pooled width -> [(width, [roi indices])], widths ascending, the ROI order
    kept inside a bucket (a stable split: the index lists together are a permutation of range(R))."""
    groups = {}
    for i, w in enumerate(widths):
        w = int(w)
        if w < 1:
            raise ValueError(f"pooled widths must be >= 1, got {w} for ROI {i}")
        groups.setdefault(w, []).append(i)
    return [(w, groups[w]) for w in sorted(groups)]


def crop_table(addresses, widths, device) -> torch.Tensor:
    """The device table of a bucketed call from host lists: (R, 2) int64 = rroi_align_crop rows {address, width | 0}."""
    rows = [[int(a), int(w) & 0xffffffff] for a, w in zip(addresses, widths)]
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).to(device)


def _pow2_divisor(values, cap=4096) -> int:
    """The largest power of two (<= cap) that divides every value."""
    a = cap
    for v in values:
        v = int(v)
        if v:
            a = min(a, v & -v)
    return a


class _BucketTables(object):
    """What a width list needs on the device, built once and cached: the buckets' index tensors and the tables' constant
    parts -- a call then costs one tiny add per distinct base address, with the address as a kernel argument (no upload,
    so the call can be captured into a graph)."""

    def __init__(self, widths, channels, pooled_height, itemsize, device):
        self.widths = tuple(int(w) for w in widths)
        self.buckets = bucket_layout(self.widths)
        R = len(self.widths)
        self.max_width = max(self.widths) if R else 0
        self.sum_widths = sum(self.widths)
        g = 0
        for w in self.widths:
            g = _gcd(g, w)
        self.width_multiple = max(g, 1)
        self.offsets, at = [], 0            # element offset of every bucket in the forward's one buffer, 256-byte aligned
        fwd = [[0, 0] for _ in range(R)]    # [byte offset in that buffer, width]
        bwd = [[0, 0] for _ in range(R)]    # [byte offset in the bucket's own tensor, width]
        in_bucket, width_of = [], []
        per = 256 // itemsize
        for w, idx in self.buckets:
            crop = channels * pooled_height * w
            self.offsets.append(at)
            hot, wd = [[0, 0] for _ in range(R)], [[0, 0] for _ in range(R)]
            for j, i in enumerate(idx):
                fwd[i] = [(at + j * crop) * itemsize, w]
                bwd[i] = [j * crop * itemsize, w]
                hot[i] = [1, 0]
                wd[i] = [0, w]
            in_bucket.append(hot)
            width_of.append(wd)
            at = (at + len(idx) * crop + per - 1) // per * per
        self.total = at
        # what divides every crop's offset from a bucket's base: with the bases' own alignment, the crops' alignment
        self.offset_alignment = _pow2_divisor([r[0] for r in fwd] + [r[0] for r in bwd])

        def up(rows):
            return torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).to(device)
        self.idx = [torch.tensor(idx, dtype=torch.int64).to(device) for _, idx in self.buckets]
        self.fwd_rel, self.bwd_rel = up(fwd), up(bwd)
        self.addr_col = up([[1, 0]] * R)
        self.in_bucket = [up(h) for h in in_bucket]
        self.width_of = [up(w) for w in width_of]


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


_tables = collections.OrderedDict()
_TABLES_MAX = 32


def _bucket_tables(widths, channels, pooled_height, itemsize, device) -> _BucketTables:
    key = (device.index, tuple(int(w) for w in widths), int(channels), int(pooled_height), int(itemsize))
    with _scratch_lock:
        t = _tables.get(key)
        if t is not None:
            _tables.move_to_end(key)
            return t
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("bucketed rroi_align: run this width list once outside the capture (its tables are uploaded "
                           "on first use)")
    t = _BucketTables(key[1], channels, pooled_height, itemsize, device)
    with _scratch_lock:
        _tables[key] = t
        while len(_tables) > _TABLES_MAX:
            _tables.popitem(last=False)
    return t


def _bucketed_stats(widths):
    widths = [int(w) for w in widths]
    g = 0
    for w in widths:
        g = _gcd(g, w)
    return len(widths), (max(widths) if widths else 1), sum(widths), max(g, 1)


def forward_bucketed_plan(batch_size, channels, height, width, pooled_height, widths, path=PATH_AUTO, trig=0,
                          dtype=DTYPE_FP32, crop_alignment=256) -> Plan:
    """The plan a bucketed forward of these pooled widths runs (host only); ValueError where the call would refuse."""
    R, mx, sm, g = _bucketed_stats(widths)
    return _plan(_lib.rroi_align_forward_bucketed_plan,
                 (dtype_code(dtype), batch_size, R, height, width, channels, pooled_height, mx, sm, g, crop_alignment,
                  _path_word(path, trig)), "rroi_align_forward_bucketed_plan")


def backward_bucketed_plan(batch_size, channels, height, width, pooled_height, widths, path=PATH_AUTO, trig=0,
                           dtype=DTYPE_FP32, bottom_diff_layout=LAYOUT_NCHW, deterministic=False) -> Plan:
    """The plan a bucketed backward of these pooled widths runs (host only); ValueError where the call would refuse."""
    R, mx, _, _ = _bucketed_stats(widths)
    return _plan(_lib.rroi_align_backward_bucketed_plan,
                 (dtype_code(dtype), bottom_diff_layout, batch_size, R, height, width, channels, pooled_height, mx,
                  _path_word(path, trig, deterministic)), "rroi_align_backward_bucketed_plan")


def forward_bucketed(features: torch.Tensor, rois: torch.Tensor, pooled_height: int, widths, spatial_scale: float,
                     path: int = PATH_AUTO, trig: int = TRIG_DOUBLE):
    """RoIRotate with one pooled width PER ROI, in one launch chain: (B,C,H,W) x (R,6) x R host ints ->
    [(index LongTensor (R_b,), crops (R_b, C, PH, W_b))] in ascending width, ROI order kept inside a bucket.  Crop j of a
    bucket is bit for bit forward(features, rois[index], PH, W_b)[j]: nothing wider is written and nothing is sliced or
    copied afterwards.  The buckets are views of ONE allocation (each starts on a 256-byte boundary).
    features: float32, bfloat16 or float16, made NCHW-contiguous; rois float32; path: PATH_AUTO / PATH_DIRECT / PATH_TILED."""
    word = _path_word(path, trig)
    code = _require_features_rois(features, rois)
    B, C, H, W = features.shape
    R, ph = rois.size(0), int(pooled_height)
    if len(widths) != R:
        raise ValueError(f"widths must have one entry per ROI: {len(widths)} for {R}")
    if ph <= 0:
        raise ValueError("pooled_height must be positive")
    if R == 0:
        return []
    features, rois = features.contiguous(), rois.contiguous()
    with torch.cuda.device_of(features):
        t = _bucket_tables(widths, C, ph, features.element_size(), features.device)
        buf = torch.empty((t.total,), dtype=features.dtype, device=features.device)
        out = [(t.idx[b], buf[off:off + len(idx) * C * ph * w].view(len(idx), C, ph, w))
               for b, ((w, idx), off) in enumerate(zip(t.buckets, t.offsets))]
        if buf.numel() == 0:
            return out
        table = torch.add(t.fwd_rel, t.addr_col, alpha=buf.data_ptr())
        align = min(_pow2_divisor([buf.data_ptr()]), t.offset_alignment)
        nbytes = 0 if path == PATH_DIRECT else _lib.rroi_align_forward_bucketed_workspace_bytes(B, C, H, W, R)
        ws = _workspace(features.device, nbytes)
        st = _lib.rroi_align_forward_bucketed_hip(features.data_ptr(), code, float(spatial_scale), B, R, H, W, C, ph,
                                                  t.max_width, t.sum_widths, t.width_multiple, align, rois.data_ptr(),
                                                  table.data_ptr(), ws.data_ptr(), nbytes, word, _stream())
    _check(st, "rroi_align_forward_bucketed_hip")
    return out


def backward_bucketed(grads, rois: torch.Tensor, feature_size, pooled_height: int, widths, spatial_scale: float,
                      path: int = PATH_AUTO, channels_last_grad: bool = False, trig: int = TRIG_DOUBLE,
                      deterministic: bool = False) -> torch.Tensor:
    """The counterpart: `grads` = one (R_b, C, PH, W_b) tensor (or None: that bucket contributes nothing) per bucket of
    bucket_layout(widths), in its order -> grad w.r.t. the features (B,C,H,W), NCHW or (channels_last_grad) channels_last.
    Every gradient tensor is consumed where it is (a non-contiguous one is made contiguous, bucket by bucket): no
    concatenation, no padding to the widest width.  path: PATH_AUTO, PATH_TILED_LISTS or PATH_TILED_BUCKETS;
    deterministic: the ORDERED plan (with PATH_AUTO) -- the bits of the dense deterministic backward on zero-padded crops."""
    word = _path_word(path, trig, deterministic)
    _require_cuda_f32(rois, "rois")
    B, C, H, W = (int(v) for v in feature_size)
    R, ph = rois.size(0), int(pooled_height)
    if len(widths) != R:
        raise ValueError(f"widths must have one entry per ROI: {len(widths)} for {R}")
    layout = bucket_layout(widths)
    grads = list(grads)
    if len(grads) != len(layout):
        raise ValueError(f"one gradient (or None) per bucket: {len(grads)} for {len(layout)} buckets")
    given = [g for g in grads if g is not None]
    dtype = given[0].dtype if given else torch.float32
    for g, (w, idx) in zip(grads, layout):
        if g is None:
            continue
        _require_cuda_f32(g, "grads[...]", _IO_DTYPES)
        if g.dtype != dtype or g.device != rois.device or tuple(g.shape) != (len(idx), C, ph, w):
            raise ValueError(f"the gradient of the width-{w} bucket must be {(len(idx), C, ph, w)} {dtype} on {rois.device}, "
                             f"got {tuple(g.shape)} {g.dtype} on {g.device}")
    rois = rois.contiguous()
    cl_grad = bool(channels_last_grad) and C % 4 == 0 and R > 0
    with torch.cuda.device_of(rois):
        grad_in = torch.empty((B, C, H, W), dtype=dtype, device=rois.device,
                              memory_format=torch.channels_last if cl_grad else torch.contiguous_format)
        if grad_in.numel() == 0:
            return grad_in
        if not given:
            return grad_in.zero_()
        code = _DTYPES[dtype]
        t = _bucket_tables(widths, C, ph, given[0].element_size(), rois.device)
        keep = []   # (the contiguous copies live until the launches are enqueued on this stream)
        table = t.bwd_rel
        for b, g in enumerate(grads):
            if g is None:
                table = torch.sub(table, t.width_of[b])          # width 0: the rows are skipped
            else:
                g = g.contiguous()
                keep.append(g)
                table = torch.add(table, t.in_bucket[b], alpha=g.data_ptr())
        nbytes = _lib.rroi_align_backward_bucketed_workspace_bytes(B, C, H, W, R, ph, t.max_width)
        ws = _workspace(rois.device, nbytes)
        st = _lib.rroi_align_backward_bucketed_hip(table.data_ptr(), code, LAYOUT_NHWC if cl_grad else LAYOUT_NCHW,
                                                   float(spatial_scale), B, R, H, W, C, ph, t.max_width, rois.data_ptr(),
                                                   grad_in.data_ptr(), ws.data_ptr(), nbytes, word, _stream())
    _check(st, "rroi_align_backward_bucketed_hip")
    return grad_in
