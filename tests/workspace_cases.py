"""The workspace table, shared by tests/test_workspace_plan.py (CPU: the plans and the size queries) and
tests/test_gpu_workspace.py (GPU: every row run through the raw ABI inside a guarded, poisoned, exactly sized workspace
at several base addresses).  Plain data.

Every tiled plan runs inside a scratch buffer the caller owns.  The rows name one problem per kernel form that indexes
that buffer -- every carve of carve / carve_bwd (fots.pytorch_amd/csrc/rroi_host_plan.h) with every consumer of it --
on maps that are deliberately tiny and awkward:
    13 x 18   HW % 4 != 0, row pitch 19 (one pad pixel per row), key space padded to 16 x 24
    13 x 19   odd HW
    12 x 20   HW % 4 == 0: the vector path of the relayout
Paths are named, so no AUTO threshold decides; `want` is the tail of the plan key (plan_cases.key without direction and
caller) the row must run under."""
import collections

import numpy as np

import plan_cases as PC
from plan_cases import Case, NHWC, TILED, ATOMIC, LISTS, INKERNEL, BUCKETS, DIRECT, FUSED, AUTO  # noqa: F401

Row = collections.namedtuple("Row", "case want det")
Row.__new__.__defaults__ = (False,)

MAPS = ((13, 18), (13, 19), (12, 20))
OFFSETS = (0, 256, 2304, 3840)    # of the workspace from a 4 KiB boundary: what the GPU test runs every row at


def key(ext, kind, plan, caller=PC.NATIVE):
    """plan_cases.key, plus the ORDERED family (the deterministic backward), which plan_cases does not name: the tuple
    is plan_cases.key's own for the exact lists ORDERED is built on, with the family's name replaced."""
    assert ext.PLAN_BWD_ORDERED not in PC.FAMILY
    if kind == "bwd" and plan.family == ext.PLAN_BWD_ORDERED:
        k = PC.key(kind, plan._replace(family=ext.PLAN_BWD_LISTS), caller)
        assert k[2] == "lists"
        return k[:2] + ("ordered",) + k[3:]
    return PC.key(kind, plan, caller)


def _fwd(name, B, C, R, ph, pw, want, maps, **kw):
    """One forward problem on each map of `maps` (indices into MAPS)."""
    return [Row(Case(f"{name}_{MAPS[m][0]}x{MAPS[m][1]}", "fwd", B, C, MAPS[m][0], MAPS[m][1], R, ph, pw, path=TILED, **kw),
                ("two_launch",) + want) for m in maps]


def _bwd(name, B, C, R, ph, pw, want, H=13, W=18, det=False, **kw):
    return Row(Case(name, "bwd", B, C, H, W, R, ph, pw, **kw), want, det)


def _b(fam, dest, nk=0, scan="-", vec="-", gy="-", zc="copy"):
    return (fam, dest, nk, scan, vec, gy, zc, "set")


FORWARD = (
    _fwd("f_strided", 2, 33, 40, 8, 16, ("strided", "1", "copy"), (0, 1))
    + _fwd("f_strided_groups", 2, 40, 70, 8, 16, ("strided", "groups", "copy"), (0, 2))
    + _fwd("f_shift", 2, 33, 40, 11, 13, ("shift", "1", "copy"), (0, 2))
    + _fwd("f_shift_groups", 2, 40, 70, 11, 13, ("shift", "groups", "copy"), (0, 1))
    + _fwd("f_cl_out", 2, 36, 40, 11, 13, ("channels_last", "1", "copy"), (0, 1), tl=NHWC)
    + _fwd("f_shift_zero_copy", 2, 36, 40, 11, 13, ("shift", "1", "zero_copy"), (0,), fl=NHWC)
    + _fwd("f_cl_groups_zero_copy", 2, 36, 70, 8, 16, ("channels_last", "groups", "zero_copy"), (0,), fl=NHWC, tl=NHWC)
    + _fwd("f_strided_four_chunks", 1, 100, 20, 8, 16, ("strided", "1", "copy"), (0, 2))      # the last chunk partial
    + _fwd("f_merge", 1, 64, 3400, 1, 63, ("strided_merge", "groups", "copy"), (0, 1))        # 52 MB of crops
    + _fwd("f_merge_zero_copy", 1, 64, 3400, 1, 63, ("strided_merge", "groups", "zero_copy"), (0,), fl=NHWC)
)

BACKWARD = [
    _bwd("b_atomic_vec4", 2, 36, 24, 8, 16, _b("atomic", "chunk_major", vec="vec4"), path=ATOMIC),
    _bwd("b_atomic_scalar", 2, 33, 24, 11, 13, _b("atomic", "chunk_major", vec="scalar"), path=ATOMIC),
    _bwd("b_inkernel_nk1", 2, 32, 24, 11, 13, _b("inkernel", "chunk_major", nk=1), path=INKERNEL),
    _bwd("b_inkernel_nk2", 2, 33, 24, 11, 13, _b("inkernel", "chunk_major", nk=2), path=INKERNEL),
    _bwd("b_inkernel_nk4", 2, 100, 24, 8, 16, _b("inkernel", "chunk_major", nk=4), path=INKERNEL),
    _bwd("b_inkernel_nk8", 1, 132, 12, 8, 16, _b("inkernel", "chunk_major", nk=8), path=INKERNEL),
    _bwd("b_inkernel_nhwc", 2, 36, 24, 11, 13, _b("inkernel", "nhwc", nk=2), tl=NHWC, path=INKERNEL),
    _bwd("b_inkernel_zero_copy", 2, 36, 24, 11, 13, _b("inkernel", "chunk_major", nk=2, zc="zero_copy"), fl=NHWC,
         path=INKERNEL),
    _bwd("b_lists_nchw", 2, 33, 24, 11, 13, _b("lists", "nchw", scan="inline"), path=LISTS),
    _bwd("b_lists_nhwc", 2, 36, 24, 11, 13, _b("lists", "nhwc", scan="inline"), tl=NHWC, path=LISTS),
    _bwd("b_lists_chunk_major", 1, 132, 60, 8, 16, _b("lists", "chunk_major", scan="inline"), path=LISTS),
    _bwd("b_lists_nchw_gy", 1, 132, 4, 1, 63, _b("lists", "nchw", scan="inline", gy="gy"), path=LISTS),
    _bwd("b_lists_zero_copy", 2, 36, 24, 11, 13, _b("lists", "nchw", scan="inline", zc="zero_copy"), fl=NHWC, path=LISTS),
    _bwd("b_lists_scan2", 2, 8, 4, 1, 63, _b("lists", "nchw", scan="scan2"), H=360, W=400, path=LISTS),   # 76 MB of workspace
    _bwd("b_buckets_nchw", 2, 33, 24, 11, 13, _b("buckets", "nchw"), path=BUCKETS),
    _bwd("b_buckets_nhwc", 2, 36, 24, 11, 13, _b("buckets", "nhwc"), tl=NHWC, path=BUCKETS),
    _bwd("b_buckets_chunk_major", 1, 132, 60, 8, 16, _b("buckets", "chunk_major"), path=BUCKETS),
    _bwd("b_buckets_nchw_gy", 1, 132, 4, 1, 63, _b("buckets", "nchw", gy="gy"), path=BUCKETS),
    # some pixel's list is longer than its bucket (kshift 5): the overflow chains are walked
    _bwd("b_buckets_chains", 2, 36, 300, 16, 9, _b("buckets", "nchw"), H=64, W=64, gen="overlap", path=BUCKETS),
    _bwd("b_ordered_nchw", 2, 33, 24, 11, 13, _b("ordered", "nchw", scan="inline"), det=True),
    _bwd("b_ordered_nhwc", 2, 36, 24, 11, 13, _b("ordered", "nhwc", scan="inline"), det=True, tl=NHWC),
    # lists longer than 64 entries: the queued LDS sort, whose queue lives in the pixel counters
    _bwd("b_ordered_queue", 2, 36, 180, 16, 9, _b("ordered", "nchw", scan="inline"), H=64, W=64, det=True, gen="overlap"),
]
CHAINS_KSHIFT = 5
SORT_REGISTER_CAP = 64    # kSortRegCap (rroi_backward_kernels.h): a longer list is queued in the pixel counters

ROWS = FORWARD + BACKWARD
ROW = {r.case.name: r for r in ROWS}
assert len(ROW) == len(ROWS)

# ---- 16-bit calls (bfloat16 and float16; NCHW features / grad_output only), sized with the FP32 query: the header says
# a typed call needs "no more than" it.  name -> the key tail in 16 bits (INKERNEL at C = 132 plans nk 4 there).
HALF = {
    "f_strided_13x18": None, "f_strided_13x19": None, "f_shift_13x18": None, "f_shift_12x20": None,
    "f_shift_groups_13x18": None, "f_shift_groups_13x19": None, "f_cl_out_13x18": None, "f_cl_out_13x19": None,
    "b_inkernel_nk2": None, "b_inkernel_nk8": _b("inkernel", "chunk_major", nk=4),
    "b_lists_nchw": None, "b_buckets_nchw": None, "b_buckets_nhwc": None,
    "b_ordered_nchw": None, "b_ordered_nhwc": None, "b_ordered_queue": None,
}
HALF_ROWS = [Row(ROW[n].case, w if w is not None else ROW[n].want, ROW[n].det) for n, w in HALF.items()]

# ---- bucketed calls (header section 2b): (2, 33, 13, 18) maps, PH = 8; sized with the two bucketed queries
BRow = collections.namedtuple("BRow", "name kind B C H W R ph choices path det want")
BUCKETED = [
    BRow("k_fwd_ragged", "fwd", 2, 33, 13, 18, 70, 8, (16, 32, 48), TILED, False, ("two_launch", "strided_ragged")),
    BRow("k_bwd_lists", "bwd", 2, 33, 13, 18, 24, 8, (1, 7, 16, 33), LISTS, False, ("lists", "nchw")),
    BRow("k_bwd_buckets", "bwd", 2, 33, 13, 18, 24, 8, (1, 7, 16, 33), BUCKETS, False, ("buckets", "nchw")),
    BRow("k_bwd_ordered", "bwd", 2, 33, 13, 18, 24, 8, (1, 7, 16, 33), AUTO, True, ("ordered", "nchw")),
]

# ---- plans that take no workspace: (NULL, 0) is accepted, and a workspace that is handed over stays untouched
NO_WORKSPACE = [
    Row(Case("n_f_k2p", "fwd", 2, 33, 13, 18, 6, 8, 16, path=DIRECT), ("k2p", "-", "1", "copy")),
    Row(Case("n_f_thread_w1", "fwd", 2, 8, 16, 1, 6, 8, 16, path=DIRECT), ("thread", "-", "1", "copy")),
    Row(Case("n_f_fused", "fwd", 1, 128, 13, 18, 8, 8, 16, path=FUSED), ("fused_strided", "strided", "1", "copy")),
    Row(Case("n_b_direct", "bwd", 2, 33, 13, 18, 6, 8, 16, path=DIRECT), _b("direct", "nchw")),
]
NO_WORKSPACE_BUCKETED = BRow("n_k_patch", "fwd", 2, 33, 13, 18, 12, 8, (1, 7, 16, 33), DIRECT, False, ("k2p", "-"))

# ---- what the union of the rows above must cover (key tails; the callers are all native)
REQUIRED = {
    ("fwd", "two_launch", "strided", "1", "copy"),               # row pitch, spare pixel, partial last chunk
    ("fwd", "two_launch", "strided", "groups", "copy"),          # + the sort tables
    ("fwd", "two_launch", "shift", "1", "copy"),
    ("fwd", "two_launch", "shift", "groups", "copy"),
    ("fwd", "two_launch", "channels_last", "1", "copy"),
    ("fwd", "two_launch", "shift", "1", "zero_copy"),            # the affine and sort tables only
    ("fwd", "two_launch", "channels_last", "groups", "zero_copy"),
    ("fwd", "two_launch", "strided_merge", "groups", "copy"),
    ("fwd", "two_launch", "strided_merge", "groups", "zero_copy"),
    ("bwd",) + _b("atomic", "chunk_major", vec="vec4"),
    ("bwd",) + _b("atomic", "chunk_major", vec="scalar"),
    *(("bwd",) + _b("inkernel", "chunk_major", nk=nk) for nk in (1, 2, 4, 8)),
    ("bwd",) + _b("inkernel", "nhwc", nk=2),
    ("bwd",) + _b("inkernel", "chunk_major", nk=2, zc="zero_copy"),
    ("bwd",) + _b("lists", "nchw", scan="inline"),
    ("bwd",) + _b("lists", "nhwc", scan="inline"),
    ("bwd",) + _b("lists", "chunk_major", scan="inline"),
    ("bwd",) + _b("lists", "nchw", scan="inline", gy="gy"),
    ("bwd",) + _b("lists", "nchw", scan="inline", zc="zero_copy"),
    ("bwd",) + _b("lists", "nchw", scan="scan2"),
    ("bwd",) + _b("buckets", "nchw"),
    ("bwd",) + _b("buckets", "nhwc"),
    ("bwd",) + _b("buckets", "chunk_major"),
    ("bwd",) + _b("buckets", "nchw", gy="gy"),
    ("bwd",) + _b("ordered", "nchw", scan="inline"),
    ("bwd",) + _b("ordered", "nhwc", scan="inline"),
}
HALF_REQUIRED = {
    ("fwd", "two_launch", "strided", "1", "copy"),
    ("fwd", "two_launch", "shift", "1", "copy"),
    ("fwd", "two_launch", "shift", "groups", "copy"),
    ("fwd", "two_launch", "channels_last", "1", "copy"),
    ("bwd",) + _b("inkernel", "chunk_major", nk=2),
    ("bwd",) + _b("inkernel", "chunk_major", nk=4),
    ("bwd",) + _b("lists", "nchw", scan="inline"),
    ("bwd",) + _b("buckets", "nchw"),
    ("bwd",) + _b("buckets", "nhwc"),
    ("bwd",) + _b("ordered", "nchw", scan="inline"),
    ("bwd",) + _b("ordered", "nhwc", scan="inline"),
}
BUCKETED_REQUIRED = {("fwd", "two_launch", "strided_ragged"), ("bwd", "lists", "nchw"), ("bwd", "buckets", "nchw"),
                     ("bwd", "ordered", "nchw")}
NO_WORKSPACE_REQUIRED = {("fwd", "k2p", "-", "1", "copy"), ("fwd", "thread", "-", "1", "copy"),
                         ("fwd", "fused_strided", "strided", "1", "copy"), ("bwd",) + _b("direct", "nchw"),
                         ("fwd", "k2p", "-")}

# forms that index a caller's workspace -- or a scratch -- and that no row runs, and why.  Nothing else is left out.
NOT_RUN = {
    "fwd two_launch shift_lines (1 or groups, copy or zero_copy)":
        "the line-window gather needs more than 320 MB of crops; it reads the same chunk-major copy (or the same "
        "channels-last map) through the same SliceLayout as the shift rows, which run",
    "the reference-ABI launchers (RROIAlignForwardLaucher / RROIAlignBackwardLaucher)":
        "their scratch is allocated by the library itself: there is no caller pointer to put a guard around",
}


def plan_of(ext, row, dtype=0):
    c = row.case
    args = (c.B, c.C, c.H, c.W, c.R, c.ph, c.pw)
    if c.kind == "fwd":
        return ext.forward_plan(*args, feature_layout=c.fl, top_layout=c.tl, path=c.path, dtype=dtype)
    return ext.backward_plan(*args, top_diff_layout=c.fl, bottom_diff_layout=c.tl, path=c.path, dtype=dtype,
                             deterministic=row.det)


def tail(row_key):
    """A plan key without its caller: (direction, ...)."""
    return (row_key[0],) + tuple(row_key[2:])


def row_key(ext, row, dtype=0):
    return tail(key(ext, row.case.kind, plan_of(ext, row, dtype)))


def workspace_bytes(ext, row):
    """What the fp32 size query reports for a row (typed calls are sized with it too)."""
    c = row.case
    if c.kind == "fwd":
        return int(ext._lib.rroi_align_forward_workspace_bytes(c.B, c.C, c.H, c.W, c.R, c.fl))
    return int(ext._lib.rroi_align_backward_workspace_bytes(c.B, c.C, c.H, c.W, c.R, c.ph, c.pw))


def bucketed_widths(b):
    """The pooled width of every ROI of a bucketed row (seeded; every choice occurs)."""
    rng = np.random.default_rng(len(b.name) + b.R)
    w = [int(v) for v in rng.choice(b.choices, b.R)]
    w[:len(b.choices)] = b.choices
    return w


def bucketed_case(b):
    """The dense problem of a bucketed row at its widest width (inputs: plan_cases.inputs)."""
    return Case(b.name, b.kind, b.B, b.C, b.H, b.W, b.R, b.ph, max(b.choices))


def bucketed_key(ext, b, dtype=0):
    widths = bucketed_widths(b)
    if b.kind == "fwd":
        p = ext.forward_bucketed_plan(b.B, b.C, b.H, b.W, b.ph, widths, path=b.path, dtype=dtype, crop_alignment=256)
        kern = "strided_ragged" if p.kernel == ext.PLAN_KERNEL_STRIDED_RAGGED else PC.KERNEL[p.kernel]
        return ("fwd", PC.FAMILY[p.family], kern)
    p = ext.backward_bucketed_plan(b.B, b.C, b.H, b.W, b.ph, widths, path=b.path, dtype=dtype, deterministic=b.det)
    return ("bwd", "ordered" if p.family == ext.PLAN_BWD_ORDERED else PC.FAMILY[p.family], PC.DEST[p.dest])


def bucketed_workspace_bytes(ext, b):
    if b.kind == "fwd":
        return int(ext._lib.rroi_align_forward_bucketed_workspace_bytes(b.B, b.C, b.H, b.W, b.R))
    return int(ext._lib.rroi_align_backward_bucketed_workspace_bytes(b.B, b.C, b.H, b.W, b.R, b.ph, max(b.choices)))


def forward_used_bytes(B, C, H, W, R, layout):
    """Host-side recomputation of carve (rroi_host_plan.h), the forward's workspace: the affine table, the sort's rank
    and order, and -- unless channels-last features are consumed in place -- the chunk-major copy with its spare pixel
    per (image, chunk) slice.  No slack: the total is the size query's (tests/test_workspace_plan.py)."""
    def up(n, a=256):
        return -(-n // a) * a
    copy = 0 if layout == NHWC else up(B * -(-C // 32) * (H * (W | 1) + 1) * 128)
    return up(max(R, 1) * 32) + 2 * up(max(R, 1) * 4) + copy


def backward_used_bytes(ext, B, C, H, W, R, ph, pw, offset):
    """Host-side recomputation of carve_bwd (rroi_host_plan.h) for a workspace that starts `offset` bytes after a 4 KiB
    boundary: (bytes from the base to the end of the last sub-array, the two roundings).  The size query adds a flat
    8192 for the two roundings to 4 KiB of the address, so 8192 - r1 - r2 bytes at the end of the workspace belong to
    no sub-array: an overrun of the last one lands there, not in a guard, unless that tail is checked too.  The
    recomputation is pinned to the library by its total (tests/test_workspace_plan.py)."""
    def up(n, a=256):
        return -(-n // a) * a
    nchunks, NB, pitch = -(-C // 32), ph * pw, W | 1
    nkeys = B * -(-H // 4) * -(-W // 8) * 32
    scan_blocks = -(-(nkeys + 1) // 4096)
    small = (up(R * 32) + up(B * nchunks * H * pitch * 128) + up(nkeys * 4) + up((nkeys + 1) * 4) + up(scan_blocks * 4))
    kshift = ext.backward_plan(B, C, H, W, R, ph, pw, path=BUCKETS).kshift
    pair = max(up(4 * R * NB * 8), up((nkeys << kshift) * 8) + up(4 * R * NB * 16))
    td = up(R * NB * nchunks * 128)
    r1 = -(offset + small) % 4096
    r2 = -(offset + small + r1 + pair) % 4096
    return small + r1 + pair + r2 + td, (r1, r2), small + pair + td + 8192


def row_used_bytes(ext, row, offset):
    """Bytes of a row's workspace that belong to some sub-array, at this offset (the forward's carve has no slack)."""
    c = row.case
    if c.kind == "fwd":
        return workspace_bytes(ext, row)
    return backward_used_bytes(ext, c.B, c.C, c.H, c.W, c.R, c.ph, c.pw, offset)[0]


def bucketed_used_bytes(ext, b, offset):
    if b.kind == "fwd":
        return bucketed_workspace_bytes(ext, b)
    return backward_used_bytes(ext, b.B, b.C, b.H, b.W, b.R, b.ph, max(b.choices), offset)[0]
