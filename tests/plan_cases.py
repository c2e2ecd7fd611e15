"""The dispatch coverage table, shared by tests/test_plan.py (CPU: the plans) and tests/test_gpu_plan_coverage.py (GPU:
every case run against the oracle).  A case names a problem -- shape, ROI generator, layouts, path, caller -- and the
library's plan query (rroi_align_forward_plan / rroi_align_backward_plan) says which kernels it runs.  REQUIRED is the
set of plan keys a shipped kernel runs under, read off the dispatch (plan_forward / plan_backward in
fots.pytorch_amd/csrc/rroi_host_plan.h); the table must cover it, every key that a sweep of shapes, layouts, paths and
callers reaches (sweep()) must be REQUIRED or NOT_RUN with a reason, and every value of every plan enum must appear in
REQUIRED or in UNREACHABLE -- so a new kernel, a new combination, or a moved threshold that leaves one unreached,
fails by name."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name kind B C H W R ph pw gen fl tl path caller")
Case.__new__.__defaults__ = ("bench", 0, 0, 0, 0)   # gen, feature / top_diff layout, top / bottom_diff layout, path, caller

NCHW, NHWC = 0, 1
AUTO, DIRECT, TILED, ATOMIC, LISTS, INKERNEL, BUCKETS, FUSED = 0, 1, 2, 3, 4, 5, 6, 7
NATIVE, LAUNCHER, LAUNCHER_CON_IDX = 0, 1, 2
SCALE = 0.25

FAMILY = {0: "none", 1: "k2p", 2: "thread", 3: "fused_strided", 4: "fused_shift", 5: "two_launch",
          11: "direct", 12: "atomic", 13: "inkernel", 14: "lists", 15: "buckets", 16: "literal"}
KERNEL = {-1: "-", 0: "strided", 1: "channels_last", 2: "shift", 3: "strided_merge", 4: "shift_lines"}
DEST = {0: "-", 1: "chunk_major", 2: "nchw", 3: "nchw_add", 4: "nhwc"}
CALLER = {0: "native", 1: "launcher", 2: "launcher_con_idx"}


def key(kind, plan, caller):
    """The part of a plan that decides which kernel instantiations run."""
    if kind == "fwd":
        return ("fwd", CALLER[caller], FAMILY[plan.family], KERNEL[plan.kernel], "groups" if plan.groups > 1 else "1",
                "zero_copy" if plan.zero_copy else "copy")
    fam = FAMILY[plan.family]
    return ("bwd", CALLER[caller], fam, DEST[plan.dest], plan.nk,
            ("scan2" if plan.raw_bsum == 0 else "inline") if fam == "lists" else "-",
            ("vec4" if plan.vec4 else "scalar") if fam == "atomic" else "-",
            "gy" if plan.gy > 1 else "-", "zero_copy" if plan.zero_copy else "copy",
            "add" if plan.accumulate else "set")


CASES = [
    # ---- forward
    Case("f_k2p", "fwd", 1, 64, 120, 160, 8, 11, 64),
    Case("f_thread_w1", "fwd", 2, 8, 16, 1, 6, 8, 16, path=DIRECT),
    Case("f_fused_strided", "fwd", 1, 256, 160, 160, 16, 8, 64),
    Case("f_fused_shift", "fwd", 1, 128, 160, 160, 32, 11, 50),
    Case("f_two_strided", "fwd", 1, 256, 160, 160, 64, 8, 64),
    Case("f_two_strided_groups", "fwd", 2, 64, 120, 160, 128, 11, 96),
    Case("f_two_shift", "fwd", 1, 96, 120, 160, 256, 11, 83),
    Case("f_two_shift_groups", "fwd", 2, 64, 120, 160, 128, 11, 83),
    Case("f_two_merge", "fwd", 2, 64, 120, 160, 512, 11, 83),
    Case("f_two_shift_lines", "fwd", 2, 64, 60, 80, 1480, 11, 83, gen="beyond"),
    Case("f_cl_out", "fwd", 1, 96, 160, 160, 64, 8, 64, tl=NHWC),
    Case("f_cl_src_cl_out", "fwd", 2, 64, 120, 160, 128, 11, 83, fl=NHWC, tl=NHWC),
    Case("f_cl_src", "fwd", 1, 96, 160, 160, 16, 8, 64, fl=NHWC),
    Case("f_cl_src_groups", "fwd", 2, 32, 120, 160, 96, 11, 83, fl=NHWC),
    Case("f_launcher_k2p", "fwd", 2, 64, 120, 160, 8, 11, 64, caller=LAUNCHER),
    Case("f_launcher_k2p_con_idx", "fwd", 2, 64, 120, 160, 8, 11, 64, caller=LAUNCHER_CON_IDX),
    Case("f_launcher_thread_w1", "fwd", 1, 8, 16, 1, 6, 8, 16, caller=LAUNCHER),
    Case("f_launcher_thread_w1_con_idx", "fwd", 1, 8, 16, 1, 6, 8, 16, caller=LAUNCHER_CON_IDX),
    Case("f_launcher_two", "fwd", 2, 256, 160, 160, 64, 8, 64, caller=LAUNCHER),
    Case("f_launcher_two_con_idx", "fwd", 2, 256, 160, 160, 64, 8, 64, caller=LAUNCHER_CON_IDX),
    Case("f_launcher_two_shift", "fwd", 2, 64, 120, 160, 256, 11, 83, caller=LAUNCHER),
    Case("f_launcher_two_shift_con_idx", "fwd", 1, 8, 16, 24, 600, 11, 83, caller=LAUNCHER_CON_IDX),
    Case("f_launcher_two_shift_lines", "fwd", 1, 256, 16, 24, 600, 11, 50, gen="beyond", caller=LAUNCHER),
    Case("f_launcher_two_shift_lines_con_idx", "fwd", 1, 256, 16, 24, 600, 11, 50, gen="beyond", caller=LAUNCHER_CON_IDX),
    Case("f_two_shift_lines_1group", "fwd", 1, 256, 16, 24, 600, 11, 50, gen="beyond"),
    Case("f_two_shift_lines_1group_cl_src", "fwd", 1, 256, 16, 24, 600, 11, 50, gen="beyond", fl=NHWC),
    Case("f_two_shift_lines_groups_cl_src", "fwd", 1, 64, 16, 24, 1500, 11, 83, gen="beyond", fl=NHWC),
    Case("f_cl_src_strided_groups", "fwd", 1, 8, 16, 24, 64, 8, 32, fl=NHWC),
    Case("f_cl_src_merge", "fwd", 1, 64, 16, 24, 4000, 1, 63, fl=NHWC),
    Case("f_cl_src_shift", "fwd", 1, 8, 16, 24, 4, 1, 63, fl=NHWC),
    Case("f_cl_src_cl_out_1group", "fwd", 1, 8, 16, 24, 4, 1, 63, fl=NHWC, tl=NHWC),
    Case("f_cl_out_groups", "fwd", 1, 8, 16, 24, 64, 1, 63, tl=NHWC),
    # ---- backward
    Case("b_direct", "bwd", 1, 3, 64, 128, 4, 8, 32),
    Case("b_atomic_vec4", "bwd", 1, 64, 64, 96, 24, 8, 64, path=ATOMIC),
    Case("b_atomic_scalar", "bwd", 1, 36, 64, 96, 24, 11, 83, path=ATOMIC),
    Case("b_inkernel_nk1", "bwd", 1, 32, 64, 96, 24, 8, 40, path=INKERNEL),
    Case("b_inkernel_nk2", "bwd", 2, 64, 64, 96, 24, 11, 83, path=INKERNEL),
    Case("b_inkernel_nk4", "bwd", 1, 100, 64, 96, 24, 8, 64, path=INKERNEL),
    Case("b_inkernel_nk8", "bwd", 1, 256, 48, 64, 12, 8, 33, path=INKERNEL),
    Case("b_inkernel_nk1_nhwc", "bwd", 1, 32, 64, 96, 24, 8, 40, tl=NHWC, path=INKERNEL),
    Case("b_inkernel_nk2_nhwc", "bwd", 2, 64, 64, 96, 24, 11, 83, tl=NHWC, path=INKERNEL),
    Case("b_inkernel_nk4_nhwc", "bwd", 1, 100, 64, 96, 24, 8, 64, tl=NHWC, path=INKERNEL),
    Case("b_inkernel_nk8_nhwc", "bwd", 1, 256, 48, 64, 12, 8, 33, tl=NHWC, path=INKERNEL),
    Case("b_inkernel_zero_copy", "bwd", 1, 64, 64, 96, 24, 8, 64, fl=NHWC, path=INKERNEL),
    Case("b_lists_nchw", "bwd", 1, 64, 64, 96, 24, 8, 64, path=LISTS),
    Case("b_lists_scan2", "bwd", 2, 32, 360, 400, 40, 8, 64, path=LISTS),
    Case("b_lists_scan2_carry", "bwd", 2, 4, 1456, 1448, 8, 8, 32, gen="corners", path=LISTS),
    Case("b_lists_chunk_major", "bwd", 1, 160, 24, 32, 100, 8, 32, path=LISTS),
    Case("b_lists_nhwc", "bwd", 1, 64, 64, 96, 24, 11, 83, tl=NHWC, path=LISTS),
    Case("b_buckets_nchw", "bwd", 1, 64, 120, 160, 64, 11, 83),
    Case("b_buckets_nchw_gy", "bwd", 1, 160, 64, 96, 24, 8, 64),
    Case("b_buckets_chunk_major", "bwd", 1, 160, 24, 32, 100, 8, 32),
    Case("b_buckets_nhwc", "bwd", 1, 64, 120, 160, 64, 11, 83, tl=NHWC),
    Case("b_buckets_zero_copy", "bwd", 1, 64, 120, 160, 64, 11, 83, fl=NHWC),
    Case("b_buckets_chains", "bwd", 2, 36, 64, 64, 300, 16, 9, gen="overlap", path=BUCKETS),
    Case("b_launcher_literal", "bwd", 1, 3, 64, 128, 4, 8, 32, caller=LAUNCHER),
    Case("b_launcher_nchw_add", "bwd", 2, 64, 120, 160, 64, 11, 83, caller=LAUNCHER),
    Case("b_launcher_chunk_major_add", "bwd", 1, 160, 24, 32, 100, 8, 32, caller=LAUNCHER),
    Case("b_launcher_nchw_add_gy", "bwd", 1, 132, 16, 24, 4, 8, 64, caller=LAUNCHER),
    Case("b_launcher_inkernel_nk1_add", "bwd", 1, 8, 16, 24, 1500, 11, 50, caller=LAUNCHER),
    Case("b_launcher_inkernel_nk2_add", "bwd", 1, 64, 16, 24, 1500, 11, 50, caller=LAUNCHER),
    Case("b_launcher_lists_nchw_add", "bwd", 1, 8, 16, 24, 9000, 8, 32, caller=LAUNCHER),
    Case("b_launcher_lists_chunk_major_add", "bwd", 1, 132, 8, 8, 2100, 1, 63, caller=LAUNCHER),
    Case("b_buckets_chunk_major_zero_copy", "bwd", 1, 132, 16, 24, 128, 1, 63, fl=NHWC),
    Case("b_buckets_nchw_gy_zero_copy", "bwd", 1, 132, 16, 24, 4, 1, 63, fl=NHWC),
    Case("b_buckets_nhwc_zero_copy", "bwd", 1, 8, 16, 24, 4, 1, 63, fl=NHWC, tl=NHWC),
    Case("b_inkernel_nk1_zero_copy", "bwd", 1, 8, 16, 24, 4, 1, 63, fl=NHWC, path=INKERNEL),
    Case("b_inkernel_nk4_zero_copy", "bwd", 1, 100, 16, 24, 4, 1, 63, fl=NHWC, path=INKERNEL),
    Case("b_inkernel_nk8_zero_copy", "bwd", 1, 132, 16, 24, 4, 1, 63, fl=NHWC, path=INKERNEL),
    Case("b_inkernel_nk1_nhwc_zero_copy", "bwd", 1, 8, 16, 24, 4, 1, 63, fl=NHWC, tl=NHWC, path=INKERNEL),
    Case("b_inkernel_nk2_nhwc_zero_copy", "bwd", 1, 64, 16, 24, 4, 1, 63, fl=NHWC, tl=NHWC, path=INKERNEL),
    Case("b_inkernel_nk4_nhwc_zero_copy", "bwd", 1, 100, 16, 24, 4, 1, 63, fl=NHWC, tl=NHWC, path=INKERNEL),
    Case("b_inkernel_nk8_nhwc_zero_copy", "bwd", 1, 132, 16, 24, 4, 1, 63, fl=NHWC, tl=NHWC, path=INKERNEL),
    Case("b_lists_chunk_major_zero_copy", "bwd", 1, 132, 16, 24, 128, 1, 63, fl=NHWC, path=LISTS),
    Case("b_lists_nchw_zero_copy", "bwd", 1, 8, 16, 24, 4, 1, 63, fl=NHWC, path=LISTS),
    Case("b_lists_nchw_gy", "bwd", 1, 132, 16, 24, 4, 1, 63, path=LISTS),
    Case("b_lists_nchw_gy_zero_copy", "bwd", 1, 132, 16, 24, 4, 1, 63, fl=NHWC, path=LISTS),
    Case("b_lists_scan2_zero_copy", "bwd", 2, 8, 360, 400, 4, 1, 63, fl=NHWC, path=LISTS),
    Case("b_lists_scan2_gy", "bwd", 2, 132, 360, 400, 4, 1, 63, path=LISTS),
    Case("b_lists_scan2_gy_zero_copy", "bwd", 2, 132, 360, 400, 4, 1, 63, fl=NHWC, path=LISTS),
    Case("b_lists_nhwc_zero_copy", "bwd", 1, 8, 16, 24, 4, 1, 63, fl=NHWC, tl=NHWC, path=LISTS),
    Case("b_lists_nhwc_scan2", "bwd", 2, 8, 360, 400, 4, 1, 63, tl=NHWC, path=LISTS),
    Case("b_lists_nhwc_scan2_zero_copy", "bwd", 2, 8, 360, 400, 4, 1, 63, fl=NHWC, tl=NHWC, path=LISTS),
]

# the plan keys a shipped kernel runs under -- each with what selects it (plan_forward / plan_backward)
REQUIRED = {
    # forward, native
    ("fwd", "native", "k2p", "-", "1", "copy"),                         # below 1.5 M output elements (or C < 128), W >= 2
    ("fwd", "native", "thread", "-", "1", "copy"),                      # direct with W < 2 (K2p reads row pairs)
    ("fwd", "native", "fused_strided", "strided", "1", "copy"),         # 1.5 M .. 3.8 M elements, C >= 128, NB % 16 == 0
    ("fwd", "native", "fused_shift", "shift", "1", "copy"),             # ... NB % 16 != 0
    ("fwd", "native", "two_launch", "strided", "1", "copy"),            # >= 3.8 M elements, NB % 16 == 0, C > 64 or R < 64
    ("fwd", "native", "two_launch", "strided", "groups", "copy"),       # ... C <= 64 and R >= 64: XCD groups
    ("fwd", "native", "two_launch", "shift", "1", "copy"),              # NB % 16 != 0 without groups
    ("fwd", "native", "two_launch", "shift", "groups", "copy"),         # ... with groups, < 48 MB of crops
    ("fwd", "native", "two_launch", "strided_merge", "groups", "copy"), # ... >= 48 MB of crops, <= 2 MB of map per XCD
    ("fwd", "native", "two_launch", "shift_lines", "groups", "copy"),   # NB % 16 != 0 beyond 320 MB of crops
    ("fwd", "native", "two_launch", "channels_last", "1", "copy"),      # NHWC crops from NCHW features
    ("fwd", "native", "two_launch", "channels_last", "groups", "zero_copy"),   # NHWC crops from NHWC features, C <= 64
    ("fwd", "native", "two_launch", "strided", "1", "zero_copy"),       # NHWC features read in place
    ("fwd", "native", "two_launch", "shift", "groups", "zero_copy"),    # ... with groups, NB % 16 != 0
    ("fwd", "native", "two_launch", "shift", "1", "zero_copy"),         # ... without groups (R < 64 or C > 64)
    ("fwd", "native", "two_launch", "strided", "groups", "zero_copy"),  # ... NB % 16 == 0 with groups
    ("fwd", "native", "two_launch", "strided_merge", "groups", "zero_copy"),   # ... >= 48 MB of crops from a small map
    ("fwd", "native", "two_launch", "shift_lines", "1", "copy"),        # > 320 MB of crops, C > 64 (no groups)
    ("fwd", "native", "two_launch", "shift_lines", "1", "zero_copy"),   # ... NHWC features
    ("fwd", "native", "two_launch", "shift_lines", "groups", "zero_copy"),     # ... NHWC features, C <= 64
    ("fwd", "native", "two_launch", "channels_last", "1", "zero_copy"), # NHWC crops from NHWC features, C > 64 or R < 64
    ("fwd", "native", "two_launch", "channels_last", "groups", "copy"), # NHWC crops from NCHW features, C <= 64, R >= 64
    # forward, reference-ABI launcher (groups off, no fused form)
    ("fwd", "launcher", "k2p", "-", "1", "copy"),                       # below the two-launch crossover
    ("fwd", "launcher_con_idx", "k2p", "-", "1", "copy"),               # ... writing con_idx
    ("fwd", "launcher", "thread", "-", "1", "copy"),                    # ... W < 2
    ("fwd", "launcher_con_idx", "thread", "-", "1", "copy"),
    ("fwd", "launcher", "two_launch", "strided", "1", "copy"),          # >= 3.8 M elements: image >= 1 by the prologue
    ("fwd", "launcher_con_idx", "two_launch", "strided", "1", "copy"),  # ... + rroi_con_idx_kernel
    ("fwd", "launcher", "two_launch", "shift", "1", "copy"),            # ... NB % 16 != 0
    ("fwd", "launcher_con_idx", "two_launch", "shift", "1", "copy"),
    ("fwd", "launcher", "two_launch", "shift_lines", "1", "copy"),      # ... beyond 320 MB of crops
    ("fwd", "launcher_con_idx", "two_launch", "shift_lines", "1", "copy"),
    # backward, native
    ("bwd", "native", "direct", "nchw", 0, "-", "-", "-", "copy", "set"),              # < 0.2 M elements, map < 8 M
    ("bwd", "native", "atomic", "chunk_major", 0, "-", "vec4", "-", "copy", "set"),    # TILED_ATOMIC, NB % 4 == 0
    ("bwd", "native", "atomic", "chunk_major", 0, "-", "scalar", "-", "copy", "set"),  # ... NB % 4 != 0
    *(("bwd", "native", "inkernel", d, nk, "-", "-", "-", "copy", "set")               # INKERNEL: nk = chunks per lane
      for nk in (1, 2, 4, 8) for d in ("chunk_major", "nhwc")),                        # NCHW via scratch / NHWC in place
    *(("bwd", "native", "inkernel", d, nk, "-", "-", "-", "zero_copy", "set")          # ... NHWC top_diff read in place
      for nk in (1, 2, 4, 8) for d in ("chunk_major", "nhwc")),
    ("bwd", "native", "lists", "nchw", 0, "inline", "-", "-", "copy", "set"),          # LISTS, <= 64 scan blocks, C <= 128
    ("bwd", "native", "lists", "nchw", 0, "scan2", "-", "-", "copy", "set"),           # ... > 64 x 4096 keys: rroi_scan2_kernel
    ("bwd", "native", "lists", "chunk_major", 0, "inline", "-", "-", "copy", "set"),   # C > 128 and > 16 bins per pixel
    ("bwd", "native", "lists", "nhwc", 0, "inline", "-", "-", "copy", "set"),          # NHWC bottom_diff
    ("bwd", "native", "lists", "nhwc", 0, "scan2", "-", "-", "copy", "set"),
    ("bwd", "native", "lists", "nchw", 0, "inline", "-", "gy", "copy", "set"),         # C > 128, <= 16 bins per pixel
    ("bwd", "native", "lists", "nchw", 0, "scan2", "-", "gy", "copy", "set"),
    # ... each with an NHWC top_diff read in place
    *(("bwd", "native", "lists", d, 0, sc, "-", gy, "zero_copy", "set")
      for d, sc, gy in (("nchw", "inline", "-"), ("nchw", "scan2", "-"), ("chunk_major", "inline", "-"), ("nhwc", "inline", "-"),
                        ("nhwc", "scan2", "-"), ("nchw", "inline", "gy"), ("nchw", "scan2", "gy"))),
    ("bwd", "native", "buckets", "nchw", 0, "-", "-", "-", "copy", "set"),             # AUTO / TILED where the bucket holds the mean list
    ("bwd", "native", "buckets", "nchw", 0, "-", "-", "gy", "copy", "set"),            # ... C > 128, <= 16 bins per pixel
    ("bwd", "native", "buckets", "chunk_major", 0, "-", "-", "-", "copy", "set"),      # ... C > 128, > 16 bins per pixel
    ("bwd", "native", "buckets", "nhwc", 0, "-", "-", "-", "copy", "set"),
    ("bwd", "native", "buckets", "nchw", 0, "-", "-", "-", "zero_copy", "set"),        # ... NHWC top_diff read in place
    ("bwd", "native", "buckets", "nchw", 0, "-", "-", "gy", "zero_copy", "set"),
    ("bwd", "native", "buckets", "chunk_major", 0, "-", "-", "-", "zero_copy", "set"),
    ("bwd", "native", "buckets", "nhwc", 0, "-", "-", "-", "zero_copy", "set"),
    # backward, reference-ABI launcher (adds to bottom_diff)
    ("bwd", "launcher", "literal", "nchw_add", 0, "-", "-", "-", "copy", "add"),       # below the tiled crossover
    ("bwd", "launcher", "buckets", "nchw_add", 0, "-", "-", "-", "copy", "add"),       # tiled, C <= 128
    ("bwd", "launcher", "buckets", "chunk_major", 0, "-", "-", "-", "copy", "add"),    # tiled, C > 128, dense: cm_to_nchw<true>
    ("bwd", "launcher", "buckets", "nchw_add", 0, "-", "-", "gy", "copy", "add"),      # tiled, C > 128, sparse
    ("bwd", "launcher", "inkernel", "chunk_major", 1, "-", "-", "-", "copy", "add"),   # bucket below the mean list, in-kernel rule
    ("bwd", "launcher", "inkernel", "chunk_major", 2, "-", "-", "-", "copy", "add"),
    ("bwd", "launcher", "lists", "nchw_add", 0, "inline", "-", "-", "copy", "add"),    # ... R x B > 8192: rroi_bwd_gather_kernel<kDstNchwAdd, false>
    ("bwd", "launcher", "lists", "chunk_major", 0, "inline", "-", "-", "copy", "add"), # ... C > 128, > 16 bins per pixel
}

# plan keys the dispatch can reach that no case runs, and why (tests/test_plan.py sweeps a grid of shapes, layouts,
# paths and callers through the plan query: every key it reaches is REQUIRED or listed here)
NOT_RUN = {
    ("bwd", "native", "lists", "chunk_major", 0, "scan2", "-", "-", "copy", "set"):
        "needs > 64 scan blocks (> 262 K map pixels) AND > 16 bins per pixel at C > 128: >= 4.2 M bins x 132 channels, "
        "2.2 GB of top_diff; scan2 and the chunk-major destination each run in other rows",
    ("bwd", "native", "lists", "chunk_major", 0, "scan2", "-", "-", "zero_copy", "set"):
        "the same problem with an NHWC top_diff",
}

# plan enum values no required key carries, and why
UNREACHABLE = {
    ("family", "none"): "no ROI: nothing is launched (the native backward zeroes bottom_diff)",
    ("dest", "-"): "the forward and the no-ROI plans have no backward destination",
}


def sweep():
    """A grid of shapes, layouts, paths and callers around every threshold of the dispatch (host only): yields
    (case, plan) for every call the library accepts and that launches something."""
    import itertools
    kinds = (("fwd", (AUTO, DIRECT, TILED, FUSED), (NATIVE, LAUNCHER, LAUNCHER_CON_IDX)),
             ("bwd", (AUTO, DIRECT, TILED, ATOMIC, LISTS, INKERNEL, BUCKETS), (NATIVE, LAUNCHER)))
    for B, C, (H, W), R, (ph, pw), fl, tl in itertools.product(
            (1, 2), (3, 8, 32, 64, 96, 160, 256), ((8, 8), (16, 1), (64, 96), (120, 160), (60, 80), (360, 400)),
            (1, 8, 64, 128, 600, 1500, 4000, 9000), ((8, 64), (11, 83), (1, 63), (8, 32)), (NCHW, NHWC), (NCHW, NHWC)):
        for kind, paths, callers in kinds:
            for path in paths:
                for caller in callers:
                    if caller != NATIVE and (path != AUTO or fl != NCHW or tl != NCHW):
                        continue
                    yield Case("sweep", kind, B, C, H, W, R, ph, pw, "bench", fl, tl, path, caller)


def enum_values():
    """Every (field, value) a plan key can carry."""
    out = {("family", v) for v in FAMILY.values()} | {("kernel", v) for v in KERNEL.values() if v != "-"}
    out |= {("dest", v) for v in DEST.values()} | {("caller", v) for v in CALLER.values()}
    out |= {("nk", v) for v in (1, 2, 4, 8)}
    return out


def key_values(k):
    if k[0] == "fwd":
        vals = {("caller", k[1]), ("family", k[2])}
        return vals | ({("kernel", k[3])} if k[3] != "-" else set())
    return {("caller", k[1]), ("family", k[2]), ("dest", k[3])} | ({("nk", k[4])} if k[4] else set())


def plan_of(ext, case):
    """The library's plan for a case (the layouts as the case states them)."""
    args = (case.B, case.C, case.H, case.W, case.R, case.ph, case.pw)
    if case.kind == "fwd":
        return ext.forward_plan(*args, feature_layout=case.fl, top_layout=case.tl, path=case.path, caller=case.caller)
    return ext.backward_plan(*args, top_diff_layout=case.fl, bottom_diff_layout=case.tl, path=case.path,
                             caller=case.caller)


def inputs(case, seed=0):
    """Features (B, C, H, W) and ROIs (R, 6) of a case, from its generator."""
    rng = np.random.default_rng(seed)
    B, C, H, W, R = case.B, case.C, case.H, case.W, case.R
    f = rng.standard_normal((B, C, H, W), dtype=np.float32)
    img_w, img_h = W / SCALE, H / SCALE
    if case.gen == "overlap":     # hundreds of ROIs on the same few pixels (test_backward_heavy_overlap)
        r = np.zeros((R, 6), np.float32)
        r[:, 0] = rng.integers(0, B, R)
        r[:, 1] = (W / 2 + rng.uniform(-3, 3, R)) / SCALE
        r[:, 2] = (H / 2 + rng.uniform(-3, 3, R)) / SCALE
        r[:, 3] = rng.uniform(8, 40, R)
        r[:, 4] = r[:, 3] * rng.uniform(1, 4, R)
        r[:, 5] = rng.uniform(-90, 90, R)
        r[: R // 3] = r[0]
        return f, r
    if case.gen == "beyond":      # test_forward_beyond_the_cache
        h = rng.uniform(8, 40, R)
        r = np.stack([rng.integers(0, B, R), rng.uniform(-10, img_w + 10, R), rng.uniform(-10, img_h + 10, R), h,
                      h * rng.uniform(1, 9, R), rng.uniform(-90, 90, R)], 1).astype(np.float32)
        return f, r
    if case.gen == "corners":     # both ends of the key space: the first rows of image 0, the last rows of image B - 1
        h = rng.uniform(16, 48, R)
        r = np.stack([rng.integers(0, B, R), rng.uniform(0.2, 0.8, R) * img_w, rng.uniform(0, img_h, R), h,
                      h * rng.uniform(2, 6, R), rng.uniform(-30, 30, R)], 1).astype(np.float32)
        r[0:2, 0], r[0:2, 2] = B - 1, img_h - rng.uniform(0, 10, 2)      # centred within 10 image pixels of the bottom edge
        r[2:4, 0], r[2:4, 2] = 0, rng.uniform(8, 40, 2)
        return f, r
    h = rng.uniform(4, min(64.0, img_h), R)
    r = np.stack([rng.integers(0, B, R), rng.uniform(0, img_w, R), rng.uniform(0, img_h, R), h,
                  h * rng.uniform(1, 8, R), rng.uniform(-90, 90, R)], 1).astype(np.float32)
    return f, r


# ---- the regime of b_lists_scan2_carry: rroi_scan2_kernel scans the totals of the level-1 scan blocks (SCAN_BLOCK keys
# each) SCAN2_ROUND at a time and carries the running sum from one round to the next
SCAN_BLOCK, SCAN2_ROUND = 4096, 1024


def key_count(case):
    """Keys of the backward's pixel lists: 32 per key tile of 4 rows x 8 columns, the tiles of every image."""
    return case.B * -(-case.H // 4) * -(-case.W // 8) * 32


def assert_scan2_carries(case, plan, n):
    """The case's level-2 scan runs a second round, and lists lie on both sides of it.  plan: the library's; n: the
    oracle's term count per gradient element (backward_bound_c), (B, C, H, W)."""
    assert plan.raw_bsum == 0, plan
    assert key_count(case) >= SCAN2_ROUND * SCAN_BLOCK + 1, key_count(case)
    # the keys past the first round are the last tile rows of the last image: ceil(keys / 32 / tiles per row) of them
    over = key_count(case) - SCAN2_ROUND * SCAN_BLOCK
    assert over >= 32 * -(-case.W // 8) * 2, "fewer than two tile rows (8 map rows) lie in the second round"
    assert (n[case.B - 1, :, -8:] > 0).any(), "no gradient in the last 8 rows of the last image"
    assert (n[0, :, :24] > 0).any(), "no gradient in the first rows of image 0: the carry would be 0"
