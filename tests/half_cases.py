"""The dispatch table of 16-bit calls (bfloat16 / float16 features, crops, grad_output and gradient), shared
by tests/test_half_plan.py (CPU: the plans) and tests/test_gpu_half.py (GPU: every case run against the oracle).
HALF_REQUIRED names the plan keys (plan_cases.key) a 16-bit call can run, each with the case that runs it; a sweep of
the shapes, layouts, paths and callers of plan_cases.sweep() in bfloat16 must reach nothing else (or a key of
HALF_NOT_RUN, with its reason)."""
import plan_cases as PC
from plan_cases import Case, NCHW, NHWC, AUTO, DIRECT, TILED, ATOMIC, LISTS, INKERNEL, BUCKETS, FUSED  # noqa: F401

HALF_CASES = [
    # ---- forward (NCHW features only; crops NCHW or NHWC)
    Case("h_f_k2p", "fwd", 1, 64, 120, 160, 8, 11, 64),
    Case("h_f_k2p_fused_range", "fwd", 1, 256, 160, 160, 16, 8, 64),          # fp32 AUTO: fused strided
    Case("h_f_k2p_fused_shift_range", "fwd", 1, 128, 160, 160, 32, 11, 50),   # fp32 AUTO: fused shift
    Case("h_f_thread_w1", "fwd", 2, 8, 16, 1, 6, 8, 16, path=DIRECT),
    Case("h_f_two_strided", "fwd", 1, 256, 160, 160, 64, 8, 64),
    Case("h_f_two_strided_groups", "fwd", 2, 64, 120, 160, 128, 11, 96),
    Case("h_f_two_shift", "fwd", 1, 96, 120, 160, 256, 11, 83),
    Case("h_f_two_shift_groups", "fwd", 2, 64, 120, 160, 128, 11, 83),
    Case("h_f_two_merge", "fwd", 2, 64, 120, 160, 512, 11, 83),               # >= 48 MB of 16-bit crops
    # > 320 MB of 16-bit crops: twice the ROIs of the fp32 table's cases (the rule counts bytes)
    Case("h_f_two_shift_lines", "fwd", 2, 64, 60, 80, 2960, 11, 83, gen="beyond"),
    Case("h_f_two_shift_lines_1group", "fwd", 1, 256, 16, 24, 1200, 11, 50, gen="beyond"),
    Case("h_f_cl_out", "fwd", 1, 96, 160, 160, 64, 8, 64, tl=NHWC),
    Case("h_f_cl_out_groups", "fwd", 1, 8, 16, 24, 64, 1, 63, tl=NHWC),
    # ---- backward (NCHW grad_output only; gradient NCHW or NHWC, written)
    Case("h_b_small_auto", "bwd", 1, 3, 64, 128, 4, 8, 32),                   # fp32 AUTO: direct
    Case("h_b_inkernel_nk1", "bwd", 1, 32, 64, 96, 24, 8, 40, path=INKERNEL),
    Case("h_b_inkernel_nk2", "bwd", 2, 64, 64, 96, 24, 11, 83, path=INKERNEL),
    Case("h_b_inkernel_nk4", "bwd", 1, 100, 64, 96, 24, 8, 64, path=INKERNEL),
    Case("h_b_inkernel_two_passes", "bwd", 1, 256, 48, 64, 12, 8, 33, path=INKERNEL),   # fp32: nk 8
    Case("h_b_inkernel_nk1_nhwc", "bwd", 1, 32, 64, 96, 24, 8, 40, tl=NHWC, path=INKERNEL),
    Case("h_b_inkernel_nk2_nhwc", "bwd", 2, 64, 64, 96, 24, 11, 83, tl=NHWC, path=INKERNEL),
    Case("h_b_inkernel_nk4_nhwc", "bwd", 1, 100, 64, 96, 24, 8, 64, tl=NHWC, path=INKERNEL),
    Case("h_b_inkernel_two_passes_nhwc", "bwd", 1, 256, 48, 64, 12, 8, 33, tl=NHWC, path=INKERNEL),
    Case("h_b_lists_nchw", "bwd", 1, 64, 64, 96, 24, 8, 64, path=LISTS),
    Case("h_b_lists_scan2", "bwd", 2, 32, 360, 400, 40, 8, 64, path=LISTS),
    Case("h_b_lists_chunk_major", "bwd", 1, 160, 24, 32, 100, 8, 32, path=LISTS),
    Case("h_b_lists_nhwc", "bwd", 1, 64, 64, 96, 24, 11, 83, tl=NHWC, path=LISTS),
    Case("h_b_lists_nhwc_scan2", "bwd", 2, 8, 360, 400, 4, 1, 63, tl=NHWC, path=LISTS),
    Case("h_b_lists_nchw_gy", "bwd", 1, 132, 16, 24, 4, 1, 63, path=LISTS),
    Case("h_b_lists_scan2_gy", "bwd", 2, 132, 360, 400, 4, 1, 63, path=LISTS),
    Case("h_b_buckets_nchw", "bwd", 1, 64, 120, 160, 64, 11, 83),
    Case("h_b_buckets_nchw_gy", "bwd", 1, 160, 64, 96, 24, 8, 64),
    Case("h_b_buckets_chunk_major", "bwd", 1, 160, 24, 32, 100, 8, 32),
    Case("h_b_buckets_nhwc", "bwd", 1, 64, 120, 160, 64, 11, 83, tl=NHWC),
    Case("h_b_buckets_chains", "bwd", 2, 36, 64, 64, 300, 16, 9, gen="overlap", path=BUCKETS),
]
HALF_CASE = {c.name: c for c in HALF_CASES}

# the plan keys a 16-bit call runs under -> the case that runs it
HALF_REQUIRED = {
    ("fwd", "native", "k2p", "-", "1", "copy"): "h_f_k2p",                        # direct range, and fp32's fused range
    ("fwd", "native", "thread", "-", "1", "copy"): "h_f_thread_w1",               # W < 2
    ("fwd", "native", "two_launch", "strided", "1", "copy"): "h_f_two_strided",
    ("fwd", "native", "two_launch", "strided", "groups", "copy"): "h_f_two_strided_groups",
    ("fwd", "native", "two_launch", "shift", "1", "copy"): "h_f_two_shift",
    ("fwd", "native", "two_launch", "shift", "groups", "copy"): "h_f_two_shift_groups",
    ("fwd", "native", "two_launch", "strided_merge", "groups", "copy"): "h_f_two_merge",
    ("fwd", "native", "two_launch", "shift_lines", "groups", "copy"): "h_f_two_shift_lines",
    ("fwd", "native", "two_launch", "shift_lines", "1", "copy"): "h_f_two_shift_lines_1group",
    ("fwd", "native", "two_launch", "channels_last", "1", "copy"): "h_f_cl_out",
    ("fwd", "native", "two_launch", "channels_last", "groups", "copy"): "h_f_cl_out_groups",
    ("bwd", "native", "inkernel", "chunk_major", 1, "-", "-", "-", "copy", "set"): "h_b_inkernel_nk1",
    ("bwd", "native", "inkernel", "chunk_major", 2, "-", "-", "-", "copy", "set"): "h_b_inkernel_nk2",
    ("bwd", "native", "inkernel", "chunk_major", 4, "-", "-", "-", "copy", "set"): "h_b_inkernel_nk4",
    ("bwd", "native", "inkernel", "nhwc", 1, "-", "-", "-", "copy", "set"): "h_b_inkernel_nk1_nhwc",
    ("bwd", "native", "inkernel", "nhwc", 2, "-", "-", "-", "copy", "set"): "h_b_inkernel_nk2_nhwc",
    ("bwd", "native", "inkernel", "nhwc", 4, "-", "-", "-", "copy", "set"): "h_b_inkernel_nk4_nhwc",
    ("bwd", "native", "lists", "nchw", 0, "inline", "-", "-", "copy", "set"): "h_b_lists_nchw",
    ("bwd", "native", "lists", "nchw", 0, "scan2", "-", "-", "copy", "set"): "h_b_lists_scan2",
    ("bwd", "native", "lists", "chunk_major", 0, "inline", "-", "-", "copy", "set"): "h_b_lists_chunk_major",
    ("bwd", "native", "lists", "nhwc", 0, "inline", "-", "-", "copy", "set"): "h_b_lists_nhwc",
    ("bwd", "native", "lists", "nhwc", 0, "scan2", "-", "-", "copy", "set"): "h_b_lists_nhwc_scan2",
    ("bwd", "native", "lists", "nchw", 0, "inline", "-", "gy", "copy", "set"): "h_b_lists_nchw_gy",
    ("bwd", "native", "lists", "nchw", 0, "scan2", "-", "gy", "copy", "set"): "h_b_lists_scan2_gy",
    ("bwd", "native", "buckets", "nchw", 0, "-", "-", "-", "copy", "set"): "h_b_buckets_nchw",
    ("bwd", "native", "buckets", "nchw", 0, "-", "-", "gy", "copy", "set"): "h_b_buckets_nchw_gy",
    ("bwd", "native", "buckets", "chunk_major", 0, "-", "-", "-", "copy", "set"): "h_b_buckets_chunk_major",
    ("bwd", "native", "buckets", "nhwc", 0, "-", "-", "-", "copy", "set"): "h_b_buckets_nhwc",
}

# keys a 16-bit call can reach that no case runs, and why
HALF_NOT_RUN = {
    ("bwd", "native", "lists", "chunk_major", 0, "scan2", "-", "-", "copy", "set"):
        "the fp32 table's NOT_RUN row: > 64 scan blocks AND > 16 bins per pixel at C > 128 (GBs of grad_output); "
        "scan2 and the chunk-major destination each run in other rows",
}

# words a 16-bit plan key never carries: the fp32-only kernels and callers
FORBIDDEN = ("fused_strided", "fused_shift", "direct", "atomic", "literal", "zero_copy", "add", "launcher",
             "launcher_con_idx")


def half_plan_of(ext, case, dtype):
    args = (case.B, case.C, case.H, case.W, case.R, case.ph, case.pw)
    if case.kind == "fwd":
        return ext.forward_plan(*args, feature_layout=case.fl, top_layout=case.tl, path=case.path, caller=case.caller,
                                dtype=dtype)
    return ext.backward_plan(*args, top_diff_layout=case.fl, bottom_diff_layout=case.tl, path=case.path,
                             caller=case.caller, dtype=dtype)


def key_of(ext, case, dtype):
    return PC.key(case.kind, half_plan_of(ext, case, dtype), case.caller)
