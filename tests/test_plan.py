"""CPU: the plan query (rroi_align_forward_plan / rroi_align_backward_plan) -- host only, no GPU.  Threshold pins: for
every threshold of the dispatch, one shape on each side, each with its exact plan key; the coverage table of
tests/plan_cases.py against REQUIRED; every plan enum value required or listed as unreachable.  Moving a threshold, or
adding a kernel without a case, fails here by name."""
import pytest

import plan_cases as PC


@pytest.fixture(scope="module")
def ext():
    import torch  # noqa: F401  (the HIP runtime before the ctypes library)
    from rroi_align._ext import rroi_align as e
    return e


def K(ext, kind, B, C, H, W, R, ph, pw, fl=0, tl=0, path=0, caller=0):
    c = PC.Case("pin", kind, B, C, H, W, R, ph, pw, "bench", fl, tl, path, caller)
    return PC.key(kind, PC.plan_of(ext, c), caller)


def F(*k):
    return ("fwd", "native") + k


def Bk(fam, dest, nk=0, scan="-", vec="-", gy="-", zc="copy", acc="set", caller="native"):
    return ("bwd", caller, fam, dest, nk, scan, vec, gy, zc, acc)


# (threshold, kind, shape B C H W R ph pw, keyword arguments, plan key) -- a pair per threshold, one on each side
PINS = [
    ("3.8 M output elements: two-launch", "fwd", (1, 64, 160, 160, 115, 8, 64), {}, F("k2p", "-", "1", "copy")),
    ("3.8 M output elements: two-launch", "fwd", (1, 64, 160, 160, 116, 8, 64), {}, F("two_launch", "strided", "groups", "copy")),
    ("1.5 M output elements: fused", "fwd", (1, 128, 160, 160, 22, 8, 64), {}, F("k2p", "-", "1", "copy")),
    ("1.5 M output elements: fused", "fwd", (1, 128, 160, 160, 23, 8, 64), {}, F("fused_strided", "strided", "1", "copy")),
    ("C >= 128: fused", "fwd", (1, 124, 160, 160, 32, 8, 64), {}, F("k2p", "-", "1", "copy")),
    ("C >= 128: fused", "fwd", (1, 128, 160, 160, 32, 8, 64), {}, F("fused_strided", "strided", "1", "copy")),
    ("R >= 64: XCD groups", "fwd", (2, 64, 120, 160, 63, 11, 96), {}, F("two_launch", "strided", "1", "copy")),
    ("R >= 64: XCD groups", "fwd", (2, 64, 120, 160, 64, 11, 96), {}, F("two_launch", "strided", "groups", "copy")),
    ("48 MB of crops: merge", "fwd", (2, 64, 120, 160, 215, 11, 83), {}, F("two_launch", "shift", "groups", "copy")),
    ("48 MB of crops: merge", "fwd", (2, 64, 120, 160, 216, 11, 83), {}, F("two_launch", "strided_merge", "groups", "copy")),
    ("2 MB of map per XCD: merge", "fwd", (2, 64, 203, 160, 512, 11, 83), {}, F("two_launch", "strided_merge", "groups", "copy")),
    ("2 MB of map per XCD: merge", "fwd", (2, 64, 204, 160, 512, 11, 83), {}, F("two_launch", "shift", "groups", "copy")),
    ("320 MB of crops: line windows", "fwd", (2, 64, 60, 80, 1435, 11, 83), {}, F("two_launch", "strided_merge", "groups", "copy")),
    ("320 MB of crops: line windows", "fwd", (2, 64, 60, 80, 1436, 11, 83), {}, F("two_launch", "shift_lines", "groups", "copy")),
    ("320 MB: not for the fused form", "fwd", (2, 64, 60, 80, 1436, 11, 83), {"path": PC.FUSED}, F("fused_shift", "shift", "1", "copy")),
    ("NB % 16: SHIFT tiles", "fwd", (1, 256, 160, 160, 64, 8, 64), {}, F("two_launch", "strided", "1", "copy")),
    ("NB % 16: SHIFT tiles", "fwd", (1, 256, 160, 160, 64, 8, 63), {}, F("two_launch", "shift", "1", "copy")),
    ("W < 2: thread per bin", "fwd", (1, 8, 16, 2, 6, 8, 16), {"path": PC.DIRECT}, F("k2p", "-", "1", "copy")),
    ("W < 2: thread per bin", "fwd", (1, 8, 16, 1, 6, 8, 16), {"path": PC.DIRECT}, F("thread", "-", "1", "copy")),
    ("NB % 4: atomic vector form", "bwd", (1, 64, 64, 96, 24, 1, 64), {"path": PC.ATOMIC}, Bk("atomic", "chunk_major", vec="vec4")),
    ("NB % 4: atomic vector form", "bwd", (1, 64, 64, 96, 24, 1, 63), {"path": PC.ATOMIC}, Bk("atomic", "chunk_major", vec="scalar")),
    ("R x B <= 8192: in-kernel", "bwd", (1, 32, 8, 8, 8192, 8, 32), {}, Bk("inkernel", "chunk_major", nk=1)),
    ("R x B <= 8192: in-kernel", "bwd", (1, 32, 8, 8, 8193, 8, 32), {}, Bk("lists", "nchw", scan="inline")),
    ("64 scan blocks: scan2", "bwd", (1, 32, 504, 520, 40, 8, 64), {"path": PC.LISTS}, Bk("lists", "nchw", scan="inline")),
    ("64 scan blocks: scan2", "bwd", (1, 32, 512, 512, 40, 8, 64), {"path": PC.LISTS}, Bk("lists", "nchw", scan="scan2")),
    ("C > 128: passes in grid y", "bwd", (1, 128, 64, 96, 24, 8, 64), {}, Bk("buckets", "nchw")),
    ("C > 128: passes in grid y", "bwd", (1, 160, 64, 96, 24, 8, 64), {}, Bk("buckets", "nchw", gy="gy")),
]


@pytest.mark.parametrize("i", range(len(PINS)), ids=[f"{p[0]}-{p[2][4]}x{p[2][5]}x{p[2][6]}-{p[2]}" for p in PINS])
def test_threshold_pins(ext, i):
    what, kind, shape, kw, want = PINS[i]
    assert K(ext, kind, *shape, **kw) == want, what


def test_every_threshold_is_pinned_on_both_sides():
    names = [p[0] for p in PINS]
    for n in set(names):
        keys = {p[4] for p in PINS if p[0] == n}
        assert names.count(n) >= 2 or n.startswith("320 MB: not"), n
        assert len(keys) >= 2 or n.startswith("320 MB: not"), (n, keys)


def test_plan_table_covers_required(ext):
    got = {}
    for c in PC.CASES:
        got.setdefault(PC.key(c.kind, PC.plan_of(ext, c), c.caller), []).append(c.name)
    missing = PC.REQUIRED - set(got)
    assert not missing, f"no case of the table runs these plans: {sorted(missing)}"
    extra = set(got) - PC.REQUIRED
    assert not extra, f"plans the table runs that REQUIRED does not list: {sorted(extra)} ({[got[k] for k in extra]})"


def test_scan2_carry_row_is_in_its_regime(ext, oracle):
    """b_lists_scan2_carry: more than 1024 level-1 scan blocks (rroi_scan2_kernel's second round, the carry between
    rounds), under LISTS and under ORDERED, with lists in the first rows of image 0 and the last rows of image B - 1."""
    import numpy as np
    case = next(c for c in PC.CASES if c.name == "b_lists_scan2_carry")
    plan = PC.plan_of(ext, case)
    assert PC.key("bwd", plan, case.caller) == Bk("lists", "nchw", scan="scan2")
    assert PC.key_count(case) == 4216576 and -(-PC.key_count(case) // PC.SCAN_BLOCK) == 1030
    ordered = ext.backward_plan(case.B, case.C, case.H, case.W, case.R, case.ph, case.pw, deterministic=True)
    assert ordered.family == ext.PLAN_BWD_ORDERED and ordered.raw_bsum == 0
    f, r = PC.inputs(case)
    gout = np.ones((case.R, case.C, case.ph, case.pw), np.float32)
    _, n = oracle.backward_bound_c(gout, r, f.shape, PC.SCALE, threads=8)
    PC.assert_scan2_carries(case, plan, n)
    below = PC.Case("below", "bwd", 2, 4, 1448, 1448, 8, 8, 32, gen="corners", path=PC.LISTS)
    assert PC.key_count(below) < PC.SCAN2_ROUND * PC.SCAN_BLOCK + 1       # (the nearest smaller map does not get there)


MI355X_CUS = 256    # compute units of the GPU the suite runs on; the aggregation threshold is eight patches per CU


def test_sparse_rois_are_in_the_full_table_regime(ext, oracle):
    """The problem of test_backward_sparse_rois_fill_the_reservation_table (tests/test_gpu_parity.py): the bucket family,
    enough patches for the per-wave reservations, and every patch on more key tiles than the wave's table has entries;
    its first 8 ROIs are as sparse but too few to aggregate."""
    import workloads as Wk
    B, C, H, W, ph, pw = 1, 8, 160, 160, 16, 16
    r = Wk.sparse_rois(520)
    assert Wk.patch_shape(ph, pw) == (8, 8, 4)
    for R in (520, 8):
        for path in ((PC.AUTO, PC.BUCKETS) if R == 520 else (PC.BUCKETS,)):
            for td in (PC.NCHW, PC.NHWC):
                plan = ext.backward_plan(B, C, H, W, R, ph, pw, top_diff_layout=td, path=path)
                assert plan.family == ext.PLAN_BWD_BUCKETS, (R, path, td, plan)
        assert Wk.pairs_aggregate(R, ph, pw, MI355X_CUS) == (R == 520)
        tiles = Wk.patch_tile_counts(oracle, (B, C, H, W), r[:R], ph, pw, PC.SCALE)
        assert len(tiles) == 4 * R and tiles.min() > 16, (R, int(tiles.min()), int(tiles.max()))
    # the densely pooled reference shapes stay within a dozen tiles or so: the regime is not reached by accident
    f, rb = Wk.bench_inputs(R=64, C=1)
    assert Wk.patch_tile_counts(oracle, (1, 1, 160, 160), rb, 8, 64, 0.25).max() <= 16


def test_every_reachable_plan_is_required(ext):
    """A sweep of shapes, layouts, paths and callers around the thresholds: every plan key the dispatch reaches is
    REQUIRED (so a case of the table runs it) or NOT_RUN with a reason -- a combination no case runs fails here."""
    reached = {}
    for c in PC.sweep():
        try:
            plan = PC.plan_of(ext, c)
        except ValueError:
            continue
        if plan.family != ext.PLAN_NONE:
            reached.setdefault(PC.key(c.kind, plan, c.caller), c)
    stray = {k: tuple(c[2:9]) + tuple(c[10:]) for k, c in reached.items() if k not in PC.REQUIRED and k not in PC.NOT_RUN}
    assert not stray, "reachable plans that no case runs:\n" + "\n".join(f"  {k} e.g. {v}" for k, v in sorted(stray.items(), key=str))
    assert set(PC.NOT_RUN) <= set(reached), "NOT_RUN lists plans the sweep no longer reaches"
    assert not set(PC.NOT_RUN) & PC.REQUIRED


def test_every_enum_value_is_required_or_unreachable():
    seen = set().union(*(PC.key_values(k) for k in PC.REQUIRED))
    for v in PC.enum_values():
        assert v in seen or v in PC.UNREACHABLE, f"plan value {v} is neither REQUIRED nor UNREACHABLE"
    for v in PC.UNREACHABLE:
        assert v not in seen, f"{v} is listed unreachable but REQUIRED"


def test_enum_tables_are_the_headers(ext):
    """The names of plan_cases are the header's RROI_PLAN_* / RROI_CALLER_* values."""
    fam = {v: k for k, v in PC.FAMILY.items()}
    assert fam["k2p"] == ext.PLAN_FWD_DIRECT_K2P and fam["thread"] == ext.PLAN_FWD_DIRECT_THREAD
    assert fam["fused_strided"] == ext.PLAN_FWD_FUSED_STRIDED and fam["fused_shift"] == ext.PLAN_FWD_FUSED_SHIFT
    assert fam["two_launch"] == ext.PLAN_FWD_TWO_LAUNCH and fam["direct"] == ext.PLAN_BWD_DIRECT
    assert fam["atomic"] == ext.PLAN_BWD_ATOMIC and fam["inkernel"] == ext.PLAN_BWD_INKERNEL
    assert fam["lists"] == ext.PLAN_BWD_LISTS and fam["buckets"] == ext.PLAN_BWD_BUCKETS
    assert fam["literal"] == ext.PLAN_BWD_LITERAL and fam["none"] == ext.PLAN_NONE
    ker = {v: k for k, v in PC.KERNEL.items()}
    assert (ker["strided"], ker["channels_last"], ker["shift"], ker["strided_merge"], ker["shift_lines"]) == (
        ext.PLAN_KERNEL_STRIDED, ext.PLAN_KERNEL_CHANNELS_LAST, ext.PLAN_KERNEL_SHIFT, ext.PLAN_KERNEL_STRIDED_MERGE,
        ext.PLAN_KERNEL_SHIFT_LINES)
    dst = {v: k for k, v in PC.DEST.items()}
    assert (dst["chunk_major"], dst["nchw"], dst["nchw_add"], dst["nhwc"]) == (
        ext.PLAN_DST_CHUNK_MAJOR, ext.PLAN_DST_NCHW, ext.PLAN_DST_NCHW_ADD, ext.PLAN_DST_NHWC)
    assert (PC.NATIVE, PC.LAUNCHER, PC.LAUNCHER_CON_IDX) == (ext.CALLER_NATIVE, ext.CALLER_LAUNCHER,
                                                              ext.CALLER_LAUNCHER_CON_IDX)


def test_plan_query_refuses_what_the_call_refuses(ext):
    """0 exactly where the entry point refuses its arguments (same checks, same function); R = 0 launches nothing."""
    q = ext.forward_plan
    with pytest.raises(ValueError):
        q(1, 6, 16, 16, 4, 8, 8, top_layout=ext.LAYOUT_NHWC)            # channels-last crops need C % 4 == 0
    with pytest.raises(ValueError):
        q(1, 8, 16, 16, 4, 8, 8, top_layout=ext.LAYOUT_NHWC, path=ext.PATH_DIRECT)
    with pytest.raises(ValueError):
        q(1, 8, 16, 16, 4, 8, 8, path=9)
    with pytest.raises(ValueError):
        q(1, 8, 16, 16, 4, 8, 8, feature_layout=ext.LAYOUT_NHWC, path=ext.PATH_FUSED)
    with pytest.raises(ValueError):
        q(1, 8, 16, 16, 4, 8, 8, feature_layout=ext.LAYOUT_NHWC, caller=ext.CALLER_LAUNCHER)   # the launcher is NCHW
    with pytest.raises(ValueError):
        ext.backward_plan(1, 8, 16, 16, 4, 8, 8, path=ext.PATH_FUSED)
    with pytest.raises(ValueError):
        ext.backward_plan(1, 6, 16, 16, 4, 8, 8, top_diff_layout=ext.LAYOUT_NHWC)
    with pytest.raises(ValueError):
        ext.backward_plan(1, 8, 16, 16, 4, 8, 8, bottom_diff_layout=ext.LAYOUT_NHWC, path=ext.PATH_TILED_ATOMIC)
    with pytest.raises(ValueError):
        ext.backward_plan(1, 8, 16, 16, 4, 8, 8, caller=ext.CALLER_LAUNCHER_CON_IDX)   # (forward only)
    with pytest.raises(ValueError):
        ext.backward_plan(1, 8, 16, 16, 4, 0, 8)
    assert q(1, 8, 16, 16, 0, 8, 8).family == ext.PLAN_NONE
    assert ext.backward_plan(1, 8, 16, 16, 0, 8, 8).family == ext.PLAN_NONE
    # the trig recipe is a flag bit: it changes no plan
    assert q(1, 64, 160, 160, 512, 8, 64, trig=ext.TRIG_FP32) == q(1, 64, 160, 160, 512, 8, 64)
    # a null plan pointer is refused
    assert ext._lib.rroi_align_forward_plan(0, 0, 1, 4, 16, 16, 8, 8, 8, 0, 0, None) == 0
