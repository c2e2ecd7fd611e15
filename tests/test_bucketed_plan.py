"""CPU: the bucketed RoIRotate's host side -- the bucket layout, the premise of the whole feature (a crop
pooled at width w is, bit for bit, the first w columns of the same crop pooled at any larger width: checked on the
oracle), the plan queries over a table of cases, and the refusals of the plan queries and of the launch entry points,
all before any launch.  No GPU is needed."""
import ctypes

import numpy as np
import pytest

import workloads as Wk


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


# ---------------------------------------------------------------- bucket layout
def test_layout_is_a_stable_ascending_split(ext):
    rng = np.random.default_rng(0)
    widths = rng.choice([64, 96, 128, 416, 7], 200).tolist()
    lay = ext.bucket_layout(widths)
    assert [w for w, _ in lay] == sorted(set(widths))
    flat = [i for _, idx in lay for i in idx]
    assert sorted(flat) == list(range(200))                      # a permutation of 0 .. R-1
    for w, idx in lay:
        assert idx == sorted(idx)                                # ROI order kept inside a bucket
        assert all(widths[i] == w for i in idx)
        assert len(idx) == widths.count(w)


def test_layout_empty_and_single_bucket(ext):
    assert ext.bucket_layout([]) == []
    assert ext.bucket_layout([96] * 5) == [(96, [0, 1, 2, 3, 4])]
    assert ext.bucket_layout((np.int32(3),)) == [(3, [0])]
    with pytest.raises(ValueError):
        ext.bucket_layout([64, 0])


# ---------------------------------------------------------------- the premise, on the oracle
@pytest.mark.parametrize("rois", ["edge", "degenerate", "tie"])
def test_oracle_crop_is_a_prefix_of_the_wider_crop(oracle, rois):
    r = {"edge": Wk.edge_rois, "degenerate": Wk.degenerate_rois, "tie": Wk.tie_rois}[rois]()
    f = np.random.default_rng(5).standard_normal((1, 5, 160, 160)).astype(np.float32)
    f.reshape(-1)[::97] = np.nan
    for ph, W in ((8, 64), (11, 37)):
        wide = oracle.forward_c(f, r, ph, W, 0.25, threads=8)
        for w in sorted({1, 2, W // 3, W - 1, W}):
            narrow = oracle.forward_c(f, r, ph, w, 0.25, threads=8)
            assert np.array_equal(wide[..., :w].view(np.uint32), narrow.view(np.uint32)), (rois, ph, W, w)


# ---------------------------------------------------------------- plan queries
# (name, B, C, H, W, PH, widths) -- few ROIs: the reference's own call shapes
FEW = [
    ("one image, 24 words", 1, 64, 176, 320, 11, [64] * 9 + [96] * 8 + [128] * 6 + [416]),
    ("one word", 1, 64, 176, 320, 11, [96]),
    ("training, 32 boxes", 2, 64, 120, 160, 11, [32 * (1 + i % 4) for i in range(32)]),
    ("arbitrary widths", 1, 64, 176, 320, 11, [1, 7, 83, 96, 100] * 6 + [7, 83]),
]
# many ROIs, every PH * W_i % 16 == 0, crops aligned
MANY = [
    ("eight images, 192 words", 8, 64, 176, 320, 11, [64] * 80 + [96] * 70 + [128] * 42),
    ("configs[1], natural widths", 1, 256, 160, 160, 8, [16 * (2 + i % 3) for i in range(512)]),
    ("training, 512 boxes", 2, 64, 120, 160, 11, [32 * (1 + i % 4) for i in range(512)]),
]


@pytest.mark.parametrize("case", FEW, ids=[c[0] for c in FEW])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_few_rois_plan_the_patch_kernel(ext, case, dtype):
    _, B, C, H, W, PH, widths = case
    p = ext.forward_bucketed_plan(B, C, H, W, PH, widths, dtype=dtype)
    assert p.family == ext.PLAN_FWD_DIRECT_K2P and p.kernel == -1, p
    assert p.grid_x % len(widths) == 0 and p.grid_x > 0   # (ROI, patch of the widest crop)
    assert ext.forward_bucketed_plan(B, C, H, W, PH, widths, path=ext.PATH_DIRECT, dtype=dtype) == p


@pytest.mark.parametrize("case", MANY, ids=[c[0] for c in MANY])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_aligned_many_rois_plan_the_ragged_gather(ext, case, dtype):
    _, B, C, H, W, PH, widths = case
    p = ext.forward_bucketed_plan(B, C, H, W, PH, widths, dtype=dtype)
    assert p.family == ext.PLAN_FWD_TWO_LAUNCH and p.kernel == ext.PLAN_KERNEL_STRIDED_RAGGED and p.groups == 1, p
    assert p.ntiles == -(-PH * max(widths) // 64)
    # ... and the patch kernel when a width, or the crops' alignment, breaks the gather's contract -- at any R
    q = ext.forward_bucketed_plan(B, C, H, W, PH, widths[:-1] + [widths[-1] + 1], dtype=dtype)
    assert q.family == ext.PLAN_FWD_DIRECT_K2P, q
    q = ext.forward_bucketed_plan(B, C, H, W, PH, widths, dtype=dtype, crop_alignment=4)
    assert q.family == ext.PLAN_FWD_DIRECT_K2P, q
    with pytest.raises(ValueError):   # named, the gather is refused where its contract does not hold
        ext.forward_bucketed_plan(B, C, H, W, PH, widths, path=ext.PATH_TILED, dtype=dtype, crop_alignment=4)


@pytest.mark.parametrize("case", FEW + MANY, ids=[c[0] for c in FEW + MANY])
def test_backward_plans_are_list_gathers_only(ext, case):
    _, B, C, H, W, PH, widths = case
    lists = (ext.PLAN_BWD_LISTS, ext.PLAN_BWD_BUCKETS)
    for dtype in (0, 1, 2):
        for nhwc in (0, 1):
            if nhwc and C % 4:
                continue
            kw = dict(dtype=dtype, bottom_diff_layout=nhwc)
            assert ext.backward_bucketed_plan(B, C, H, W, PH, widths, **kw).family in lists
            assert ext.backward_bucketed_plan(B, C, H, W, PH, widths, path=ext.PATH_TILED_LISTS, **kw).family == ext.PLAN_BWD_LISTS
            assert ext.backward_bucketed_plan(B, C, H, W, PH, widths, path=ext.PATH_TILED_BUCKETS, **kw).family == ext.PLAN_BWD_BUCKETS
            p = ext.backward_bucketed_plan(B, C, H, W, PH, widths, deterministic=True, **kw)
            assert p.family == ext.PLAN_BWD_ORDERED
            assert p.dest == (ext.PLAN_DST_NHWC if nhwc else ext.PLAN_DST_NCHW)
    # the dense call of the same shape may plan the in-kernel gather or the scatter: the ragged one never does
    for path in (ext.PATH_DIRECT, ext.PATH_TILED, ext.PATH_TILED_ATOMIC, ext.PATH_TILED_INKERNEL, ext.PATH_FUSED):
        with pytest.raises(ValueError):
            ext.backward_bucketed_plan(B, C, H, W, PH, widths, path=path)
    with pytest.raises(ValueError):   # the deterministic bit goes with AUTO only
        ext.backward_bucketed_plan(B, C, H, W, PH, widths, path=ext.PATH_TILED_LISTS, deterministic=True)


def test_no_roi_plans_nothing(ext):
    assert ext.forward_bucketed_plan(1, 64, 176, 320, 11, []).family == ext.PLAN_NONE
    assert ext.backward_bucketed_plan(1, 64, 176, 320, 11, []).family == ext.PLAN_NONE


def _fplan(ext, dtype=0, B=1, R=24, H=176, W=320, C=64, PH=11, mx=96, sm=24 * 64, mult=32, align=256, path=0):
    p = ext._Plan()
    return ext._lib.rroi_align_forward_bucketed_plan(dtype, B, R, H, W, C, PH, mx, sm, mult, align, path, ctypes.byref(p))


def _bplan(ext, dtype=0, layout=0, B=1, R=24, H=176, W=320, C=64, PH=11, mx=96, path=0):
    p = ext._Plan()
    return ext._lib.rroi_align_backward_bucketed_plan(dtype, layout, B, R, H, W, C, PH, mx, path, ctypes.byref(p))


def test_plan_queries_refuse(ext):
    assert _fplan(ext) == 1 and _bplan(ext) == 1
    assert _fplan(ext, dtype=3) == 0 and _bplan(ext, dtype=3) == 0                   # bad dtype
    assert _fplan(ext, dtype=-1) == 0 and _bplan(ext, dtype=-1) == 0
    assert _bplan(ext, layout=2) == 0                                                # unknown destination layout
    assert _bplan(ext, layout=1, C=66) == 0                                          # channels-last needs C % 4 == 0
    assert _fplan(ext, path=ext.PATH_FUSED) == 0                                     # FUSED
    assert _bplan(ext, path=ext.PATH_DIRECT) == 0                                    # DIRECT backward
    assert _bplan(ext, path=ext.PATH_TILED_ATOMIC) == 0 and _bplan(ext, path=ext.PATH_TILED_INKERNEL) == 0
    assert _fplan(ext, mx=0) == 0 and _bplan(ext, mx=0) == 0                         # max_width < 1
    assert _fplan(ext, mx=-5) == 0 and _bplan(ext, mx=-5) == 0
    assert _fplan(ext, path=ext.PATH_DETERMINISTIC) == 0                             # a backward flag
    assert _fplan(ext, path=0x400) == 0 and _bplan(ext, path=0x400) == 0             # unknown flag bits
    assert _fplan(ext, sm=23) == 0 and _fplan(ext, sm=24 * 96 + 1) == 0              # a sum no table of R rows can have
    assert _fplan(ext, mult=0) == 0 and _fplan(ext, align=0) == 0
    assert _fplan(ext, B=0) == 0 and _fplan(ext, R=-1) == 0 and _fplan(ext, C=0) == 0 and _fplan(ext, PH=0) == 0
    assert _bplan(ext, B=0) == 0 and _bplan(ext, R=-1) == 0 and _bplan(ext, H=0) == 0
    assert ext._lib.rroi_align_forward_bucketed_plan(0, 1, 24, 176, 320, 64, 11, 96, 24 * 64, 32, 256, 0, None) == 0
    assert ext._lib.rroi_align_backward_bucketed_plan(0, 0, 1, 24, 176, 320, 64, 11, 96, 0, None) == 0


def test_launch_entry_points_refuse_before_any_launch(ext):
    """The same arguments, and null pointers with R > 0, return 0 from the launching calls (there is no GPU here: a
    launch would return a negative HIP error)."""
    f, b = ext._lib.rroi_align_forward_bucketed_hip, ext._lib.rroi_align_backward_bucketed_hip

    def fwd(dtype=0, B=1, R=24, C=64, PH=11, mx=96, sm=24 * 64, mult=32, align=256, path=0, feats=None, rois=None, table=None):
        return f(feats, dtype, 0.25, B, R, 176, 320, C, PH, mx, sm, mult, align, rois, table, None, 0, path, None)

    def bwd(dtype=0, layout=0, B=1, R=24, C=64, PH=11, mx=96, path=0, table=None, rois=None, out=None):
        return b(table, dtype, layout, 0.25, B, R, 176, 320, C, PH, mx, rois, out, None, 0, path, None)
    for kw in (dict(dtype=3), dict(path=ext.PATH_FUSED), dict(mx=0), dict(sm=5), dict(path=ext.PATH_DETERMINISTIC),
               dict(B=0), dict(mult=0), dict(path=ext.PATH_TILED, align=4)):
        assert fwd(**kw) == 0, kw
    for kw in (dict(dtype=3), dict(layout=2), dict(layout=1, C=66), dict(path=ext.PATH_DIRECT), dict(mx=0), dict(B=0),
               dict(path=ext.PATH_TILED_INKERNEL), dict(path=ext.PATH_TILED_LISTS | ext.PATH_DETERMINISTIC)):
        assert bwd(**kw) == 0, kw
    # null pointers with R > 0 (a non-null value is never dereferenced on the host)
    assert fwd() == 0 and bwd() == 0
    assert fwd(feats=64, rois=64) == 0 and fwd(feats=64, table=64) == 0 and fwd(rois=64, table=64) == 0
    assert bwd(table=64, rois=64) == 0            # no bottom_diff
    assert bwd(out=64, rois=64) == 0 and bwd(out=64, table=64) == 0
    # R = 0: nothing to launch in the forward
    assert fwd(R=0, sm=0) == 1
    assert bwd(R=0) == 0                           # (the zero fill needs a bottom_diff)


def test_workspace_queries(ext):
    fw, bw = ext._lib.rroi_align_forward_bucketed_workspace_bytes, ext._lib.rroi_align_backward_bucketed_workspace_bytes
    assert fw(1, 64, 176, 320, 24) == ext._lib.rroi_align_forward_workspace_bytes(1, 64, 176, 320, 24, ext.LAYOUT_NCHW)
    assert bw(1, 64, 176, 320, 24, 11, 416) == ext._lib.rroi_align_backward_workspace_bytes(1, 64, 176, 320, 24, 11, 416)
    assert fw(0, 64, 176, 320, 24) == 0 and bw(1, 64, 176, 320, 24, 11, 0) == 0


def test_python_surface_checks_its_arguments(ext):
    import torch
    with pytest.raises(RuntimeError):   # no CPU fallback
        ext.forward_bucketed(torch.zeros(1, 4, 8, 8), torch.zeros(1, 6), 4, [8], 0.25)
    with pytest.raises(ValueError):
        ext.backward_bucketed_plan(1, 64, 176, 320, 11, [64], trig=2)
