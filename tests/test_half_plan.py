"""CPU: the plan queries of 16-bit calls (rroi_align_forward_plan_typed / rroi_align_backward_plan_typed, 0.10.0) -- host
only, no GPU.  For fp32 the typed queries are the untyped ones; a 16-bit call reaches only the plans of
tests/half_cases.py's HALF_REQUIRED (every one named with a case), never an fp32-only kernel, layout or caller; and what
a 16-bit call refuses, it refuses by name."""
import pytest

import half_cases as HC
import plan_cases as PC


@pytest.fixture(scope="module")
def ext():
    import torch  # noqa: F401  (the HIP runtime before the ctypes library)
    from rroi_align._ext import rroi_align as e
    return e


def _typed(ext, case, dtype):
    """The typed C query itself (None where it refuses)."""
    p = ext._Plan()
    if case.kind == "fwd":
        st = ext._lib.rroi_align_forward_plan_typed(dtype, case.fl, case.tl, case.B, case.R, case.H, case.W, case.C, case.ph,
                                                    case.pw, case.path, case.caller, ext.ctypes.byref(p))
    else:
        st = ext._lib.rroi_align_backward_plan_typed(dtype, case.fl, case.tl, case.B, case.R, case.H, case.W, case.C,
                                                     case.ph, case.pw, case.path, case.caller, ext.ctypes.byref(p))
    return ext.Plan(*(getattr(p, n) for n in ext.Plan._fields)) if st == 1 else None


def _untyped(ext, case):
    try:
        return PC.plan_of(ext, case)
    except ValueError:
        return None


def test_version_and_exports(ext):
    assert ext.version().startswith("rroi_align_hip 0.10.0")
    for n in ("rroi_align_forward_typed_hip", "rroi_align_backward_typed_hip", "rroi_align_forward_plan_typed",
              "rroi_align_backward_plan_typed"):
        assert n in ext.EXPORTS and hasattr(ext._lib, n)
    assert (ext.DTYPE_FP32, ext.DTYPE_BF16, ext.DTYPE_FP16) == (0, 1, 2)


def test_fp32_typed_queries_are_the_untyped_ones(ext):
    n = 0
    for case in PC.sweep():
        assert _typed(ext, case, ext.DTYPE_FP32) == _untyped(ext, case), case
        n += 1
    assert n > 10000
    for case in PC.CASES:
        assert _typed(ext, case, ext.DTYPE_FP32) == PC.plan_of(ext, case), case.name


def test_every_required_key_has_its_case(ext):
    names = [c.name for c in HC.HALF_CASES]
    assert len(names) == len(set(names))
    for k, name in HC.HALF_REQUIRED.items():
        case = HC.HALF_CASE[name]
        for dt in (ext.DTYPE_BF16, ext.DTYPE_FP16):
            assert HC.key_of(ext, case, dt) == k, (name, HC.key_of(ext, case, dt), k)
    for case in HC.HALF_CASES:   # the extra cases: a required key each
        assert HC.key_of(ext, case, ext.DTYPE_BF16) in HC.HALF_REQUIRED, case.name


def test_every_gather_kernel_and_destination_is_required():
    fwd_kernels = {k[3] for k in HC.HALF_REQUIRED if k[0] == "fwd" and k[2] == "two_launch"}
    assert fwd_kernels == {"strided", "channels_last", "shift", "strided_merge", "shift_lines"}
    for fam in ("inkernel", "lists", "buckets"):
        dests = {k[3] for k in HC.HALF_REQUIRED if k[0] == "bwd" and k[2] == fam}
        assert {"nchw", "nhwc"} <= dests | ({"nchw"} if "chunk_major" in dests else set()), (fam, dests)
        assert "nhwc" in dests, fam
    # every NCHW destination of a gather (in place, or through the chunk-major scratch)
    assert {k[3] for k in HC.HALF_REQUIRED if k[0] == "bwd" and k[2] == "lists"} >= {"nchw", "chunk_major", "nhwc"}
    assert {k[3] for k in HC.HALF_REQUIRED if k[0] == "bwd" and k[2] == "buckets"} >= {"nchw", "chunk_major", "nhwc"}
    assert {k[3] for k in HC.HALF_REQUIRED if k[0] == "bwd" and k[2] == "inkernel"} >= {"chunk_major", "nhwc"}
    for k in HC.HALF_REQUIRED:
        assert not set(k) & set(HC.FORBIDDEN), k


def test_half_sweep_reaches_only_required_keys(ext):
    """The sweep of plan_cases (every shape, layout, path and caller) in bfloat16: nothing but HALF_REQUIRED (or a
    HALF_NOT_RUN key) -- no fused form, no direct / atomic / literal backward, no zero copy, no accumulation, no
    launcher -- and fp16 plans exactly as bf16 does."""
    reached = set()
    for case in PC.sweep():
        try:
            p = HC.half_plan_of(ext, case, ext.DTYPE_BF16)
        except ValueError:
            assert _typed(ext, case, ext.DTYPE_FP16) is None, case
            continue
        assert _typed(ext, case, ext.DTYPE_FP16) == p, case
        if p.family == ext.PLAN_NONE:
            continue
        k = PC.key(case.kind, p, case.caller)
        assert not set(k) & set(HC.FORBIDDEN), (k, case)
        assert k in HC.HALF_REQUIRED or k in HC.HALF_NOT_RUN, (k, case)
        reached.add(k)
    assert reached >= set(HC.HALF_REQUIRED), set(HC.HALF_REQUIRED) - reached


def test_half_refusals(ext):
    c = PC.Case("x", "fwd", 1, 256, 160, 160, 16, 8, 64)
    for dt in (ext.DTYPE_BF16, ext.DTYPE_FP16):
        kw = dict(dtype=dt)
        with pytest.raises(ValueError):                                      # FUSED: fp32 only
            ext.forward_plan(1, 256, 160, 160, 16, 8, 64, path=ext.PATH_FUSED, **kw)
        with pytest.raises(ValueError):                                      # NHWC features: no zero copy
            ext.forward_plan(1, 64, 120, 160, 128, 11, 83, feature_layout=ext.LAYOUT_NHWC, **kw)
        for caller in (ext.CALLER_LAUNCHER, ext.CALLER_LAUNCHER_CON_IDX):    # the reference ABI is fp32
            with pytest.raises(ValueError):
                ext.forward_plan(1, 64, 120, 160, 8, 11, 64, caller=caller, **kw)
        with pytest.raises(ValueError):
            ext.backward_plan(1, 64, 120, 160, 64, 11, 83, caller=ext.CALLER_LAUNCHER, **kw)
        for path in (ext.PATH_DIRECT, ext.PATH_TILED_ATOMIC):               # fp32 atomics
            with pytest.raises(ValueError):
                ext.backward_plan(1, 64, 64, 96, 24, 8, 64, path=path, **kw)
        with pytest.raises(ValueError):                                      # NHWC top_diff: no zero copy
            ext.backward_plan(1, 64, 120, 160, 64, 11, 83, top_diff_layout=ext.LAYOUT_NHWC, **kw)
        # ... and what the same call accepts in fp32
        ext.forward_plan(1, 256, 160, 160, 16, 8, 64, path=ext.PATH_FUSED)
        ext.forward_plan(1, 64, 120, 160, 128, 11, 83, feature_layout=ext.LAYOUT_NHWC)
        ext.backward_plan(1, 64, 64, 96, 24, 8, 64, path=ext.PATH_DIRECT)
        ext.backward_plan(1, 64, 120, 160, 64, 11, 83, top_diff_layout=ext.LAYOUT_NHWC)
    for bad in (3, -1, 100):
        assert _typed(ext, c, bad) is None
        assert _typed(ext, c._replace(kind="bwd"), bad) is None
    # the typed entry points refuse the same before any launch (no GPU touched: host checks only)
    f = ext._lib.rroi_align_forward_typed_hip
    assert f(None, 3, 0, 0, 0.25, 1, 4, 16, 16, 8, 8, 8, None, None, None, 0, 0, None) == 0
    assert f(None, ext.DTYPE_BF16, 0, 0, 0.25, 1, 4, 16, 16, 8, 8, 8, None, None, None, 0, ext.PATH_FUSED, None) == 0
    assert f(None, ext.DTYPE_BF16, 1, 0, 0.25, 1, 4, 16, 16, 8, 8, 8, None, None, None, 0, 0, None) == 0
    b = ext._lib.rroi_align_backward_typed_hip
    assert b(None, 3, 0, 0, 0.25, 1, 4, 16, 16, 8, 8, 8, None, None, None, 0, 0, None) == 0
    assert b(None, ext.DTYPE_FP16, 0, 0, 0.25, 1, 4, 16, 16, 8, 8, 8, None, None, None, 0, ext.PATH_DIRECT, None) == 0
    assert b(None, ext.DTYPE_FP16, 1, 0, 0.25, 1, 4, 16, 16, 8, 8, 8, None, None, None, 0, 0, None) == 0


def test_byte_thresholds_count_bytes(ext):
    """The two rules that stand for bytes of crops -- the merging form from 48 MB, the line-aligned windows beyond
    320 MB -- take 16-bit crops there at twice the elements; the element-count rules do not move."""
    import torch
    bf = torch.bfloat16
    # 48 MB: fp32 crops of 64 x 11 x 83 reach it at 216 ROIs (tests/test_plan.py pins 215 / 216), 16-bit ones at 431
    assert ext.forward_plan(2, 64, 120, 160, 216, 11, 83).kernel == ext.PLAN_KERNEL_STRIDED_MERGE
    assert ext.forward_plan(2, 64, 120, 160, 216, 11, 83, dtype=bf).kernel == ext.PLAN_KERNEL_SHIFT
    assert ext.forward_plan(2, 64, 120, 160, 430, 11, 83, dtype=bf).kernel == ext.PLAN_KERNEL_SHIFT
    assert ext.forward_plan(2, 64, 120, 160, 431, 11, 83, dtype=bf).kernel == ext.PLAN_KERNEL_STRIDED_MERGE
    # 320 MB: fp32 at 1436 ROIs (pinned 1435 / 1436), 16-bit at 2872
    assert ext.forward_plan(2, 64, 60, 80, 1436, 11, 83).kernel == ext.PLAN_KERNEL_SHIFT_LINES
    assert ext.forward_plan(2, 64, 60, 80, 1436, 11, 83, dtype=bf).kernel == ext.PLAN_KERNEL_STRIDED_MERGE
    assert ext.forward_plan(2, 64, 60, 80, 2871, 11, 83, dtype=bf).kernel == ext.PLAN_KERNEL_STRIDED_MERGE
    assert ext.forward_plan(2, 64, 60, 80, 2872, 11, 83, dtype=bf).kernel == ext.PLAN_KERNEL_SHIFT_LINES
    # counts: the two-launch crossover at 3.8 M output elements
    assert ext.forward_plan(1, 64, 160, 160, 115, 8, 64, dtype=bf).family == ext.PLAN_FWD_DIRECT_K2P
    assert ext.forward_plan(1, 64, 160, 160, 116, 8, 64, dtype=bf).family == ext.PLAN_FWD_TWO_LAUNCH
