"""CPU: the plan queries of the deterministic backward (RROI_PATH_DETERMINISTIC, plan RROI_PLAN_BWD_ORDERED).
With the bit, every native AUTO backward the library accepts -- every dtype, every layout pair -- plans ORDERED (the zero
fill for R = 0); explicit paths, the reference-ABI launcher and the forward refuse the bit."""
import os
import re

import pytest

import plan_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (0, 1, 2)   # DTYPE_FP32, DTYPE_BF16, DTYPE_FP16


@pytest.fixture(scope="module")
def ext():
    import torch  # noqa: F401  (the HIP runtime before the ctypes library)
    from rroi_align._ext import rroi_align as e
    return e


def _query(ext, c, dtype=0, deterministic=False, path=None, caller=None):
    try:
        return ext.backward_plan(c.B, c.C, c.H, c.W, c.R, c.ph, c.pw, top_diff_layout=c.fl, bottom_diff_layout=c.tl,
                                 path=c.path if path is None else path, caller=c.caller if caller is None else caller,
                                 dtype=dtype, deterministic=deterministic)
    except ValueError:
        return None


def _bwd_cases(native_auto):
    for c in PC.sweep():
        if c.kind == "bwd" and (c.path == PC.AUTO and c.caller == PC.NATIVE) == native_auto:
            yield c


def test_constants_are_the_headers(ext):
    with open(os.path.join(ROOT, "include", "rroi_align_hip.h")) as fh:
        text = fh.read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (RROI_\w+) (0x[0-9a-fA-F]+|\d+)", text)}
    assert defs["RROI_PATH_DETERMINISTIC"] == ext.PATH_DETERMINISTIC == 0x200
    assert defs["RROI_PLAN_BWD_ORDERED"] == ext.PLAN_BWD_ORDERED == 17
    assert not ext.PATH_DETERMINISTIC & (0xff | ext.PATH_TRIG_FP32)
    assert ext.version().startswith("rroi_align_hip 0.10.0")


def test_native_auto_plans_ordered(ext):
    """Every native AUTO backward of the sweep, in every dtype the typed query accepts: with the bit, ORDERED --
    written in place in the gradient's layout, channels-last top_diff read in place -- wherever the call without the
    bit is accepted and a gather can index the problem (an fp32 AUTO call falls back to the atomic scatter only where
    none can)."""
    n = 0
    for c in _bwd_cases(True):
        for dtype in DTYPES:
            base = _query(ext, c, dtype)
            det = _query(ext, c, dtype, deterministic=True)
            if base is None:
                assert det is None, (c, dtype)
                continue
            if base.family == ext.PLAN_BWD_ATOMIC:
                assert det is None, (c, dtype)
                continue
            assert det is not None, (c, dtype, base)
            assert det.family == ext.PLAN_BWD_ORDERED, (c, dtype, det)
            assert det.dest == (ext.PLAN_DST_NHWC if c.tl == PC.NHWC else ext.PLAN_DST_NCHW), (c, dtype, det)
            assert det.zero_copy == (c.fl == PC.NHWC), (c, dtype, det)
            assert not det.accumulate and det.raw_bsum in (0, 1) and det.grid_x > 0
            assert det == _query(ext, c, dtype, deterministic=True, path=PC.AUTO)   # the query is a pure function
            n += 1
    assert n > 1000


def test_zero_rois_plan_the_zero_fill(ext):
    for dtype in DTYPES:
        for fl, tl in ((0, 0), (0, 1), (1, 0), (1, 1)):
            if dtype and fl:
                continue   # 16-bit calls read an NCHW top_diff
            c = PC.Case("r0", "bwd", 2, 64, 120, 160, 0, 11, 96, "bench", fl, tl)
            plan = _query(ext, c, dtype, deterministic=True)
            assert plan is not None and plan.family == ext.PLAN_NONE, (dtype, fl, tl)


def test_explicit_paths_and_the_launcher_refuse_the_bit(ext):
    n = 0
    for c in _bwd_cases(False):
        assert _query(ext, c, deterministic=True) is None, c
        n += 1
    assert n > 1000
    c = PC.Case("x", "bwd", 1, 64, 120, 160, 64, 11, 83)
    for path in (PC.DIRECT, PC.TILED, PC.ATOMIC, PC.LISTS, PC.INKERNEL, PC.BUCKETS):
        for dtype in DTYPES:
            assert _query(ext, c, dtype, deterministic=True, path=path) is None, (path, dtype)
    assert _query(ext, c, deterministic=True, caller=PC.LAUNCHER) is None
    assert _query(ext, c, deterministic=True, caller=PC.LAUNCHER_CON_IDX) is None
    assert _query(ext, c, deterministic=True).family == ext.PLAN_BWD_ORDERED


def test_forward_refuses_the_bit(ext):
    """A backward flag: every forward plan is deterministic already, and the forward query refuses the bit as an unknown
    flag wherever it accepts the call without it (the forward entry points do the same: tests/test_abi.py)."""
    n = 0
    for c in PC.sweep():
        if c.kind != "fwd":
            continue
        for dtype in (0, 1):
            ok = []
            for bit in (0, ext.PATH_DETERMINISTIC):
                try:
                    ext.forward_plan(c.B, c.C, c.H, c.W, c.R, c.ph, c.pw, feature_layout=c.fl, top_layout=c.tl,
                                     path=c.path | bit, caller=c.caller, dtype=dtype)
                    ok.append(True)
                except ValueError:
                    ok.append(False)
            assert not ok[1], (c, dtype)
            n += ok[0]
    assert n > 1000
