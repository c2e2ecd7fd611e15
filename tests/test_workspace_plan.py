"""CPU: the workspace table (tests/workspace_cases.py) against the host-only plan and size queries.  Every row runs
under the plan key it states, the rows together cover the REQUIRED sets written out in the table, and every size query
is positive and a multiple of 256 bytes -- so the table that tests/test_gpu_workspace.py runs stays honest on a machine
without a GPU, and fails by name when a threshold of the dispatch moves."""
import pytest

import plan_cases as PC
import workspace_cases as WC


@pytest.fixture(scope="module")
def ext():
    import torch  # noqa: F401  (the HIP runtime before the ctypes library)
    from rroi_align._ext import rroi_align as e
    return e


@pytest.mark.parametrize("row", WC.ROWS + WC.NO_WORKSPACE, ids=[r.case.name for r in WC.ROWS + WC.NO_WORKSPACE])
def test_row_plans_what_it_states(ext, row):
    assert WC.row_key(ext, row) == (row.case.kind,) + tuple(row.want)


@pytest.mark.parametrize("dtype", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("row", WC.HALF_ROWS, ids=[r.case.name for r in WC.HALF_ROWS])
def test_half_row_plans_what_it_states(ext, row, dtype):
    assert row.case.fl == PC.NCHW, "16-bit calls read NCHW features / grad_output"
    assert WC.row_key(ext, row, dtype) == (row.case.kind,) + tuple(row.want)


@pytest.mark.parametrize("dtype", [0, 1, 2], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("b", WC.BUCKETED + [WC.NO_WORKSPACE_BUCKETED], ids=lambda b: b.name)
def test_bucketed_row_plans_what_it_states(ext, b, dtype):
    widths = WC.bucketed_widths(b)
    assert len(widths) == b.R and set(widths) == set(b.choices)
    assert WC.bucketed_key(ext, b, dtype)[:len(b.want) + 1] == (b.kind,) + tuple(b.want)


def test_the_rows_cover_required(ext):
    got = {WC.row_key(ext, r) for r in WC.ROWS}
    assert got == WC.REQUIRED, (sorted(WC.REQUIRED - got, key=str), sorted(got - WC.REQUIRED, key=str))
    for dtype in (1, 2):
        got = {WC.row_key(ext, r, dtype) for r in WC.HALF_ROWS}
        assert got == WC.HALF_REQUIRED, (dtype, sorted(WC.HALF_REQUIRED - got, key=str), sorted(got - WC.HALF_REQUIRED, key=str))
    for dtype in (0, 1, 2):
        assert {WC.bucketed_key(ext, b, dtype) for b in WC.BUCKETED} == WC.BUCKETED_REQUIRED, dtype
    none = {WC.row_key(ext, r) for r in WC.NO_WORKSPACE} | {WC.bucketed_key(ext, WC.NO_WORKSPACE_BUCKETED)[:3]}
    assert none == WC.NO_WORKSPACE_REQUIRED, none


def test_forward_copy_rows_run_on_two_maps():
    maps = {}
    for r in WC.FORWARD:
        maps.setdefault(r.case.name.rsplit("_", 1)[0], set()).add((r.case.H, r.case.W))
    for name, m in maps.items():
        copy = WC.ROW[next(n for n in WC.ROW if n.startswith(name + "_1"))].want[-1] == "copy"
        assert len(m) == (2 if copy else 1) and m <= set(WC.MAPS), (name, m)
    assert {hw for m in maps.values() for hw in m} == set(WC.MAPS)


def test_every_size_query_is_positive_and_a_multiple_of_256(ext):
    for r in WC.ROWS:
        n = WC.workspace_bytes(ext, r)
        assert n > 0 and n % 256 == 0, (r.case.name, n)
    for b in WC.BUCKETED:
        n = WC.bucketed_workspace_bytes(ext, b)
        assert n > 0 and n % 256 == 0, (b.name, n)
    # the sizes the table was written around
    assert WC.workspace_bytes(ext, WC.ROW["f_strided_13x18"]) == 128768
    assert WC.workspace_bytes(ext, WC.ROW["f_shift_zero_copy_13x18"]) == 1792      # the affine and sort tables only
    assert 70 << 20 < WC.workspace_bytes(ext, WC.ROW["b_lists_scan2"]) < 80 << 20
    c = WC.ROW["f_merge_13x18"].case
    assert c.R * c.C * c.ph * c.pw * 4 >= 48 << 20                                 # what makes it the merging form


def test_the_chains_row_plans_the_bucket_it_overflows(ext):
    assert WC.plan_of(ext, WC.ROW["b_buckets_chains"]).kshift == WC.CHAINS_KSHIFT


def test_the_long_list_rows_have_their_long_lists(ext, oracle):
    """The chains row: some pixel's list is longer than its bucket.  The queue row: some list is longer than the register
    sort takes (kSortRegCap), so it goes through the queue that lives in the pixel counters.  Their plan keys are those
    of the plain rows: only the lists' lengths tell them apart."""
    from test_gpu_plan_coverage import distinct_bins_per_pixel
    for name, least in (("b_buckets_chains", 1 << WC.CHAINS_KSHIFT), ("b_ordered_queue", WC.SORT_REGISTER_CAP)):
        c = WC.ROW[name].case
        f, r = PC.inputs(c)
        assert int(distinct_bins_per_pixel(oracle, f.shape, r, c.ph, c.pw).max()) > least, name


def test_the_carve_recomputation_is_the_librarys_and_the_offsets_move_both_roundings(ext):
    """backward_used_bytes restates carve_bwd on the host: its total is the size query's for every backward row.  The
    four offsets give the FIRST rounding to 4 KiB four different values; the second starts from a page boundary, so it
    depends on the pair storage's size alone: the rows differ in it, the offsets do not.  What is left of the flat 8192
    bytes is the tail the GPU test checks like a guard."""
    shapes = [(r.case.name, (r.case.B, r.case.C, r.case.H, r.case.W, r.case.R, r.case.ph, r.case.pw), WC.workspace_bytes(ext, r))
              for r in WC.BACKWARD]
    shapes += [(b.name, (b.B, b.C, b.H, b.W, b.R, b.ph, max(b.choices)), WC.bucketed_workspace_bytes(ext, b))
               for b in WC.BUCKETED if b.kind == "bwd"]
    seconds = set()
    for name, shape, nbytes in shapes:
        r1s, r2s = set(), set()
        for off in WC.OFFSETS:
            used, (r1, r2), total = WC.backward_used_bytes(ext, *shape, off)
            assert total == nbytes, (name, total, nbytes)
            assert used == nbytes - (8192 - r1 - r2) and 0 <= r1 < 4096 and 0 <= r2 < 4096 and used % 256 == 0
            r1s.add(r1)
            r2s.add(r2)
        assert len(r1s) == len(WC.OFFSETS) and max(r1s) > 0 and len(r2s) == 1, (name, r1s, r2s)
        seconds |= r2s
    assert len(seconds) >= 3 and max(seconds) > 0, seconds


def test_the_forward_carve_recomputation_is_the_librarys(ext):
    """forward_used_bytes restates carve on the host: it is the size query for every forward row and every bucketed
    forward row, and for a shape whose five extents all differ -- so that one of them taken for another shows."""
    for r in WC.FORWARD:
        c = r.case
        assert WC.forward_used_bytes(c.B, c.C, c.H, c.W, c.R, c.fl) == WC.workspace_bytes(ext, r), c.name
    for b in WC.BUCKETED + [WC.NO_WORKSPACE_BUCKETED]:
        if b.kind == "fwd":
            assert WC.forward_used_bytes(b.B, b.C, b.H, b.W, b.R, PC.NCHW) == WC.bucketed_workspace_bytes(ext, b), b.name
    B, C, H, W, R = 3, 40, 17, 29, 5
    assert WC.forward_used_bytes(B, C, H, W, R, PC.NCHW) == 380160
    assert int(ext._lib.rroi_align_forward_workspace_bytes(B, C, H, W, R, PC.NCHW)) == 380160
    assert int(ext._lib.rroi_align_forward_bucketed_workspace_bytes(B, C, H, W, R)) == 380160
    assert int(ext._lib.rroi_align_forward_workspace_bytes(B, C, H, W, R, PC.NHWC)) == WC.forward_used_bytes(B, C, H, W, R, PC.NHWC)


def test_not_run_names_its_reasons():
    assert len(WC.NOT_RUN) == 2 and all(len(v) > 40 for v in WC.NOT_RUN.values())
