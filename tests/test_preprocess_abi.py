"""CPU: native preprocessing -- the two entry points are exported, declared and host-checked; the plan query
is pure and equals the mirrored rule; the Python surface refuses CPU tensors and bad arguments; `preprocess_ok` needs no
GPU and declines each disqualifying property; the pipeline's new keyword defaults to off and `preprocess` keeps its
signature; the float64 restatement, rounded once, is within the stock chain's own error of `preprocess` on the CPU and
equals it bit for bit where no resize happens.  No kernel is launched here."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import preprocess_cases as PC
from test_abi import declared_functions

NAMES = ("rroi_preprocess_forward_hip", "rroi_preprocess_plan")
FP32, BF16, FP16 = 0, 1, 2
P = 0x7f0000000000   # non-null, never dereferenced: every call it is passed to is refused on the host


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


@pytest.fixture(scope="module")
def pp():
    from rroi_align._ext.rroi_align import preprocess
    return preprocess


def test_symbols_are_exported_and_declared(ext, pp):
    lib = ctypes.CDLL(ext.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions() and name in ext.EXPORTS and hasattr(lib, name), name
    assert ext.version() == "rroi_align_hip 0.10.0 gfx950"      # the version string stays
    # the package's `_*_run` callables stay the closed list the network's ledger reads
    assert not any(k.startswith("_") and k.endswith("_run") for k in vars(pp))
    assert callable(pp.run_preprocess_images) and callable(pp.preprocess_images) and callable(pp.preprocess_plan)


def test_plan_query_equals_the_mirrored_rule(pp):
    shapes = [(len(c[0]), c[1]) for c in PC.CASES] + [(1, (704, 1280)), (2, (704, 1280)), (8, (704, 1280)), (2, (512, 1024))]
    for n, size in shapes:
        for dtype in PC.DTYPES:
            p = pp.preprocess_plan(n, size[0], size[1], dtype)
            assert (p.columns_per_thread, p.rows_per_thread, p.strips, p.bands, p.items, p.grid_x, p.wide_store) == \
                PC.plan_of(n, size, dtype), (n, size, dtype)
            assert p.block == 256
            # a sane grid: every output element belongs to exactly one item's run, no workgroup is empty
            assert p.strips * p.columns_per_thread >= size[1] > (p.strips - 1) * p.columns_per_thread
            assert p.bands * p.rows_per_thread >= size[0] > (p.bands - 1) * p.rows_per_thread
            assert p.grid_x * 256 >= p.items > (p.grid_x - 1) * 256 or (n == 0 and p.grid_x == 0)
            assert pp.preprocess_plan(n, size[0], size[1], dtype) == p                   # pure
    # the workload: a batch of eight shares geometry over four rows, a single image keeps its waves
    assert pp.preprocess_plan(8, 704, 1280, torch.bfloat16)[:4] == (880, 256, 8, 4)
    assert pp.preprocess_plan(1, 704, 1280, torch.bfloat16)[:4] == (440, 256, 8, 1)
    assert pp.preprocess_plan(2, 704, 1280, torch.bfloat16).rows_per_thread == 2
    assert pp.preprocess_plan(2, 512, 1024, torch.float32).rows_per_thread == 4
    assert {pp.preprocess_plan(1, c[1][0], c[1][1], torch.bfloat16).wide_store for c in PC.CASES} == {0, 1}


BAD = ((-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -4, 8), (1, 8, -4),
       (1, 1 << 15, 1 << 15), (3, 1 << 14, 1 << 14), (1 << 30, 1, 1), (0x7fffffff, 0x7fffffff, 0x7fffffff))


def test_refusals_return_zero_before_any_launch(ext, pp):
    call, plan = ext._lib.rroi_preprocess_forward_hip, ext._lib.rroi_preprocess_plan
    info = pp._PreprocessPlan()
    for dtype in (3, -1):
        assert call(dtype, P, P, P, 1, 8, 8, None) == 0
        assert plan(dtype, 1, 8, 8, ctypes.byref(info)) == 0
    for dtype in (FP32, BF16, FP16):
        assert plan(dtype, 1, 8, 8, ctypes.byref(info)) == 1 and plan(dtype, 1, 1, 1, ctypes.byref(info)) == 1
        assert plan(dtype, 1, 8, 8, None) == 0
        for dims in BAD:
            assert call(dtype, P, P, P, *dims, None) == 0, dims
            assert plan(dtype, *dims, ctypes.byref(info)) == 0, dims
        for ptrs in ((None, P, P), (P, None, P), (P, P, None)):                  # a NULL pointer with batch_size > 0
            assert call(dtype, *ptrs, 1, 8, 8, None) == 0
        assert call(dtype, None, None, None, 0, 8, 8, None) == 1                 # N == 0 is a no-op, whatever the pointers
        assert plan(dtype, 0, 8, 8, ctypes.byref(info)) == 1 and info.grid_x == 0 and info.items == 0
    with pytest.raises(ValueError):
        pp.preprocess_plan(1, 0, 8)
    with pytest.raises(TypeError):
        pp.preprocess_plan(1, 8, 8, torch.float64)


def test_binding_refuses_cpu_tensors_and_bad_arguments(pp):
    src, table = torch.zeros(3 * 4 * 4, dtype=torch.uint8), torch.tensor([[0, 4, 4, 0]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU only"):
        pp.preprocess_images(src, table, (8, 8), torch.float32)
    with pytest.raises(TypeError):
        pp.preprocess_images(src, table, (8, 8), torch.float64)
    with pytest.raises(TypeError):
        pp.preprocess_images(src.numpy(), table, (8, 8), torch.float32)


def test_preprocess_ok_needs_no_gpu_and_declines(monkeypatch):
    import fots_e2e.pipeline as pl
    dev = torch.device("cuda", 0)
    im = PC.image(64, 96, "random", 0)
    assert pl.preprocess_ok([im], dev) and pl.preprocess_ok([im, im], "cuda") and pl.preprocess_ok((im,), "cuda:1")
    for dtype in PC.DTYPES:
        assert pl.preprocess_ok([im], dev, dtype)
    # different sources that resize to one size
    assert pl.preprocess_ok([PC.image(70, 100, "random", 1), PC.image(64, 127, "random", 2)], dev)
    assert not pl.preprocess_ok([im], torch.device("cpu")) and not pl.preprocess_ok([im], "cpu")
    assert not pl.preprocess_ok([], dev)
    assert not pl.preprocess_ok(torch.zeros(1, 3, 64, 96), dev)                       # already preprocessed
    assert not pl.preprocess_ok([im.astype(np.float32)], dev)                         # float images
    assert not pl.preprocess_ok([PC.image(64, 192, "random", 0)[:, ::2]], dev)        # non-contiguous
    assert not pl.preprocess_ok([np.asfortranarray(im)], dev)
    assert not pl.preprocess_ok([im[:, :, 0]], dev) and not pl.preprocess_ok([im[:, :, :2]], dev)
    assert not pl.preprocess_ok([torch.from_numpy(im)], dev)
    assert not pl.preprocess_ok([im, PC.image(96, 96, "random", 3)], dev)             # mixed target sizes
    assert not pl.preprocess_ok([PC.image(20, 30, "random", 0)], dev)                 # resizes to nothing
    assert not pl.preprocess_ok([im], dev, torch.float64)
    monkeypatch.setattr(pl, "_preprocess_slower", lambda n, size, dtype: True)        # the hook declines
    assert not pl.preprocess_ok([im], dev)


def test_preprocess_batch_raises_the_batch_error_for_mixed_sizes():
    import fots_e2e.pipeline as pl
    ims = [PC.image(64, 96, "random", 0), PC.image(96, 96, "random", 1)]
    with pytest.raises(ValueError, match="must resize to one size"):
        pl.preprocess_batch(ims, "cuda")
    with pytest.raises(ValueError, match="must resize to one size"):
        pl._front_input(ims, "cpu", torch.float32, True)
    with pytest.raises(TypeError):
        pl.preprocess_batch([ims[0].astype(np.float32)], "cuda")


def test_keywords_default_off_and_preprocess_keeps_its_signature():
    import fots_e2e.pipeline as pl
    assert list(inspect.signature(pl.preprocess).parameters) == ["im_u8", "device", "dtype"]
    assert list(inspect.signature(pl.preprocess_batch).parameters) == ["ims", "device", "dtype"]
    assert inspect.signature(pl.preprocess_batch).parameters["dtype"].default == torch.float32
    assert list(inspect.signature(pl.preprocess_ok).parameters)[:2] == ["ims", "device"]
    for fn in (pl.infer_image, pl.infer_batch, pl.infer_stream, pl._batch_front):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "native_preprocess" and params[-1].default is False, fn.__name__


def test_keyword_on_a_cpu_device_runs_the_stock_front():
    import fots_e2e.pipeline as pl
    im = PC.image(90, 161, "random", 5)
    want = pl.preprocess(im, "cpu")
    assert torch.equal(pl._front_input([im], "cpu", torch.float32, True), want)
    assert torch.equal(pl._front_input([im], "cpu", torch.float32, False), want)


@pytest.mark.parametrize("h0,w0", [(90, 161), (45, 77), (720, 1280)])
def test_restatement_is_within_the_stock_chains_error_of_preprocess(h0, w0):
    from fots_e2e.pipeline import preprocess, resize_rule
    im = PC.image(h0, w0, "random", 3)
    size = resize_rule(h0, w0)
    assert size != (h0, w0) and min(size) >= 32
    ref = PC.ref64(im, size)
    stock = preprocess(im, "cpu")[0].numpy()
    assert stock.shape == ref.shape
    want = PC.rounded(ref, torch.float32).numpy()
    err_stock = float(np.abs(stock.astype(np.float64) - ref).max())
    err_ref32 = float(np.abs(want.astype(np.float64) - ref).max())
    bound = PC.stock_error_bound(h0, w0)
    print("(%d, %d) -> %s: stock %.3e, restatement rounded once %.3e, bound %.3e" % (h0, w0, size, err_stock, err_ref32, bound))
    assert err_ref32 <= 2.0 ** -24                       # one rounding of a value in [-1, 1)
    assert err_ref32 <= err_stock <= bound
    assert float(np.abs(want.astype(np.float64) - stock).max()) <= bound
    for dtype in (torch.bfloat16, torch.float16):        # both are within one 16-bit rounding of the same double
        u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
        d = (PC.rounded(ref, dtype).double() - preprocess(im, "cpu", dtype)[0].double()).abs().max()
        assert float(d) <= 2 * u + bound


def test_restatement_equals_preprocess_bit_for_bit_where_nothing_is_resized():
    from fots_e2e.pipeline import preprocess, resize_rule
    for fill in ("random", "full", "checker"):
        im = PC.image(64, 96, fill, 9)
        assert resize_rule(64, 96) == (64, 96)
        ref = PC.ref64(im, (64, 96))
        for dtype in PC.DTYPES:
            assert torch.equal(PC.bits(PC.rounded(ref, dtype)), PC.bits(preprocess(im, "cpu", dtype)[0])), (fill, dtype)


def test_case_table_covers_what_it_claims():
    offs = PC.pack(PC.images_of(PC.CASES[8]))[1][:, 0]
    assert len(offs) == 3 and offs[1] % 2 == 1 and offs[2] % 2 == 1
    assert len({tuple(s) for s in PC.CASES[8][0]}) == 3
    assert any(len(c[0]) == 0 for c in PC.CASES)
    assert {c[2] for c in PC.CASES} == {"random", "full", "checker"}
    chk = PC.image(4, 4, "checker", 0)
    assert set(np.unique(chk)) == {0, 255} and chk[0, 0, 0] != chk[0, 1, 0] and chk[0, 0, 0] != chk[1, 0, 0]
    # the restatement's edges: identity reads the source as it is; the far taps are clamped
    i0, i1, l = PC.axis(33, 64)
    assert i0.max() == 32 and i1.max() == 32 and l.min() >= 0 and l.max() < 1 and l[0] == 0
    i0, i1, l = PC.axis(64, 64)
    assert np.array_equal(i0, np.arange(64)) and np.array_equal(i0, i1) and not l.any()
