"""The callers' kernels on bfloat16 / float16 data -- RBOX decode of a 16-bit detector's maps, greedy CTC of a 16-bit
head's log-probabilities -- as far as a machine without a GPU can check them: the two typed entry points exist, refuse
bad arguments before any launch, and the Python surface keeps checking the device before the dtype."""
import ctypes

import pytest
import torch

DTYPES = (torch.float32, torch.bfloat16, torch.float16)


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as E
    return E


def test_typed_callers_are_exported(ext):
    for name in ("rroi_rbox_decode_typed_hip", "rroi_ctc_greedy_decode_typed_hip"):
        assert name in ext.EXPORTS
        assert ctypes.cast(getattr(ext._lib, name), ctypes.c_void_p).value
    assert ext.version().startswith("rroi_align_hip 0.10.0")   # found by symbol, not by version


def test_typed_callers_refuse_before_any_launch(ext):
    """No GPU touched: host checks only (null pointers throughout)."""
    d = ext._lib.rroi_rbox_decode_typed_hip
    c = ext._lib.rroi_ctc_greedy_decode_typed_hip
    for bad in (3, -1):
        assert d(bad, None, None, None, 8, 8, 0.5, None, 0, None, None) == 0
        assert c(bad, None, 1, 4, 8, None, None, None, None, None) == 0
    for dt in (ext.DTYPE_FP32, ext.DTYPE_BF16, ext.DTYPE_FP16):
        assert d(dt, None, None, None, 8, 8, 0.5, None, 0, None, None) == 0          # null maps
        assert d(dt, None, None, None, 0, 8, 0.5, None, 0, None, None) == 0          # height <= 0
        assert d(dt, None, None, None, -1, 8, 0.5, None, 0, None, None) == 0
        assert d(dt, None, None, None, 8, 0, 0.5, None, 0, None, None) == 0
        assert d(dt, None, None, None, 8, 8, 0.5, None, -1, None, None) == 0         # capacity < 0
        assert c(dt, None, 1, 0, 8, None, None, None, None, None) == 0               # num_classes <= 0
        assert c(dt, None, 1, -2, 8, None, None, None, None, None) == 0
        assert c(dt, None, -1, 4, 8, None, None, None, None, None) == 0
        assert c(dt, None, 1, 4, -1, None, None, None, None, None) == 0
        assert c(dt, None, 1, 4, 8, None, None, None, None, None) == 0               # null logits / outputs
        assert c(dt, None, 0, 4, 8, None, None, None, None, None) == 1               # no sequence: nothing to do
    # the untyped entry points refuse the same
    assert ext._lib.rroi_rbox_decode_hip(None, None, None, 8, 8, 0.5, None, 0, None, None) == 0
    assert ext._lib.rroi_ctc_greedy_decode_hip(None, 1, 0, 8, None, None, None, None, None) == 0


@pytest.mark.parametrize("dtype", DTYPES + (torch.float64, torch.int32), ids=lambda d: str(d).replace("torch.", ""))
def test_cpu_tensors_are_refused_before_the_dtype_is_looked_at(dtype):
    """GPU only, for every dtype -- also for one the GPU call would refuse with TypeError: the device is checked first."""
    from rroi_align.decode import CTCLabelConverter, ctc_greedy_decode
    from rroi_align.nms import decode, decode_batch, get_boxes
    s, r, a = (torch.zeros(shape).to(dtype) for shape in ((6, 10), (4, 6, 10), (2, 6, 10)))
    with pytest.raises(RuntimeError, match="GPU only"):
        decode(s, r, a)
    with pytest.raises(RuntimeError, match="GPU only"):
        get_boxes(s, r, a)
    with pytest.raises(RuntimeError, match="GPU only"):
        decode_batch(s[None], r[None], a[None])
    logits = torch.zeros(2, 5, 7).to(dtype)
    with pytest.raises(RuntimeError, match="GPU only"):
        ctc_greedy_decode(logits)
    with pytest.raises(RuntimeError, match="GPU only"):
        CTCLabelConverter("abcd").decode_logits(logits)


def test_preprocess_signature_defaults_to_float32():
    import inspect
    from fots_e2e.pipeline import preprocess
    p = inspect.signature(preprocess).parameters
    assert list(p) == ["im_u8", "device", "dtype"] and p["dtype"].default is torch.float32
