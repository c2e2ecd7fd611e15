"""rroi_align._ext.rroi_align.callers -- the bindings of the callers' kernels (header section 4; `csrc/rroi_nms_host.h`
and the launches of `rroi_callers_kernels.h`): the RBOX decode and the host merge that `rroi_align.nms` and `decode` call
through `_lib`, and the greedy CTC decode that `batched` calls as `ctc_greedy_decode`."""
import torch

from ._core import _DTYPES, _IO_DTYPES, _bind, _check, _f, _i, _lib, _require_cuda_f32, _stream, _vp

_bind("rroi_nms_record_format", [])
_bind("rroi_rbox_decode_hip", [_vp, _vp, _vp, _i, _i, _f, _vp, _i, _vp, _vp])
_bind("rroi_nms_merge_host", [_vp, _i, _i, _i, _f, _f, _vp, _i])
_bind("rroi_ctc_greedy_decode_hip", [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp])
# ... on bfloat16 / float16 data (after 0.10.0, same version string: found by symbol)
_bind("rroi_rbox_decode_typed_hip", [_i, _vp, _vp, _vp, _i, _i, _f, _vp, _i, _vp, _vp])
_bind("rroi_ctc_greedy_decode_typed_hip", [_i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp])


def ctc_greedy_decode(logits: torch.Tensor, lengths=None, return_labels: bool = False):
    """(N, nclass, T) logits -> (decoded (N, T) int32 zero-padded, decoded_len (N,) int32
    [, raw arg-max labels (N, T) int32]), all on the device; one launch for all sequences.
    Replaces `labels_pred.max(1)` + strLabelConverter.decode (tools/ocr_utils.py:183-186).
    logits: float32, bfloat16 or float16 (a head that runs in 16 bits): a 16-bit element is widened exactly where the
    kernel loads it, so the result is that of the float32 call on `logits.float()`, ties and NaN included."""
    _require_cuda_f32(logits, "logits", _IO_DTYPES)
    code = _DTYPES[logits.dtype]
    if logits.dim() != 3:
        raise ValueError("logits must be (N, nclass, T)")
    logits = logits.contiguous()
    N, K, T = logits.shape
    if K == 0:
        raise ValueError("logits must have at least one class")
    with torch.cuda.device_of(logits):
        dev = logits.device
        if lengths is not None:
            lengths = torch.as_tensor(lengths, dtype=torch.int32, device=dev).contiguous()
            if lengths.numel() != N:
                raise ValueError("lengths must have one entry per sequence")
        decoded = torch.empty((N, T), dtype=torch.int32, device=dev)
        dlen = torch.empty((N,), dtype=torch.int32, device=dev)
        labels = torch.empty((N, T), dtype=torch.int32, device=dev) if return_labels else None
        st = _lib.rroi_ctc_greedy_decode_typed_hip(code, logits.data_ptr(), N, K, T,
                                                   lengths.data_ptr() if lengths is not None else None,
                                                   labels.data_ptr() if labels is not None else None,
                                                   decoded.data_ptr(), dlen.data_ptr(), _stream())
    _check(st, "rroi_ctc_greedy_decode_typed_hip")
    return (decoded, dlen, labels) if return_labels else (decoded, dlen)
