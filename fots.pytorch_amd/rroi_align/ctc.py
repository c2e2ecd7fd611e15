"""rroi_align.ctc -- the training-time twin of rroi_align.decode: a native CTC loss with `torch.nn.functional.ctc_loss`'s
signature and reductions.

What it adds to the stock loss: a DETERMINISTIC gradient (no atomic, every sum in a fixed order, so it runs under
`torch.use_deterministic_algorithms(True)` and gives the same bits on every run), float32 / bfloat16 / float16
log-probabilities without a widening copy, and the recogniser's (N, K, T) output read where it lies --
`net.forward_ocr(x).permute(2, 0, 1)` is accepted as it is.  One launch gives the loss of every sequence and the unscaled
gradient; autograd's backward is a broadcast multiply.  Everything is evaluated in double (include/rroi_align_hip.h
section 15 is the arithmetic contract); the losses come out in float32 whatever the input's dtype.

Where it differs from the stock loss on purpose: the gradient is 0, not NaN, where a log-probability is -inf and for a
sequence whose loss is infinite; a sequence with a label outside [0, K), a target length beyond the targets' width or the
time steps, or an input length outside [0, T] has loss +inf (0 with zero_infinity) and gradient 0 instead of undefined
behaviour.  GPU only, as the rest of the package."""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from ._ext.rroi_align import _IO_DTYPES, _require_cuda_f32
from ._ext.rroi_align.ctc_loss import run_ctc_loss

_REDUCTIONS = ("none", "mean", "sum")


def _lengths(v, name, N, device):
    """A length argument as it came -> (device int32 tensor or None, host list or None): exactly one is set."""
    if isinstance(v, torch.Tensor):
        if v.dtype not in (torch.int32, torch.int64) or v.dim() != 1 or v.numel() != N:
            raise ValueError(f"{name} must be {N} int32 or int64 lengths, got {tuple(v.shape)} of {v.dtype}")
        if v.is_cuda:
            if v.device != device:
                raise ValueError(f"{name} is on {v.device}, log_probs on {device}")
            if v.dtype == torch.int64:
                v = v.clamp(-1, 2 ** 31 - 1)      # so that narrowing cannot carry an out-of-range length into range
            return v.to(torch.int32).contiguous(), None
        v = v.tolist()
    try:
        host = [int(x) for x in v]
    except TypeError:
        raise ValueError(f"{name} must be a list, a tuple or a tensor of {N} lengths, got {v!r}") from None
    if len(host) != N:
        raise ValueError(f"{name} must hold {N} lengths, got {len(host)}")
    return None, host


def _prepare(log_probs, targets, input_lengths, target_lengths):
    """Checked arguments -> what run_ctc_loss takes: log_probs (copied only where neither stride_t nor stride_k is 1),
    padded int32 targets, int32 device lengths.  Host lists go up in one copy; device tensors are never read back."""
    _require_cuda_f32(log_probs, "log_probs", _IO_DTYPES)
    if log_probs.dim() != 3:
        raise ValueError(f"log_probs must be (T, N, K), got {tuple(log_probs.shape)}")
    T, N, K = log_probs.shape
    if K < 1:
        raise ValueError("log_probs must have at least one class")
    dev = log_probs.device
    _require_cuda_f32(targets, "targets", (torch.int32, torch.int64))
    if targets.device != dev:
        raise ValueError(f"targets is on {targets.device}, log_probs on {dev}")
    if targets.dim() not in (1, 2) or (targets.dim() == 2 and targets.size(0) != N):
        raise ValueError(f"targets must be flat (sum L,) or padded ({N}, L_max), got {tuple(targets.shape)}")
    in_dev, in_host = _lengths(input_lengths, "input_lengths", N, dev)
    tg_dev, tg_host = _lengths(target_lengths, "target_lengths", N, dev)
    st, _, sk = log_probs.stride()
    if not (st == 1 or sk == 1 or T == 1 or K == 1):
        log_probs = log_probs.contiguous()
    if targets.dtype == torch.int64:
        targets = targets.clamp(-1, K)          # so that narrowing cannot carry an out-of-range label into range
    targets = targets.to(torch.int32)

    flat = targets.dim() == 1
    # the padded width of flat targets: the longest target where the lengths are on the host, else the most one can be
    width = (max(tg_host, default=0) if tg_host is not None else min(targets.numel(), T)) if flat else targets.size(1)
    width = max(0, min(width, targets.numel())) if flat else width
    index_host = None
    if flat and tg_host is not None and width > 0 and N > 0:
        # the gather that pads them, built on the host and uploaded with the lengths
        lens = np.maximum(np.asarray(tg_host, dtype=np.int64), 0)
        start = np.cumsum(lens) - lens
        index_host = np.clip(start[:, None] + np.arange(width)[None, :], 0, targets.numel() - 1).reshape(-1)
    host = np.concatenate([np.asarray(v, dtype=np.int64).reshape(-1) for v in (in_host, tg_host, index_host) if v is not None] or
                          [np.zeros(0, dtype=np.int64)])
    up = torch.from_numpy(np.clip(host, -1, 2 ** 31 - 1).astype(np.int32)).to(dev) if host.size else None
    pos = 0
    if in_host is not None:
        in_dev, pos = up[pos:pos + N], pos + N
    if tg_host is not None:
        tg_dev, pos = up[pos:pos + N], pos + N
    if not flat:
        padded = targets.contiguous()
    elif width == 0 or N == 0:
        padded = torch.zeros((N, 0), dtype=torch.int32, device=dev)
    elif index_host is not None:
        padded = targets[up[pos:].long()].view(N, width)
    else:
        lens = tg_dev.long().clamp(min=0)
        start = torch.cumsum(lens, 0) - lens
        index = (start[:, None] + torch.arange(width, device=dev)[None, :]).clamp(max=targets.numel() - 1)
        padded = targets[index]
    return log_probs, padded, in_dev, tg_dev


class _CTCLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_probs, targets, input_lengths, target_lengths, blank, zero_infinity, want):
        nll, grad = run_ctc_loss(log_probs, targets, input_lengths, target_lengths, blank, zero_infinity, want)
        if want:
            ctx.save_for_backward(grad)
        return nll

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        grad, = ctx.saved_tensors
        g = grad_output.to(torch.float32).view(1, -1, 1)
        if grad.dtype == torch.float32:
            return grad * g, None, None, None, None, None, None
        return (grad.to(torch.float32) * g).to(grad.dtype), None, None, None, None, None, None


def ctc_loss(log_probs, targets, input_lengths, target_lengths, blank=0, reduction="mean", zero_infinity=False):
    """`torch.nn.functional.ctc_loss` on the GPU, native and deterministic.
    log_probs: (T, N, K) float32, bfloat16 or float16, any strides with stride_t == 1 or stride_k == 1 (so both torch's
    contiguous layout and `net.forward_ocr(x).permute(2, 0, 1)`); any other striding takes one contiguous copy.
    targets: flat (sum L,) or padded (N, L_max), int32 or int64, on the same device.  input_lengths, target_lengths: lists,
    tuples or int tensors on either device; device tensors cause no host synchronisation.  Returns float32: (N,) for
    'none', a scalar for 'sum' and for 'mean' (each loss divided by its target length clamped to 1, then averaged).
    RuntimeError for CPU tensors, TypeError for other dtypes, ValueError for bad shapes or arguments."""
    if reduction not in _REDUCTIONS:
        raise ValueError(f"reduction must be one of {_REDUCTIONS}, got {reduction!r}")
    log_probs, padded, in_len, tg_len = _prepare(log_probs, targets, input_lengths, target_lengths)
    K = log_probs.size(2)
    if not 0 <= int(blank) < K:
        raise ValueError(f"blank must be in [0, {K}), got {blank!r}")
    want = torch.is_grad_enabled() and log_probs.requires_grad      # else the beta pass and the gradient store are skipped
    nll = _CTCLoss.apply(log_probs, padded, in_len, tg_len, int(blank), bool(zero_infinity), want)
    if reduction == "none":
        return nll
    if reduction == "sum":
        return nll.sum()
    return (nll / tg_len.clamp(min=1).to(torch.float32)).mean()


class CTCLoss(torch.nn.Module):
    """`torch.nn.CTCLoss` with the native loss behind it: the same keywords, `ctc_loss` above in forward."""

    def __init__(self, blank=0, reduction="mean", zero_infinity=False):
        super().__init__()
        if reduction not in _REDUCTIONS:
            raise ValueError(f"reduction must be one of {_REDUCTIONS}, got {reduction!r}")
        self.blank, self.reduction, self.zero_infinity = blank, reduction, zero_infinity

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        return ctc_loss(log_probs, targets, input_lengths, target_lengths, self.blank, self.reduction, self.zero_infinity)
