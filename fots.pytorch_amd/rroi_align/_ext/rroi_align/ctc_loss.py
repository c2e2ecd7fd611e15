"""rroi_align._ext.rroi_align.ctc_loss -- the binding of the native CTC loss (header section 15): the negative
log-likelihood of every sequence and the unscaled gradient with respect to the log-probabilities in one launch,
deterministic, for float32 / bfloat16 / float16 log-probabilities read where they lie.

A module of the binding like the package's own (`csrc/rroi_ctc_loss_host.h`), loaded on first use by `rroi_align.ctc`: the
package's `_*_run` callables are a closed list that the network's ledger test reads, so the hot call here is
`run_ctc_loss`.  Its workspace is `_core`'s per-stream scratch, the one table of the process.  The public surface (argument
forms, autograd, reductions) is rroi_align.ctc."""
import collections
import ctypes

import torch

from ._core import _DTYPES, DTYPE_FP32, _bind, _check, _i, _lib, _ll, _plan_query, _stream, _sz, _vp, _workspace, dtype_code


class _CtcLossPlan(ctypes.Structure):
    _fields_ = [(n, _i) for n in ("grid_x", "block", "lds_bytes", "lds_limit", "positions", "chunk_steps", "stage_along_t",
                                  "alpha_in_workspace")]


_bind("rroi_ctc_loss_forward_hip", [_i, _vp, _ll, _ll, _ll, _i, _i, _i, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _ll, _ll, _ll,
                                    _vp, _sz, _vp])
_bind("rroi_ctc_loss_plan", [_i] * 5 + [_ll, _ll, _i, ctypes.POINTER(_CtcLossPlan)])
_bind("rroi_ctc_loss_workspace_bytes", [_i] * 5, _sz)

CtcLossPlan = collections.namedtuple("CtcLossPlan", [n for n, _ in _CtcLossPlan._fields_])


def ctc_loss_plan(batch_size, classes, steps, max_target_length, stride_t=None, stride_k=1, want_grad=True,
                  dtype=DTYPE_FP32) -> CtcLossPlan:
    """What `run_ctc_loss` launches for (steps, batch_size, classes) log-probabilities and targets padded to
    max_target_length (host only, no GPU needed): grid, block, the LDS bytes and their limit, the positions S_max, the steps
    per chunk, whether the log-probabilities are staged along t, and whether the alpha rows live in the workspace.
    stride_t / stride_k: the element strides of log_probs (default: contiguous (T, N, K)).  ValueError where the call would
    refuse the arguments."""
    if stride_t is None:
        stride_t = int(batch_size) * int(classes)
    return _plan_query(_lib.rroi_ctc_loss_plan, _CtcLossPlan, CtcLossPlan, "rroi_ctc_loss_plan",
                       (dtype_code(dtype), batch_size, classes, steps, max_target_length, stride_t, stride_k, bool(want_grad)))


def ctc_loss_workspace_bytes(batch_size, classes, steps, max_target_length, want_grad=True) -> int:
    """Bytes of workspace the call needs (0: the alpha rows fit in LDS, or no gradient is wanted)."""
    return int(_lib.rroi_ctc_loss_workspace_bytes(int(batch_size), int(classes), int(steps), int(max_target_length),
                                                  int(bool(want_grad))))


def run_ctc_loss(log_probs, targets, input_lengths, target_lengths, blank=0, zero_infinity=False, want_grad=True, grad=None):
    """The call itself, for arguments already checked (rroi_align.ctc.ctc_loss): log_probs (T, N, K) float32 / bfloat16 /
    float16 on the GPU with any strides; targets (N, L_max) contiguous int32; input_lengths and target_lengths (N) contiguous
    int32, all on log_probs' device.  Returns (nll, grad): nll (N) float32; grad the unscaled gradient (`grad` where given --
    a tensor of log_probs' shape and dtype with any strides -- else a new tensor with log_probs' strides where those are
    dense), or None where want_grad is false, in which case the beta pass does not run."""
    index = log_probs.device.index
    if index != torch.cuda.current_device():
        with torch.cuda.device(index):
            return run_ctc_loss(log_probs, targets, input_lengths, target_lengths, blank, zero_infinity, want_grad, grad)
    T, N, K = log_probs.shape
    Lmax = targets.size(1)
    nll = torch.empty((N,), dtype=torch.float32, device=log_probs.device)
    if not want_grad:
        grad = None
    elif grad is None:
        grad = torch.empty_like(log_probs)          # every element is written by the launch: no memset
    if N == 0:
        return nll, grad
    nbytes = _lib.rroi_ctc_loss_workspace_bytes(N, K, T, Lmax, int(want_grad))
    ws = _workspace(log_probs.device, nbytes) if nbytes else None
    gs = grad.stride() if grad is not None else (0, 0, 0)
    st = _lib.rroi_ctc_loss_forward_hip(_DTYPES[log_probs.dtype], log_probs.data_ptr(), *log_probs.stride(), N, K, T,
                                        targets.data_ptr(), Lmax, input_lengths.data_ptr(), target_lengths.data_ptr(),
                                        int(blank), int(bool(zero_infinity)), nll.data_ptr(),
                                        grad.data_ptr() if grad is not None else None, *gs,
                                        ws.data_ptr() if ws is not None else None, nbytes, _stream())
    if st != 1:
        _check(st, "rroi_ctc_loss_forward_hip")
    return nll, grad
