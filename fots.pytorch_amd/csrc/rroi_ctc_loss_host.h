// rroi_ctc_loss_host.h -- the native CTC loss, host part: argument checks, the plan (a pure function of the shapes, the
// strides and whether a gradient is wanted), the one launch.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_host_launch.h (status helpers, with_dtype).
#pragma once

// ------------------------------------------------------------------------------------
// What rroi_ctc_loss_forward_hip launches: one workgroup of 256 threads per sequence.  status 0: what the call refuses
// before any launch.  S_max = 2 min(L_max, T) + 1 positions (a longer target is infeasible whatever the rest).
//
// LDS, in doubles: two recurrence rows of S_max for alpha and two for beta, the two staged chunks TC x S_max, the tile of
// class sums TC x K, and -- with a gradient, where they still fit in kCtcLdsLimit -- every alpha and beta row, 2 x T x S_max;
// then three int arrays of S_max and one flag.  TC, the steps per chunk, is 16 (a 64-byte run of float32 gradients along t) and halves
// while the chunk's three arrays exceed half the limit; a shape whose arrays do not fit at TC = 1 is refused.  Where the
// rows do not fit they live in the caller's workspace, N x 2 x T x S_max doubles, and only the combine reads them.
// ------------------------------------------------------------------------------------
constexpr long long kCtcLdsLimit = 64 * 1024;

struct CtcPlan {
    int status = 0;
    int smax = 0, chunk = 0, along_t = 0, rows_in_lds = 0;
    unsigned grid = 0;
    long long lds_bytes = 0;
    size_t workspace_bytes = 0;
};

inline CtcPlan plan_ctc_loss(int dtype, int N, int K, int T, int Lmax, long long stride_t, long long stride_k, int want_grad)
{
    CtcPlan P;
    if (!dtype_ok(dtype)) return P;
    if (N < 0 || K < 1 || T < 0 || Lmax < 0) return P;
    const long long smax = 2LL * std::min(Lmax, T) + 1;
    const long long fixed = 4 * smax * 8 + 3 * smax * 4 + 4;
    int tc = 16;
    while (tc > 1 && tc * (2 * smax + K) * 8 > kCtcLdsLimit / 2) tc /= 2;
    const long long base = fixed + tc * (2 * smax + K) * 8;
    if (base > kCtcLdsLimit) return P;
    const long long rows = 2LL * T * smax * 8;
    if ((long long)N * rows / 8 >= (1LL << 40)) return P;      // the workspace's element count stays far from overflow
    P.status = 1;
    P.smax = (int)smax;
    P.chunk = tc;
    P.along_t = stride_t == 1 && stride_k != 1;
    P.rows_in_lds = want_grad && base + rows <= kCtcLdsLimit;
    P.lds_bytes = base + (P.rows_in_lds ? rows : 0);
    P.workspace_bytes = want_grad && !P.rows_in_lds ? (size_t)N * (size_t)rows : 0;
    P.grid = (unsigned)N;
    return P;
}

template <class T>
int launch_ctc_loss(const CtcPlan& P, const T* lp, CtcStrides ls, int K, int Tmax, const int* targets, int Lmax,
                    const int* in_len, const int* tgt_len, int blank, int zero_infinity, float* nll, T* grad, CtcStrides gs,
                    void* workspace, hipStream_t stream)
{
    hipLaunchKernelGGL((rroi_ctc_loss_kernel<T>), dim3(P.grid), dim3(kCtcThreads), (size_t)P.lds_bytes, stream, lp, ls, K, Tmax,
                       targets, Lmax, in_len, tgt_len, blank, zero_infinity, nll, grad, gs, static_cast<double*>(workspace),
                       P.rows_in_lds, P.chunk);
    return launch_status();
}
