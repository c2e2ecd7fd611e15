// rroi_detection_loss_host.h -- the native detection loss, host part: argument checks, the plan (a pure function of the
// shape: never of the device), the workspace, the launches.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_host_launch.h (status helpers, with_dtype).
#pragma once

// ------------------------------------------------------------------------------------
// The item space: N H W pixels of 1/4, then N H8 W8 pixels of 1/8 (none for a single scale, height8 == width8 == 0).
// Items per thread: 1 up to 4096 items in all, 2 up to 16384, 4 up to 262144, 8 beyond -- so that the reference's training
// shape (2 x 128 x 128 + 2 x 64 x 64 = 40960 items) is 40 workgroups and the finishing workgroup adds 40 slots, and the
// largest measured shape (8 x 176 x 320 + 8 x 88 x 160) 275.  A workgroup works on one scale: the grid is
// ceil(items4 / (256 ipt)) + ceil(items8 / (256 ipt)).  status 0: what the calls refuse before any launch.
// The workspace: grid slots of ten doubles, then the state of twenty.
// ------------------------------------------------------------------------------------
constexpr long long kDlMaxItems = 1LL << 30;       // per scale: every item index and the workgroup's overshoot fit in 32 bits

struct DlPlan {
    int status = 0;
    DlShape S{};
    long long items4 = 0, items8 = 0;
    unsigned grid = 0;
    size_t workspace_bytes = 0;
};

inline DlPlan plan_detection_loss(int dtype, int N, int H, int W, int H8, int W8)
{
    DlPlan P;
    if (!dtype_ok(dtype)) return P;
    if (N < 1 || H < 1 || W < 1 || H8 < 0 || W8 < 0 || (H8 == 0) != (W8 == 0)) return P;
    const long long hw4 = (long long)H * W, hw8 = (long long)H8 * W8;        // each below 2^62: no overflow
    if (hw4 > kDlMaxItems || hw8 > kDlMaxItems) return P;
    P.items4 = N * hw4;                                                      // below 2^61
    P.items8 = N * hw8;
    if (P.items4 > kDlMaxItems || P.items8 > kDlMaxItems) return P;
    const long long items = P.items4 + P.items8;
    const int ipt = items <= 4096 ? 1 : items <= 16384 ? 2 : items <= 262144 ? 4 : 8;
    const long long per = (long long)kDlThreads * ipt;
    P.S = DlShape{N, H, W, H8, W8, H8 > 1 ? (double)(H - 1) / (double)(H8 - 1) : 0.0, W8 > 1 ? (double)(W - 1) / (double)(W8 - 1) : 0.0,
                  (unsigned)((P.items4 + per - 1) / per), (unsigned)((P.items8 + per - 1) / per), ipt};
    P.grid = P.S.blocks4 + P.S.blocks8;
    P.workspace_bytes = ((size_t)P.grid * kDlSums + 2 * kDlSums) * sizeof(double);
    P.status = 1;
    return P;
}

inline bool dl_aligned(const void* p, size_t a) { return reinterpret_cast<size_t>(p) % a == 0; }

template <class T>
int launch_detection_loss_forward(const DlPlan& P, DlPreds<T> p4, DlPreds<T> p8, DlTruth gt, float* terms, void* workspace,
                                  hipStream_t stream)
{
    double* slots = static_cast<double*>(workspace);
    double* state = slots + (size_t)P.grid * kDlSums;
    hipLaunchKernelGGL((rroi_detection_loss_partial_kernel<T>), dim3(P.grid), dim3(kDlThreads), 0, stream, p4, p8, gt, P.S, slots);
    const int st = launch_status();
    if (st != 1) return st;
    hipLaunchKernelGGL(rroi_detection_loss_finish_kernel, dim3(1), dim3(kDlFinishThreads), 0, stream, slots, P.S.blocks4, P.S.blocks8,
                       state, terms);
    return launch_status();
}

template <class T>
int launch_detection_loss_backward(const DlPlan& P, DlPreds<T> p4, DlPreds<T> p8, DlTruth gt, const double* state, const float* gw,
                                   DlGrads<T> g4, DlGrads<T> g8, hipStream_t stream)
{
    hipLaunchKernelGGL((rroi_detection_loss_backward_kernel<T>), dim3(P.grid), dim3(kDlThreads), 0, stream, p4, p8, gt, P.S, state, gw,
                       g4, g8);
    return launch_status();
}
