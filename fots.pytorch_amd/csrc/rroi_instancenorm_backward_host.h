// rroi_instancenorm_backward_host.h -- InstanceNorm2d's training forward and backward, host part: the
// backward's form rule, its workspace, the launches.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_instancenorm_host.h (the rule's body, InormPlan).
#pragma once

// ------------------------------------------------------------------------------------
// The backward's rule between the two forms is the forward's (plan_inorm_forms) with thresholds of its own, which start
// where the forward's are (DESIGN 5.24 has what was measured).  Its workspace: one {t1, t2} pair of doubles per plane,
// which the parameter-gradient kernel reads, and behind it -- split form only -- one pair per workgroup of the partials
// launch.  The size query knows neither the dtype nor which gradients a call wants: it answers for both regions.
// ------------------------------------------------------------------------------------
#ifndef RROI_INORM_BWD_SPLIT_MIN_PLANE          // (a measurement build may move the threshold, as the forward's)
#define RROI_INORM_BWD_SPLIT_MIN_PLANE 32768
#endif
#ifndef RROI_INORM_BWD_SPLIT_PLANES_PER_CU
#define RROI_INORM_BWD_SPLIT_PLANES_PER_CU 1
#endif
constexpr unsigned kInBwdSplitMinPlane = RROI_INORM_BWD_SPLIT_MIN_PLANE;
constexpr unsigned kInBwdSplitPlanesPerCu = RROI_INORM_BWD_SPLIT_PLANES_PER_CU;

struct InormBwdPlan {
    InormPlan P;               // form, planes, segments, grid; P.ws_bytes: the partials' region
    size_t sums_bytes = 0;     // the plane pairs' region, in front of the partials
    size_t ws_bytes = 0;
};

inline InormBwdPlan plan_instancenorm_backward(int dtype, int batch_size, int channels, int height, int width, int cus)
{
    InormBwdPlan B;
    B.P = plan_inorm_forms(dtype, batch_size, channels, height, width, cus, kInBwdSplitMinPlane, kInBwdSplitPlanesPerCu);
    if (!B.P.status) return B;
    B.sums_bytes = align_up((size_t)B.P.planes * sizeof(double2), 256);
    B.ws_bytes = B.sums_bytes + B.P.ws_bytes;
    return B;
}

// the training forward under the forward's plan: its launches with the {mean, var} store
template <class T>
int launch_instancenorm_train(const InormPlan& P, const T* x, const T* gamma, const T* beta, T* y, double2* stats, unsigned C,
                              double eps, float slope, void* workspace, hipStream_t stream)
{
    if (P.form == RROI_INORM_PLANE) {
        hipLaunchKernelGGL(rroi_inorm_train_plane_kernel<T>, dim3(P.grid), dim3(kInThreads), 0, stream, x, gamma, beta, y, stats,
                           C, P.n, P.planes, eps, slope);
        return launch_status();
    }
    double2* pairs = static_cast<double2*>(workspace);
    hipLaunchKernelGGL(rroi_inorm_stats_kernel<T>, dim3(P.grid), dim3(kInThreads), 0, stream, x, pairs, P.n, P.seg, P.nseg);
    const int st = launch_status();
    if (st != 1) return st;
    hipLaunchKernelGGL(rroi_inorm_train_apply_kernel<T>, dim3(P.grid), dim3(kInThreads), 0, stream, x, gamma, beta, y, stats,
                       pairs, C, P.n, P.seg, P.nseg, eps, slope);
    return launch_status();
}

// dx and / or (dgamma, dbeta); `workspace` may be NULL where neither the split form nor parameter gradients need it
template <class T>
int launch_instancenorm_backward(const InormBwdPlan& B, const T* dy, const T* x, const double2* stats, const T* gamma,
                                 const T* beta, T* dx, T* dgamma, T* dbeta, unsigned N, unsigned C, double eps, float slope,
                                 void* workspace, hipStream_t stream)
{
    const InormPlan& P = B.P;
    double2* sums = dgamma ? static_cast<double2*>(workspace) : nullptr;
    int st;
    if (P.form == RROI_INORM_PLANE) {
        hipLaunchKernelGGL(rroi_inorm_bwd_plane_kernel<T>, dim3(P.grid), dim3(kInThreads), 0, stream, dy, x, stats, gamma, beta,
                           dx, sums, C, P.n, P.planes, eps, slope);
        st = launch_status();
    } else {
        double2* pairs = reinterpret_cast<double2*>(static_cast<char*>(workspace) + B.sums_bytes);
        hipLaunchKernelGGL(rroi_inorm_bwd_partial_kernel<T>, dim3(P.grid), dim3(kInThreads), 0, stream, dy, x, stats, gamma,
                           beta, pairs, C, P.n, P.seg, P.nseg, eps, slope);
        st = launch_status();
        if (st != 1) return st;
        hipLaunchKernelGGL(rroi_inorm_bwd_apply_kernel<T>, dim3(P.grid), dim3(kInThreads), 0, stream, dy, x, stats, gamma, beta,
                           dx, pairs, sums, C, P.n, P.seg, P.nseg, eps, slope);
        st = launch_status();
    }
    if (st != 1 || !dgamma) return st;
    hipLaunchKernelGGL(rroi_inorm_bwd_param_kernel<T>, dim3((C + kInThreads - 1) / kInThreads), dim3(kInThreads), 0, stream,
                       sums, dgamma, dbeta, N, C);
    return launch_status();
}
