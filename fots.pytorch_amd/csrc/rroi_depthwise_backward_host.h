// rroi_depthwise_backward_host.h -- the depthwise 3x3 convolution's backward, host part: its band and
// segment rules, its workspace, the launches.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_depthwise_host.h (depthwise_shape_ok,
// depthwise_band).
#pragma once

// ------------------------------------------------------------------------------------
// All three kernels stream rows of dy, kDwCols columns per thread, so all three take their band height from the forward's
// rule on dy's planes: depthwise_band(N * C, Ho, Wo).  (At stride 2 a dx thread owns 2 * band dx rows and 2 * kDwCols dx
// columns.)  The partials launch is plane-aligned: a plane's ceil(Ho / band) * ceil(Wo / kDwCols) items go to
// `segments` = ceil(items / kDwThreads) workgroups of its own, so many tiny planes give one workgroup each and a few large
// ones several -- 176 x 320 at band 8 is seven.  Each workgroup leaves nine doubles in the workspace.
// tests/depthwise_backward_cases.py mirrors these rules (plan_of) to pick its shapes: change both together.
// ------------------------------------------------------------------------------------
struct DwBwdPlan {
    int status = 0;
    int Ho = 0, Wo = 0;
    long long planes = 0;
    int band = 0;                       // dy rows per thread, every launch
    unsigned nstrips = 0, nbands = 0;   // of a dy plane
    unsigned dx_items = 0, dx_grid = 0;
    unsigned plane_items = 0, nseg = 0, slots = 0, dw_grid = 0;   // slots = planes * nseg: nine doubles each
    size_t ws_bytes = 0;
};

inline DwBwdPlan plan_depthwise_backward(int dtype, int N, int C, int H, int W, int stride)
{
    DwBwdPlan P;
    if (!depthwise_shape_ok(dtype, N, C, H, W, stride)) return P;
    P.Ho = (H - 1) / stride + 1;
    P.Wo = (W - 1) / stride + 1;
    P.planes = (long long)N * C;
    P.band = depthwise_band(P.planes, P.Ho, P.Wo);
    P.nstrips = (unsigned)ceil_div(P.Wo, kDwCols);
    P.nbands = (unsigned)ceil_div(P.Ho, P.band);
    P.plane_items = P.nbands * P.nstrips;                          // <= Ho * Wo
    P.dx_items = (unsigned)(P.planes * P.plane_items);             // <= N * C * Ho * Wo < 2^31
    P.dx_grid = (unsigned)ceil_div((long)P.dx_items, (long)kDwThreads);
    P.nseg = (unsigned)ceil_div((long)P.plane_items, (long)kDwThreads);
    P.slots = (unsigned)(P.planes * P.nseg);                       // nseg <= plane_items: < 2^31 too
    P.dw_grid = std::min(P.slots, kDwbMaxGrid);
    P.ws_bytes = align_up((size_t)P.slots * 9 * sizeof(double), 256);
    P.status = 1;
    return P;
}

// dx and / or dweight; `workspace` may be NULL where dweight is
template <class T>
int launch_depthwise3x3_backward(const DwBwdPlan& P, const T* dy, const T* x, const T* w, T* dx, T* dweight, int N, int C, int H,
                                 int W, int stride, void* workspace, hipStream_t stream)
{
    int st = 1;
    if (dx) {
        if (stride == 1)
            hipLaunchKernelGGL(rroi_depthwise3x3_dx_s1_kernel<T>, dim3(P.dx_grid), dim3(kDwThreads), 0, stream, dy, w, dx, C, H, W,
                               P.band, P.nstrips, P.nbands, P.dx_items);
        else
            hipLaunchKernelGGL(rroi_depthwise3x3_dx_s2_kernel<T>, dim3(P.dx_grid), dim3(kDwThreads), 0, stream, dy, w, dx, C, H, W,
                               P.Ho, P.Wo, P.band, P.nstrips, P.nbands, P.dx_items);
        st = launch_status();
    }
    if (st != 1 || !dweight) return st;
    double* partials = static_cast<double*>(workspace);
    if (stride == 1)
        hipLaunchKernelGGL((rroi_depthwise3x3_dw_partial_kernel<T, 1>), dim3(P.dw_grid), dim3(kDwThreads), 0, stream, dy, x,
                           partials, H, W, P.Ho, P.Wo, P.band, P.nstrips, P.plane_items, P.nseg, P.slots);
    else
        hipLaunchKernelGGL((rroi_depthwise3x3_dw_partial_kernel<T, 2>), dim3(P.dw_grid), dim3(kDwThreads), 0, stream, dy, x,
                           partials, H, W, P.Ho, P.Wo, P.band, P.nstrips, P.plane_items, P.nseg, P.slots);
    st = launch_status();
    if (st != 1) return st;
    hipLaunchKernelGGL(rroi_depthwise3x3_dw_finish_kernel<T>, dim3((unsigned)C), dim3(kDwThreads), 0, stream, partials, dweight,
                       (unsigned)N, (unsigned)C, P.nseg);
    return launch_status();
}
