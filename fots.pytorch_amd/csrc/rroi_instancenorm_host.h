// rroi_instancenorm_host.h -- InstanceNorm2d, host part: the form rule (one function for the plan query, the size query and
// the launch), argument checks, the one or two launches.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_host_launch.h (status helpers, with_dtype).
#pragma once

// ------------------------------------------------------------------------------------
// The rule between the two forms (DESIGN 5.11 has the measurements): a pure function of (dtype, N, C, H, W, CU count).
//   split   where the planes are fewer than the chip's CUs -- one workgroup per plane would leave CUs idle -- and a plane
//           has at least kInSplitMinPlane elements, below which the second launch costs more than the idle CUs;
//   plane   everywhere else.
// Segments of the split form: about kInWgPerCu workgroups per CU over all planes, a segment a multiple of kInSegQuantum
// elements (whole vectors of either width for every lane, so a plane on a 16-byte boundary has every segment on one) and
// at least kInMinSeg, at most kInMaxSegs = kInThreads segments per plane (rroi_inorm_apply_kernel: one pair per lane).
// `dtype` does not enter the rule today: the size query has no dtype, and the thresholds measured alike in elements.
// tests/instancenorm_cases.py mirrors these constants to pick its shapes: change both together.
// ------------------------------------------------------------------------------------
#ifndef RROI_INORM_SPLIT_MIN_PLANE          // (a measurement build may move the threshold: tools/instancenorm_bench.py --lib)
#define RROI_INORM_SPLIT_MIN_PLANE 32768
#endif
#ifndef RROI_INORM_SPLIT_PLANES_PER_CU
#define RROI_INORM_SPLIT_PLANES_PER_CU 1
#endif
constexpr unsigned kInSplitMinPlane = RROI_INORM_SPLIT_MIN_PLANE;
constexpr unsigned kInSplitPlanesPerCu = RROI_INORM_SPLIT_PLANES_PER_CU;   // split below this many planes per CU
constexpr unsigned kInSegQuantum = 2048;
constexpr unsigned kInMinSeg = 8192;
constexpr unsigned kInMaxSegs = kInThreads;
constexpr unsigned kInWgPerCu = 8;

struct InormPlan {
    int status = 0;            // 0: the call refuses these arguments
    int form = 0;              // RROI_INORM_PLANE / RROI_INORM_SPLIT
    unsigned planes = 0, n = 0;
    unsigned nseg = 1, seg = 0;
    unsigned grid = 0;         // split: planes * nseg; plane: min(planes, kInMaxPlaneGrid)
    size_t ws_bytes = 0;       // one {s1, s2} pair of doubles per workgroup, split form only
};

// the rule itself, for a threshold pair: the forward's (plan_instancenorm) or the backward's (rroi_instancenorm_backward_host.h)
inline InormPlan plan_inorm_forms(int dtype, int batch_size, int channels, int height, int width, int cus, unsigned min_plane,
                                  unsigned planes_per_cu)
{
    InormPlan P;
    if (!dtype_ok(dtype)) return P;
    if (batch_size < 1 || channels < 1 || height < 1 || width < 1) return P;
    long long total = batch_size;
    for (const int d : {channels, height, width}) {
        if (total > ((1LL << 31) - 1) / d) return P;
        total *= d;
    }
    P.status = 1;
    P.planes = (unsigned)((long long)batch_size * channels);
    P.n = (unsigned)((long long)height * width);
    if (P.planes >= (unsigned)cus * planes_per_cu || P.n < min_plane) {
        P.form = RROI_INORM_PLANE;
        P.seg = P.n;
        P.grid = std::min(P.planes, kInMaxPlaneGrid);
        return P;
    }
    P.form = RROI_INORM_SPLIT;
    const unsigned want = std::min(kInMaxSegs, (kInWgPerCu * (unsigned)cus + P.planes - 1) / P.planes);
    P.seg = std::max(kInMinSeg, ((P.n + want - 1) / want + kInSegQuantum - 1) / kInSegQuantum * kInSegQuantum);
    P.nseg = (P.n + P.seg - 1) / P.seg;
    P.grid = P.planes * P.nseg;    // < cus * planes_per_cu * kInMaxSegs
    P.ws_bytes = align_up((size_t)P.grid * sizeof(double2), 256);
    return P;
}

inline InormPlan plan_instancenorm(int dtype, int batch_size, int channels, int height, int width, int cus)
{
    return plan_inorm_forms(dtype, batch_size, channels, height, width, cus, kInSplitMinPlane, kInSplitPlanesPerCu);
}

template <class T>
int launch_instancenorm(const InormPlan& P, const T* x, const T* gamma, const T* beta, T* y, unsigned C, double eps,
                        float slope, void* workspace, hipStream_t stream)
{
    if (P.form == RROI_INORM_PLANE) {
        hipLaunchKernelGGL(rroi_inorm_plane_kernel<T>, dim3(P.grid), dim3(kInThreads), 0, stream, x, gamma, beta, y, C, P.n,
                           P.planes, eps, slope);
        return launch_status();
    }
    double2* pairs = static_cast<double2*>(workspace);
    hipLaunchKernelGGL(rroi_inorm_stats_kernel<T>, dim3(P.grid), dim3(kInThreads), 0, stream, x, pairs, P.n, P.seg, P.nseg);
    const int st = launch_status();
    if (st != 1) return st;
    hipLaunchKernelGGL(rroi_inorm_apply_kernel<T>, dim3(P.grid), dim3(kInThreads), 0, stream, x, gamma, beta, y, pairs, C, P.n,
                       P.seg, P.nseg, eps, slope);
    return launch_status();
}

// The fused epilogues under the same plan, which is the plan of x's shape: the grid runs over x's planes in
// both modes, and the first launch of the split form is the plain one.
template <class T, int MODE>
int launch_instancenorm_fused(const InormPlan& P, const T* x, const T* gamma, const T* beta, const T* r, T* y, unsigned C,
                              double eps, float slope, void* workspace, hipStream_t stream)
{
    if (P.form == RROI_INORM_PLANE) {
        hipLaunchKernelGGL((rroi_inorm_fused_plane_kernel<T, MODE>), dim3(P.grid), dim3(kInThreads), 0, stream, x, gamma, beta,
                           r, y, C, P.n, P.planes, eps, slope);
        return launch_status();
    }
    double2* pairs = static_cast<double2*>(workspace);
    hipLaunchKernelGGL(rroi_inorm_stats_kernel<T>, dim3(P.grid), dim3(kInThreads), 0, stream, x, pairs, P.n, P.seg, P.nseg);
    const int st = launch_status();
    if (st != 1) return st;
    hipLaunchKernelGGL((rroi_inorm_fused_apply_kernel<T, MODE>), dim3(P.grid), dim3(kInThreads), 0, stream, x, gamma, beta, r,
                       y, pairs, C, P.n, P.seg, P.nseg, eps, slope);
    return launch_status();
}
