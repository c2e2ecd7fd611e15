// rroi_merge_backward_host.h -- the gated merge's backward and the stand-alone resize, host part: the plan
// rules (one function each for the plan query and the launch), the argument checks they carry, the launches.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_merge_host.h (plan_merge, merge_scale,
// merge_count_ok).
#pragma once

// ------------------------------------------------------------------------------------
// The stand-alone resize y = R x takes plan_merge's rule as it stands (an ungated merge without f: V = 2 where x is
// resized, 4 where it is copied).
// The gathers (dx = R^T dy, dgate) give a lane one element of the SMALL map: tiles of 256 pixels, and for dx channel blocks
// by plan_merge's rule on those tiles.  Their bits depend on no plan value.
// The merge backward's first launch sums over a block's channels, so its blocks are a function of the shape alone: the
// rule of plan_merge asked for kMgbCus = 256 CUs on every device, with at least kMgbMinChannels = 32 channels in the last
// block -- a block costs a map of doubles in the workspace, 8 bytes per pixel against 32 elements read twice; with
// plan_merge's 8 the workspace was as large as the maps at one image and the blocks' sum took longer than the rest --
// then blocks of at most kMgbMaxBlock channels.
// Refused beside what plan_merge refuses, so that no chain of additions exceeds 8192 terms: a resize whose
// gather would meet more than kRsMaxFootprint output rows (columns) in one source row (column) -- rs_max_footprint, an upper
// bound; a 2x resize has 5 -- and more than kMgbMaxBlocks channel blocks.
// tests/merge_backward_cases.py mirrors these rules: change both together.
// ------------------------------------------------------------------------------------
constexpr int kMgbCus = 256;
constexpr int kMgbMinChannels = 32;

// an upper bound of hi - lo over rs_footprint(s, in, out, i, ...)
inline long long rs_max_footprint(int in, int out)
{
    if (out == 1) return 1;
    if (in == 1) return out;
    return std::min<long long>(out, (long long)(2.0 / merge_scale(in, out)) + 2);
}

struct ResizeBwdPlan {
    int status = 0;
    bool ident = false;
    int K = 1;
    unsigned hw = 0, tiles = 0, grid = 0, cb = 0;
    double sy = 0.0, sx = 0.0;
    int max_rows = 0, max_cols = 0;
};

// dx (N, C, h, w) from dy (N, C, H, W)
inline ResizeBwdPlan plan_resize_backward(int dtype, int N, int C, int h, int w, int H, int W, int cus)
{
    ResizeBwdPlan P;
    if (!dtype_ok(dtype) || N < 1 || C < 1 || h < 1 || w < 1 || H < 1 || W < 1) return P;
    if (!merge_count_ok(N, C, h, w) || !merge_count_ok(N, C, H, W)) return P;
    const long long my = rs_max_footprint(h, H), mx = rs_max_footprint(w, W);
    if (my > kRsMaxFootprint || mx > kRsMaxFootprint) return P;
    P.ident = h == H && w == W;
    P.hw = (unsigned)((long long)h * w);
    const long long tiles = (P.hw + (unsigned)kMgThreads - 1) / (unsigned)kMgThreads;
    long long K = 1;
    while (K < C && N * tiles * K < (long long)kMgGroupsPerCu * cus) K *= 2;
    while (K > 1 && C - (K - 1) * ((C + K - 1) / K) < kMgMinChannels) K /= 2;
    P.K = (int)K;
    P.tiles = (unsigned)tiles;
    P.grid = (unsigned)(N * tiles * K);          // <= N * C * h * w < 2^31
    P.cb = (unsigned)((C + K - 1) / K);
    P.sy = merge_scale(h, H);
    P.sx = merge_scale(w, W);
    P.max_rows = (int)my;
    P.max_cols = (int)mx;
    P.status = 1;
    return P;
}

struct MergeBwdPlan {
    int status = 0;
    int V = 4, K = 1;
    bool gated = false, resize_g = false;
    unsigned hw = 0, tiles = 0, grid = 0, cb = 0;
    unsigned images = 0;
    unsigned ghw = 0, gtiles = 0, ggrid = 0;     // the dgate launch (0 without a gate)
    MgSource G{1, 1, 0.0, 0.0};
    size_t ws_bytes = 0;                         // what dgate needs (0 without a gate)
};

inline MergeBwdPlan plan_merge_backward(int dtype, int N, int C, int H, int W, int g_h, int g_w, int gated)
{
    MergeBwdPlan P;
    const MergePlan F = plan_merge(dtype, N, C, H, W, H, W, g_h, g_w, gated, kMgbCus);   // `a` takes no part: as if of f's size
    if (!F.status) return P;
    if (gated && (rs_max_footprint(g_h, H) > kRsMaxFootprint || rs_max_footprint(g_w, W) > kRsMaxFootprint)) return P;
    long long K0 = 1;
    while (K0 < C && N * (long long)F.tiles * K0 < (long long)kMgGroupsPerCu * kMgbCus) K0 *= 2;
    while (K0 > 1 && C - (K0 - 1) * ((C + K0 - 1) / K0) < kMgbMinChannels) K0 /= 2;
    P.cb = (unsigned)std::min<long long>((C + K0 - 1) / K0, kMgbMaxBlock);
    const long long K = ((long long)C + P.cb - 1) / P.cb;
    if (K > kMgbMaxBlocks) return P;
    P.V = F.V;
    P.K = (int)K;
    P.gated = gated != 0;
    P.resize_g = F.resize_g;
    P.hw = F.hw;
    P.images = (unsigned)N;
    P.tiles = F.tiles;
    P.grid = (unsigned)(N * (long long)F.tiles * K);   // <= N * C * H * W < 2^31
    P.G = F.G;
    if (gated) {
        P.ghw = (unsigned)((long long)g_h * g_w);
        P.gtiles = (P.ghw + (unsigned)kMgThreads - 1) / (unsigned)kMgThreads;
        P.ggrid = (unsigned)N * P.gtiles;               // <= N * g_h * g_w < 2^31
        P.ws_bytes = align_up((size_t)N * (size_t)K * P.hw * sizeof(double), 256);
    }
    P.status = 1;
    return P;
}

// whether [a, a + na) and [b, b + nb) share a byte
inline bool bytes_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const char *p = static_cast<const char*>(a), *q = static_cast<const char*>(b);
    return p && q && p < q + nb && q < p + na;
}

template <class T>
int launch_resize(const MergePlan& P, const T* x, T* y, unsigned C, unsigned W, hipStream_t stream)
{
    if (P.resize_a)
        hipLaunchKernelGGL((rroi_resize_kernel<T, 2, true>), dim3(P.grid), dim3(kMgThreads), 0, stream, x, y, C, W, P.hw,
                           P.tiles, (unsigned)P.K, P.cb, P.A);
    else
        hipLaunchKernelGGL((rroi_resize_kernel<T, 4, false>), dim3(P.grid), dim3(kMgThreads), 0, stream, x, y, C, W, P.hw,
                           P.tiles, (unsigned)P.K, P.cb, P.A);
    return launch_status();
}

template <class T>
int launch_resize_backward(const ResizeBwdPlan& P, const T* dy, T* dx, unsigned C, int h, int w, int H, int W,
                           hipStream_t stream)
{
    hipLaunchKernelGGL(rroi_resize_backward_kernel<T>, dim3(P.grid), dim3(kMgThreads), 0, stream, dy, dx, C, h, w, H, W, P.hw,
                       P.tiles, (unsigned)P.K, P.cb, P.sy, P.sx, P.ident ? 1 : 0);
    return launch_status();
}

// df and / or dgate; `workspace` may be NULL where dgate is
template <class T>
int launch_merge_backward(const MergeBwdPlan& P, const T* dy, const T* f, const T* gate, T* df, T* dgate, unsigned C, int H,
                          int W, void* workspace, hipStream_t stream)
{
    double* ws = static_cast<double*>(workspace);
    const auto run = [&](auto want_df, auto want_dg) {
        hipLaunchKernelGGL((rroi_merge_backward_kernel<T, 4, decltype(want_df)::value, decltype(want_dg)::value>), dim3(P.grid),
                           dim3(kMgThreads), 0, stream, dy, f, gate, df, ws, C, (unsigned)W, P.hw, P.tiles, (unsigned)P.K, P.cb,
                           P.G, P.resize_g ? 1 : 0);
        return launch_status();
    };
    const int st = df && dgate ? run(std::true_type{}, std::true_type{})
                   : df        ? run(std::true_type{}, std::false_type{})
                               : run(std::false_type{}, std::true_type{});
    if (st != 1 || !dgate) return st;
    if (P.K > 1) {
        const unsigned total = P.images * P.hw;                // N * HW < 2^31
        hipLaunchKernelGGL(rroi_merge_blocksum_kernel, dim3((total + kMgThreads - 1) / kMgThreads), dim3(kMgThreads), 0, stream, ws,
                           (unsigned)P.K, P.hw, total);
        const int st2 = launch_status();
        if (st2 != 1) return st2;
    }
    hipLaunchKernelGGL(rroi_merge_dgate_kernel<T>, dim3(P.ggrid), dim3(kMgThreads), 0, stream, ws, dgate, (unsigned)P.K, P.G.h,
                       P.G.w, H, W, P.ghw, P.hw, P.gtiles, P.G.sy, P.G.sx, P.resize_g ? 0 : 1);
    return launch_status();
}
