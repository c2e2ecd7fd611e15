// rroi_heads_backward_host.h -- the heads' and the gate's training forward and backward, host part: the
// backward's plan rule (one function for the plan query, the workspace size and the launch) and the launches.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_heads_host.h (plan_heads).
#pragma once

// ------------------------------------------------------------------------------------
// The backward's plan, a pure function of (dtype, outputs, N, C, H, W, CU count):
//   V     pixels per lane: 2 where that leaves N * ceil(HW / 128) >= CUs tiles, else 1.
//   cb    channels per wave: ceil(C / kHbWaves) rounded up to the kPwChunk channels of a step; a wave whose block lies behind
//         C idles.
//   tpw   tiles per workgroup: ceil(total / (kHbGridPerCu * CUs)), so that `rows` = ceil(total / tpw) workgroups -- and
//         partial rows of the workspace, outputs * (C + 1) doubles each -- never exceed kHbGridPerCu * CUs.
// `dtype` and `outputs` do not enter the rule today.  tests/heads_backward_cases.py mirrors it (plan_of): change both
// together.
// ------------------------------------------------------------------------------------
constexpr unsigned kHbGridPerCu = 4;

struct HeadsBwdPlan {
    int status = 0;            // 0: the call refuses these arguments
    int V = 1;
    unsigned hw = 0;
    unsigned tiles = 0;        // per image, of 64 * V pixels
    unsigned total = 0;        // N * tiles
    unsigned tpw = 0;          // tiles per workgroup
    unsigned rows = 0;         // workgroups = partial rows
    unsigned cb = 0;           // channels per wave
    unsigned lds_bytes = 0;    // of a launch that leaves partials
    size_t ws_bytes = 0;       // rows * outputs * (C + 1) doubles
};

inline HeadsBwdPlan plan_heads_backward(int dtype, int outputs, int batch_size, int channels, int height, int width, int cus)
{
    HeadsBwdPlan P;
    if (!plan_heads(dtype, outputs, batch_size, channels, height, width, cus).status) return P;   // section 7's refusals
    if ((long long)outputs * ((long long)channels + 1) >= (1LL << 31)) return P;                  // a row's entries
    P.status = 1;
    P.hw = (unsigned)((long long)height * width);
    const auto tiles_of = [&](int v) { return (long long)batch_size * ((P.hw + 64u * v - 1) / (64u * v)); };
    P.V = tiles_of(2) >= cus ? 2 : 1;
    const long long total = tiles_of(P.V), cap = (long long)kHbGridPerCu * cus;
    P.tiles = (unsigned)(total / batch_size);
    P.total = (unsigned)total;                              // <= N * H * W < 2^31
    P.tpw = (unsigned)((total + cap - 1) / cap);
    P.rows = (unsigned)((total + P.tpw - 1) / P.tpw);
    P.cb = (unsigned)(((long long)channels + kHbWaves * kPwChunk - 1) / (kHbWaves * kPwChunk)) * kPwChunk;
    P.lds_bytes = (unsigned)(kHbWaves * (std::min(P.cb, kHbPassBlock) / kPwChunk) * 64 * sizeof(double));   // <= 32 KiB
    P.ws_bytes = (size_t)P.rows * outputs * ((size_t)channels + 1) * sizeof(double);
    return P;
}

template <class T, int NOUT, int EPI>
int launch_pointwise_train(const HeadsPlan& P, const T* x, const T* w0, const T* b0, const T* w1, const T* b1, const T* w2,
                           const T* b2, T* y0, T* y1, T* y2, double* z, unsigned C, double rbox_scale, hipStream_t stream)
{
    return with_choice<2, 1>(P.V, [&](auto v) {
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((rroi_pointwise_train_kernel<T, NOUT, EPI, V>), dim3(P.grid), dim3((unsigned)P.S * 64u), P.lds_bytes,
                           stream, x, w0, b0, w1, b1, w2, b2, y0, y1, y2, z, C, P.hw, P.tiles, P.cb, rbox_scale);
        return launch_status();
    });
}

// g0 g1 g2: the output gradients; dw0 db0 dw1 db1 dw2 db2: T* or NULL each; NOUT 1 uses (g0, w0, dw0, db0) alone.
// `workspace` may be NULL where no dw / db is wanted.
template <class T, int NOUT>
int launch_heads_backward(const HeadsBwdPlan& P, const T* g0, const T* g1, const T* g2, const T* x, const double* z,
                          const T* w0, const T* w1, const T* w2, T* dx, T* dw0, T* db0, T* dw1, T* db1, T* dw2, T* db2,
                          unsigned C, double rbox_scale, void* workspace, hipStream_t stream)
{
    const bool params = dw0 || db0 || dw1 || db1 || dw2 || db2;
    double* partials = params ? static_cast<double*>(workspace) : nullptr;
    const int st = with_choice<2, 1>(P.V, [&](auto v) {
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((rroi_heads_backward_kernel<T, NOUT, V>), dim3(P.rows), dim3(kHbThreads), params ? P.lds_bytes : 0u,
                           stream, g0, g1, g2, x, z, w0, w1, w2, dx, partials, C, P.hw, P.tiles, P.total, P.tpw, P.cb,
                           rbox_scale);
        return launch_status();
    });
    if (st != 1 || !params) return st;
    const unsigned entries = (unsigned)NOUT * (C + 1);
    hipLaunchKernelGGL((rroi_heads_backward_finish_kernel<T, NOUT>), dim3((entries + 63u) / 64u), dim3(64 * kHbFinishParts), 0,
                       stream, partials, dw0, db0, dw1, db1, dw2, db2, C, P.rows);
    return launch_status();
}
