// rroi_conv1x1_host.h -- the 1x1 convolution, host part: the plan rule (one function for the plan query and the launch),
// the argument checks it carries, the one launch.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_conv3x3_host.h (merge_count_ok, with_choice).
#pragma once

// ------------------------------------------------------------------------------------
// The plan, a pure function of (dtype, N, Cin, Cout, H, W, stride) (profiles/native_conv1x1.md):
//   the tile is 32 * MT output channels by 128 output pixels (flat over the output plane), K chunks of 64;
//   MT  accumulator tiles of 32 output channels per workgroup: 2 where Cout > 32 and that still leaves at least
//       kC1MinGroups workgroups (one per CU of an MI355X: a constant, so that the plan depends on the arguments alone),
//       1 otherwise -- two tiles halve how often the X tile is staged, one tile keeps the small maps' grids from
//       halving (44x80 and 22x40 give 28 and 7 pixel tiles per image).
// The measurement build (`make conv1x1-forms`, tools/conv1x1_bench.py --forms) has one more entry point that passes
// force_mt.
// tests/conv1x1_cases.py mirrors this rule (plan_of) to pick its shapes: change both together.
// ------------------------------------------------------------------------------------
constexpr long long kC1MinGroups = 256;

struct Conv1x1Plan {
    int status = 0;            // 0: the call refuses these arguments
    int MT = 1;
    int Ho = 0, Wo = 0;
    unsigned P = 0, m_tiles = 0, p_tiles = 0, grid = 0, k_chunks = 0;
    int lds_bytes = 0;
};

inline Conv1x1Plan plan_conv1x1(int dtype, int batch_size, int cin, int cout, int height, int width, int stride,
                                int force_mt = 0)
{
    Conv1x1Plan P;
    if (dtype != RROI_DTYPE_BF16 && dtype != RROI_DTYPE_FP16) return P;
    if (batch_size < 1 || cin < 1 || cout < 1 || height < 1 || width < 1 || (stride != 1 && stride != 2)) return P;
    P.Ho = (height - 1) / stride + 1;
    P.Wo = (width - 1) / stride + 1;
    if (!merge_count_ok(batch_size, cin, height, width) || !merge_count_ok(batch_size, cout, P.Ho, P.Wo) ||
        !merge_count_ok(cout, cin, 1, 1))
        return P;
    P.status = 1;
    P.P = (unsigned)P.Ho * (unsigned)P.Wo;
    P.p_tiles = (P.P + kC1Pixels - 1) / kC1Pixels;
    P.MT = cout > 32 && (long long)batch_size * ((cout + 63) / 64) * P.p_tiles >= kC1MinGroups ? 2 : 1;
#ifdef RROI_CONV1X1_MEASURE
    if (force_mt == 1 || force_mt == 2) P.MT = force_mt;
#else
    (void)force_mt;
#endif
    P.m_tiles = (unsigned)((cout + 32 * P.MT - 1) / (32 * P.MT));
    P.grid = (unsigned)batch_size * P.m_tiles * P.p_tiles;            // <= N * Cout * Ho * Wo < 2^31
    P.k_chunks = (unsigned)((cin + kC1Chunk - 1) / kC1Chunk);
    P.lds_bytes = c1_lds_bytes(P.MT);
    return P;
}

// the shortcut's BatchNorm as the call takes it: all four NULL is no norm
struct Conv1x1Norm {
    const void *weight, *bias, *mean, *var;
    float eps;
    bool given() const { return mean != nullptr; }
};

template <class T>
int launch_conv1x1(const Conv1x1Plan& P, const T* x, const T* w, T* y, const Conv1x1Norm& bn, unsigned Cin, unsigned Cout,
                   unsigned H, unsigned W, int stride, float slope, hipStream_t stream)
{
    return with_choice<1, 2>(P.MT, [&](auto mt) {
        return with_choice<1, 2>(stride, [&](auto s) {
            return with_flag(bn.given(), [&](auto norm) {
                hipLaunchKernelGGL((rroi_conv1x1_kernel<T, decltype(mt)::value, decltype(s)::value, decltype(norm)::value>),
                                   dim3(P.grid), dim3(kC1Threads), 0, stream, x, w, y, static_cast<const T*>(bn.weight),
                                   static_cast<const T*>(bn.bias), static_cast<const T*>(bn.mean),
                                   static_cast<const T*>(bn.var), bn.eps, Cin, Cout, H, W, (unsigned)P.Wo, P.P, P.m_tiles,
                                   P.p_tiles, slope);
                return launch_status();
            });
        });
    });
}
