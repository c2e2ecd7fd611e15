// rroi_conv3x3_host.h -- the dense 3x3 convolution, host part: the plan rule (one function for the plan query and the
// launch), the argument checks it carries, the one launch.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_merge_host.h (merge_count_ok).
#pragma once

// ------------------------------------------------------------------------------------
// The plan, a pure function of (dtype, N, Cin, Cout, H, W, stride) (profiles/native_conv3x3.md):
//   MT  accumulator tiles of 32 output channels per workgroup: 1
//   NT  output rows per wave (the tile is 4 * NT rows by 32 columns): 1
//   KC  input channels per staged chunk: 16 (one MFMA k step per tap)
// that is, ONE form: 32 channels x 4 rows x 32 columns, K chunks of 16.  The starting rule -- 64 channels where
// Cout > 32, 8 rows where that still left a workgroup per CU -- lost to it in 9 of the 11 shapes the network runs one
// image or 24 crops at a time, by 5 - 39 %, and won the other two by 6 - 11 % (the forms table): the kernel hides its
// staging behind other workgroups, not behind its own MFMAs, so the form with the most workgroups in flight wins.  KC = 32
// lost everywhere.  MT = 2, NT = 2 and KC = 32 are instantiated by the measurement build alone (`make conv-forms`,
// tools/conv3x3_bench.py --forms), whose extra entry point passes force_mt / force_nt / force_kc; KC = 32 only where the
// tile's LDS stays within the 64 KiB a kernel may declare.
// tests/conv3x3_cases.py mirrors this rule (plan_of) to pick its shapes: change both together.
// ------------------------------------------------------------------------------------
struct ConvPlan {
    int status = 0;            // 0: the call refuses these arguments
    int MT = 1, NT = 1, KC = 16;
    int Ho = 0, Wo = 0;
    unsigned m_tiles = 0, y_tiles = 0, x_tiles = 0, grid = 0, k_chunks = 0;
    int lds_bytes = 0;
};

inline ConvPlan plan_conv3x3(int dtype, int batch_size, int cin, int cout, int height, int width, int stride,
                             int force_mt = 0, int force_nt = 0, int force_kc = 0)
{
    ConvPlan P;
    if (dtype != RROI_DTYPE_BF16 && dtype != RROI_DTYPE_FP16) return P;
    if (batch_size < 1 || cin < 1 || cout < 1 || height < 1 || width < 1 || (stride != 1 && stride != 2)) return P;
    P.Ho = (height - 1) / stride + 1;
    P.Wo = (width - 1) / stride + 1;
    if (!merge_count_ok(batch_size, cin, height, width) || !merge_count_ok(batch_size, cout, P.Ho, P.Wo) ||
        !merge_count_ok(cout, cin, 3, 3))
        return P;
    P.status = 1;
#ifdef RROI_CONV3X3_MEASURE
    if (force_mt == 1 || force_mt == 2) P.MT = force_mt;
    if (force_nt == 1 || force_nt == 2) P.NT = force_nt;
    if (force_kc == 32 && cv_lds_bytes(P.MT, P.NT, stride, 32) <= 65536) P.KC = 32;
#endif
    P.m_tiles = (unsigned)((cout + 32 * P.MT - 1) / (32 * P.MT));
    P.y_tiles = (unsigned)((P.Ho + 4 * P.NT - 1) / (4 * P.NT));
    P.x_tiles = (unsigned)((P.Wo + kCvTileW - 1) / kCvTileW);
    P.grid = (unsigned)batch_size * P.m_tiles * P.y_tiles * P.x_tiles;            // <= N * Cout * Ho * Wo < 2^31
    P.k_chunks = (unsigned)((cin + P.KC - 1) / P.KC);
    P.lds_bytes = cv_lds_bytes(P.MT, P.NT, stride, P.KC);
    return P;
}

template <class T>
int launch_conv3x3(const ConvPlan& P, const T* x, const T* w, T* y, unsigned Cin, unsigned Cout, unsigned H, unsigned W,
                   int stride, float slope, hipStream_t stream)
{
    const auto run = [&](auto mt, auto nt, auto s, auto kc) {
        hipLaunchKernelGGL((rroi_conv3x3_kernel<T, decltype(mt)::value, decltype(nt)::value, decltype(s)::value,
                                                decltype(kc)::value>),
                           dim3(P.grid), dim3(kCvThreads), 0, stream, x, w, y, Cin, Cout, H, W, (unsigned)P.Ho,
                           (unsigned)P.Wo, P.m_tiles, P.y_tiles, P.x_tiles, slope);
        return launch_status();
    };
#ifdef RROI_CONV3X3_MEASURE
    return with_choice<1, 2>(P.MT, [&](auto mt) {
        return with_choice<1, 2>(P.NT, [&](auto nt) {
            return with_choice<1, 2>(stride, [&](auto s) {
                if constexpr (cv_lds_bytes(decltype(mt)::value, decltype(nt)::value, decltype(s)::value, 32) <= 65536)
                    if (P.KC == 32) return run(mt, nt, s, int_c<32>{});
                return run(mt, nt, s, int_c<16>{});
            });
        });
    });
#else
    return with_choice<1, 2>(stride, [&](auto s) { return run(int_c<1>{}, int_c<1>{}, s, int_c<16>{}); });
#endif
}
