// rroi_merge_host.h -- the gated merge, host part: the plan rule (one function for the plan query and the launch), the
// argument checks it carries, the one launch.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_host_launch.h (status helpers, with_dtype).
#pragma once

// ------------------------------------------------------------------------------------
// The plan, a pure function of (dtype, N, C, H, W, a's size, gate's size, gated, CU count) (DESIGN 5.14,
// profiles/native_merge.md):
//   V   pixels per lane: 4 where `a` has f's size (16 bytes of fp32, 8 of a 16-bit type), 2 where `a` is resized.  The
//       starting rule -- 16 bytes per lane: 4 for fp32, 8 for 16 bits, 4 for a 16-bit resize because V = 8 needs 168 VGPRs
//       there -- lost to this one on every row of the forms table: 16 bits at V = 4 by 3-28 %, the resize at V = 2 by 27-36 %
//       (more lanes for the same taps, which come through the cache one element at a time).  V = 8 is instantiated by the
//       measurement build alone.
//   K   channel blocks of ceil(C / K) channels: the smallest power of two with N * tiles * K >= kMgGroupsPerCu * CUs,
//       halved until the last block holds at least kMgMinChannels channels (the per-tile set-up -- the gate's four taps and
//       the indices -- is paid once per block) or K == 1.
// The scales of the two resizes are computed here, in double, and travel in the plan: (in - 1) / (out - 1), 0 where
// out == 1.  force_v / force_k replace the rule's choice where they are not 0: only the measurement build's extra entry
// point passes them (`make merge-forms`, tools/merge_bench.py --forms).
// tests/merge_cases.py mirrors this rule (plan_of) to pick its shapes: change both together.
// ------------------------------------------------------------------------------------
constexpr int kMgGroupsPerCu = 4;
constexpr int kMgMinChannels = 8;

struct MergePlan {
    int status = 0;            // 0: the call refuses these arguments
    int V = 4, K = 1;
    bool resize_a = false, resize_g = false;
    unsigned hw = 0;
    unsigned tiles = 0;        // per image
    unsigned grid = 0;         // N * K * tiles
    unsigned cb = 0;           // channels per block
    MgSource A{1, 1, 0.0, 0.0}, G{1, 1, 0.0, 0.0};
};

inline double merge_scale(int in, int out) { return out == 1 ? 0.0 : (double)(in - 1) / (double)(out - 1); }

inline bool merge_count_ok(int n, int c, int h, int w)   // n * c * h * w < 2^31, every factor >= 1
{
    long long total = n;
    for (const int d : {c, h, w}) {
        if (total > ((1LL << 31) - 1) / d) return false;
        total *= d;
    }
    return true;
}

inline MergePlan plan_merge(int dtype, int batch_size, int channels, int height, int width, int a_h, int a_w, int g_h, int g_w,
                            int gated, int cus, int force_v = 0, int force_k = 0)
{
    MergePlan P;
    if (!dtype_ok(dtype) || (gated != 0 && gated != 1)) return P;
    if (batch_size < 1 || channels < 1 || height < 1 || width < 1 || a_h < 1 || a_w < 1) return P;
    if (gated && (g_h < 1 || g_w < 1)) return P;
    if (!merge_count_ok(batch_size, channels, height, width) || !merge_count_ok(batch_size, channels, a_h, a_w)) return P;
    if (gated && !merge_count_ok(batch_size, 1, g_h, g_w)) return P;
    P.status = 1;
    P.hw = (unsigned)((long long)height * width);
    P.resize_a = a_h != height || a_w != width;
    P.V = P.resize_a ? 2 : 4;
#ifdef RROI_MERGE_MEASURE
    if (force_v == 2 || force_v == 4 || (force_v == 8 && dtype != RROI_DTYPE_FP32)) P.V = force_v;
#endif
    const long long tiles = (P.hw + (unsigned)(kMgThreads * P.V) - 1) / (unsigned)(kMgThreads * P.V);
    long long K = 1;
    while (K < channels && batch_size * tiles * K < (long long)kMgGroupsPerCu * cus) K *= 2;
    const auto last_block = [&](long long k) { return channels - (k - 1) * ((channels + k - 1) / k); };
#ifdef RROI_MERGE_MEASURE
    if (force_k > 0 && (force_k & (force_k - 1)) == 0) {
        K = force_k;
        while (K > 1 && last_block(K) < 1) K /= 2;
    } else
#endif
    while (K > 1 && last_block(K) < kMgMinChannels) K /= 2;
    P.K = (int)K;
    P.tiles = (unsigned)tiles;
    P.grid = (unsigned)(batch_size * tiles * K);    // <= N * C * H * W < 2^31
    P.cb = (unsigned)((channels + K - 1) / K);
    P.resize_g = gated && (g_h != height || g_w != width);
    P.A = MgSource{a_h, a_w, merge_scale(a_h, height), merge_scale(a_w, width)};
    if (gated) P.G = MgSource{g_h, g_w, merge_scale(g_h, height), merge_scale(g_w, width)};
    return P;
}

template <class T>
int launch_merge(const MergePlan& P, const T* a, const T* gate, const T* f, T* y, unsigned C, unsigned W, hipStream_t stream)
{
    const auto run = [&](auto v, auto up) {
        hipLaunchKernelGGL((rroi_merge_kernel<T, decltype(v)::value, decltype(up)::value>), dim3(P.grid), dim3(kMgThreads), 0,
                           stream, a, gate, f, y, C, W, P.hw, P.tiles, (unsigned)P.K, P.cb, P.A, P.G, P.resize_g ? 1 : 0);
        return launch_status();
    };
    return with_flag(P.resize_a, [&](auto up) {
#ifdef RROI_MERGE_MEASURE
        if constexpr (sizeof(T) == 4) return with_choice<2, 4>(P.V, [&](auto v) { return run(v, up); });
        else return with_choice<2, 4, 8>(P.V, [&](auto v) { return run(v, up); });
#else
        if constexpr (decltype(up)::value) return run(int_c<2>{}, up);
        else return run(int_c<4>{}, up);
#endif
    });
}
