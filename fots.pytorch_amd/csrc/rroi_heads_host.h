// rroi_heads_host.h -- detection heads and attention gate, host part: the plan rule (one function for the plan query and
// the launch), argument checks, the one launch.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_host_launch.h (status helpers, with_dtype).
#pragma once

// ------------------------------------------------------------------------------------
// The plan, a pure function of (dtype, outputs, N, C, H, W, CU count); every (V, S) was measured against the others
// (profiles/native_heads.md):
//   V   pixels per lane: 2 where that leaves N * ceil(HW / 128) >= 5/8 * CUs tiles, else 1.  Two pixels per lane won at
//       every measured map from 220 such tiles upwards (fp32 by 20-30 %, 16 bits by 0-6 %) and lost at 110 (the 1/8 map
//       of one image: too few waves).  Four pixels per lane never won by more than 7 % and lost by up to 40 %: the rule
//       does not return it, and only the measurement build instantiates it.
//   S   waves per tile, each on its own block of ceil(C / S) channels: the smallest of 1, 2, 4, 8, 16 with
//       tiles * S >= kPwWavesPerCu * CUs, at most 16 / V (the kernel's launch bounds), halved until no wave's block is
//       empty ((S - 1) * ceil(C / S) < C).
// `dtype` and `outputs` do not enter the rule today.  force_v / force_s replace the rule's choice where they are not 0:
// only the measurement build's extra entry point passes them (`make heads-forms`, tools/heads_bench.py --forms); S stays
// capped by C, by the kernel's launch bounds and by 64 KiB of LDS, all of which the rule itself stays inside.
// tests/heads_cases.py mirrors this rule (plan_of) to pick its shapes: change both together.
// ------------------------------------------------------------------------------------
constexpr unsigned kPwWavesPerCu = 16;

struct HeadsPlan {
    int status = 0;            // 0: the call refuses these arguments
    int V = 1, S = 1;
    unsigned hw = 0;
    unsigned tiles = 0;        // per image
    unsigned grid = 0;         // N * tiles
    unsigned cb = 0;           // channels per wave
    unsigned lds_bytes = 0;    // (S - 1) * outputs * V * 64 doubles
};

inline HeadsPlan plan_heads(int dtype, int outputs, int batch_size, int channels, int height, int width, int cus,
                            int force_v = 0, int force_s = 0)
{
    HeadsPlan P;
    if (!dtype_ok(dtype) || (outputs != 1 && outputs != 7)) return P;
    if (batch_size < 1 || channels < 1 || height < 1 || width < 1) return P;
    long long total = batch_size;
    for (const int d : {channels, height, width}) {
        if (total > ((1LL << 31) - 1) / d) return P;
        total *= d;
    }
    P.status = 1;
    P.hw = (unsigned)((long long)height * width);
    const auto tiles_of = [&](int v) { return (long long)batch_size * ((P.hw + 64u * v - 1) / (64u * v)); };
    P.V = 8 * tiles_of(2) >= 5LL * cus ? 2 : 1;
#ifdef RROI_HEADS_MEASURE
    if (force_v == 1 || force_v == 2 || force_v == 4) P.V = force_v;
#endif
    const long long tiles = tiles_of(P.V);
    P.S = 1;
    while (P.S < kPwMaxWaves && tiles * P.S < (long long)kPwWavesPerCu * cus) P.S *= 2;
    if (force_s == 1 || force_s == 2 || force_s == 4 || force_s == 8 || force_s == 16) P.S = force_s;
    while (P.S * P.V > kPwMaxWaves || (P.S - 1) * outputs * P.V * 512 > 65536) P.S /= 2;
    while (P.S > 1 && (long long)(P.S - 1) * ((channels + P.S - 1) / P.S) >= channels) P.S /= 2;
    P.tiles = (unsigned)(tiles / batch_size);
    P.grid = (unsigned)tiles;                       // <= N * H * W < 2^31
    P.cb = (unsigned)((channels + P.S - 1) / P.S);
    P.lds_bytes = (unsigned)((P.S - 1) * outputs * P.V * 64 * sizeof(double));   // <= 15 * 7 * 64 * 8 = 53,760 (V = 1),
    return P;                                                                     // 7 * 7 * 2 * 64 * 8 = 50,176 (V = 2)
}

// T* or NULL for each of: w0 b0 w1 b1 w2 b2 (kernel's argument list); NOUT 1 uses (w0, b0, y0) alone
template <class T, int NOUT, int EPI>
int launch_pointwise(const HeadsPlan& P, const T* x, const T* w0, const T* b0, const T* w1, const T* b1, const T* w2,
                     const T* b2, T* y0, T* y1, T* y2, unsigned C, double rbox_scale, hipStream_t stream)
{
#ifdef RROI_HEADS_MEASURE
    return with_choice<4, 2, 1>(P.V, [&](auto v) {
#else
    return with_choice<2, 1>(P.V, [&](auto v) {
#endif
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((rroi_pointwise_kernel<T, NOUT, EPI, V>), dim3(P.grid), dim3((unsigned)P.S * 64u), P.lds_bytes, stream,
                           x, w0, b0, w1, b1, w2, b2, y0, y1, y2, C, P.hw, P.tiles, P.cb, rbox_scale);
        return launch_status();
    });
}
