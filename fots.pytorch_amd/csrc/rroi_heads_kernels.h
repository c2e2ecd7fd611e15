// rroi_heads_kernels.h -- the detection heads and the attention gate of the network in one launch each, DESIGN 5.12
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_device_common.h); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// A skinny 1x1 convolution over an NCHW map -- many input channels, 7 outputs (heads: score 1, rbox 4, angle 2) or 1
// (gate) -- with the elementwise chain behind it, with the arithmetic of header section 7:
//     z_o = b_o + p_0 + p_1 + ... + p_{S-1}  (left to right),  p_k = sum over channel block k, from +0.0 in channel order,
//                                            of the exact double products w[o][c] * x[c]
//     s_o = 1 / (1 + exp(-z_o));  heads: score = s_0, rbox_j = rbox_scale * s_{1+j}, a_i = 2 s_{5+i} - 1,
//                                 angle_i = a_i / sqrt(a_0 a_0 + a_1 a_1);  gate: y = s_0          all in double
//     out = (T)(float)value
// The product of two widened 24-bit significands is exact in double, so the fma below and a separate multiply and add
// give the same bits.  No channel is skipped (0 * inf = NaN, as the convolution gives).
//
// A streaming kernel along pixels.  A workgroup is S waves on one tile of 64 * V consecutive pixels of one image; lane l
// owns pixels l * V .. l * V + V - 1 of the tile and wave k the channels [k * cb, min((k + 1) * cb, C)).  A wave walks
// its block kPwChunk channels at a time: kPwChunk loads per lane are issued before the first is used -- one V-element
// vector where the address allows and the V pixels exist, single elements otherwise (a plane starts (n * C + c) * H * W
// elements into the tensor, so with an odd H * W or a 16-bit type the alignment moves from channel to channel and is
// decided per channel) -- then NOUT * V double accumulators take the chunk in channel order.
// Weights are wave-uniform: per chunk, lane o * 8 + k loads w[o][c + k] and widens it once; the arithmetic reads it out
// of that lane into scalar registers (pw_bcast), so a weight costs one load per wave whatever the element type.
// Waves 1 .. S-1 leave their partials in LDS ([wave][o][j][lane]: a wave's access is 512 contiguous bytes); wave 0 adds
// them in wave order onto b_o + p_0, runs the epilogue and stores with vector stores where the address allows.
// No atomics, no workspace, no hand-off between workgroups: the same arguments give the same bits.
// ------------------------------------------------------------------------------------
constexpr int kPwChunk = 8;           // channels per step: loads in flight per lane
constexpr int kPwMaxWaves = 16;       // S <= 16 / V (plan_heads): at most 1024 threads, and the registers of NOUT * V
                                      // double accumulators beside kPwChunk loads
constexpr int kPwEpiHeads = 0, kPwEpiSigmoid = 1;

template <class T, int V>
__device__ __forceinline__ bool pw_aligned(const T* p) { return (reinterpret_cast<size_t>(p) & (V * sizeof(T) - 1)) == 0; }

// the lane's V pixels of one channel plane: r[j] = p[j] for j < left, +0.0 behind the plane's end (never stored)
template <class T, int V>
__device__ __forceinline__ void pw_load(const T* __restrict__ p, int left, T* r)
{
    if constexpr (V == 1) {
        r[0] = left > 0 ? p[0] : (T)0.0f;
    } else {
        typedef T vt __attribute__((ext_vector_type(V)));
        if (left >= V && pw_aligned<T, V>(p)) {
            const vt v = *reinterpret_cast<const vt*>(p);
#pragma unroll
            for (int j = 0; j < V; ++j) r[j] = v[j];
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) r[j] = j < left ? p[j] : (T)0.0f;
        }
    }
}

template <class T, int V>
__device__ __forceinline__ void pw_store(T* __restrict__ p, int left, const double* val)
{
    T o[V];
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = from_f32<T>((float)val[j]);   // fp32 result, then one plain conversion
    if constexpr (V == 1) {
        if (left > 0) p[0] = o[0];
    } else {
        typedef T vt __attribute__((ext_vector_type(V)));
        if (left >= V && pw_aligned<T, V>(p)) {
            vt v;
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = o[j];
            *reinterpret_cast<vt*>(p) = v;
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (j < left) p[j] = o[j];
        }
    }
}

// the double that lane `l` (a constant) holds, in every lane
__device__ __forceinline__ double pw_bcast(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// channels c .. c + m - 1 (FULL: m = kPwChunk) of the wave's block onto acc
template <class T, int NOUT, int V, bool FULL>
__device__ __forceinline__ void pw_chunk(const T* __restrict__ xc, const T* __restrict__ wlane, unsigned HW, unsigned m, int left,
                                         unsigned wk, double (&acc)[NOUT][V])
{
    T r[kPwChunk][V];
#pragma unroll
    for (int k = 0; k < kPwChunk; ++k)
        if (FULL || (unsigned)k < m) pw_load<T, V>(xc + (size_t)k * HW, left, r[k]);
    const double wl = (wlane && (FULL || wk < m)) ? (double)to_f32(wlane[wk]) : 0.0;
#pragma unroll
    for (int k = 0; k < kPwChunk; ++k)
        if (FULL || (unsigned)k < m) {
#pragma unroll
            for (int o = 0; o < NOUT; ++o) {
                const double wd = pw_bcast(wl, o * kPwChunk + k);
#pragma unroll
                for (int j = 0; j < V; ++j) acc[o][j] = __builtin_fma(wd, (double)to_f32(r[k][j]), acc[o][j]);
            }
        }
}

__device__ __forceinline__ double pw_sigmoid(double z) { return 1.0 / (1.0 + exp(-z)); }

// grid: N * tiles workgroups (tile fastest) of S * 64 threads; dynamic LDS: (S - 1) * NOUT * V * 64 doubles.
// (w0, b0): NOUT 1: the one output; NOUT 7: score.  (w1, b1): rbox (4, C).  (w2, b2): angle (2, C).  A NULL bias is +0.0.
template <class T, int NOUT, int EPI, int V>
__global__ __launch_bounds__(kPwMaxWaves / V * 64) void rroi_pointwise_kernel(
    const T* __restrict__ x, const T* __restrict__ w0, const T* __restrict__ b0, const T* __restrict__ w1,
    const T* __restrict__ b1, const T* __restrict__ w2, const T* __restrict__ b2, T* __restrict__ y0, T* __restrict__ y1,
    T* __restrict__ y2, unsigned C, unsigned HW, unsigned tiles, unsigned cb, double rbox_scale)
{
    static_assert(NOUT * kPwChunk <= 64, "one weight of a chunk per lane");
    static_assert((NOUT == 7 && EPI == kPwEpiHeads) || (NOUT == 1 && EPI == kPwEpiSigmoid), "heads or gate");
    extern __shared__ double pw_partials[];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), S = blockDim.x >> 6;
    const unsigned n = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const unsigned px = (tile * 64u + lane) * V;           // < HW + 64 * V
    const int left = px < HW ? (int)min(HW - px, (unsigned)V) : 0;   // this lane's pixels that exist
    const unsigned c0 = wave * cb, c1 = min(c0 + cb, C);   // plan_heads: c0 < C for every wave
    const T* xp = x + ((size_t)n * C * HW + px);

    // lane o * kPwChunk + k carries w[o][c + k] of the current chunk
    const unsigned wo = lane / kPwChunk, wk = lane % kPwChunk;
    const T* wrow = nullptr;
    if (wo < (unsigned)NOUT) wrow = wo == 0 ? w0 : wo < 5 ? w1 + (size_t)(wo - 1) * C : w2 + (size_t)(wo - 5) * C;

    double acc[NOUT][V];
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
        for (int j = 0; j < V; ++j) acc[o][j] = 0.0;
    unsigned c = c0;
    for (; c + kPwChunk <= c1; c += kPwChunk)
        pw_chunk<T, NOUT, V, true>(xp + (size_t)c * HW, wrow ? wrow + c : nullptr, HW, kPwChunk, left, wk, acc);
    if (c < c1) pw_chunk<T, NOUT, V, false>(xp + (size_t)c * HW, wrow ? wrow + c : nullptr, HW, c1 - c, left, wk, acc);

    if (wave != 0) {
#pragma unroll
        for (int o = 0; o < NOUT; ++o)
#pragma unroll
            for (int j = 0; j < V; ++j) pw_partials[(((wave - 1) * NOUT + o) * V + j) * 64 + lane] = acc[o][j];
    }
    __syncthreads();
    if (wave != 0) return;

    double s[NOUT][V];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
        const T* bp = o == 0 ? b0 : o < 5 ? b1 : b2;
        const double b = bp ? (double)to_f32(bp[o == 0 ? 0 : o < 5 ? o - 1 : o - 5]) : 0.0;
#pragma unroll
        for (int j = 0; j < V; ++j) s[o][j] = b + acc[o][j];
    }
    for (unsigned k = 1; k < S; ++k)
#pragma unroll
        for (int o = 0; o < NOUT; ++o)
#pragma unroll
            for (int j = 0; j < V; ++j) s[o][j] += pw_partials[(((k - 1) * NOUT + o) * V + j) * 64 + lane];
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
        for (int j = 0; j < V; ++j) s[o][j] = pw_sigmoid(s[o][j]);

    pw_store<T, V>(y0 + ((size_t)n * HW + px), left, s[0]);
    if constexpr (EPI == kPwEpiHeads) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int j = 0; j < V; ++j) s[1 + q][j] = rbox_scale * s[1 + q][j];
            pw_store<T, V>(y1 + (((size_t)n * 4 + q) * HW + px), left, s[1 + q]);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const double a0 = 2.0 * s[5][j] - 1.0, a1 = 2.0 * s[6][j] - 1.0;
            const double r = sqrt(a0 * a0 + a1 * a1);      // 0 / 0 = NaN where both vanish, as the stock chain gives
            s[5][j] = a0 / r;
            s[6][j] = a1 / r;
        }
        pw_store<T, V>(y2 + (((size_t)n * 2 + 0) * HW + px), left, s[5]);
        pw_store<T, V>(y2 + (((size_t)n * 2 + 1) * HW + px), left, s[6]);
    }
}
