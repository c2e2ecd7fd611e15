// rroi_recogniser_kernels.h -- the two kernels of the recogniser's tail and pools, DESIGN 5.16: the 1x1 convolution to the
// classes with its bias and the log-softmax over them in one launch, and a leaky ReLU + (2,1) max-pool in one launch.
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_heads_kernels.h, whose pw_load / pw_aligned the pool uses); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// A. The head:  y[n, k, t] = z[n, k, t] - logsumexp_j z[n, j, t],  z[n, k, t] = b[k] + sum_c w[k, c] * x[n, c, t]
// with the arithmetic of header section 10 (the recipe of section 7):
//     z_k = ((b_k + w[k][0] x[0]) + w[k][1] x[1]) + ...   in channel order, every product exact in double
//     m = max_j z_j;   e_j = exp(z_j - m);   s = ((0 + e_0) + e_1) + ...  in class order;   L = m + log(s)
//     out = (T)(float)(z_k - L)
// The product of two widened 24-bit significands is exact in double, so the fma below and a separate multiply and add
// give the same bits.  No channel of the tensor is skipped (0 * inf = NaN, as the convolution gives).
//
// T is 32 - 128 and N 1 - 24 in the pipeline: there are few columns, and a column costs K * C double FMAs.  So a workgroup
// takes only 16 columns of one crop, and a wave is 4 rows of 16 lanes: lane (g, t) owns column t and the 8 classes
// [32 wave + 8 g, + 8) over all C channels -- 8 double accumulators, 32 classes per wave, S = ceil(K / 32) waves.
// Weights are uniform within a row of 16 lanes.  Per chunk of 32 channels a row needs 8 x 32 of them: lane t loads the 16
// w[class t / 2][c + 16 (t % 2) + i], widens them once, and the arithmetic reads each out of its lane with a DPP row
// broadcast (row_newbcast: two v_mov_b32_dpp per double), so a weight costs one load per row whatever the element type.
// The next chunk's 48 loads are issued before the current chunk's arithmetic (a wave has a SIMD to itself in the
// pipeline's shapes: nothing else would hide the latency; with chunks of 8 channels the kernel took 39 us at every small
// grid, a memory latency per chunk).  No load depends on the lane: a lane behind the row's end reads the last
// column and a lane without a class the last class, and what they compute is dropped; a channel behind the last one is
// +0.0 on both sides, so its products are +0.0 and change no sum.
// The softmax crosses rows and waves through LDS, three barriers, no atomics:
//     1  every lane leaves the maximum of its own logits, [wave][row][column]; all take the maximum of those (a maximum
//        does not depend on the order; a NaN logit is ignored here and reaches every output through the sum below)
//     2  every lane leaves e_j = exp(z_j - m) of its own classes, [class][column], in the same buffer
//     3  every lane adds all K of its column in class order, takes L and stores its own classes: 16 consecutive t per class.
// m = +inf or m = -inf makes inf - inf = NaN in the sum, so the whole column is NaN, as the float64 reference gives.
// The same arguments give the same bits.
// ------------------------------------------------------------------------------------
constexpr int kOhCols = 16;                              // columns per workgroup: one DPP row of lanes
constexpr int kOhRowClasses = 8;                         // classes per row: kOhRowClasses * kOhChunk = 16 lanes * kOhLaneW
constexpr int kOhClasses = 4 * kOhRowClasses;            // classes per wave
constexpr int kOhChunk = 32;                             // channels per step: loads in flight per lane
constexpr int kOhLaneW = kOhChunk / 2;                   // weights of a chunk per lane: two lanes share a class
constexpr int kOhMaxWaves = 4;
constexpr int kOhMaxClasses = kOhClasses * kOhMaxWaves;  // RROI_OCR_HEAD_MAX_CLASSES

template <int I, int N, class F>
__device__ __forceinline__ void oh_static_for(F&& f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        oh_static_for<I + 1, N>(f);
    }
}

// the double that lane L of the caller's row of 16 lanes holds (every lane of the wave is active)
template <int L>
__device__ __forceinline__ double oh_row_bcast(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x150 + L, 0xf, 0xf, false);   // row_newbcast:L
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x150 + L, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

template <class T>
struct OhChunk {
    T x[kOhChunk];   // the lane's column, channels c .. c + kOhChunk - 1
    T w[kOhLaneW];   // the lane's weights of the row's kOhRowClasses x kOhChunk
};

// xp: the lane's column at channel 0; wp: the lane's class row + its half of a chunk.  Both point at real elements for
// every lane (the kernel clamps the column and the class), so that no load sits under a per-lane condition: a chunk's 48
// loads are issued back to back.  FULL: channels c .. c + kOhChunk - 1 exist.  Otherwise a channel >= C reads the last one
// and is replaced by +0.0 on both sides: the product is +0.0 whatever the other side holds.
template <class T, bool FULL>
__device__ __forceinline__ void oh_load(OhChunk<T>& r, const T* __restrict__ xp, const T* __restrict__ wp, unsigned c, unsigned C,
                                        unsigned Tn, unsigned wc)
{
#pragma unroll
    for (int k = 0; k < kOhChunk; ++k) {
        const unsigned ck = FULL ? c + k : min(c + k, C - 1u);
        const T v = xp[(size_t)ck * Tn];
        r.x[k] = (FULL || c + k < C) ? v : (T)0.0f;
    }
#pragma unroll
    for (int i = 0; i < kOhLaneW; ++i) {
        const unsigned ci = FULL ? c + wc + i : min(c + wc + i, C - 1u);
        const T v = wp[ci];
        r.w[i] = (FULL || c + wc + i < C) ? v : (T)0.0f;
    }
}

// chunk i of the row: the full form for every chunk but a last partial one (a uniform branch)
template <class T>
__device__ __forceinline__ void oh_load_chunk(OhChunk<T>& r, const T* __restrict__ xp, const T* __restrict__ wp, unsigned i,
                                              unsigned C, unsigned Tn, unsigned wc)
{
    if ((i + 1u) * kOhChunk <= C)
        oh_load<T, true>(r, xp, wp, i * kOhChunk, C, Tn, wc);
    else
        oh_load<T, false>(r, xp, wp, i * kOhChunk, C, Tn, wc);
}

template <class T>
__device__ __forceinline__ void oh_fma(const OhChunk<T>& r, double (&acc)[kOhRowClasses])
{
    double wl[kOhLaneW], xd[kOhChunk];
#pragma unroll
    for (int i = 0; i < kOhLaneW; ++i) wl[i] = (double)to_f32(r.w[i]);
#pragma unroll
    for (int k = 0; k < kOhChunk; ++k) xd[k] = (double)to_f32(r.x[k]);
    oh_static_for<0, kOhChunk>([&](auto kk) {                  // channels outermost: every class takes them in order
        constexpr int k = decltype(kk)::value;
        oh_static_for<0, kOhRowClasses>([&](auto oo) {
            constexpr int o = decltype(oo)::value;
            acc[o] = __builtin_fma(oh_row_bcast<o * 2 + k / kOhLaneW>(wl[k % kOhLaneW]), xd[k], acc[o]);
        });
    });
}

// grid: N * tiles workgroups (tile fastest) of S * 64 threads; dynamic LDS: max(64 S, 16 K) doubles.  b may be NULL (+0.0).
template <class T>
__global__ __launch_bounds__(kOhMaxWaves * 64) void rroi_ocr_head_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                                        const T* __restrict__ b, T* __restrict__ y, unsigned C,
                                                                        unsigned K, unsigned Tn, unsigned tiles)
{
    static_assert(kOhRowClasses * kOhChunk == kOhCols * kOhLaneW, "kOhLaneW weights of a chunk per lane of a row");
    static_assert(kOhMaxClasses * kOhCols * sizeof(double) <= 65536 && kOhMaxWaves * 64 * sizeof(double) <= 65536, "LDS");
    extern __shared__ double oh_lds[];
    const unsigned lane = threadIdx.x & 63u, row = lane >> 4, tl = lane & 15u;
    const unsigned wave = threadIdx.x >> 6, S = blockDim.x >> 6;
    const unsigned n = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const unsigned t = tile * kOhCols + tl;                // < Tn + 16
    const bool col = t < Tn;                               // a lane behind the row's end loads and stores nothing
    const unsigned k0 = wave * kOhClasses + row * kOhRowClasses;                     // may be >= K: a row without classes
    const unsigned kn = k0 < K ? min(K - k0, (unsigned)kOhRowClasses) : 0u;
    // a lane behind the row's end reads the last column, a lane whose class does not exist the last class: what they
    // compute is never used (columns and classes do not mix before the maxima, which take existing classes alone)
    const T* xp = x + ((size_t)n * C * Tn + min(t, Tn - 1u));
    const unsigned wc = (unsigned)kOhLaneW * (tl & 1u);    // lane tl carries w[k0 + tl / 2][c + wc .. c + wc + kOhLaneW - 1]
    const T* wp = w + (size_t)min(k0 + (tl >> 1), K - 1u) * C;

    double acc[kOhRowClasses];
#pragma unroll
    for (int o = 0; o < kOhRowClasses; ++o) acc[o] = (b && (unsigned)o < kn) ? (double)to_f32(b[k0 + o]) : 0.0;
    OhChunk<T> ra, rb;
    const unsigned chunks = (C + kOhChunk - 1u) / kOhChunk;
    oh_load_chunk(ra, xp, wp, 0u, C, Tn, wc);
    for (unsigned i = 0;;) {                               // two chunks per round: the buffers keep their registers
        if (i + 1u < chunks) oh_load_chunk(rb, xp, wp, i + 1u, C, Tn, wc);
        oh_fma(ra, acc);
        if (++i >= chunks) break;
        if (i + 1u < chunks) oh_load_chunk(ra, xp, wp, i + 1u, C, Tn, wc);
        oh_fma(rb, acc);
        if (++i >= chunks) break;
    }

    double m = -__builtin_huge_val();
#pragma unroll
    for (int o = 0; o < kOhRowClasses; ++o)
        if ((unsigned)o < kn) m = __builtin_fmax(m, acc[o]);
    oh_lds[wave * 64u + lane] = m;
    __syncthreads();
    for (unsigned s = 0; s < 4u * S; ++s) m = __builtin_fmax(m, oh_lds[s * kOhCols + tl]);
    __syncthreads();                                       // every lane has read the maxima: the buffer is free
#pragma unroll
    for (int o = 0; o < kOhRowClasses; ++o)
        if ((unsigned)o < kn) oh_lds[(k0 + o) * kOhCols + tl] = exp(acc[o] - m);
    __syncthreads();
    double sum = 0.0;
    for (unsigned j = 0; j < K; ++j) sum += oh_lds[j * kOhCols + tl];
    const double L = m + log(sum);
    if (!col) return;
    T* yp = y + (((size_t)n * K + k0) * Tn + t);
#pragma unroll
    for (int o = 0; o < kOhRowClasses; ++o)
        if ((unsigned)o < kn) yp[(size_t)o * Tn] = from_f32<T>((float)(acc[o] - L));   // fp32, then one plain conversion
}

// ------------------------------------------------------------------------------------
// B. Activation + (2,1) max-pool:  y[n, c, i, j] = max(act(x[n, c, 2i, j]), act(x[n, c, 2i + 1, j])),  Ho = H / 2
//     act(v) = v < 0 ? v * negative_slope : v   in fp32, rounded once to T; the two rounded values are compared:
//     the lower row's element is taken where it is greater or a NaN, the upper row's otherwise (a tie, signed zeros
//     included, keeps the upper one) -- `F.max_pool2d(F.leaky_relu(x, s), (2, 1), stride=(2, 1))` bit for bit.
// A streaming kernel: a thread owns V consecutive columns (16 bytes) of one output row, that is of two input rows.  W is
// arbitrary, so whether a row's address allows a vector access is decided per row and per tensor, as pw_load does; the
// last chunk of a row and every misaligned row go element by element.  An odd last input row is never read.
// ------------------------------------------------------------------------------------
constexpr int kApThreads = 256;

// act(v) with the product as an fp32 value of its own.  Left to the compiler, the multiply and the conversion to float16
// become one v_fma_mixlo_f16 with an addend of +0.0, and (-0.0) + (+0.0) = +0.0: every v < 0 at a slope of 0.0 came out
// as +0.0 where the rule -- and torch on the CPU -- give -0.0.  (torch's own float16 leaky ReLU on this GPU shows the same
// +0.0.)  The empty asm keeps the product in a register between the two instructions.
__device__ __forceinline__ float ap_act(float v, float slope)
{
    float p = v * slope;
    asm volatile("" : "+v"(p));
    return v < 0.0f ? p : v;
}

template <class T, int V>
__device__ __forceinline__ void ap_store(T* __restrict__ p, int left, const T* o)
{
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

// grid: ceil(rows * chunks / kApThreads) workgroups of kApThreads threads; rows = N * C * Ho, chunks = ceil(W / V)
template <class T, int V>
__global__ __launch_bounds__(kApThreads) void rroi_act_maxpool2x1_kernel(const T* __restrict__ x, T* __restrict__ y, unsigned H,
                                                                        unsigned W, unsigned Ho, unsigned chunks, unsigned items,
                                                                        float slope)
{
    const unsigned idx = blockIdx.x * (unsigned)kApThreads + threadIdx.x;   // < items + kApThreads <= 2^31 + 256
    if (idx >= items) return;
    const unsigned row = idx / chunks, j0 = (idx % chunks) * V;             // row = plane * Ho + i;  j0 < W
    const unsigned plane = row / Ho, i = row % Ho;
    const int left = (int)min(W - j0, (unsigned)V);
    const T* up = x + (((size_t)plane * H + 2u * i) * W + j0);              // rows 2i and 2i + 1 <= H - 1 exist
    T a[V], c[V], o[V];
    pw_load<T, V>(up, left, a);
    pw_load<T, V>(up + W, left, c);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float va = to_f32(a[j]), vc = to_f32(c[j]);
        const T ta = from_f32<T>(ap_act(va, slope)), tc = from_f32<T>(ap_act(vc, slope));
        const float fa = to_f32(ta), fc = to_f32(tc);
        o[j] = (fc > fa || fc != fc) ? tc : ta;
    }
    ap_store<T, V>(y + ((size_t)row * W + j0), left, o);
}
