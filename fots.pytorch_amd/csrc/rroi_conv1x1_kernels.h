// rroi_conv1x1_kernels.h -- the network's bias-free 1x1 convolutions on the matrix cores, bfloat16 / float16, with the
// shortcut's BatchNorm folded in, DESIGN 5.17
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_conv3x3_kernels.h: cv_mfma, v16f, Vec8); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// y[n,k,i,j] = act(s[k] * sum_c w[k,c] x[n,c,S i,S j] + t[k]) with the contract of header section 11: x (N, Cin, H, W),
// w (Cout, Cin), y (N, Cout, Ho, Wo), contiguous NCHW of one 16-bit type; act(v) = v < 0 ? v * slope : v in fp32; one
// rounding to the tensor's type after it.  Without a norm (NORM = false) s and t do not exist: the fp32 sum goes straight
// into act.
//
// A GEMM per image on v_mfma_f32_32x32x16_{bf16,f16}: M = output channels, N = output pixels -- the flat index
// p = i * Wo + j of the output plane, which at stride 1 is the flat index of the input plane too -- K = input channels,
// fp32 accumulators.  A workgroup of 4 waves owns BM = 32 * MT output channels of 128 consecutive output pixels of one
// image; wave v owns pixels 32 v .. 32 v + 31, that is MT accumulator tiles of 32 channels by 32 pixels.  The input
// channels are walked 64 at a time; a chunk is fetched into registers while the chunk before it is multiplied.  Per chunk
// the workgroup stages through LDS
//     xs[channel of the chunk][pixel of the tile]   as it lies in memory: a thread moves 8 consecutive pixels of one
//                                                   channel, in one 16-byte load where they are the plane's own
//                                                   neighbours (stride 1), all exist and the address is 16-byte aligned
//                                                   -- decided per item, so any element-aligned x works -- and one by
//                                                   one otherwise; a pixel >= Ho * Wo and a channel >= Cin are ZEROS
//     ws[BM][channel of the chunk]                  rows of w: 16-byte loads under the same rule; a row >= Cout and a
//                                                   channel >= Cin are zeros
// and every wave then runs, 16 channels at a time, one MFMA per accumulator tile.  The A fragment of lane l is
// ws[32 m + (l & 31)][16 ks + 8 (l >> 5) .. + 7], one 16-byte read.  The B fragment is the same 8 channels of pixel
// l & 31, which lie a row of xs apart: two ds_read_b64_tr_b16, each handing a group of 16 lanes the transpose of a block
// of 4 channels x 16 pixels (lane 4 q + p of the group supplies the address of channel q, pixels 4 p .. 4 p + 3; lane i
// receives pixel i's four channels).  Every lane supplies an address inside xs and no lane is masked when they are
// issued (the reads cross lanes); the addresses are multiples of 8 bytes (kC1Row is a multiple of 4).  kC1Row = 160
// elements = 80 dwords: the four channel rows of a block start 16 banks apart, so a half-wave's read covers all 64
// banks once.  Both operands number k the same way.  Result: column (pixel) l & 31, row (channel)
// (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) in register reg.
// The order of accumulation -- chunk, 16-channel step, the instruction's own -- is the same for every element and every
// launch: no atomic, no split of K across workgroups, so two calls give the same bits.  A 16-channel step that lies
// wholly past Cin is skipped (by every wave alike).
// The norm: the first BM threads compute s = g / sqrt(var + eps), t = b - mean * s for the workgroup's channel rows in
// fp32, once, into LDS; nothing is cached between calls.
// Stores are masked by Cout and Ho * Wo; for one register the 32 lanes of a half-wave store 32 consecutive pixels of one
// channel's plane.
// ------------------------------------------------------------------------------------
constexpr int kC1Threads = 256;
constexpr int kC1Pixels = 128;          // output pixels per workgroup: 32 per wave
constexpr int kC1Chunk = 64;            // input channels per staged chunk
constexpr int kC1Row = kC1Pixels + 32;  // elements per channel row of xs
constexpr int kC1WRow = kC1Chunk + 8;   // elements per output-channel row of ws
constexpr int c1_lds_bytes(int MT) { return kC1Chunk * kC1Row * 2 + 32 * MT * kC1WRow * 2 + 32 * MT * 8; }

// the two transposed reads of 4 channels x 16 pixels per 16 lanes (see above) that make one B fragment; lo / hi: this
// lane's addresses inside a __shared__ array for channels 0 .. 3 and 4 .. 7 of its eight
template <class T>
__device__ __forceinline__ typename Vec8<T>::type c1_read_tr(const T* lo, const T* hi)
{
    typedef short vec4 __attribute__((ext_vector_type(4)));       // 16-bit lanes moved as they are, whatever they hold
    typedef short bits8 __attribute__((ext_vector_type(8)));
    typedef __attribute__((address_space(3))) vec4* lds4;
    const vec4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(lo));
    const vec4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(hi));
    return __builtin_bit_cast(typename Vec8<T>::type, (bits8)__builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

// grid: N * p_tiles * m_tiles workgroups (channel tile fastest, then pixel tile) of 256 threads
template <class T, int MT, int S, bool NORM>
__global__ __launch_bounds__(kC1Threads) void rroi_conv1x1_kernel(
    const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y, const T* __restrict__ gamma,
    const T* __restrict__ beta, const T* __restrict__ mean, const T* __restrict__ var, float eps, unsigned Cin,
    unsigned Cout, unsigned H, unsigned W, unsigned Wo, unsigned P, unsigned m_tiles, unsigned p_tiles, float slope)
{
    typedef typename Vec8<T>::type vec8;
    constexpr int BM = 32 * MT, KC = kC1Chunk;
    __shared__ __attribute__((aligned(16))) T xs[KC * kC1Row];
    __shared__ __attribute__((aligned(16))) T ws[BM * kC1WRow];
    __shared__ float fold_s[BM], fold_t[BM];

    unsigned b = blockIdx.x;
    const unsigned mt = b % m_tiles;  b /= m_tiles;
    const unsigned pt = b % p_tiles;
    const unsigned n = b / p_tiles;
    const unsigned co0 = mt * BM, p0 = pt * kC1Pixels;
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, r = lane & 31u, h = lane >> 5;
    const size_t plane = (size_t)H * W;
    const T* xn = x + (size_t)n * Cin * plane;
    const T zero = from_f32<T>(0.0f);

    if constexpr (NORM) {
        if (tid < (unsigned)BM) {
            const unsigned co = co0 + tid;
            float s = 0.0f, t = 0.0f;
            if (co < Cout) {
                const float g = gamma ? to_f32(gamma[co]) : 1.0f, bb = beta ? to_f32(beta[co]) : 0.0f;
                s = g / sqrtf(to_f32(var[co]) + eps);
                t = bb - to_f32(mean[co]) * s;
            }
            fold_s[tid] = s;       // read after the K loop: its barriers lie in between
            fold_t[tid] = t;
        }
    }

    v16f acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[m][i] = 0.0f;

    // What a thread stages per chunk.  X: XI items of one channel x 8 consecutive output pixels; item = tid + 256 k is
    // channel item >> 4, pixel group item & 15 = tid & 15 -- the same 8 pixels in every item of a thread, so where they
    // lie in the input plane is worked out once.  W: WI items of one row x 8 consecutive channels.
    constexpr int XI = KC * (kC1Pixels / 8) / kC1Threads, WI = BM * (KC / 8) / kC1Threads;
    const unsigned pg = p0 + 8 * (tid & 15u);            // the group's first output pixel
    const unsigned live = pg >= P ? 0u : (P - pg < 8u ? P - pg : 8u);   // how many of the 8 exist
    unsigned src[S == 1 ? 1 : 8];                        // their offsets in the input plane (stride 1: pg + j)
    if constexpr (S == 1) {
        src[0] = pg;
    } else {
        unsigned oy = pg / Wo, ox = pg - oy * Wo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            src[j] = (oy * S) * W + ox * S;              // (only the first `live` are used: those lie inside the plane)
            if (++ox == Wo) ox = 0, ++oy;
        }
    }
    vec8 xr[XI], wr[WI];
    const auto fetch = [&](unsigned c0) {
#pragma unroll
        for (int k = 0; k < XI; ++k) {
            const unsigned c = c0 + ((tid + k * kC1Threads) >> 4);
#pragma unroll
            for (int j = 0; j < 8; ++j) xr[k][j] = zero;
            if (c < Cin && live) {
                const T* pc = xn + (size_t)c * plane;
                if (S == 1 && live == 8u && (reinterpret_cast<uintptr_t>(pc + src[0]) & 15u) == 0) {
                    xr[k] = *reinterpret_cast<const vec8*>(pc + src[0]);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if ((unsigned)j < live) xr[k][j] = pc[S == 1 ? src[0] + j : src[(S - 1) * j]];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < WI; ++k) {
            const unsigned item = tid + k * kC1Threads;
            const unsigned co = co0 + (item >> 3), c = c0 + 8 * (item & 7u);
#pragma unroll
            for (int j = 0; j < 8; ++j) wr[k][j] = zero;
            if (co < Cout && c < Cin) {
                const T* pw = w + ((size_t)co * Cin + c);
                if (c + 8 <= Cin && (reinterpret_cast<uintptr_t>(pw) & 15u) == 0) {
                    wr[k] = *reinterpret_cast<const vec8*>(pw);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (c + j < Cin) wr[k][j] = pw[j];
                }
            }
        }
    };

    // this lane's addresses for the transposed reads: channel (row of xs) 8 h + q, pixels 32 wave + 16 (group & 1) + 4 p
    const unsigned grp = (lane >> 4) & 1u, q = (lane >> 2) & 3u, pp = lane & 3u;
    const T* xb = &xs[(8 * h + q) * kC1Row + 32 * wave + 16 * grp + 4 * pp];

    fetch(0);
    for (unsigned c0 = 0; c0 < Cin; c0 += KC) {
        __syncthreads();      // the previous chunk's fragments have been read
#pragma unroll
        for (int k = 0; k < XI; ++k) {
            const unsigned item = tid + k * kC1Threads;
            *reinterpret_cast<vec8*>(&xs[(item >> 4) * kC1Row + 8 * (item & 15u)]) = xr[k];
        }
#pragma unroll
        for (int k = 0; k < WI; ++k) {
            const unsigned item = tid + k * kC1Threads;
            *reinterpret_cast<vec8*>(&ws[(item >> 3) * kC1WRow + 8 * (item & 7u)]) = wr[k];
        }
        __syncthreads();
        if (c0 + KC < Cin) fetch(c0 + KC);      // in flight while this chunk is multiplied
#pragma unroll
        for (int ks = 0; ks < KC / 16; ++ks) {
            if (c0 + 16 * ks >= Cin) break;     // uniform: the whole step is past Cin (its rows of xs and ws are zeros)
            const vec8 bf = c1_read_tr<T>(xb + 16 * ks * kC1Row, xb + (16 * ks + 4) * kC1Row);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const vec8 af = *reinterpret_cast<const vec8*>(&ws[(32 * m + r) * kC1WRow + 16 * ks + 8 * h]);
                acc[m] = cv_mfma<T>(af, bf, acc[m]);
            }
        }
    }

    const unsigned p = p0 + 32 * wave + r;
    if (p >= P) return;
    T* yp = y + ((size_t)n * Cout * P + p);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const unsigned ro = 32 * m + (i & 3) + 8 * (i >> 2) + 4 * h, co = co0 + ro;
            if (co < Cout) {
                float v = acc[m][i];
                if constexpr (NORM) v = v * fold_s[ro] + fold_t[ro];
                v = v < 0.0f ? v * slope : v;
                yp[(size_t)co * P] = from_f32<T>(v);
            }
        }
}
