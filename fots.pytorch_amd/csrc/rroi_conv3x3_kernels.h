// rroi_conv3x3_kernels.h -- the network's dense 3x3 convolution on the matrix cores, bfloat16 / float16, DESIGN 5.15
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_merge_kernels.h); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// y = act(conv2d(x, w, stride = S, padding = 1)) with the contract of header section 9: x (N, Cin, H, W), w (Cout, Cin, 3, 3),
// y (N, Cout, Ho, Wo), contiguous NCHW of one 16-bit type; act(v) = v < 0 ? v * slope : v in fp32; one rounding to the
// tensor's type after it.
//
// An implicit GEMM on v_mfma_f32_32x32x16_{bf16,f16}: M = output channels, N = output pixels, K = (tap, cin), fp32
// accumulators.  A workgroup of 4 waves owns BM = 32 * MT output channels of a tile of TH = 4 * NT rows by 32 columns of
// output pixels of one image; wave w owns rows w * NT .. w * NT + NT - 1, that is MT x NT accumulator tiles of 32 channels
// by 32 pixels.  The input channels are walked KC at a time; a chunk is fetched into registers while the chunk before it
// is multiplied.  Per chunk the workgroup stages through LDS
//     xs[pixel of the input tile with its halo][KC]     the NCHW -> (pixel, cin) rearrangement happens on the way in;
//                                                      a pixel outside x and a channel >= Cin are ZEROS (the padding
//                                                      is this zero fill: nothing is read outside x)
//     ws[tap][BM][KC]                                   (cout, cin, tap) -> (tap, cout, cin) likewise; a row >= Cout and a
//                                                      channel >= Cin are zeros
// and every wave then runs, tap by tap and 16 channels at a time, one MFMA per accumulator tile: the A fragment of lane
// l is ws[tap][32 m + (l & 31)][8 (l >> 5) .. + 7], the B fragment xs[the tap's pixel of output column l & 31][the same 8
// channels] -- 16 contiguous bytes each, and both operands number k the same way, so the instruction's own k order does
// not matter.  Result: column (pixel) l & 31, row (channel) (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) in register reg.
// The order of accumulation -- chunk, tap, 16-channel step -- is the same for every element and every launch: no atomic,
// no split of K across workgroups, so two calls give the same bits.  Stores are masked by Cout, Ho and Wo; for one
// register the 32 lanes of a half-wave store 32 consecutive pixels of one channel's row.
// ------------------------------------------------------------------------------------
constexpr int kCvThreads = 256;
constexpr int kCvTileW = 32;            // output columns per tile: the MFMA's N

typedef float v16f __attribute__((ext_vector_type(16)));

template <class T>
__device__ __forceinline__ v16f cv_mfma(typename Vec8<T>::type a, typename Vec8<T>::type b, v16f c)
{
    if constexpr (std::is_same<T, bf16_t>::value) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

constexpr int cv_in_h(int NT, int S) { return (4 * NT - 1) * S + 3; }   // rows of the input tile with its halo
constexpr int cv_in_w(int S) { return (kCvTileW - 1) * S + 3; }
constexpr int cv_lds_bytes(int MT, int NT, int S, int KC) { return (cv_in_h(NT, S) * cv_in_w(S) + 9 * 32 * MT) * KC * 2; }

// grid: N * m_tiles * y_tiles * x_tiles workgroups (x tile fastest, then y tile, then channel tile) of 256 threads
template <class T, int MT, int NT, int S, int KC>
__global__ __launch_bounds__(kCvThreads) void rroi_conv3x3_kernel(
    const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y, unsigned Cin, unsigned Cout, unsigned H, unsigned W,
    unsigned Ho, unsigned Wo, unsigned m_tiles, unsigned y_tiles, unsigned x_tiles, float slope)
{
    typedef typename Vec8<T>::type vec8;
    constexpr int BM = 32 * MT, IH = cv_in_h(NT, S), IW = cv_in_w(S), NPIX = IH * IW, OCT = KC / 8;
    __shared__ __attribute__((aligned(16))) T xs[NPIX * KC];
    __shared__ __attribute__((aligned(16))) T ws[9 * BM * KC];

    unsigned b = blockIdx.x;
    const unsigned xt = b % x_tiles;  b /= x_tiles;
    const unsigned yt = b % y_tiles;  b /= y_tiles;
    const unsigned mt = b % m_tiles;
    const unsigned n = b / m_tiles;
    const unsigned co0 = mt * BM, oy0 = yt * (4 * NT), ox0 = xt * kCvTileW;
    const int gy0 = (int)(oy0 * S) - 1, gx0 = (int)(ox0 * S) - 1;        // the input tile's first row / column: -1 is padding
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, r = lane & 31u, h = lane >> 5;
    const size_t plane = (size_t)H * W;
    const T* xn = x + (size_t)n * Cin * plane;
    const T zero = from_f32<T>(0.0f);

    v16f acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < NT; ++q)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][q][i] = 0.0f;

    // What a thread stages per chunk: XI items of the input tile (one item = one pixel x 8 channels, lanes along the
    // tile's row) and WI items of the weights (one item = one (cout, cin), its nine taps consecutive in w).  A chunk is
    // loaded into registers while the previous one is multiplied, and written to LDS between the two barriers.
    constexpr int XI = (NPIX * OCT + kCvThreads - 1) / kCvThreads, WI = BM * KC / kCvThreads;
    vec8 xr[XI];
    T wr[WI][9];
    const auto fetch = [&](unsigned c0) {
#pragma unroll
        for (int k = 0; k < XI; ++k) {
            const unsigned item = tid + k * kCvThreads;
            const unsigned g = item / NPIX, pix = item - g * NPIX;
            const unsigned iy = pix / IW, ix = pix - iy * IW;
            const int gy = gy0 + (int)iy, gx = gx0 + (int)ix;
            const bool inside = item < (unsigned)(NPIX * OCT) && gy >= 0 && gy < (int)H && gx >= 0 && gx < (int)W;
            const unsigned c = c0 + 8 * g;
#pragma unroll
            for (int j = 0; j < 8; ++j) xr[k][j] = zero;
            if (inside) {
                const T* p = xn + ((size_t)c * plane + (size_t)gy * W + (size_t)gx);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (c + j < Cin) xr[k][j] = p[(size_t)j * plane];
            }
        }
#pragma unroll
        for (int k = 0; k < WI; ++k) {
            const unsigned item = tid + k * kCvThreads;
            const unsigned ro = item / KC, ci = item - ro * KC;
            const unsigned co = co0 + ro, c = c0 + ci;
            const bool live = co < Cout && c < Cin;
            const T* p = w + ((size_t)co * Cin + c) * 9;
#pragma unroll
            for (int t = 0; t < 9; ++t) wr[k][t] = live ? p[t] : zero;
        }
    };

    fetch(0);
    for (unsigned c0 = 0; c0 < Cin; c0 += KC) {
        __syncthreads();      // the previous chunk's fragments have been read
#pragma unroll
        for (int k = 0; k < XI; ++k) {
            const unsigned item = tid + k * kCvThreads;
            const unsigned g = item / NPIX, pix = item - g * NPIX;
            if (item < (unsigned)(NPIX * OCT)) *reinterpret_cast<vec8*>(&xs[pix * KC + 8 * g]) = xr[k];
        }
#pragma unroll
        for (int k = 0; k < WI; ++k) {
            const unsigned item = tid + k * kCvThreads;
            const unsigned ro = item / KC, ci = item - ro * KC;
#pragma unroll
            for (int t = 0; t < 9; ++t) ws[(t * BM + ro) * KC + ci] = wr[k][t];
        }
        __syncthreads();
        if (c0 + KC < Cin) fetch(c0 + KC);      // in flight while this chunk is multiplied
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int ky = t / 3, kx = t - 3 * ky;
#pragma unroll
            for (int ks = 0; ks < KC / 16; ++ks) {
                vec8 af[MT], bf[NT];
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    af[m] = *reinterpret_cast<const vec8*>(&ws[(t * BM + 32 * m + r) * KC + 16 * ks + 8 * h]);
#pragma unroll
                for (int q = 0; q < NT; ++q)
                    bf[q] = *reinterpret_cast<const vec8*>(
                        &xs[(((wave * NT + q) * S + ky) * IW + r * S + kx) * KC + 16 * ks + 8 * h]);
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int q = 0; q < NT; ++q) acc[m][q] = cv_mfma<T>(af[m], bf[q], acc[m][q]);
            }
        }
    }

    const unsigned ox = ox0 + r;
    if (ox >= Wo) return;
    const size_t oplane = (size_t)Ho * Wo;
    T* yn = y + (size_t)n * Cout * oplane;
#pragma unroll
    for (int q = 0; q < NT; ++q) {
        const unsigned oy = oy0 + wave * NT + q;
        if (oy >= Ho) continue;
        T* yp = yn + ((size_t)oy * Wo + ox);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const unsigned co = co0 + 32 * m + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (co < Cout) {
                    float v = acc[m][q][i];
                    v = v < 0.0f ? v * slope : v;
                    yp[(size_t)co * oplane] = from_f32<T>(v);
                }
            }
    }
}
