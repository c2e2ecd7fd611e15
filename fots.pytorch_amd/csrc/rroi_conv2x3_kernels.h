// rroi_conv2x3_kernels.h -- the recogniser's (2,3) convolution on the matrix cores, bfloat16 / float16, DESIGN 5.19
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_conv3x3_kernels.h, whose cv_mfma, v16f and Vec8 it uses); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// y = act(conv2d(x, w, stride 1, padding (0, 1))) with the contract of header section 12: x (N, Cin, H, W), H >= 2,
// w (Cout, Cin, 2, 3), y (N, Cout, H - 1, W), contiguous NCHW of one 16-bit type; act(v) = v < 0 ? v * slope : v in fp32; one
// rounding to the tensor's type after it.
//
// The implicit GEMM of rroi_conv3x3_kernel -- M = output channels, N = output pixels, K = (ky, kx, cin), fp32 accumulators
// on v_mfma_f32_32x32x16_{bf16,f16}, the same staging through LDS -- with another tile and another way in.  The
// network's output has ONE row ((N, 256, 2, T) -> (N, 256, 1, T)), so a tile of 4 rows would idle three waves of four:
// here the output is a flat list of items (n, oy, tile of 32 columns), x tile fastest, and a workgroup of 4 waves owns 32
// output channels of 4 consecutive items, one item per wave.  Per chunk of KC = 32 input channels the workgroup stages
//     xs[item][2 rows][34 columns][KC]   the item's input rows oy and oy + 1 with one halo column on either side; a column
//                                        outside x, a channel >= Cin and an item past the list are ZEROS (the padding is
//                                        this zero fill: nothing is read outside x; there is no padding along y)
//     ws[tap][32][KC]                    (cout, cin, tap) -> (tap, cout, cin); a row >= Cout and a channel >= Cin are zeros
// (a row of KC channels is kC2Pitch = KC + 8 elements apart: 80 bytes, so that the 16-byte fragment reads of 16 lanes fall
// into 16 different groups of four banks) and every wave runs, tap by tap and 16 channels at a time, one MFMA: the A
// fragment of lane l is ws[tap][l & 31][16 ks + 8 (l >> 5) .. + 7], the B fragment xs[its item][ky][(l & 31) + kx][the same 8
// channels].  Result: column (pixel) l & 31, row (channel) (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) in register reg.
//
// The grids this kernel sees are small (96 workgroups for 24 crops of 64 columns: fewer than there are CUs), so nothing
// hides a workgroup's own staging, and that is bound by the NUMBER of loads: one 2-byte load per element took nearly as
// long with two chunks in flight as with one.  So the way in is 4 bytes wide: a thread loads two neighbouring
// pixels of one channel (tile columns 2 q - 1 and 2 q, an even column of x) and the six taps of a (cout, cin) as three
// words, wherever the address is a multiple of 4 -- for a 4-byte-aligned tensor with an even W * H, every pair of the
// network's shapes -- and single elements elsewhere (decided per load: any element-aligned address works).  Two chunks
// are in flight in registers (sets A and B).  The order of accumulation -- chunk, tap, 16-channel step -- is the same for
// every element and every launch: no atomic, no split of K, so two calls give the same bits.  Stores are masked by Cout,
// W and the item count; for one register the 32 lanes of a half-wave store 32 consecutive pixels of one channel's row.
// ------------------------------------------------------------------------------------
constexpr int kC2Threads = 256;
constexpr int kC2Items = 4;              // items per workgroup: one per wave
constexpr int kC2TileW = 32;             // output columns per item: the MFMA's N
constexpr int kC2KC = 32;                // input channels per staged chunk: two MFMA k steps per tap
constexpr int kC2Pitch = kC2KC + 8;      // elements between two rows of a chunk in LDS
constexpr int kC2InW = kC2TileW + 2;     // the input columns of an item with its halo
constexpr int kC2Pix = 2 * kC2InW;       // the input pixels of an item
constexpr int kC2Pairs = kC2InW / 2 + 1; // column pairs (2 q - 1, 2 q), q = 0 .. 17: the first and the last are half outside
constexpr int kC2LdsBytes = (kC2Items * kC2Pix + 6 * 32) * kC2Pitch * 2;

template <class T>
__device__ __forceinline__ unsigned c2_bits(T v) { return (unsigned)__builtin_bit_cast(unsigned short, v); }

// grid: groups * m_tiles workgroups
template <class T>
__global__ __launch_bounds__(kC2Threads) void rroi_conv2x3_kernel(
    const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y, unsigned Cin, unsigned Cout, unsigned H, unsigned W,
    unsigned Ho, unsigned x_tiles, unsigned m_tiles, unsigned items, float slope)
{
    typedef typename Vec8<T>::type vec8;
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    constexpr int KC = kC2KC, KP = kC2Pitch, OCT = KC / 8;
    constexpr int ROWP = 2 * kC2Pairs, GRP = kC2Items * ROWP;     // pairs of an item, of a workgroup (per 8-channel group)
    constexpr int NE = GRP * OCT;                                 // entries of x per chunk: (pair, 8-channel group)
    __shared__ __attribute__((aligned(16))) unsigned short xs[kC2Items * kC2Pix * KP];
    __shared__ __attribute__((aligned(16))) unsigned short ws[6 * 32 * KP];

    // Workgroups go to the chip's 8 XCDs round robin, each with an L2 of its own: the m_tiles workgroups that read one
    // group's input tiles are given indices 8 apart, so that they share one L2 (whole blocks of 8 groups; the last
    // groups % 8 groups, channel tile slowest, take the rest of the grid).
    const unsigned groups = (items + kC2Items - 1) / kC2Items, whole = groups / 8u * 8u;
    unsigned mt, grp;
    if (blockIdx.x < whole * m_tiles) {
        grp = blockIdx.x % 8u + 8u * (blockIdx.x / (8u * m_tiles));
        mt = blockIdx.x / 8u % m_tiles;
    } else {
        const unsigned b = blockIdx.x - whole * m_tiles, rem = groups - whole;
        grp = whole + b % rem;
        mt = b / rem;
    }
    const unsigned co0 = mt * 32, item0 = grp * kC2Items;
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, r = lane & 31u, h = lane >> 5;
    const size_t plane = (size_t)H * W;

    v16f acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;

    // What a thread stages per chunk: XI entries of the input tiles (one entry = two neighbouring pixels x 8 channels,
    // lanes along an item's row) and WI of the weights (one entry = one (cout, cin), its six taps consecutive in w).
    // Where an entry of x lies does not depend on the chunk: it is worked out once.  x has fewer than 2^31 elements.
    constexpr int XI = (NE + kC2Threads - 1) / kC2Threads, WI = 32 * KC / kC2Threads;
    unsigned xoff[XI];        // of channel 8 g of the pair's first pixel, from x (used where xmode says a pixel exists)
    int xpix[XI];             // the pair's first pixel in xs (-1 .. ): item * 68 + row * 34 + 2 q - 1
    unsigned xmode[XI];       // bit 0 / 1: the first / second pixel is inside x; bit 2 / 3: it is a column of the tile
#pragma unroll
    for (int k = 0; k < XI; ++k) {
        const unsigned e = tid + k * kC2Threads;
        const unsigned g = e / GRP, pr = e - g * GRP;
        const unsigned it = pr / ROWP, q2 = pr - it * ROWP;
        const unsigned iy = q2 / kC2Pairs, q = q2 - iy * kC2Pairs;
        const unsigned item = item0 + it;
        const unsigned xt = item % x_tiles, rest = item / x_tiles;
        const unsigned oy = rest % Ho, n = rest / Ho;
        const int gx0 = (int)(xt * kC2TileW + 2 * q) - 2;              // the pair's columns of x: gx0 (even), gx0 + 1
        const bool real = e < (unsigned)NE, live = real && item < items && 8 * g < Cin;
        const bool t0 = real && q >= 1, t1 = real && q + 1 < (unsigned)kC2Pairs;          // columns of the tile
        const bool in0 = live && t0 && gx0 >= 0 && gx0 < (int)W, in1 = live && t1 && gx0 + 1 >= 0 && gx0 + 1 < (int)W;
        xmode[k] = (in0 ? 1u : 0u) | (in1 ? 2u : 0u) | (t0 ? 4u : 0u) | (t1 ? 8u : 0u);
        xpix[k] = (int)(it * kC2Pix + iy * kC2InW + 2 * q) - 1;
        // in0 or in1 implies gx0 >= 0 (gx0 is even, so gx0 + 1 >= 0 does): the index below is not negative
        xoff[k] = (in0 || in1) ? (unsigned)(((size_t)n * Cin + 8 * g) * plane + (size_t)(oy + iy) * W + (size_t)gx0) : 0u;
    }
    struct Regs {
        unsigned x[XI][8];    // per channel: both pixels (first in the low half) where `wide` says so, else the first
        unsigned x1[XI][8];   // ... and the second, each in the low half of its own register
        unsigned wide[XI];    // bit j: channel j of the entry came as one word
        unsigned w[WI][3];    // the six taps of one (cout, cin), two to a word
    };
    const auto fetch = [&](unsigned c0, Regs& R) {
#pragma unroll
        for (int k = 0; k < XI; ++k) {
            const unsigned g = (tid + k * kC2Threads) / GRP;
            const unsigned c = c0 + 8 * g, m = xmode[k] & 3u;
            // Nothing below computes on a loaded value (the halves are sorted out when the registers go to LDS): a
            // use inside these branches would make every load wait for the one before it.
            unsigned wide = 0u;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                unsigned a = 0u, b = 0u;
                if (m != 0u && c + j < Cin) {
                    const T* p = x + ((size_t)xoff[k] + ((size_t)c0 + j) * plane);
                    if (m == 3u && (reinterpret_cast<size_t>(p) & 3u) == 0) {
                        a = *reinterpret_cast<const unsigned*>(p);
                        wide |= 1u << j;
                    } else {
                        if (m & 1u) a = c2_bits(p[0]);
                        if (m & 2u) b = c2_bits(p[1]);
                    }
                }
                R.x[k][j] = a;
                R.x1[k][j] = b;
            }
            R.wide[k] = wide;
        }
#pragma unroll
        for (int k = 0; k < WI; ++k) {
            const unsigned e = tid + k * kC2Threads;
            const unsigned ro = e / KC, ci = e - ro * KC;
            const unsigned co = co0 + ro, c = c0 + ci;
            R.w[k][0] = R.w[k][1] = R.w[k][2] = 0u;
            if (co < Cout && c < Cin) {
                const T* p = w + ((size_t)co * Cin + c) * 6;
                if ((reinterpret_cast<size_t>(p) & 3u) == 0) {
                    const unsigned* p32 = reinterpret_cast<const unsigned*>(p);
#pragma unroll
                    for (int i = 0; i < 3; ++i) R.w[k][i] = p32[i];
                } else {
#pragma unroll
                    for (int i = 0; i < 3; ++i) R.w[k][i] = c2_bits(p[2 * i]) | c2_bits(p[2 * i + 1]) << 16;
                }
            }
        }
    };
    // one chunk: its registers go to LDS, the same registers are refilled with the chunk two ahead, the chunk is multiplied
    const auto step = [&](unsigned c0, Regs& R) {
        __syncthreads();      // the previous chunk's fragments have been read
#pragma unroll
        for (int k = 0; k < XI; ++k) {
            const unsigned g = (tid + k * kC2Threads) / GRP;
            unsigned p0[8], p1[8];      // the first and the second pixel's channels, each in the low half
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool one_word = (R.wide[k] >> j & 1u) != 0u;
                p0[j] = R.x[k][j] & 0xffffu;
                p1[j] = one_word ? R.x[k][j] >> 16 : R.x1[k][j];
            }
            v4u lo, hi;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                lo[i] = p0[2 * i] | p0[2 * i + 1] << 16;
                hi[i] = p1[2 * i] | p1[2 * i + 1] << 16;
            }
            if (xmode[k] & 4u) *reinterpret_cast<v4u*>(&xs[xpix[k] * KP + 8 * (int)g]) = lo;
            if (xmode[k] & 8u) *reinterpret_cast<v4u*>(&xs[(xpix[k] + 1) * KP + 8 * (int)g]) = hi;
        }
#pragma unroll
        for (int k = 0; k < WI; ++k) {
            const unsigned e = tid + k * kC2Threads;
            const unsigned ro = e / KC, ci = e - ro * KC;
#pragma unroll
            for (int t = 0; t < 6; ++t)
                ws[(t * 32 + ro) * KP + ci] = (unsigned short)(t & 1 ? R.w[k][t >> 1] >> 16 : R.w[k][t >> 1] & 0xffffu);
        }
        if (c0 + 2 * KC < Cin) fetch(c0 + 2 * KC, R);      // in flight while this chunk and the next are multiplied
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int ky = t / 3, kx = t - 3 * ky;
#pragma unroll
            for (int ks = 0; ks < KC / 16; ++ks) {
                const vec8 af = *reinterpret_cast<const vec8*>(&ws[(t * 32 + r) * KP + 16 * ks + 8 * h]);
                const vec8 bf =
                    *reinterpret_cast<const vec8*>(&xs[(wave * kC2Pix + ky * kC2InW + r + kx) * KP + 16 * ks + 8 * h]);
                acc = cv_mfma<T>(af, bf, acc);
            }
        }
    };

    Regs A, B;
    fetch(0, A);
    if (KC < Cin) fetch(KC, B);
    for (unsigned c0 = 0; c0 < Cin; c0 += 2 * KC) {
        step(c0, A);
        if (c0 + KC < Cin) step(c0 + KC, B);
    }

    const unsigned item = item0 + wave;
    if (item >= items) return;
    const unsigned xt = item % x_tiles, rest = item / x_tiles;
    const unsigned oy = rest % Ho, n = rest / Ho;
    const unsigned ox = xt * kC2TileW + r;
    if (ox >= W) return;
    const size_t oplane = (size_t)Ho * W;
    T* yp = y + ((size_t)n * Cout * oplane + (size_t)oy * W + ox);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned co = co0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (co < Cout) {
            float v = acc[i];
            v = v < 0.0f ? v * slope : v;
            yp[(size_t)co * oplane] = from_f32<T>(v);
        }
    }
}
