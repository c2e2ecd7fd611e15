// rroi_preprocess_kernels.h -- uint8 images to the network's input tensor in one launch, DESIGN 5.21
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_device_common.h, whose bf16_t / fp16_t it uses); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// y[n, c, oy, ox] = (T)(float)(v / 128 - 1), v the half-pixel bilinear resize (align_corners = false) of image n's channel
// c to (Ho, Wo), every operation rounded to double, in this order (include/rroi_align_hip.h section 14):
//     per axis, source extent n0, output extent n:   n0 == n:  i0 = i1 = i, l = 0
//                                                    else      s = max(0, (i + 0.5) * ((double)n0 / (double)n) - 0.5),
//                                                              i0 = min((int)floor(s), n0 - 1), i1 = min(i0 + 1, n0 - 1), l = s - i0
//     top = (1 - lx) * p[y0][x0] + lx * p[y0][x1],  bot likewise on row y1,  v = (1 - ly) * top + ly * bot
//
// The streaming structure.  A thread owns V = 16 / sizeof(T) consecutive output columns over `band` output rows of one
// image, for all three channels: the column geometry (two byte offsets and a weight per column) is computed once, the row
// geometry once per row, and an item's index is divided three times, never an element's.  The horizontal blend of a SOURCE
// row does not depend on the output row, so a thread keeps the 3 * V blends of source rows y0 and y1 in registers and, going
// down its band, reads a source row again only when it changes (in a slight downscale y1 of one output row is y0 of the
// next: one new source row per output row).  The same operations on the same operands in the same order as the recipe:
// the same bits.  Adjacent lanes own adjacent column runs: their byte taps fall into one or two cache lines of the
// interleaved source row, and each of the three planes gets one 16-byte store per lane, 1 KiB per wave and row.
//
// WIDE: Wo is a multiple of V and y is 16-byte aligned, so every run is whole and every row segment aligned -- one
// 16-byte store per plane.  Otherwise element stores, the columns past Wo skipped (their geometry is computed on the
// clamped column, so every tap stays inside the image).
//
// The table's rows {byte offset, H0, W0, 0} are trusted, as ROI rows are.
// ------------------------------------------------------------------------------------
constexpr int kPpThreads = 256;

template <class T>
struct PpCols { static constexpr int value = 16 / (int)sizeof(T); };

struct PpAxis { int i0, i1; double l; };

__host__ __device__ __forceinline__ PpAxis pp_axis(int i, int n0, int n, double scale)
{
    if (n0 == n) return PpAxis{i, i, 0.0};
    double s = ((double)i + 0.5) * scale - 0.5;
    s = s > 0.0 ? s : 0.0;
    int i0 = (int)floor(s);
    i0 = i0 < n0 - 1 ? i0 : n0 - 1;
    const int i1 = i0 + 1 < n0 - 1 ? i0 + 1 : n0 - 1;
    return PpAxis{i0, i1, s - (double)i0};
}

// one item: V columns x band rows x 3 channels of one image (host and device: the host form is what a CPU build checks)
template <class T, bool WIDE>
__host__ __device__ __forceinline__ void pp_item(unsigned item, const unsigned char* __restrict__ src,
                                                 const int* __restrict__ table, T* __restrict__ y, int Ho, int Wo, int band,
                                                 unsigned nstrips, unsigned nbands)
{
    constexpr int V = PpCols<T>::value;
    typedef T vec_t __attribute__((ext_vector_type(V)));
    const unsigned strip = item % nstrips, rest = item / nstrips;
    const unsigned b = rest % nbands, n = rest / nbands;
    const int* row4 = table + (size_t)n * 4;
    const int H0 = row4[1], W0 = row4[2];
    const unsigned char* im = src + (size_t)(unsigned)row4[0];
    const int ox0 = (int)strip * V;
    const int oy0 = (int)b * band, oy1 = oy0 + band < Ho ? oy0 + band : Ho;
    const double sx = (double)W0 / (double)Wo, sy = (double)H0 / (double)Ho;
    const size_t pitch = (size_t)W0 * 3;

    int x0[V], x1[V];            // byte offsets of the two taps' first channel within a source row
    double lx[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        int col = ox0 + j;
        if (!WIDE) col = col < Wo - 1 ? col : Wo - 1;
        const PpAxis ax = pp_axis(col, W0, Wo, sx);
        x0[j] = 3 * ax.i0;
        x1[j] = 3 * ax.i1;
        lx[j] = ax.l;
    }

    double Ha[3][V], Hb[3][V];   // the horizontal blends of source rows sa and sb (-1: none yet)
    int sa = -1, sb = -1;
    const auto hblend = [&](int r, double (&H)[3][V]) {
        const unsigned char* p = im + (size_t)r * pitch;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const double l1 = lx[j], l0 = 1.0 - l1;
#pragma unroll
            for (int c = 0; c < 3; ++c) H[c][j] = l0 * (double)p[x0[j] + c] + l1 * (double)p[x1[j] + c];
        }
    };
    const auto copy = [&](double (&D)[3][V], const double (&S)[3][V]) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < V; ++j) D[c][j] = S[c][j];
    };

    T* yn = y + (size_t)n * 3 * Ho * Wo;
    for (int oy = oy0; oy < oy1; ++oy) {
        const PpAxis ay = pp_axis(oy, H0, Ho, sy);
        if (ay.i0 != sa) {
            if (ay.i0 == sb) copy(Ha, Hb);
            else hblend(ay.i0, Ha);
            sa = ay.i0;
        }
        if (ay.i1 != sb) {
            if (ay.i1 == sa) copy(Hb, Ha);
            else hblend(ay.i1, Hb);
            sb = ay.i1;
        }
        const double l1 = ay.l, l0 = 1.0 - l1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            T out[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const double v = l0 * Ha[c][j] + l1 * Hb[c][j];
                out[j] = (T)(float)(v / 128.0 - 1.0);
            }
            T* p = yn + ((size_t)c * Ho + oy) * Wo + ox0;
            if (WIDE) {
                vec_t w;
#pragma unroll
                for (int j = 0; j < V; ++j) w[j] = out[j];
                *reinterpret_cast<vec_t*>(p) = w;
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j)
                    if (ox0 + j < Wo) p[j] = out[j];
            }
        }
    }
}

template <class T, bool WIDE>
__global__ __launch_bounds__(kPpThreads) void rroi_preprocess_kernel(
    const unsigned char* __restrict__ src, const int* __restrict__ table, T* __restrict__ y, int Ho, int Wo, int band,
    unsigned nstrips, unsigned nbands, unsigned items)
{
    const unsigned item = blockIdx.x * kPpThreads + threadIdx.x;
    if (item >= items) return;
    pp_item<T, WIDE>(item, src, table, y, Ho, Wo, band, nstrips, nbands);
}
