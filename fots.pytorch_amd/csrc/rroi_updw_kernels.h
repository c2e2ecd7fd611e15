// rroi_updw_kernels.h -- bilinear resize + depthwise 3x3 convolution in one launch, DESIGN 5.20
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_depthwise_kernels.h and rroi_merge_kernels.h, whose dw_* helpers, mg_axis and MgSource it uses); not a standalone
// header.
#pragma once

// ------------------------------------------------------------------------------------
// y = depthwise3x3(U, w), stride 1, padding 1, where U[n, c] is the align_corners = true bilinear resize of a[n, c] to
// (Ho, Wo), rounded to the tensor's type: U = (T)(float)value with `value` as rroi_merge_kernels.h defines it (mg_axis and
// the order of mg_blend, every operation rounded to double; a source of the target's size is read as it is), and the nine
// taps summed by the recipe of rroi_depthwise_kernels.h on those rounded values.  So y is, bit for bit, what the depthwise
// kernel gives on the stored resized map -- and that map is never stored.
//
// The streaming structure of rroi_depthwise3x3_kernel: a thread owns kDwCols output columns over `band` output rows of
// one plane, every row of U is produced ONCE per thread (six columns: the four and one on either side) and used for up to
// three output rows whose double accumulators live in registers.  The row loader is what differs.  The blend
//     value = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)
// splits into a horizontal blend per SOURCE row and a vertical blend of two of them, and the horizontal blend of a source
// row does not depend on the output row: a thread keeps the six horizontal blends of source rows i0 and i1 in registers
// and, going down the band, recomputes one only when the source row changes -- when enlarging by two, one new source row
// (12 element loads through the cache; the source is four times smaller than the output) per two output rows.  The same
// operations on the same operands in the same order as mg_blend: the same bits.  A column or row outside U is +0.0 and is
// still multiplied (never skipped), as in the depthwise kernel.
// ------------------------------------------------------------------------------------
constexpr int kUdIn = kDwCols + 2;       // the columns of U a thread needs: ox0 - 1 .. ox0 + 4

template <class T>
__device__ __forceinline__ double ud_round(double v) { return (double)to_f32(from_f32<T>((float)v)); }   // (T)(float)v, widened

// UP: a is (N, C, A.h, A.w) and is resized to (Ho, Wo); else it is (N, C, Ho, Wo) and is read as it is.
template <class T, bool UP>
__global__ __launch_bounds__(kDwThreads) void rroi_updw_kernel(
    const T* __restrict__ a, const T* __restrict__ w, T* __restrict__ y, int C, int Ho, int Wo, int band, unsigned nstrips,
    unsigned nbands, unsigned items, MgSource A)
{
    const unsigned item = blockIdx.x * kDwThreads + threadIdx.x;
    if (item >= items) return;
    const unsigned strip = item % nstrips, rest = item / nstrips;
    const unsigned b = rest % nbands, plane = rest / nbands;
    const int c = (int)(plane % (unsigned)C);
    double wd[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wd[k] = (double)to_f32(w[(size_t)c * 9 + k]);
    const int ox0 = (int)strip * kDwCols;
    const int oy0 = (int)b * band, oy1 = min(oy0 + band, Ho);
    const T* ap = a + (size_t)plane * A.h * A.w;
    T* yp = y + (size_t)plane * Ho * Wo;

    bool live[kUdIn];         // whether column ox0 - 1 + j exists in U
    int xi0[kUdIn], xi1[kUdIn];
    double lx1[kUdIn];
#pragma unroll
    for (int j = 0; j < kUdIn; ++j) {
        const int col = ox0 - 1 + j;
        live[j] = col >= 0 && col < Wo;
        xi0[j] = live[j] ? col : 0;
        xi1[j] = xi0[j];
        lx1[j] = 0.0;
        if constexpr (UP) {
            const MgAxis ax = mg_axis(A.sx, (unsigned)xi0[j], A.w);
            xi0[j] = ax.i0;
            xi1[j] = ax.i0 + ax.step;
            lx1[j] = ax.l1;
        }
    }

    double H0[kUdIn], H1[kUdIn];      // UP: the horizontal blends of source rows s0 and s1 (-1: none yet)
    int s0 = -1, s1 = -1;
    const auto hblend = [&](int sy, double* Hh) {
        const T* row = ap + (size_t)sy * A.w;
#pragma unroll
        for (int j = 0; j < kUdIn; ++j) {
            Hh[j] = 0.0;
            if (live[j]) {
                const double v0 = (double)to_f32(row[xi0[j]]), v1 = (double)to_f32(row[xi1[j]]);
                const double lx0 = 1.0 - lx1[j];
                Hh[j] = lx0 * v0 + lx1[j] * v1;
            }
        }
    };
    // row r of U, widened: slot j is column ox0 - 1 + j; a row or column of the padding is +0.0
    const auto load_row = [&](int r, double* v) {
#pragma unroll
        for (int j = 0; j < kUdIn; ++j) v[j] = 0.0;
        if (r < 0 || r >= Ho) return;
        if constexpr (UP) {
            const MgAxis ay = mg_axis(A.sy, (unsigned)r, A.h);
            const int i0 = ay.i0, i1 = ay.i0 + ay.step;
            if (i0 != s0) {
                if (i0 == s1) {
#pragma unroll
                    for (int j = 0; j < kUdIn; ++j) H0[j] = H1[j];
                } else {
                    hblend(i0, H0);
                }
                s0 = i0;
            }
            if (i1 != s1) {
                if (i1 == s0) {
#pragma unroll
                    for (int j = 0; j < kUdIn; ++j) H1[j] = H0[j];
                } else {
                    hblend(i1, H1);
                }
                s1 = i1;
            }
            const double ly1 = ay.l1, ly0 = 1.0 - ly1;
#pragma unroll
            for (int j = 0; j < kUdIn; ++j)
                if (live[j]) v[j] = ud_round<T>(ly0 * H0[j] + ly1 * H1[j]);
        } else {
            const T* row = ap + (size_t)r * Wo;
#pragma unroll
            for (int j = 0; j < kUdIn; ++j)
                if (live[j]) v[j] = (double)to_f32(row[xi0[j]]);
        }
    };

    double v[kUdIn];
    double Aa[kDwCols], Bb[kDwCols], Cc[kDwCols];
    dw_clear(Aa);
    dw_clear(Bb);
    dw_clear(Cc);
    // row r of U is tap row 0 of output row r + 1 (S: starts it), 1 of r (M) and 2 of r - 1 (F: finishes and stores it)
    int r = oy0 - 1;
    auto step = [&](double* S, double* M, double* F) {
        load_row(r, v);
        if (r + 1 < oy1) {
            dw_clear(S);
            dw_tap_row<1>(S, v, wd, 0);
        }
        if (r >= oy0 && r < oy1) dw_tap_row<1>(M, v, wd, 1);
        if (r > oy0) {
            dw_tap_row<1>(F, v, wd, 2);
            dw_store_row<T>(yp, r - 1, ox0, Wo, F);
        }
        return ++r > oy1;
    };
    for (;;) {
        if (step(Aa, Bb, Cc)) break;
        if (step(Cc, Aa, Bb)) break;
        if (step(Bb, Cc, Aa)) break;
    }
}
