// rroi_depthwise_kernels.h -- depthwise 3x3 convolution (padding 1, stride 1 or 2), DESIGN 5.10
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_device_common.h); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// The depthwise convolutions of the network (tools/models.py:70-102 of the reference: conv_dw_plain, conv_dw_in,
// conv_dw_res -- `nn.Conv2d(c, c, 3, stride, 1, groups=c, bias=False)`), which stock torch hands to a generic kernel
// that accumulates in double.  The arithmetic here is that class, with the ORDER fixed so that a test compares bits:
//     acc = +0.0 (double);  for ky, for kx:  acc = acc + (double)w[c, ky, kx] * (double)x[n, c, iy, ix]  (0.0 outside)
//     y = (T)(float)acc
// The product of two widened 24-bit significands is exact in double, so the fma below and a separate multiply and add give
// the same bits.  A tap outside the image is w * (+0.0) and is never skipped (NaN for a non-finite weight).
//
// A streaming kernel along rows.  A thread owns kDwCols output columns over `band` output rows of one (n, c) plane; the
// flat item index (plane, band, strip) covers large planes with few channels and many tiny planes alike.  Every input
// row is loaded ONCE per thread -- one or two vector loads for the aligned middle, one element each for the column to
// the left and (stride 1) to the right -- widened once per element, and used for up to three output rows whose double
// accumulators live in registers: a row is tap row 0 of the output row below, 1 of its own and 2 of the one above, which
// is also the order (ky ascending) the recipe prescribes.  The next row's loads are issued before the current row's
// arithmetic.  ix = -1 and ix = W are the neighbouring row's elements in memory, so column borders are decided per
// element, not by a descriptor's range.
// Any element-aligned base works: a row's middle is one vector access where its address allows and the strip is whole,
// element accesses otherwise (decided per row: an odd W changes the alignment from row to row).
// ------------------------------------------------------------------------------------
constexpr int kDwCols = 4;        // output columns per thread: one 16-byte (fp32) / 8-byte (16-bit) store
constexpr int kDwThreads = 256;
constexpr int kDwMaxBand = 8;     // output rows per thread: 8, 4 or 2, chosen on the host (depthwise_band)

template <class T, int STRIDE>
struct DwRow {                    // one input row of a strip as loaded (not yet widened: nothing here waits for the loads)
    typename Vec4<T>::type m[STRIDE];   // columns ix0 .. ix0 + 4 * STRIDE - 1
    T l, r;                             // columns ix0 - 1 and (stride 1) ix0 + 4
};

template <class T>
__device__ __forceinline__ bool dw_aligned4(const T* p) { return (reinterpret_cast<size_t>(p) & (4 * sizeof(T) - 1)) == 0; }

template <class T, int STRIDE>
__device__ __forceinline__ DwRow<T, STRIDE> dw_load_row(const T* __restrict__ plane, int iy, int ix0, int H, int W)
{
    typedef typename Vec4<T>::type vt;
    constexpr int NM = kDwCols * STRIDE;
    DwRow<T, STRIDE> R;
    const T zero = (T)0.0f;
#pragma unroll
    for (int q = 0; q < STRIDE; ++q) R.m[q] = vt{zero, zero, zero, zero};
    R.l = R.r = zero;
    if (iy < 0 || iy >= H) return R;   // a row of the padding: +0.0 taps, still multiplied
    const T* row = plane + (size_t)iy * W;
    if (ix0 > 0) R.l = row[ix0 - 1];
    if (ix0 + NM <= W && dw_aligned4(row + ix0)) {
#pragma unroll
        for (int q = 0; q < STRIDE; ++q) R.m[q] = *reinterpret_cast<const vt*>(row + ix0 + 4 * q);
    } else {
#pragma unroll
        for (int k = 0; k < NM; ++k)
            if (ix0 + k < W) R.m[k / 4][k % 4] = row[ix0 + k];
    }
    if (STRIDE == 1 && ix0 + NM < W) R.r = row[ix0 + NM];
    return R;
}

// widened once per loaded element: slot j is column ix0 - 1 + j
template <class T, int STRIDE>
__device__ __forceinline__ void dw_widen_row(const DwRow<T, STRIDE>& R, double* v)
{
    v[0] = (double)to_f32(R.l);
#pragma unroll
    for (int k = 0; k < kDwCols * STRIDE; ++k) v[1 + k] = (double)to_f32<T>(R.m[k / 4][k % 4]);
    if (STRIDE == 1) v[1 + kDwCols] = (double)to_f32(R.r);
}

// tap row ky of kDwCols outputs: acc = acc + w[ky][kx] * v, kx ascending
template <int STRIDE>
__device__ __forceinline__ void dw_tap_row(double* acc, const double* v, const double* wd, int ky)
{
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int j = 0; j < kDwCols; ++j) acc[j] = __builtin_fma(wd[3 * ky + kx], v[j * STRIDE + kx], acc[j]);
}

template <class T>
__device__ __forceinline__ void dw_store_row(T* __restrict__ out_plane, int oy, int ox0, int Wo, const double* acc)
{
    typedef typename Vec4<T>::type vt;
    T* p = out_plane + (size_t)oy * Wo + ox0;
    T o[kDwCols];
#pragma unroll
    for (int j = 0; j < kDwCols; ++j) o[j] = from_f32<T>((float)acc[j]);   // fp32 result, then one plain conversion
    if (ox0 + kDwCols <= Wo && dw_aligned4(p)) {
        *reinterpret_cast<vt*>(p) = vt{o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
        for (int j = 0; j < kDwCols; ++j)
            if (ox0 + j < Wo) p[j] = o[j];
    }
}

__device__ __forceinline__ void dw_clear(double* acc)
{
#pragma unroll
    for (int j = 0; j < kDwCols; ++j) acc[j] = 0.0;
}

template <class T, int STRIDE>
__global__ __launch_bounds__(kDwThreads) void rroi_depthwise3x3_kernel(
    const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y, int C, int H, int W, int Ho, int Wo, int band,
    unsigned nstrips, unsigned nbands, unsigned items)
{
    constexpr int NIN = kDwCols * STRIDE + (STRIDE == 1 ? 2 : 1);   // 6 / 9 input columns feed 4 output columns
    const unsigned item = blockIdx.x * kDwThreads + threadIdx.x;
    if (item >= items) return;
    const unsigned strip = item % nstrips, rest = item / nstrips;
    const unsigned b = rest % nbands, plane = rest / nbands;
    const int c = (int)(plane % (unsigned)C);
    double wd[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wd[k] = (double)to_f32(w[(size_t)c * 9 + k]);
    const int ox0 = (int)strip * kDwCols, ix0 = ox0 * STRIDE;
    const int oy0 = (int)b * band, oy1 = min(oy0 + band, Ho);
    const T* xp = x + (size_t)plane * H * W;
    T* yp = y + (size_t)plane * Ho * Wo;
    double v[NIN];
    double A[kDwCols], B[kDwCols], Cc[kDwCols];
    dw_clear(A);
    dw_clear(B);
    dw_clear(Cc);

    if constexpr (STRIDE == 1) {
        // input row r is tap row 0 of output row r + 1 (S: starts it), 1 of r (M) and 2 of r - 1 (F: finishes and stores it)
        DwRow<T, 1> cur = dw_load_row<T, 1>(xp, oy0 - 1, ix0, H, W);
        int r = oy0 - 1;
        auto step = [&](double* S, double* M, double* F) {
            const DwRow<T, 1> nxt = dw_load_row<T, 1>(xp, r < oy1 ? r + 1 : -1, ix0, H, W);
            dw_widen_row<T, 1>(cur, v);
            if (r + 1 < oy1) {
                dw_clear(S);
                dw_tap_row<1>(S, v, wd, 0);
            }
            if (r >= oy0 && r < oy1) dw_tap_row<1>(M, v, wd, 1);
            if (r > oy0) {
                dw_tap_row<1>(F, v, wd, 2);
                dw_store_row<T>(yp, r - 1, ox0, Wo, F);
            }
            cur = nxt;
            return ++r > oy1;
        };
        for (;;) {
            if (step(A, B, Cc)) break;
            if (step(Cc, A, B)) break;
            if (step(B, Cc, A)) break;
        }
    } else {
        // output row oy takes input rows 2 oy - 1, 2 oy, 2 oy + 1; the last is also tap row 0 of output row oy + 1
        DwRow<T, 2> r0 = dw_load_row<T, 2>(xp, 2 * oy0 - 1, ix0, H, W);
        DwRow<T, 2> r1 = dw_load_row<T, 2>(xp, 2 * oy0, ix0, H, W);
        dw_widen_row<T, 2>(r0, v);
        dw_tap_row<2>(A, v, wd, 0);
        int oy = oy0;
        auto step = [&](double* cur, double* nxt) {
            const DwRow<T, 2> r2 = dw_load_row<T, 2>(xp, 2 * oy + 1, ix0, H, W);
            dw_widen_row<T, 2>(r1, v);
            dw_tap_row<2>(cur, v, wd, 1);
            const bool more = oy + 1 < oy1;
            r1 = dw_load_row<T, 2>(xp, more ? 2 * oy + 2 : -1, ix0, H, W);
            dw_widen_row<T, 2>(r2, v);
            dw_tap_row<2>(cur, v, wd, 2);
            dw_store_row<T>(yp, oy, ox0, Wo, cur);
            if (more) {
                dw_clear(nxt);
                dw_tap_row<2>(nxt, v, wd, 0);
            }
            ++oy;
            return !more;
        };
        for (;;) {
            if (step(A, B)) break;
            if (step(B, A)) break;
        }
    }
}
