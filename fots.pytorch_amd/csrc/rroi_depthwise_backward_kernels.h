// rroi_depthwise_backward_kernels.h -- the backward of the depthwise 3x3 convolution (padding 1, stride 1 or 2), DESIGN 5.25
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_depthwise_kernels.h, whose row helpers it uses as they are, and rroi_ctc_loss_kernels.h, whose ctc_narrow rounds a
// double once to T); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// Input gradient (header section 5b), the ORDER fixed so that a test compares bits -- dy is visited in row-major order:
//     acc = +0.0 (double);  for ky = 2, 1, 0: for kx = 2, 1, 0, where iy + 1 - ky and ix + 1 - kx are multiples of s:
//         acc = acc + (double)w[c, ky, kx] * (double)dy[n, c, (iy + 1 - ky) / s, (ix + 1 - kx) / s]   (0.0 outside)
//     dx = (T)(float)acc
// A tap of the right parity outside dy is w * (+0.0) and is never skipped (NaN for a non-finite weight).
//   rroi_depthwise3x3_dx_s1_kernel   stride 1: the forward's recipe on dy with the weight turned by 180 degrees, so the
//       forward's streaming scheme as it stands -- a dy row is loaded once, widened once and used for three dx rows.
//   rroi_depthwise3x3_dx_s2_kernel   stride 2: a thread owns EIGHT dx columns over 2 * band dx rows, which are four dy
//       columns -- one aligned vector -- and the element to their right.  Row and column parity are decided in registers:
//           dx[2m,     2j]     = w11 dy[m, j]
//           dx[2m,     2j + 1] = w12 dy[m, j] + w10 dy[m, j + 1]
//           dx[2m + 1, 2j]     = w21 dy[m, j] + w01 dy[m + 1, j]
//           dx[2m + 1, 2j + 1] = w22 dy[m, j] + w20 dy[m, j + 1] + w02 dy[m + 1, j] + w00 dy[m + 1, j + 1]
//       each from +0.0 in that order.  With H or W even the last dx row / column sees dy row Ho / column Wo: +0.0 taps.
//
// Weight gradient, deterministic: dweight[c, ky, kx] = sum over n, oy, ox of dy[n, c, oy, ox] * x[n, c, s oy - 1 + ky,
// s ox - 1 + kx] (0.0 outside), every product exact in double, every sum in double in an order that depends on the
// argument list alone, one rounding (ctc_narrow).  No atomics.
//   rroi_depthwise3x3_dw_partial_kernel   a workgroup per slot (plane, segment): thread t owns item segment * 256 + t of
//       the plane, kDwCols dy columns over `band` dy rows, and keeps the nine sums of its tile.  An x row is loaded once
//       and shared between the three ky, as in the forward.  The workgroup's nine sums are a fixed tree -- an xor
//       butterfly over the 64 lanes of a wave, then the four waves' results from LDS in wave order -- and go to the slot's
//       nine doubles of the workspace.  A workgroup never mixes planes.
//   rroi_depthwise3x3_dw_finish_kernel    workgroup c: thread t adds the slots t, t + 256, ... of channel c's
//       N * segments slots in (n, segment) order -- in blocks of kDwbFinishBlock, so that no chain of additions grows with
//       the shape without bound -- then the same tree, and thread k < 9 stores dweight[c, k].
// Longest chain of additions on the way to one dweight value, at any legal shape: 4 * kDwMaxBand in a thread + 6 + 3 in
// the partials' tree + kDwbFinishBlock + 2^31 / (256 * kDwbFinishBlock) in a finishing thread + 6 + 3 = 6194 <= 8192.
// ------------------------------------------------------------------------------------
constexpr int kDwbFinishBlock = 2048;
constexpr unsigned kDwbMaxGrid = 1u << 22;   // workgroups of the partials launch (kDwThreads times it stays below 2^32)

// the flat item of a dx thread: (plane, band, strip), as in rroi_depthwise3x3_kernel
struct DwbItem {
    unsigned strip, b, plane;
};
__device__ __forceinline__ DwbItem dwb_item(unsigned item, unsigned nstrips, unsigned nbands)
{
    const unsigned rest = item / nstrips;
    return {item % nstrips, rest % nbands, rest / nbands};
}

// the weight of channel c turned by 180 degrees: slot 3 a + b multiplies dy[iy - 1 + a, ix - 1 + b]
template <class T>
__device__ __forceinline__ void dwb_turned_weight(const T* __restrict__ w, int c, double* wd)
{
#pragma unroll
    for (int k = 0; k < 9; ++k) wd[k] = (double)to_f32(w[(size_t)c * 9 + 8 - k]);
}

template <class T>
__global__ __launch_bounds__(kDwThreads) void rroi_depthwise3x3_dx_s1_kernel(
    const T* __restrict__ dy, const T* __restrict__ w, T* __restrict__ dx, int C, int H, int W, int band, unsigned nstrips,
    unsigned nbands, unsigned items)
{
    const unsigned item = blockIdx.x * kDwThreads + threadIdx.x;
    if (item >= items) return;
    const DwbItem it = dwb_item(item, nstrips, nbands);
    double wd[9];
    dwb_turned_weight<T>(w, (int)(it.plane % (unsigned)C), wd);
    const int ix0 = (int)it.strip * kDwCols;
    const int iy0 = (int)it.b * band, iy1 = min(iy0 + band, H);
    const T* gp = dy + (size_t)it.plane * H * W;
    T* op = dx + (size_t)it.plane * H * W;
    double v[kDwCols + 2];
    double A[kDwCols], B[kDwCols], Cc[kDwCols];
    dw_clear(A);
    dw_clear(B);
    dw_clear(Cc);
    // dy row r is tap row 0 of dx row r + 1 (S: starts it), 1 of r (M) and 2 of r - 1 (F: finishes and stores it)
    DwRow<T, 1> cur = dw_load_row<T, 1>(gp, iy0 - 1, ix0, H, W);
    int r = iy0 - 1;
    auto step = [&](double* S, double* M, double* F) {
        const DwRow<T, 1> nxt = dw_load_row<T, 1>(gp, r < iy1 ? r + 1 : -1, ix0, H, W);
        dw_widen_row<T, 1>(cur, v);
        if (r + 1 < iy1) {
            dw_clear(S);
            dw_tap_row<1>(S, v, wd, 0);
        }
        if (r >= iy0 && r < iy1) dw_tap_row<1>(M, v, wd, 1);
        if (r > iy0) {
            dw_tap_row<1>(F, v, wd, 2);
            dw_store_row<T>(op, r - 1, ix0, W, F);
        }
        cur = nxt;
        return ++r > iy1;
    };
    for (;;) {
        if (step(A, B, Cc)) break;
        if (step(Cc, A, B)) break;
        if (step(B, Cc, A)) break;
    }
}

// columns ox0 .. ox0 + 4 of a dy row, widened: the aligned vector and the element to its right
template <class T>
__device__ __forceinline__ void dwb_widen5(const DwRow<T, 1>& R, double* v)
{
#pragma unroll
    for (int k = 0; k < kDwCols; ++k) v[k] = (double)to_f32<T>(R.m[0][k]);
    v[kDwCols] = (double)to_f32(R.r);
}

template <class T>
__global__ __launch_bounds__(kDwThreads) void rroi_depthwise3x3_dx_s2_kernel(
    const T* __restrict__ dy, const T* __restrict__ w, T* __restrict__ dx, int C, int H, int W, int Ho, int Wo, int band,
    unsigned nstrips, unsigned nbands, unsigned items)
{
    const unsigned item = blockIdx.x * kDwThreads + threadIdx.x;
    if (item >= items) return;
    const DwbItem it = dwb_item(item, nstrips, nbands);
    const int c = (int)(it.plane % (unsigned)C);
    double wd[9];   // as stored: wd[3 ky + kx]
#pragma unroll
    for (int k = 0; k < 9; ++k) wd[k] = (double)to_f32(w[(size_t)c * 9 + k]);
    const int ox0 = (int)it.strip * kDwCols, ix0 = 2 * ox0;
    const int m0 = (int)it.b * band, m1 = min(m0 + band, Ho);
    const T* gp = dy + (size_t)it.plane * Ho * Wo;
    T* op = dx + (size_t)it.plane * H * W;
    double v[kDwCols + 1], u[kDwCols + 1], o[2 * kDwCols];
    // (a row at or below Ho comes back as +0.0 taps; the column to the left, which dw_load_row also fetches, is not used)
    DwRow<T, 1> nxt = dw_load_row<T, 1>(gp, m0, ox0, Ho, Wo);
    dwb_widen5<T>(nxt, v);
    nxt = dw_load_row<T, 1>(gp, m0 + 1, ox0, Ho, Wo);
    for (int m = m0; m < m1; ++m) {
        const DwRow<T, 1> ahead = dw_load_row<T, 1>(gp, m + 1 < m1 ? m + 2 : -1, ox0, Ho, Wo);
        dwb_widen5<T>(nxt, u);
#pragma unroll
        for (int j = 0; j < kDwCols; ++j) {
            o[2 * j] = __builtin_fma(wd[4], v[j], 0.0);
            o[2 * j + 1] = __builtin_fma(wd[3], v[j + 1], __builtin_fma(wd[5], v[j], 0.0));
        }
        dw_store_row<T>(op, 2 * m, ix0, W, o);
        dw_store_row<T>(op, 2 * m, ix0 + kDwCols, W, o + kDwCols);
        if (2 * m + 1 < H) {
#pragma unroll
            for (int j = 0; j < kDwCols; ++j) {
                o[2 * j] = __builtin_fma(wd[1], u[j], __builtin_fma(wd[7], v[j], 0.0));
                double a = __builtin_fma(wd[8], v[j], 0.0);
                a = __builtin_fma(wd[6], v[j + 1], a);
                a = __builtin_fma(wd[2], u[j], a);
                o[2 * j + 1] = __builtin_fma(wd[0], u[j + 1], a);
            }
            dw_store_row<T>(op, 2 * m + 1, ix0, W, o);
            dw_store_row<T>(op, 2 * m + 1, ix0 + kDwCols, W, o + kDwCols);
        }
#pragma unroll
        for (int k = 0; k <= kDwCols; ++k) v[k] = u[k];
        nxt = ahead;
    }
}

// ------------------------------------------------------------------------------------
// Weight gradient.
// ------------------------------------------------------------------------------------
// tap row ky of the nine sums: acc[3 ky + kx] += d[j] * v[j * STRIDE + kx], j ascending; under PARTIAL only the strip's
// `nv` columns that exist (a dy column past Wo is no term of the sum, whatever x holds beside it)
template <int STRIDE, bool PARTIAL>
__device__ __forceinline__ void dwb_tap_row(double* acc, const double* d, const double* v, int ky, int nv)
{
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int j = 0; j < kDwCols; ++j)
            if (!PARTIAL || j < nv) acc[3 * ky + kx] = __builtin_fma(d[j], v[j * STRIDE + kx], acc[3 * ky + kx]);
}

template <class T>
__device__ __forceinline__ void dwb_widen_dy(const typename Vec4<T>::type& g, double* d)
{
#pragma unroll
    for (int j = 0; j < kDwCols; ++j) d[j] = (double)to_f32<T>(g[j]);
}

// columns ox0 .. ox0 + 3 of dy row oy as loaded: the middle of the forward's row (its neighbours to the left and right are
// not used here, so their loads go); +0.0 for a row outside [0, Ho) (never multiplied: the callers skip such a row) and
// for a column past Wo
template <class T>
__device__ __forceinline__ typename Vec4<T>::type dwb_load_dy(const T* __restrict__ plane, int oy, int ox0, int Ho, int Wo)
{
    return dw_load_row<T, 1>(plane, oy, ox0, Ho, Wo).m[0];
}

// the nine sums of one thread's tile: dy rows [oy0, oy1), columns ox0 .. ox0 + 3
template <class T, int STRIDE, bool PARTIAL>
__device__ __forceinline__ void dwb_tile(const T* __restrict__ gp, const T* __restrict__ xp, int oy0, int oy1, int ox0, int H,
                                         int W, int Ho, int Wo, double* acc)
{
    typedef typename Vec4<T>::type vt;
    constexpr int NIN = kDwCols * STRIDE + (STRIDE == 1 ? 2 : 1);
    const int ix0 = ox0 * STRIDE, nv = min(kDwCols, Wo - ox0);
    double v[NIN];
    if constexpr (STRIDE == 1) {
        // x row r meets dy row r + 1 at ky = 0, r at ky = 1 and r - 1 at ky = 2: three widened dy rows are live
        double dA[kDwCols], dB[kDwCols], dC[kDwCols];   // dy rows r - 1, r, r + 1 at the top of a step
        dw_clear(dA);
        dw_clear(dB);
        dwb_widen_dy<T>(dwb_load_dy<T>(gp, oy0, ox0, Ho, Wo), dC);
        DwRow<T, 1> cur = dw_load_row<T, 1>(xp, oy0 - 1, ix0, H, W);
        vt gn = dwb_load_dy<T>(gp, oy0 + 1 < oy1 ? oy0 + 1 : -1, ox0, Ho, Wo);
        for (int r = oy0 - 1; r <= oy1; ++r) {
            const DwRow<T, 1> nxt = dw_load_row<T, 1>(xp, r < oy1 ? r + 1 : -1, ix0, H, W);
            const vt ga = dwb_load_dy<T>(gp, r + 3 < oy1 ? r + 3 : -1, ox0, Ho, Wo);
            dw_widen_row<T, 1>(cur, v);
            if (r + 1 < oy1) dwb_tap_row<1, PARTIAL>(acc, dC, v, 0, nv);
            if (r >= oy0 && r < oy1) dwb_tap_row<1, PARTIAL>(acc, dB, v, 1, nv);
            if (r > oy0) dwb_tap_row<1, PARTIAL>(acc, dA, v, 2, nv);
#pragma unroll
            for (int j = 0; j < kDwCols; ++j) {
                dA[j] = dB[j];
                dB[j] = dC[j];
            }
            dwb_widen_dy<T>(gn, dC);
            gn = ga;
            cur = nxt;
        }
    } else {
        // dy row oy meets x rows 2 oy - 1, 2 oy, 2 oy + 1; the last is also the ky = 0 row of dy row oy + 1
        double dB[kDwCols], dC[kDwCols];                // dy rows oy and oy + 1
        dwb_widen_dy<T>(dwb_load_dy<T>(gp, oy0, ox0, Ho, Wo), dB);
        DwRow<T, 2> r0 = dw_load_row<T, 2>(xp, 2 * oy0 - 1, ix0, H, W);
        DwRow<T, 2> r1 = dw_load_row<T, 2>(xp, 2 * oy0, ix0, H, W);
        dw_widen_row<T, 2>(r0, v);
        dwb_tap_row<2, PARTIAL>(acc, dB, v, 0, nv);
        for (int oy = oy0; oy < oy1; ++oy) {
            const bool more = oy + 1 < oy1;
            const DwRow<T, 2> r2 = dw_load_row<T, 2>(xp, 2 * oy + 1, ix0, H, W);
            const vt gn = dwb_load_dy<T>(gp, more ? oy + 1 : -1, ox0, Ho, Wo);
            dw_widen_row<T, 2>(r1, v);
            dwb_tap_row<2, PARTIAL>(acc, dB, v, 1, nv);
            r1 = dw_load_row<T, 2>(xp, more ? 2 * oy + 2 : -1, ix0, H, W);
            dw_widen_row<T, 2>(r2, v);
            dwb_tap_row<2, PARTIAL>(acc, dB, v, 2, nv);
            dwb_widen_dy<T>(gn, dC);
            if (more) dwb_tap_row<2, PARTIAL>(acc, dC, v, 0, nv);
#pragma unroll
            for (int j = 0; j < kDwCols; ++j) dB[j] = dC[j];
        }
    }
}

// the fixed tree over a workgroup's nine sums: a butterfly over the wave's 64 lanes (every lane ends with the same bits),
// then the waves in order; thread k < 9 returns sum k, the others nothing of use.  All kDwThreads threads must call it.
__device__ __forceinline__ double dwb_block_sum(double* s, double (*lds)[9])
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] += __shfl_xor(s[k], off, 64);
    if ((threadIdx.x & 63u) == 0)
#pragma unroll
        for (int k = 0; k < 9; ++k) lds[threadIdx.x >> 6][k] = s[k];
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x < 9) {
        r = lds[0][threadIdx.x];
#pragma unroll
        for (int wv = 1; wv < kDwThreads / 64; ++wv) r += lds[wv][threadIdx.x];
    }
    return r;
}

// slot = plane * nseg + segment, `slots` of them; grid: min(slots, kDwbMaxGrid) workgroups, a workgroup takes the slots
// blockIdx.x, + gridDim.x, ... (more than one only beyond kDwbMaxGrid slots: millions of planes)
template <class T, int STRIDE>
__global__ __launch_bounds__(kDwThreads) void rroi_depthwise3x3_dw_partial_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, double* __restrict__ partials, int H, int W, int Ho, int Wo, int band,
    unsigned nstrips, unsigned items_per_plane, unsigned nseg, unsigned slots)
{
    __shared__ double lds[kDwThreads / 64][9];
    for (unsigned slot = blockIdx.x; slot < slots; slot += gridDim.x) {
        const unsigned plane = slot / nseg, item = (slot % nseg) * kDwThreads + threadIdx.x;
        double acc[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[k] = 0.0;
        if (item < items_per_plane) {
            const int ox0 = (int)(item % nstrips) * kDwCols;
            const int oy0 = (int)(item / nstrips) * band, oy1 = min(oy0 + band, Ho);
            const T* gp = dy + (size_t)plane * Ho * Wo;
            const T* xp = x + (size_t)plane * H * W;
            if (ox0 + kDwCols <= Wo)
                dwb_tile<T, STRIDE, false>(gp, xp, oy0, oy1, ox0, H, W, Ho, Wo, acc);
            else
                dwb_tile<T, STRIDE, true>(gp, xp, oy0, oy1, ox0, H, W, Ho, Wo, acc);
        }
        const double r = dwb_block_sum(acc, lds);
        if (threadIdx.x < 9) partials[(size_t)slot * 9 + threadIdx.x] = r;
        if (slot + gridDim.x < slots) __syncthreads();   // the next slot's sums reuse lds (the condition is the workgroup's)
    }
}

// grid: C workgroups; channel c's slots are (n * C + c) * nseg + s, added in (n, s) order
template <class T>
__global__ __launch_bounds__(kDwThreads) void rroi_depthwise3x3_dw_finish_kernel(const double* __restrict__ partials,
                                                                                 T* __restrict__ dweight, unsigned N, unsigned C,
                                                                                 unsigned nseg)
{
    __shared__ double lds[kDwThreads / 64][9];
    const unsigned c = blockIdx.x;
    const unsigned long long terms = (unsigned long long)N * nseg;
    double tot[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) tot[k] = 0.0;
    for (unsigned long long lo = threadIdx.x; lo < terms; lo += (unsigned long long)kDwThreads * kDwbFinishBlock) {
        double s[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] = 0.0;
        const unsigned long long end = lo + (unsigned long long)kDwThreads * kDwbFinishBlock, hi = end < terms ? end : terms;
        for (unsigned long long i = lo; i < hi; i += kDwThreads) {
            const unsigned long long n = i / nseg, sg = i % nseg;
            const double* p = partials + ((n * C + c) * nseg + sg) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) s[k] += p[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) tot[k] += s[k];
    }
    const double r = dwb_block_sum(tot, lds);
    if (threadIdx.x < 9) ctc_narrow(r, dweight + (size_t)c * 9 + threadIdx.x);
}
