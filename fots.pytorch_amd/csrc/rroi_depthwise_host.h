// rroi_depthwise_host.h -- depthwise 3x3 convolution, host part: argument checks, band height, the one launch
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_host_launch.h (status helpers, with_dtype).
#pragma once

// ------------------------------------------------------------------------------------
// What rroi_depthwise3x3_forward_hip refuses before any launch (include/rroi_align_hip.h section 5): an unknown dtype, a
// stride other than 1 or 2, a dimension below 1, N * C * H * W >= 2^31 (the kernel's item index and the callers' 32-bit
// sizes).  Pointers are checked by the entry point.
// ------------------------------------------------------------------------------------
inline bool depthwise_shape_ok(int dtype, int batch_size, int channels, int height, int width, int stride)
{
    if (!dtype_ok(dtype) || (stride != 1 && stride != 2)) return false;
    if (batch_size < 1 || channels < 1 || height < 1 || width < 1) return false;
    long long total = batch_size;
    for (const int d : {channels, height, width}) {
        if (total > ((1LL << 31) - 1) / d) return false;
        total *= d;
    }
    return true;
}

// Output rows per thread.  A taller band re-reads fewer halo rows (band + 2 input rows per band at stride 1) but makes
// fewer threads: the tallest of 8, 4, 2 that still gives every SIMD of the chip a wave (256 CUs x 4 SIMDs x 64 lanes).
// The network's planes run from 176 x 320 (band 8) down to 22 x 40 with 512 channels (band 2).
// tests/depthwise_cases.py mirrors this rule (band_of) to pick shapes that reach every band height: change both together.
inline int depthwise_band(long long planes, int out_height, int out_width)
{
    const long long nstrips = ceil_div(out_width, kDwCols);
    int band = kDwMaxBand;
    while (band > 2 && planes * ceil_div(out_height, band) * nstrips < 65536) band >>= 1;
    return band;
}

template <class T>
int launch_depthwise3x3(const T* x, const T* w, T* y, int N, int C, int H, int W, int stride, hipStream_t stream)
{
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const long long planes = (long long)N * C;
    const int band = depthwise_band(planes, Ho, Wo);
    const unsigned nstrips = (unsigned)ceil_div(Wo, kDwCols), nbands = (unsigned)ceil_div(Ho, band);
    const long long items = planes * nbands * nstrips;   // <= N * C * Ho * Wo < 2^31
    const dim3 grid((unsigned)ceil_div(items, (long long)kDwThreads));
    if (stride == 1)
        hipLaunchKernelGGL((rroi_depthwise3x3_kernel<T, 1>), grid, dim3(kDwThreads), 0, stream, x, w, y, C, H, W, Ho, Wo, band,
                           nstrips, nbands, (unsigned)items);
    else
        hipLaunchKernelGGL((rroi_depthwise3x3_kernel<T, 2>), grid, dim3(kDwThreads), 0, stream, x, w, y, C, H, W, Ho, Wo, band,
                           nstrips, nbands, (unsigned)items);
    return launch_status();
}
