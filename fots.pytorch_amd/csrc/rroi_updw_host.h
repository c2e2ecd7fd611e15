// rroi_updw_host.h -- bilinear resize + depthwise 3x3, host part: argument checks, the scales, band height, the one launch
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_depthwise_host.h (depthwise_band) and
// rroi_merge_host.h (merge_scale, merge_count_ok).
#pragma once

// ------------------------------------------------------------------------------------
// What rroi_up_depthwise3x3_forward_hip refuses before any launch (include/rroi_align_hip.h section 13): an unknown dtype,
// a dimension below 1 on either side, N * C * h * w or N * C * Ho * Wo >= 2^31.  Pointers are checked by the entry point.
// ------------------------------------------------------------------------------------
inline bool updw_shape_ok(int dtype, int batch_size, int channels, int in_h, int in_w, int out_h, int out_w)
{
    if (!dtype_ok(dtype)) return false;
    if (batch_size < 1 || channels < 1 || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1) return false;
    return merge_count_ok(batch_size, channels, in_h, in_w) && merge_count_ok(batch_size, channels, out_h, out_w);
}

// The geometry is the depthwise kernel's, on the OUTPUT's size (depthwise_band); the two scales are the merge's
// (merge_scale: (in - 1) / (out - 1) in double, 0 where out == 1).
template <class T>
int launch_updw(const T* a, const T* w, T* y, int N, int C, int in_h, int in_w, int Ho, int Wo, hipStream_t stream)
{
    const long long planes = (long long)N * C;
    const int band = depthwise_band(planes, Ho, Wo);
    const unsigned nstrips = (unsigned)ceil_div(Wo, kDwCols), nbands = (unsigned)ceil_div(Ho, band);
    const long long items = planes * nbands * nstrips;   // <= N * C * Ho * Wo < 2^31
    const dim3 grid((unsigned)ceil_div(items, (long long)kDwThreads));
    const MgSource A{in_h, in_w, merge_scale(in_h, Ho), merge_scale(in_w, Wo)};
    if (in_h != Ho || in_w != Wo)
        hipLaunchKernelGGL((rroi_updw_kernel<T, true>), grid, dim3(kDwThreads), 0, stream, a, w, y, C, Ho, Wo, band, nstrips,
                           nbands, (unsigned)items, A);
    else
        hipLaunchKernelGGL((rroi_updw_kernel<T, false>), grid, dim3(kDwThreads), 0, stream, a, w, y, C, Ho, Wo, band, nstrips,
                           nbands, (unsigned)items, A);
    return launch_status();
}
