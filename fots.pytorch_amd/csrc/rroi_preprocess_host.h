// rroi_preprocess_host.h -- native preprocessing, host part: argument checks, the plan (a pure function of the output's
// shape), the one launch.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_host_launch.h (status helpers, with_dtype).
#pragma once

// ------------------------------------------------------------------------------------
// What rroi_preprocess_forward_hip launches for a y of (batch_size, 3, out_height, out_width): one item per V = 16 /
// sizeof(T) output columns x `band` output rows of one image, one thread per item.  status 0: what the call refuses
// before any launch (an unknown dtype, batch_size < 0, a size below 1, y of 2^31 elements or more).
//
// band: rows per thread share the column geometry and, where consecutive output rows share a source row, its taps; but a
// thread's rows are a serial chain, so the band grows only while the grid keeps kPpBandWaves waves (four per CU of a
// 256-CU chip): 4 rows for the workload's batch of eight 704 x 1280 images (3520 waves), 1 for a single one (1760).
// ------------------------------------------------------------------------------------
constexpr long long kPpBandWaves = 1024;

struct PreprocessPlan {
    int status = 0;
    int V = 0, band = 0, wide = 0;
    unsigned nstrips = 0, nbands = 0, items = 0, grid = 0;
};

inline PreprocessPlan plan_preprocess(int dtype, int batch_size, int out_h, int out_w)
{
    PreprocessPlan P;
    if (!dtype_ok(dtype)) return P;
    if (batch_size < 0 || out_h < 1 || out_w < 1) return P;
    if ((long long)out_h * out_w > ((1LL << 31) - 1) / 3) return P;
    if ((long long)batch_size * 3 * out_h * out_w >= (1LL << 31)) return P;
    P.status = 1;
    P.V = dtype == RROI_DTYPE_FP32 ? 4 : 8;
    P.wide = out_w % P.V == 0;
    P.nstrips = (unsigned)((out_w + P.V - 1) / P.V);
    const long long row_items = (long long)batch_size * out_h * P.nstrips;
    P.band = 1;
    while (P.band < 4 && P.band * 2 <= out_h && row_items / (P.band * 2) >= kPpBandWaves * 64) P.band *= 2;
    P.nbands = (unsigned)((out_h + P.band - 1) / P.band);
    P.items = (unsigned)((long long)batch_size * P.nbands * P.nstrips);    // <= y's elements < 2^31
    P.grid = (P.items + kPpThreads - 1) / kPpThreads;
    return P;
}

template <class T>
int launch_preprocess(const PreprocessPlan& P, const unsigned char* src, const int* table, T* y, int Ho, int Wo,
                      hipStream_t stream)
{
    // the wide form needs every row segment 16-byte aligned: whole runs (the plan) and an aligned base (this call's y)
    if (P.wide && reinterpret_cast<size_t>(y) % 16 == 0)
        hipLaunchKernelGGL((rroi_preprocess_kernel<T, true>), dim3(P.grid), dim3(kPpThreads), 0, stream, src, table, y, Ho, Wo,
                           P.band, P.nstrips, P.nbands, P.items);
    else
        hipLaunchKernelGGL((rroi_preprocess_kernel<T, false>), dim3(P.grid), dim3(kPpThreads), 0, stream, src, table, y, Ho, Wo,
                           P.band, P.nstrips, P.nbands, P.items);
    return launch_status();
}
