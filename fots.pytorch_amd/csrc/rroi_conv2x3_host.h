// rroi_conv2x3_host.h -- the (2,3) convolution, host part: the plan rule (one function for the plan query and the
// launch), the argument checks it carries, the one launch.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_merge_host.h (merge_count_ok).
#pragma once

// ------------------------------------------------------------------------------------
// The plan, a pure function of (dtype, N, Cin, Cout, H, W): ONE form.  The output is a flat list of
// N * (H - 1) * ceil(W / 32) items of 32 columns of one output row; a workgroup takes 32 output channels of 4 consecutive
// items, one per wave, and walks Cin in chunks of 32, two of them in flight.
// tests/conv2x3_cases.py mirrors this rule (plan_of) to pick its shapes: change both together.
// ------------------------------------------------------------------------------------
struct Conv2x3Plan {
    int status = 0;            // 0: the call refuses these arguments
    int Ho = 0;
    unsigned m_tiles = 0, x_tiles = 0, items = 0, groups = 0, grid = 0, k_chunks = 0;
};

inline Conv2x3Plan plan_conv2x3(int dtype, int batch_size, int cin, int cout, int height, int width)
{
    Conv2x3Plan P;
    if (dtype != RROI_DTYPE_BF16 && dtype != RROI_DTYPE_FP16) return P;
    if (batch_size < 1 || cin < 1 || cout < 1 || height < 2 || width < 1) return P;
    P.Ho = height - 1;
    if (!merge_count_ok(batch_size, cin, height, width) || !merge_count_ok(batch_size, cout, P.Ho, width) ||
        !merge_count_ok(cout, cin, 2, 3))
        return P;
    P.status = 1;
    P.m_tiles = (unsigned)((cout + 31) / 32);
    P.x_tiles = (unsigned)((width + kC2TileW - 1) / kC2TileW);
    P.items = (unsigned)batch_size * (unsigned)P.Ho * P.x_tiles;                 // <= N * Ho * W
    P.groups = (P.items + kC2Items - 1) / kC2Items;
    P.grid = P.groups * P.m_tiles;                                              // <= N * Cout * Ho * W < 2^31
    P.k_chunks = (unsigned)((cin + kC2KC - 1) / kC2KC);
    return P;
}

template <class T>
int launch_conv2x3(const Conv2x3Plan& P, const T* x, const T* w, T* y, unsigned Cin, unsigned Cout, unsigned H, unsigned W,
                   float slope, hipStream_t stream)
{
    hipLaunchKernelGGL((rroi_conv2x3_kernel<T>), dim3(P.grid), dim3(kC2Threads), 0, stream, x, w, y, Cin, Cout, H, W,
                       (unsigned)P.Ho, P.x_tiles, P.m_tiles, P.items, slope);
    return launch_status();
}
