// rroi_recogniser_host.h -- the recogniser's head and its activation + pool, host part: the plan rules (one function each
// for the plan query and the launch), the argument checks they carry, the one launch each.
// Included by rroi_align_hip.hip inside its anonymous namespace, after rroi_merge_host.h (merge_count_ok).
#pragma once

// ------------------------------------------------------------------------------------
// The head's plan, a pure function of (dtype, N, C, K, T): ONE form --
//   S      waves per workgroup: ceil(K / 32); a wave is 4 rows of 16 lanes, a row owns 8 classes and all C channels (the
//          last wave's last rows may own none)
//   tiles  of 16 columns per crop: ceil(T / 16);  grid N * tiles
//   LDS    max(64 S, 16 K) doubles: the lanes' maxima ([S][64]), then the exponentials ([K][16])
// K <= kOhMaxClasses = 128: 4 waves.  `dtype` does not enter the rule.
// tests/recogniser_cases.py mirrors this rule (head_plan_of): change both together.
// ------------------------------------------------------------------------------------
struct OcrHeadPlan {
    int status = 0;            // 0: the call refuses these arguments
    int S = 1;
    unsigned tiles = 0;        // per crop
    unsigned grid = 0;         // N * tiles
    unsigned lds_bytes = 0;
};

inline OcrHeadPlan plan_ocr_head(int dtype, int batch_size, int channels, int classes, int steps)
{
    OcrHeadPlan P;
    if (!dtype_ok(dtype)) return P;
    if (batch_size < 1 || channels < 1 || classes < 1 || steps < 1 || classes > kOhMaxClasses) return P;
    if (!merge_count_ok(batch_size, channels, steps, 1) || !merge_count_ok(batch_size, classes, steps, 1) ||
        !merge_count_ok(classes, channels, 1, 1))
        return P;
    P.status = 1;
    P.S = (classes + kOhClasses - 1) / kOhClasses;
    P.tiles = ((unsigned)steps + (unsigned)kOhCols - 1u) / (unsigned)kOhCols;
    P.grid = (unsigned)batch_size * P.tiles;                          // <= N * T < 2^31
    P.lds_bytes = (unsigned)(std::max(64 * P.S, kOhCols * classes) * sizeof(double));   // <= 16,384
    return P;
}

template <class T>
int launch_ocr_head(const OcrHeadPlan& P, const T* x, const T* w, const T* b, T* y, unsigned C, unsigned K, unsigned Tn,
                    hipStream_t stream)
{
    hipLaunchKernelGGL((rroi_ocr_head_kernel<T>), dim3(P.grid), dim3((unsigned)P.S * 64u), P.lds_bytes, stream, x, w, b, y, C, K,
                       Tn, P.tiles);
    return launch_status();
}

// ------------------------------------------------------------------------------------
// The pool's plan: V = 16 bytes of the element type per thread (4 / 8), one thread per chunk of V columns of an output row.
// ------------------------------------------------------------------------------------
struct ActPoolPlan {
    int status = 0;
    int V = 4, Ho = 0;
    unsigned chunks = 0;       // per row: ceil(W / V)
    unsigned items = 0;        // N * C * Ho * chunks
    unsigned grid = 0;
};

inline ActPoolPlan plan_act_pool(int dtype, int batch_size, int channels, int height, int width)
{
    ActPoolPlan P;
    if (!dtype_ok(dtype)) return P;
    if (batch_size < 1 || channels < 1 || height < 2 || width < 1) return P;
    if (!merge_count_ok(batch_size, channels, height, width)) return P;   // the output is smaller
    P.status = 1;
    P.V = dtype == RROI_DTYPE_FP32 ? 4 : 8;
    P.Ho = height / 2;
    P.chunks = ((unsigned)width + (unsigned)P.V - 1u) / (unsigned)P.V;
    P.items = (unsigned)((long long)batch_size * channels * P.Ho * P.chunks);   // <= N * C * Ho * W < 2^30
    P.grid = (P.items + (unsigned)kApThreads - 1u) / (unsigned)kApThreads;
    return P;
}

template <class T>
int launch_act_pool(const ActPoolPlan& P, const T* x, T* y, unsigned H, unsigned W, float slope, hipStream_t stream)
{
    constexpr int V = 16 / sizeof(T);
    hipLaunchKernelGGL((rroi_act_maxpool2x1_kernel<T, V>), dim3(P.grid), dim3(kApThreads), 0, stream, x, y, H, W, (unsigned)P.Ho,
                       P.chunks, P.items, slope);
    return launch_status();
}
