// rroi_host_launch.h -- host side, part 3 of 3: the launches.  Every launch_* runs the plan it is handed (rroi_host_plan.h) on
// the Shape that plan carries, so a launch cannot run on another shape than its plan.  Plain templates over the element
// type T of the caller's tensors (float, bf16_t, fp16_t).  Included by rroi_align_hip.hip inside its anonymous namespace.
#pragma once

inline int status_of(hipError_t e) { return e == hipSuccess ? 1 : -(int)e; }
inline int launch_status() { return status_of(hipGetLastError()); }

// f(T{}) for the element type a `dtype` code names (dtype_ok(dtype) holds): the one place a code becomes a type.
template <class F>
auto with_dtype(int dtype, F&& f)
{
    return dtype == RROI_DTYPE_BF16 ? f(bf16_t{}) : dtype == RROI_DTYPE_FP16 ? f(fp16_t{}) : f(float{});
}

// Where the forward gather finds a pixel's 32 channels (SliceLayout, rroi_device_common.h).  The chunk-major copy of the
// workspace: (B, nchunks, H * pitch + 1, 32) ...
SliceLayout chunk_major_layout(const Shape& S)
{
    const unsigned pitch = (unsigned)row_pitch(S.width);
    SliceLayout lay;
    lay.px_bytes = kLineBytes;
    lay.row_bytes = pitch * kLineBytes;
    lay.slice_bytes = (unsigned)S.height * lay.row_bytes;
    lay.chunk_stride = ((unsigned)S.height * pitch + 1u) * kChunk;
    lay.img_stride = lay.chunk_stride * (unsigned)S.nchunks();
    return lay;
}
// ... channels-last features consumed in place ...
SliceLayout zero_copy_layout(const Shape& S)
{
    SliceLayout lay;
    lay.px_bytes = (unsigned)S.channels * 4u;
    lay.row_bytes = (unsigned)S.width * lay.px_bytes;
    lay.slice_bytes = (unsigned)S.HW() * lay.px_bytes;  // to the end of the image (base = chunk k of pixel 0)
    lay.chunk_stride = kChunk;
    lay.img_stride = (unsigned)S.HW() * (unsigned)S.channels;
    return lay;
}
// ... or the NCHW map itself (the one-launch form).
SliceLayout nchw_src_layout(const Shape& S)
{
    const unsigned HWu = (unsigned)S.height * (unsigned)S.width;
    SliceLayout lay;
    lay.px_bytes = 4u;                       // a "pixel" of a channel plane
    lay.row_bytes = (unsigned)S.width * 4u;
    lay.slice_bytes = HWu * 4u;              // ONE plane: the kernel's descriptor covers the chunk's planes < C
    lay.chunk_stride = kChunk * HWu;         // floats (shape_ok: C * H * W * 4 < 2^30)
    lay.img_stride = (unsigned)S.channels * HWu;
    return lay;
}

// How the backward's gathers address top_diff.  A list entry names a bin; its chunk k is the 128-byte line at
// entry * line_stride + k * 32 floats: in the relaid-out copy (R, NB, nchunks * 32) or in a channels-last top_diff
// (R, NB, C) consumed in place.
struct ListAddressing {
    unsigned lines_per_roi, chunk_stride, line_stride;
    FastDiv dpw;
    PatchMap dnb;
};
ListAddressing list_addressing(const Shape& S, bool td_nhwc)
{
    return {(unsigned)S.NB(), (unsigned)kChunk, td_nhwc ? (unsigned)S.channels : (unsigned)S.nchunks() * (unsigned)kChunk,
            make_fastdiv((unsigned)S.pooled_width), make_patch_map(S.pooled_height, S.pooled_width)};
}

template <class T>
void launch_patch_forward(const FwdDispatch& P, const T* features, const float* rois, T* top_data, float* idx_x, float* idx_y,
                          float spatial_scale, hipStream_t stream)
{
    const PatchPlan& p = P.patch;
    const Shape& S = P.shape;
    const int num_rois = S.num_rois, channels = S.channels, height = S.height, width = S.width;
    const int pooled_height = S.pooled_height, pooled_width = S.pooled_width, trig = P.trig, batch_size = P.direct_batch();
    if constexpr (!std::is_same<T, float>::value)   // (the reference ABI's con_idx: fp32 calls only)
        hipLaunchKernelGGL((rroi_fwd_patch_kernel<4, false, T>), p.grid, dim3(256), 0, stream, features, rois, top_data, num_rois,
                           channels, height, width, pooled_height, pooled_width, spatial_scale, trig, batch_size, p.cw, p.npx,
                           p.npatches, p.prows, p.pcols, (float*)nullptr, (float*)nullptr);
    else if (idx_x)
        hipLaunchKernelGGL((rroi_fwd_patch_kernel<4, true>), p.grid, dim3(256), 0, stream, features, rois, top_data, num_rois, channels,
                           height, width, pooled_height, pooled_width, spatial_scale, trig, batch_size, p.cw, p.npx, p.npatches,
                           p.prows, p.pcols, idx_x, idx_y);
    else
        hipLaunchKernelGGL((rroi_fwd_patch_kernel<4, false>), p.grid, dim3(256), 0, stream, features, rois, top_data, num_rois, channels,
                           height, width, pooled_height, pooled_width, spatial_scale, trig, batch_size, p.cw, p.npx, p.npatches,
                           p.prows, p.pcols, (float*)nullptr, (float*)nullptr);
}

// The forward prologue launch (relayout to the chunk-major copy + affine table [+ ROI sort, + the launcher's rest blocks]):
// shared by the dense two-launch plan and the bucketed one (which runs it unchanged: one group, no launcher).
template <class T>
int launch_forward_prologue(const FwdDispatch& P, const Workspace& ws, const T* features, const float* rois, T* top_data,
                            float spatial_scale, hipStream_t stream)
{
    constexpr bool kF32 = std::is_same<T, float>::value;
    const Shape& S = P.shape;
    const int batch_size = S.batch_size, num_rois = S.num_rois, width = S.width, channels = S.channels;
    const int HW = S.HW(), nchunks = S.nchunks(), groups = P.groups;
    const bool zero_copy = P.zero_copy, launcher_rest = P.launcher;
    const int pitch = row_pitch(width);
    const int ptiles = ceil_div(HW, kRelayoutPx);
    const int relayout_tiles = zero_copy ? 0 : ptiles * nchunks * batch_size;
    // ~3 resident blocks per CU, each streaming several tiles with the next tile prefetched
    int relayout_blocks = relayout_tiles;
    if (groups > 1) relayout_blocks = (relayout_blocks + 7) / 8 * 8;   // whole XCD rounds (a block without a tile leaves)
    if (relayout_blocks > num_cus() * g_tune.prologue_blocks_per_cu) {
        relayout_blocks = num_cus() * g_tune.prologue_blocks_per_cu;
        const long unit = lcm8(nchunks);   // keeps block -> chunk -> XCD stable
        if (relayout_blocks >= unit) relayout_blocks = (int)(relayout_blocks / unit * unit);
    }
    const int aff_blocks = ceil_div(num_rois, 256);
    const int rest_blocks = launcher_rest ? num_rois : 0;
    float* rest_out = nullptr;   // (the launcher: fp32)
    if constexpr (kF32) rest_out = launcher_rest ? top_data : nullptr;
    // <0>: plain stores: the copy stays in the L2s that wrote it (write-through: 1.8 us faster alone, the step is not)
    hipLaunchKernelGGL((rroi_prologue_kernel<0, T>), dim3(relayout_blocks + aff_blocks + (groups > 1 ? 1 : 0) + rest_blocks),
                       dim3(256), 0, stream, features, ws.cm, channels, HW, width, pitch, make_fastdiv((unsigned)width), nchunks,
                       ptiles, relayout_blocks, relayout_tiles, batch_size, rois, num_rois, S.pooled_height, spatial_scale,
                       P.trig, ws.aff, aff_blocks, rest_out, S.pooled_width, groups, ws.sort_rank, ws.sort_order);
    return launch_status();
}

// Launches the plan `P` on P.shape.  The launcher's tiled plan (P.launcher): ROIs whose
// image index is >= batch_size are sampled from the NCHW tensor by extra blocks of the prologue launch and left alone
// by the gather; its direct kernels get no batch count (-1) and write con_idx where P.con_idx.
// T: the element type of the map and the crops (float, bf16_t, fp16_t; the plan of a 16-bit call has no fused form, no
// zero copy and no launcher)
template <class T>
int launch_forward(const FwdDispatch& P, const T* features, const float* rois, T* top_data, float* idx_x, float* idx_y,
                   float spatial_scale, void* workspace, size_t workspace_bytes, int stages, hipStream_t stream)
{
    constexpr bool kF32 = std::is_same<T, float>::value;
    const Shape& S = P.shape;
    const int batch_size = S.batch_size, num_rois = S.num_rois, height = S.height, width = S.width, channels = S.channels;
    const int pooled_height = S.pooled_height, pooled_width = S.pooled_width, NB = S.NB(), nchunks = S.nchunks();
    const int trig = P.trig;
    switch (P.family) {
    case RROI_PLAN_NONE:
        return 1;
    case RROI_PLAN_FWD_DIRECT_K2P:
        if (!(stages & RROI_STAGE_GATHER)) return 1;  // the direct path has no prologue
        launch_patch_forward(P, features, rois, top_data, P.con_idx ? idx_x : nullptr, P.con_idx ? idx_y : nullptr,
                             spatial_scale, stream);
        return launch_status();
    case RROI_PLAN_FWD_DIRECT_THREAD:
        if (!(stages & RROI_STAGE_GATHER)) return 1;
        hipLaunchKernelGGL(rroi_fwd_direct_kernel<T>, P.dgrid, dim3(256), 0, stream, features, rois, top_data,
                           P.con_idx ? idx_x : nullptr, P.con_idx ? idx_y : nullptr, num_rois, channels, height, width,
                           pooled_height, pooled_width, spatial_scale, trig, P.direct_batch(), P.cslab);
        return launch_status();
    case RROI_PLAN_FWD_FUSED_STRIDED:
    case RROI_PLAN_FWD_FUSED_SHIFT: {
        if constexpr (!kF32) {   // (fp32 only: no 16-bit plan)
            return 0;
        } else {
        if (!(stages & RROI_STAGE_GATHER)) return 1;  // one launch, run under the gather stage
        const ForwardPlan& plan = P.gather;
        const SliceLayout lay = nchw_src_layout(S);
        const FastDiv dt = make_fastdiv((unsigned)plan.ntiles), dp = make_fastdiv((unsigned)pooled_width);
        const RoiSource rsrc = {rois, pooled_height, spatial_scale, trig};
#define RROI_FUSED(...)                                                                                                   \
    hipLaunchKernelGGL((rroi_fwd_split_kernel<__VA_ARGS__>), dim3(plan.grid), dim3(2 * kWave), 0, stream, features,          \
                       (const Affine*)nullptr, top_data, num_rois, channels, height, width, pooled_width, NB, batch_size,    \
                       nchunks, plan.ntiles, lay, dt, dp, plan.dbg, XcdGroups{1, nullptr}, rsrc)
        if (P.family == RROI_PLAN_FWD_FUSED_SHIFT) RROI_FUSED(true, 0, 4, 3, false, 1, true);
        else RROI_FUSED(true, 0, 4, 3, false, 0, true);
#undef RROI_FUSED
        return launch_status();
        }
    }
    case RROI_PLAN_FWD_TWO_LAUNCH:
        break;
    default:
        return 0;
    }

    const bool zero_copy = P.zero_copy;   // channels-last features: the workspace holds no copy of the map
    const Workspace ws = carve(workspace, S, zero_copy ? RROI_LAYOUT_NHWC : RROI_LAYOUT_NCHW);
    if (!workspace_ok(workspace) || workspace_bytes < ws.bytes) return 0;
    const float* map = ws.cm;
    if constexpr (kF32) map = zero_copy ? features : ws.cm;
    const int groups = P.groups;

    // prologue: relayout + affine table in one launch
    if (stages & RROI_STAGE_PROLOGUE) {
        const int st = launch_forward_prologue(P, ws, features, rois, top_data, spatial_scale, stream);
        if (st != 1) return st;
    }
    if (stages & RROI_STAGE_GATHER) {
        const ForwardPlan& plan = P.gather;
        const int ntiles = plan.ntiles;
        const SliceLayout lay = zero_copy ? zero_copy_layout(S) : chunk_major_layout(S);
        const FastDiv dt = make_fastdiv((unsigned)ntiles), dp = make_fastdiv((unsigned)pooled_width);
        // the shipped instantiations of rroi_fwd_split_kernel<VEC_STORE, EARLY, OCC, HID, ONHWC, SHIFT, NCHW_SRC, WAUX, T>,
        // one per FwdKernel and element type
#define RROI_GATHER(...)                                                                                              \
    hipLaunchKernelGGL((rroi_fwd_split_kernel<__VA_ARGS__>), dim3(plan.grid), dim3(2 * kWave), 0, stream, map, ws.aff, \
                       top_data, num_rois, channels, height, width, pooled_width, NB, batch_size, nchunks, ntiles, lay, \
                       dt, dp, plan.dbg, XcdGroups{groups, ws.sort_order})
        switch (plan.kernel) {
        case FwdKernel::kStrided:       RROI_GATHER(true, 0, 6, 3, false, 0, false, -1, T); break;   // 62-64 VGPRs, 12.1 KB of LDS: 12 per CU
        case FwdKernel::kChannelsLast:  RROI_GATHER(true, 2, 5, 2, true, 0, false, -1, T); break;    // 91 VGPRs: 10 per CU
        case FwdKernel::kShift:         RROI_GATHER(true, 0, 6, 3, false, 1, false, -1, T); break;   // 79 VGPRs, 12.4 KB of LDS: 12 per CU
        case FwdKernel::kStridedMerge:  RROI_GATHER(true, 0, 6, 3, false, 0, false, 0, T); break;    // plain stores (write-through: 32.1 against 30.1 us)
        case FwdKernel::kShiftLines:    RROI_GATHER(true, 0, 5, 3, false, 2, false, -1, T); break;   // 84 VGPRs, 14.8 KB of LDS: 10 per CU
        case FwdKernel::kStridedRagged: return 0;   // (launch_forward_bucketed's own)
        }
#undef RROI_GATHER
    }
    return launch_status();
}

template <class T>
int launch_forward_bucketed(const FwdDispatch& P, const T* features, const float* rois, const CropRow* crops,
                            float spatial_scale, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    const Shape& S = P.shape;
    const int batch_size = S.batch_size, num_rois = S.num_rois, height = S.height, width = S.width, channels = S.channels;
    const int pooled_height = S.pooled_height, max_pooled_width = S.pooled_width, nchunks = S.nchunks();
    if (P.family == RROI_PLAN_FWD_DIRECT_K2P) {
        const PatchPlan& p = P.patch;
        hipLaunchKernelGGL((rroi_fwd_patch_kernel<4, false, T, true>), p.grid, dim3(256), 0, stream, features, rois, crops,
                           num_rois, channels, height, width, pooled_height, max_pooled_width, spatial_scale, P.trig, batch_size,
                           p.cw, p.npx, p.npatches, p.prows, p.pcols, (float*)nullptr, (float*)nullptr);
        return launch_status();
    }
    if (P.family != RROI_PLAN_FWD_TWO_LAUNCH) return 0;
    const Workspace ws = carve(workspace, S, RROI_LAYOUT_NCHW);
    if (!workspace_ok(workspace) || workspace_bytes < ws.bytes) return 0;
    const int st = launch_forward_prologue(P, ws, features, rois, (T*)nullptr, spatial_scale, stream);
    if (st != 1) return st;
    const SliceLayout lay = chunk_major_layout(S);
    const ForwardPlan& plan = P.gather;
    const FastDiv dt = make_fastdiv((unsigned)plan.ntiles), dp = make_fastdiv((unsigned)max_pooled_width);
    hipLaunchKernelGGL((rroi_fwd_split_kernel<true, 0, 6, 3, false, 0, false, -1, T, true>), dim3(plan.grid), dim3(2 * kWave), 0,
                       stream, ws.cm, ws.aff, crops, num_rois, channels, height, width, max_pooled_width,
                       pooled_height * max_pooled_width, batch_size, nchunks, plan.ntiles, lay, dt, dp, plan.dbg,
                       XcdGroups{1, nullptr}, RoiSource{nullptr, 0, 0.0f, 0});
    return launch_status();
}

// Launches the plan `P` on P.shape; P.accumulate: bottom_diff += gradient.
// T: the element type of top_diff and bottom_diff (the plan of a 16-bit call is a gather, NCHW top_diff, not accumulating)
template <class T>
int launch_backward(const BwdDispatch& P, const T* top_diff, const float* rois, T* bottom_diff, float spatial_scale,
                    void* workspace, size_t workspace_bytes, hipStream_t stream,
                    const CropRow* ragged = nullptr)   // the bucketed call: the gradient crops' table (top_diff is NULL)
{
    constexpr bool kF32 = std::is_same<T, float>::value;
    const Shape& S = P.shape;
    const int batch_size = S.batch_size, num_rois = S.num_rois, height = S.height, width = S.width, channels = S.channels;
    const int pooled_height = S.pooled_height, pooled_width = S.pooled_width, NB = S.NB(), nchunks = S.nchunks();
    const int trig = P.trig;
    const size_t HW = S.HW();
    const size_t in_bytes = (size_t)batch_size * channels * HW * sizeof(T);
    const bool td_nhwc = P.td_nhwc, accumulate = P.accumulate;
    switch (P.family) {
    case RROI_PLAN_NONE:
        return accumulate ? 1 : status_of(hipMemsetAsync(bottom_diff, 0, in_bytes, stream));
    case RROI_PLAN_BWD_DIRECT: {
        if constexpr (!kF32) {   // (fp32 atomics: no 16-bit plan)
            return 0;
        } else {
            hipError_t e = hipMemsetAsync(bottom_diff, 0, in_bytes, stream);
            if (e != hipSuccess) return status_of(e);
            hipLaunchKernelGGL(rroi_bwd_direct_kernel, P.grid, dim3(256), 0, stream, top_diff, rois,
                               bottom_diff, num_rois, channels, height, width, pooled_height,
                               pooled_width, spatial_scale, trig, batch_size, P.cslab);
            return launch_status();
        }
    }
    case RROI_PLAN_BWD_ATOMIC:
    case RROI_PLAN_BWD_INKERNEL:
    case RROI_PLAN_BWD_LISTS:
    case RROI_PLAN_BWD_BUCKETS:
    case RROI_PLAN_BWD_ORDERED:
        break;
    default:   // (the literal kernel is the launcher's own)
        return 0;
    }

    const BwdWorkspace ws = carve_bwd(workspace, S);
    if (!workspace_ok(workspace) || workspace_bytes < ws.bytes) return 0;
    if (!kF32 && (P.family == RROI_PLAN_BWD_ATOMIC || td_nhwc || accumulate)) return 0;
    if (ragged && (td_nhwc || accumulate || !(P.family == RROI_PLAN_BWD_LISTS || P.family == RROI_PLAN_BWD_BUCKETS ||
                                               P.family == RROI_PLAN_BWD_ORDERED)))
        return 0;
    // where the gather reads top_diff: the relaid-out fp32 copy, or an fp32 channels-last top_diff in place
    const float* srcT = ws.tdT;
    if constexpr (kF32) srcT = td_nhwc ? top_diff : ws.tdT;
    const int pitch = row_pitch(width);
    const int ptiles = ceil_div((long)HW, kRelayoutPx);
    const bool gather = P.family != RROI_PLAN_BWD_ATOMIC;
    const bool buckets = P.family == RROI_PLAN_BWD_BUCKETS;
    const bool ordered = P.family == RROI_PLAN_BWD_ORDERED;
    const bool lists = buckets || ordered || P.family == RROI_PLAN_BWD_LISTS;
    const BucketLists BL = {ws.kshift, reinterpret_cast<int*>(ws.off), ws.bsum, ws.ov};
    {
        // affine table; the list passes' pixel counters (K3g) are cleared by the same launch
        const unsigned nzero = lists ? ws.keys.keys : 0u;
        int ablocks = ceil_div(num_rois, 256);
        const int zblocks = nzero ? (int)std::min<long>(ceil_div((long)nzero, 1024), 2L * num_cus()) : 0;
        if (zblocks > ablocks) ablocks = zblocks;
        hipLaunchKernelGGL(rroi_affine_kernel, dim3(ablocks), dim3(256), 0, stream, rois, num_rois, pooled_height,
                           spatial_scale, trig, ws.aff, ws.cnt, nzero, buckets ? BL.head : (int*)nullptr,
                           buckets ? BL.ovcnt : (unsigned*)nullptr);
    }
    int st = launch_status();
    if (st != 1) return st;

    const KeyLayout KL = ws.keys;
    const ListAddressing A = list_addressing(S, td_nhwc);
    if (P.family == RROI_PLAN_BWD_INKERNEL) {
        // K3t: relayout of top_diff (one launch, masked bins skipped), then the tile gather
        if (!td_nhwc) {
            const long blocks = P.relayout_blocks;
            hipLaunchKernelGGL((rroi_bwd_pairs_relayout_kernel<0, kBwdRelayoutAux, T>), dim3((unsigned)blocks), dim3(256), 0,
                               stream, ws.aff, num_rois, height, width, pooled_width, NB, batch_size, A.lines_per_roi, A.dnb,
                               A.dpw, KL, ws.cnt, ws.off, ws.bsum, ws.pairs, 0, top_diff, ws.tdT, channels, nchunks, P.tt,
                               (int)blocks, 0, (int)P.tiles, ws.scan_blocks, 0, BucketLists{0u, nullptr, nullptr, nullptr},
                               g_tune.bwd_skip_dead);
            st = launch_status();
            if (st != 1) return st;
        }
        const unsigned ntiles = KL.keys / 32u;
        const unsigned per_xcd = P.grid.x / 8u;
        const FastDiv dbt = make_fastdiv(KL.Ht * KL.Wt), dwt = make_fastdiv(KL.Wt), dph = make_fastdiv((unsigned)pooled_height);
        // NHWC: the caller's bottom_diff in place (its type); else the fp32 chunk-major scratch
#define RROI_LAUNCH_TG(NK, NHWC)                                                                          \
    hipLaunchKernelGGL((rroi_bwd_tile_gather_kernel<NK, NHWC, std::conditional_t<NHWC, T, float>>), P.grid,  \
                       dim3(kTgThreads), 0, stream,                                                          \
                       srcT, ws.aff, NHWC ? (std::conditional_t<NHWC, T, float>*)(void*)bottom_diff          \
                                          : (std::conditional_t<NHWC, T, float>*)(void*)ws.gcm,              \
                       num_rois, channels, height, width, pitch, pooled_height,                              \
                       pooled_width, batch_size, nchunks, A.chunk_stride, A.line_stride, A.lines_per_roi,    \
                       KL, ntiles, per_xcd, dbt, dwt, dph)
#define RROI_LAUNCH_TG_NK(NHWC)                          \
    do {                                                 \
        if constexpr (kF32)   /* (16-bit: nk <= 4) */    \
            if (P.nk == 8) {                             \
                RROI_LAUNCH_TG(8, NHWC);                 \
                break;                                   \
            }                                            \
        if (P.nk == 4) RROI_LAUNCH_TG(4, NHWC);          \
        else if (P.nk == 2) RROI_LAUNCH_TG(2, NHWC);     \
        else RROI_LAUNCH_TG(1, NHWC);                    \
    } while (0)
        if (P.dest == RROI_PLAN_DST_NHWC) {
            RROI_LAUNCH_TG_NK(true);
            return launch_status();  // written in place: no relayout back
        }
        RROI_LAUNCH_TG_NK(false);
#undef RROI_LAUNCH_TG_NK
#undef RROI_LAUNCH_TG
        st = launch_status();
        if (st != 1) return st;
    } else
    if (gather) {
        // (1) pixel -> (bin, weight) lists: count, scan, fill
        const int raw_bsum = P.raw_bsum;
        const int pblocks = P.pblocks;
        const bool aggregate = P.aggregate;
        const int tt = P.tt;
        const long tiles = P.tiles, half = P.half;
#define RROI_LAUNCH_PR_(FILL, SAUX, RAGGED, SRC, BLOCKS, T0, T1)                                     \
    hipLaunchKernelGGL((rroi_bwd_pairs_relayout_kernel<FILL, SAUX, T, RAGGED>), dim3((unsigned)(pblocks + (BLOCKS))), \
                       dim3(256), 0, stream, ws.aff, num_rois, height, width, pooled_width, NB,          \
                       batch_size, A.lines_per_roi, A.dnb, A.dpw, KL, ws.cnt, ws.off, ws.bsum, ws.pairs,  \
                       pblocks, SRC, ws.tdT, channels, nchunks, tt, (int)(BLOCKS), (int)(T0), (int)(T1),            \
                       ws.scan_blocks, raw_bsum, BL, (g_tune.bwd_skip_dead ? 1 : 0) | (aggregate ? 2 : 0))
#define RROI_LAUNCH_PR(FILL, SAUX, BLOCKS, T0, T1)                                  \
    do {                                                                            \
        if (ragged) RROI_LAUNCH_PR_(FILL, SAUX, true, ragged, BLOCKS, T0, T1);      \
        else RROI_LAUNCH_PR_(FILL, SAUX, false, top_diff, BLOCKS, T0, T1);          \
    } while (0)
        if (buckets) {
            // ONE launch: every pair into its pixel's bucket (or overflow chain) || the whole relayout
            const long blocks = relayout_blocks(tiles, nchunks);
            RROI_LAUNCH_PR(2, kBwdRelayoutAux, blocks, 0, tiles);
        } else {
        {
            const long blocks = relayout_blocks(half, nchunks);
            RROI_LAUNCH_PR(0, kBwdRelayoutAux, blocks, 0, half);
        }
        hipLaunchKernelGGL(rroi_scan1_kernel, dim3(ws.scan_blocks), dim3(1024), 0, stream, ws.cnt, ws.off,
                           ws.bsum, KL.keys);
        if (!raw_bsum) hipLaunchKernelGGL(rroi_scan2_kernel, dim3(1), dim3(1024), 0, stream, ws.bsum, ws.scan_blocks);
        {
            const long blocks = relayout_blocks(tiles - half, nchunks);
            RROI_LAUNCH_PR(1, kBwdRelayoutAux, blocks, half, tiles);
        }
        }
#undef RROI_LAUNCH_PR
#undef RROI_LAUNCH_PR_
        st = launch_status();
        if (st != 1) return st;
        // (3) gather: one thread group per key, no grid-stride
        const unsigned sub_shift = P.sub_shift, tile_run = P.tile_run;
        if (ordered) {
            // (2b) every list in bin order: the short ones in registers, the rest queued in the counters (which the
            // fill left at zero) for one workgroup each; then the in-order fp64 gather, in place
            unsigned* const queue = reinterpret_cast<unsigned*>(ws.cnt);
            hipLaunchKernelGGL(rroi_bwd_sort_lists_kernel, dim3(ceil_div((long)KL.keys, 4L)), dim3(256), 0, stream,
                               ws.off, ws.bsum, ws.pairs, KL.keys, ws.scan_blocks, raw_bsum, queue);
            hipLaunchKernelGGL(rroi_bwd_sort_queue_kernel, dim3(num_cus() * 4), dim3(kSortQueueThreads), 0, stream,
                               ws.off, ws.bsum, ws.pairs, queue, ws.scan_blocks, raw_bsum);
#define RROI_LAUNCH_OG(DSTK)                                                                                   \
    hipLaunchKernelGGL((rroi_bwd_ordered_gather_kernel<DSTK, T>), P.grid, dim3(256), 0, stream, srcT, ws.off,   \
                       ws.bsum, ws.pairs, bottom_diff, channels, height, width, nchunks, A.chunk_stride,          \
                       A.line_stride, sub_shift, KL, make_fastdiv(KL.Ht * KL.Wt), make_fastdiv(KL.Wt),              \
                       ws.scan_blocks, raw_bsum, tile_run)
            if (P.dest == RROI_PLAN_DST_NHWC) RROI_LAUNCH_OG(kDstNhwc);
            else RROI_LAUNCH_OG(kDstNchw);
#undef RROI_LAUNCH_OG
            return launch_status();
        }
        // the lists: count / scan / fill segments (`off` = scanned offsets) or buckets (`off` = the counters)
        const unsigned* loff = buckets ? reinterpret_cast<const unsigned*>(ws.cnt) : ws.off;
#define RROI_LAUNCH_G(DSTK, BUCK, DST)                                                                        \
    hipLaunchKernelGGL((rroi_bwd_gather_kernel<DSTK, BUCK, std::remove_pointer_t<decltype(DST)>>), P.grid,    \
                       dim3(256), 0, stream,                                                                  \
                       srcT, loff, ws.bsum, ws.pairs, DST, channels, height, width,                           \
                       pitch, nchunks, A.chunk_stride, A.line_stride, sub_shift, KL, make_fastdiv(KL.Ht * KL.Wt), \
                       make_fastdiv(KL.Wt), ws.scan_blocks, raw_bsum, BL, tile_run)
        switch (P.dest) {
        case RROI_PLAN_DST_NHWC:   // written in place: no relayout back
            if (buckets) RROI_LAUNCH_G(kDstNhwc, true, bottom_diff);
            else RROI_LAUNCH_G(kDstNhwc, false, bottom_diff);
            return launch_status();
        case RROI_PLAN_DST_NCHW_ADD:
            if constexpr (kF32) {   // (the launcher)
                if (buckets) RROI_LAUNCH_G(kDstNchwAdd, true, bottom_diff);
                else RROI_LAUNCH_G(kDstNchwAdd, false, bottom_diff);
            }
            return launch_status();
        case RROI_PLAN_DST_NCHW:
            if (buckets) RROI_LAUNCH_G(kDstNchw, true, bottom_diff);
            else RROI_LAUNCH_G(kDstNchw, false, bottom_diff);
            return launch_status();
        default:
            break;
        }
        if (buckets) RROI_LAUNCH_G(kDstChunkMajor, true, ws.gcm);
        else RROI_LAUNCH_G(kDstChunkMajor, false, ws.gcm);
#undef RROI_LAUNCH_G
        st = launch_status();
        if (st != 1) return st;
    } else if constexpr (kF32) {
        hipError_t e = hipMemsetAsync(ws.gcm, 0, (size_t)batch_size * nchunks * height * pitch * kLineBytes, stream);
        if (e != hipSuccess) return status_of(e);
        const int ntiles = P.ntiles;
        const FastDiv dt = make_fastdiv((unsigned)ntiles), dp = make_fastdiv((unsigned)pooled_width);
        if (P.vec4)
            hipLaunchKernelGGL(rroi_bwd_tiled_kernel<true>, P.grid, dim3(kWave), 0, stream,
                               top_diff, ws.aff, ws.gcm, num_rois, channels, height, width, pitch,
                               pooled_width, NB, batch_size, nchunks, ntiles, dt, dp);
        else
            hipLaunchKernelGGL(rroi_bwd_tiled_kernel<false>, P.grid, dim3(kWave), 0, stream,
                               top_diff, ws.aff, ws.gcm, num_rois, channels, height, width, pitch,
                               pooled_width, NB, batch_size, nchunks, ntiles, dt, dp);
        st = launch_status();
        if (st != 1) return st;
    }
    if (accumulate) {
        if constexpr (kF32)
            hipLaunchKernelGGL(rroi_cm_to_nchw_kernel<true>, dim3(ptiles * nchunks * batch_size), dim3(256), 0,
                               stream, ws.gcm, bottom_diff, channels, (int)HW, width, pitch,
                               make_fastdiv((unsigned)width), nchunks, ptiles);
    } else
        hipLaunchKernelGGL((rroi_cm_to_nchw_kernel<false, T>), dim3(ptiles * nchunks * batch_size), dim3(256), 0,
                           stream, ws.gcm, bottom_diff, channels, (int)HW, width, pitch,
                           make_fastdiv((unsigned)width), nchunks, ptiles);
    return launch_status();
}

// one decode call for maps of element type T (float: the kernels of every release; bf16_t / fp16_t: the typed ones)
template <class T>
int rbox_decode_impl(const T* segm, const T* rbox, const T* angle, int height, int width, float segm_thresh,
                     void* candidates, int capacity, int* count, hipStream_t stream)
{
    const int hw = height * width;
    const int slabs = ceil_div(hw, 1024);
    unsigned* slab_counts = nullptr;
    // large map: per-slab counts from a first launch, kept behind the records the caller's buffer can ever
    // need (a map of hw pixels yields at most hw records) -- when the buffer has that room.  A buffer sized
    // for fewer records (a caller relying on *count to report the overflow, or one sized to exactly h * w)
    // keeps the one-launch form, in which every workgroup counts the pixels before its slab itself.
    if (slabs > 256 && (long)capacity >= (long)hw + ceil_div((long)slabs * 4, 64)) {
        slab_counts = reinterpret_cast<unsigned*>(static_cast<NmsCandidate*>(candidates) + hw);
        if constexpr (sizeof(T) == 4)
            hipLaunchKernelGGL(rroi_rbox_count_kernel, dim3(slabs), dim3(1024), 0, stream, segm, hw, segm_thresh, slab_counts);
        else
            hipLaunchKernelGGL(rroi_rbox_count_typed_kernel<T>, dim3(slabs), dim3(1024), 0, stream, segm, hw, segm_thresh,
                               slab_counts);
        const int st = launch_status();
        if (st != 1) return st;
    }
    if constexpr (sizeof(T) == 4)
        hipLaunchKernelGGL(rroi_rbox_decode_kernel, dim3(slabs), dim3(1024), 0, stream, segm, rbox, angle, height, width,
                           segm_thresh, static_cast<NmsCandidate*>(candidates), slab_counts ? hw : capacity, count, slab_counts);
    else
        hipLaunchKernelGGL(rroi_rbox_decode_typed_kernel<T>, dim3(slabs), dim3(1024), 0, stream, segm, rbox, angle, height,
                           width, segm_thresh, static_cast<NmsCandidate*>(candidates), slab_counts ? hw : capacity, count,
                           slab_counts);
    return launch_status();
}
