// rroi_host_launch.h -- host side, part 3 of 3: the launches.  Every launch_* runs the plan it is handed (rroi_host_plan.h) on
// the Shape that plan carries, so a launch cannot run on another shape than its plan.  Nothing here looks at the device or
// at the tuning table: every grid, block count and flag word is a field of the plan; what a launch derives itself is a
// pure function of the Shape (row pitch, layouts, memset sizes).  Each kernel template has ONE function that writes its
// argument list; runtime values become template arguments through with_dtype / with_flag / with_choice.  Plain templates
// over the element type T of the caller's tensors (float, bf16_t, fp16_t).  Included by rroi_align_hip.hip inside its
// anonymous namespace.
#pragma once

inline int status_of(hipError_t e) { return e == hipSuccess ? 1 : -(int)e; }
inline int launch_status() { return status_of(hipGetLastError()); }

// f(T{}) for the element type a `dtype` code names (dtype_ok(dtype) holds): the one place a code becomes a type.
template <class F>
auto with_dtype(int dtype, F&& f)
{
    return dtype == RROI_DTYPE_BF16 ? f(bf16_t{}) : dtype == RROI_DTYPE_FP16 ? f(fp16_t{}) : f(float{});
}
// f(std::true_type{}) or f(std::false_type{}): a runtime flag as a template argument
template <class F>
auto with_flag(bool flag, F&& f)
{
    return flag ? f(std::true_type{}) : f(std::false_type{});
}
template <int V>
using int_c = std::integral_constant<int, V>;
// f(int_c<V>{}) for the V that `v` equals; the last V stands for every other value
template <int V, int... Rest, class F>
auto with_choice(int v, F&& f)
{
    if constexpr (sizeof...(Rest) == 0) return f(int_c<V>{});
    else return v == V ? f(int_c<V>{}) : with_choice<Rest...>(v, f);
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

// ------------------------------------------------------------------------------------
// Forward.
// ------------------------------------------------------------------------------------
// rroi_fwd_patch_kernel<4, WITH_IDX, T, RAGGED> (K2p).  `out`: the crops, or RAGGED the crop table.
template <bool WITH_IDX, class T, bool RAGGED = false>
void launch_patch_kernel(const FwdDispatch& P, const T* features, const float* rois,
                         std::conditional_t<RAGGED, const CropRow*, T*> out, float* idx_x, float* idx_y, float spatial_scale,
                         hipStream_t stream)
{
    static_assert(!WITH_IDX || (std::is_same<T, float>::value && !RAGGED), "con_idx: the reference ABI's, fp32 calls only");
    const PatchPlan& p = P.patch;
    const Shape& S = P.shape;
    hipLaunchKernelGGL((rroi_fwd_patch_kernel<4, WITH_IDX, T, RAGGED>), p.grid, dim3(256), 0, stream, features, rois, out,
                       S.num_rois, S.channels, S.height, S.width, S.pooled_height, S.pooled_width, spatial_scale, P.trig,
                       P.direct_batch(), p.cw, p.npx, p.npatches, p.prows, p.pcols, idx_x, idx_y);
}

// rroi_fwd_split_kernel<VEC_STORE = true, EARLY, OCC, HID, ONHWC, SHIFT, NCHW_SRC, WAUX, TO, RAGGED>.  Its three callers
// differ in where the map is (`map`, `lay`), where the affines come from (`aff`; NCHW_SRC: `rsrc`), what `out` is (crops of
// TO; RAGGED: the crop table) and the XCD groups.
template <int EARLY, int OCC, int HID, bool ONHWC, int SHIFT, int WAUX, class TO, bool NCHW_SRC = false, bool RAGGED = false>
void launch_split_kernel(const FwdDispatch& P, const float* map, const SliceLayout& lay, const Affine* aff,
                         std::conditional_t<RAGGED, const CropRow*, TO*> out, XcdGroups xg, hipStream_t stream,
                         RoiSource rsrc = RoiSource{nullptr, 0, 0.0f, 0})
{
    static_assert(!NCHW_SRC || (std::is_same<TO, float>::value && !RAGGED), "the one-launch forms are fp32 only");
    const ForwardPlan& plan = P.gather;
    const Shape& S = P.shape;
    hipLaunchKernelGGL((rroi_fwd_split_kernel<true, EARLY, OCC, HID, ONHWC, SHIFT, NCHW_SRC, WAUX, TO, RAGGED>), dim3(plan.grid),
                       dim3(2 * kWave), 0, stream, map, aff, out, S.num_rois, S.channels, S.height, S.width, S.pooled_width,
                       S.NB(), S.batch_size, S.nchunks(), plan.ntiles, lay, make_fastdiv((unsigned)plan.ntiles),
                       make_fastdiv((unsigned)S.pooled_width), plan.dbg, xg, rsrc);
}

// The forward prologue launch (relayout to the chunk-major copy + affine table [+ ROI sort, + the launcher's rest blocks]):
// shared by the dense two-launch plan and the bucketed one (which runs it unchanged: one group, no launcher).
template <class T>
int launch_forward_prologue(const FwdDispatch& P, const Workspace& ws, const T* features, const float* rois, T* top_data,
                            float spatial_scale, hipStream_t stream)
{
    const Shape& S = P.shape;
    const ProloguePlan& p = P.prologue;
    float* rest_out = nullptr;   // (the launcher: fp32)
    if constexpr (std::is_same<T, float>::value) rest_out = P.launcher ? top_data : nullptr;
    // <0>: plain stores: the copy stays in the L2s that wrote it (write-through: 1.8 us faster alone, the step is not)
    hipLaunchKernelGGL((rroi_prologue_kernel<0, T>), dim3(p.grid()), dim3(256), 0, stream, features, ws.cm, S.channels, S.HW(),
                       S.width, row_pitch(S.width), make_fastdiv((unsigned)S.width), S.nchunks(), p.ptiles, p.relayout_blocks,
                       p.relayout_tiles, S.batch_size, rois, S.num_rois, S.pooled_height, spatial_scale, P.trig, ws.aff,
                       p.aff_blocks, rest_out, S.pooled_width, P.groups, ws.sort_rank, ws.sort_order);
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
    switch (P.family) {
    case RROI_PLAN_NONE:
        return 1;
    case RROI_PLAN_FWD_DIRECT_K2P:
        if (!(stages & RROI_STAGE_GATHER)) return 1;  // the direct path has no prologue
        if constexpr (kF32) {
            if (P.con_idx && idx_x) {
                launch_patch_kernel<true>(P, features, rois, top_data, idx_x, idx_y, spatial_scale, stream);
                return launch_status();
            }
        }
        launch_patch_kernel<false>(P, features, rois, top_data, nullptr, nullptr, spatial_scale, stream);
        return launch_status();
    case RROI_PLAN_FWD_DIRECT_THREAD:
        if (!(stages & RROI_STAGE_GATHER)) return 1;
        hipLaunchKernelGGL(rroi_fwd_direct_kernel<T>, P.dgrid, dim3(256), 0, stream, features, rois, top_data,
                           P.con_idx ? idx_x : nullptr, P.con_idx ? idx_y : nullptr, S.num_rois, S.channels, S.height, S.width,
                           S.pooled_height, S.pooled_width, spatial_scale, P.trig, P.direct_batch(), P.cslab);
        return launch_status();
    case RROI_PLAN_FWD_FUSED_STRIDED:
    case RROI_PLAN_FWD_FUSED_SHIFT:
        if constexpr (!kF32) {   // (fp32 only: no 16-bit plan)
            return 0;
        } else {
            if (!(stages & RROI_STAGE_GATHER)) return 1;  // one launch, run under the gather stage
            const RoiSource rsrc = {rois, S.pooled_height, spatial_scale, P.trig};
            with_flag(P.family == RROI_PLAN_FWD_FUSED_SHIFT, [&](auto shift) {
                launch_split_kernel<0, 4, 3, false, decltype(shift)::value ? 1 : 0, -1, float, true>(
                    P, features, nchw_src_layout(S), nullptr, top_data, XcdGroups{1, nullptr}, stream, rsrc);
            });
            return launch_status();
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

    // prologue: relayout + affine table in one launch
    if (stages & RROI_STAGE_PROLOGUE) {
        const int st = launch_forward_prologue(P, ws, features, rois, top_data, spatial_scale, stream);
        if (st != 1) return st;
    }
    if (stages & RROI_STAGE_GATHER) {
        const SliceLayout lay = zero_copy ? zero_copy_layout(S) : chunk_major_layout(S);
        const XcdGroups xg{P.groups, ws.sort_order};
        // the shipped instantiations <EARLY, OCC, HID, ONHWC, SHIFT, WAUX, T>, one per FwdKernel and element type
        switch (P.gather.kernel) {
        case FwdKernel::kStrided:       launch_split_kernel<0, 6, 3, false, 0, -1, T>(P, map, lay, ws.aff, top_data, xg, stream); break;   // 62-64 VGPRs, 12.1 KB of LDS: 12 per CU
        case FwdKernel::kChannelsLast:  launch_split_kernel<2, 5, 2, true, 0, -1, T>(P, map, lay, ws.aff, top_data, xg, stream); break;    // 91 VGPRs: 10 per CU
        case FwdKernel::kShift:         launch_split_kernel<0, 6, 3, false, 1, -1, T>(P, map, lay, ws.aff, top_data, xg, stream); break;   // 79 VGPRs, 12.4 KB of LDS: 12 per CU
        case FwdKernel::kStridedMerge:  launch_split_kernel<0, 6, 3, false, 0, 0, T>(P, map, lay, ws.aff, top_data, xg, stream); break;    // plain stores (write-through: 32.1 against 30.1 us)
        case FwdKernel::kShiftLines:    launch_split_kernel<0, 5, 3, false, 2, -1, T>(P, map, lay, ws.aff, top_data, xg, stream); break;   // 84 VGPRs, 14.8 KB of LDS: 10 per CU
        case FwdKernel::kStridedRagged: return 0;   // (launch_forward_bucketed's own)
        }
    }
    return launch_status();
}

template <class T>
int launch_forward_bucketed(const FwdDispatch& P, const T* features, const float* rois, const CropRow* crops,
                            float spatial_scale, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    const Shape& S = P.shape;   // (pooled_width: the call's largest)
    if (P.family == RROI_PLAN_FWD_DIRECT_K2P) {
        launch_patch_kernel<false, T, true>(P, features, rois, crops, nullptr, nullptr, spatial_scale, stream);
        return launch_status();
    }
    if (P.family != RROI_PLAN_FWD_TWO_LAUNCH) return 0;
    const Workspace ws = carve(workspace, S, RROI_LAYOUT_NCHW);
    if (!workspace_ok(workspace) || workspace_bytes < ws.bytes) return 0;
    const int st = launch_forward_prologue(P, ws, features, rois, (T*)nullptr, spatial_scale, stream);
    if (st != 1) return st;
    launch_split_kernel<0, 6, 3, false, 0, -1, T, false, true>(P, ws.cm, chunk_major_layout(S), ws.aff, crops,
                                                               XcdGroups{1, nullptr}, stream);
    return launch_status();
}

// ------------------------------------------------------------------------------------
// Backward.
// ------------------------------------------------------------------------------------
// What the launches of one tiled backward call share, and one method per kernel template they run.
template <class T>
struct BwdLaunch {
    static constexpr bool kF32 = std::is_same<T, float>::value;
    const BwdDispatch& P;
    const Shape& S;
    BwdWorkspace ws;          // the caller's workspace, carved
    ListAddressing A;
    const float* srcT;        // where the gather reads top_diff: the relaid-out fp32 copy, or an fp32 channels-last top_diff in place
    const T* top_diff;        // the gradient crops, or ...
    const CropRow* ragged;    // ... the bucketed call: their table (top_diff is NULL)
    T* bottom_diff;
    hipStream_t stream;

    // bucket lists: the chains' heads in `off`, the overflow counter in `bsum`
    BucketLists bucket_lists() const { return {ws.kshift, reinterpret_cast<int*>(ws.off), ws.bsum, ws.ov}; }
    FastDiv div_key_tiles() const { return make_fastdiv(ws.keys.Ht * ws.keys.Wt); }

    // rroi_bwd_pairs_relayout_kernel<MODE, kBwdRelayoutAux, T, RAGGED>: `pair_blocks` pair blocks (MODE 0 count, 1 fill,
    // 2 buckets) in front of `blocks` blocks that relay out the tiles [tile_begin, tile_end) of top_diff
    template <int MODE>
    void pairs_relayout(int pair_blocks, int tt, long blocks, long tile_begin, long tile_end, int raw_bsum, const BucketLists& bl,
                        int flags) const
    {
        auto run = [&](auto is_ragged, auto src) {
            hipLaunchKernelGGL((rroi_bwd_pairs_relayout_kernel<MODE, kBwdRelayoutAux, T, decltype(is_ragged)::value>),
                               dim3((unsigned)(pair_blocks + blocks)), dim3(256), 0, stream, ws.aff, S.num_rois, S.height, S.width,
                               S.pooled_width, S.NB(), S.batch_size, A.lines_per_roi, A.dnb, A.dpw, ws.keys, ws.cnt, ws.off,
                               ws.bsum, ws.pairs, pair_blocks, src, ws.tdT, S.channels, S.nchunks(), tt, (int)blocks,
                               (int)tile_begin, (int)tile_end, ws.scan_blocks, raw_bsum, bl, flags);
        };
        if (ragged) run(std::true_type{}, ragged);
        else run(std::false_type{}, top_diff);
    }

    // rroi_bwd_tile_gather_kernel<NK, NHWC, TO>.  NHWC: the caller's bottom_diff in place (its type); else the fp32
    // chunk-major scratch.  A 16-bit call has no eight-chunk instantiation (plan_backward: nk <= 4).
    void tile_gather() const
    {
        auto run = [&](auto nk, auto nhwc) {
            constexpr bool kNhwc = decltype(nhwc)::value;
            typedef std::conditional_t<kNhwc, T, float> TO;
            TO* dst;
            if constexpr (kNhwc) dst = bottom_diff;
            else dst = ws.gcm;
            hipLaunchKernelGGL((rroi_bwd_tile_gather_kernel<decltype(nk)::value, kNhwc, TO>), P.grid, dim3(kTgThreads), 0, stream,
                               srcT, ws.aff, dst, S.num_rois, S.channels, S.height, S.width, row_pitch(S.width), S.pooled_height,
                               S.pooled_width, S.batch_size, S.nchunks(), A.chunk_stride, A.line_stride, A.lines_per_roi, ws.keys,
                               ws.keys.keys / 32u, P.grid.x / 8u, div_key_tiles(), make_fastdiv(ws.keys.Wt),
                               make_fastdiv((unsigned)S.pooled_height));
        };
        with_flag(P.dest == RROI_PLAN_DST_NHWC, [&](auto nhwc) {
            if constexpr (kF32) with_choice<8, 4, 2, 1>(P.inkernel.nk, [&](auto nk) { run(nk, nhwc); });
            else with_choice<4, 2, 1>(P.inkernel.nk, [&](auto nk) { run(nk, nhwc); });
        });
    }

    // rroi_bwd_gather_kernel<DST, BUCKET, TO>: the lists are count / scan / fill segments (`off` = scanned offsets) or
    // buckets (`off` = the counters).  kDstNchwAdd (the launcher's) is fp32 only.
    void list_gather() const
    {
        const bool buckets = P.family == RROI_PLAN_BWD_BUCKETS;
        const unsigned* loff = buckets ? reinterpret_cast<const unsigned*>(ws.cnt) : ws.off;
        with_flag(buckets, [&](auto buck) {
            auto run = [&](auto dstk, auto* dst) {
                hipLaunchKernelGGL((rroi_bwd_gather_kernel<decltype(dstk)::value, decltype(buck)::value, std::remove_pointer_t<decltype(dst)>>),
                                   P.grid, dim3(256), 0, stream, srcT, loff, ws.bsum, ws.pairs, dst, S.channels, S.height, S.width,
                                   row_pitch(S.width), S.nchunks(), A.chunk_stride, A.line_stride, P.lists.sub_shift, ws.keys,
                                   div_key_tiles(), make_fastdiv(ws.keys.Wt), ws.scan_blocks, P.lists.raw_bsum, bucket_lists(),
                                   P.lists.tile_run);
            };
            switch (P.dest) {
            case RROI_PLAN_DST_NHWC: run(int_c<kDstNhwc>{}, bottom_diff); break;
            case RROI_PLAN_DST_NCHW: run(int_c<kDstNchw>{}, bottom_diff); break;
            case RROI_PLAN_DST_NCHW_ADD: if constexpr (kF32) run(int_c<kDstNchwAdd>{}, bottom_diff); break;
            default: run(int_c<kDstChunkMajor>{}, ws.gcm); break;
            }
        });
    }

    // rroi_bwd_ordered_gather_kernel<kDstNhwc | kDstNchw, T>: in place, in either layout
    void ordered_gather() const
    {
        with_flag(P.dest == RROI_PLAN_DST_NHWC, [&](auto nhwc) {
            constexpr int kDst = decltype(nhwc)::value ? kDstNhwc : kDstNchw;
            hipLaunchKernelGGL((rroi_bwd_ordered_gather_kernel<kDst, T>), P.grid, dim3(256), 0, stream, srcT, ws.off, ws.bsum,
                               ws.pairs, bottom_diff, S.channels, S.height, S.width, S.nchunks(), A.chunk_stride, A.line_stride,
                               P.lists.sub_shift, ws.keys, div_key_tiles(), make_fastdiv(ws.keys.Wt), ws.scan_blocks,
                               P.lists.raw_bsum, P.lists.tile_run);
        });
    }

    // rroi_cm_to_nchw_kernel<ACCUM, T>: the chunk-major scratch to the caller's NCHW bottom_diff (= ; the launcher, fp32: +=)
    void cm_to_nchw() const
    {
        const int ptiles = ceil_div((long)S.HW(), kRelayoutPx);
        with_flag(P.accumulate, [&](auto accum) {
            if constexpr (!decltype(accum)::value || kF32)
                hipLaunchKernelGGL((rroi_cm_to_nchw_kernel<decltype(accum)::value, T>), dim3(ptiles * S.nchunks() * S.batch_size),
                                   dim3(256), 0, stream, ws.gcm, bottom_diff, S.channels, S.HW(), S.width, row_pitch(S.width),
                                   make_fastdiv((unsigned)S.width), S.nchunks(), ptiles);
        });
    }
};

// K3t: relayout of top_diff (one launch, masked bins skipped), then the tile gather
template <class T>
int launch_bwd_inkernel(const BwdLaunch<T>& c)
{
    const BwdDispatch::InKernel& K = c.P.inkernel;
    if (!c.P.td_nhwc) {
        c.template pairs_relayout<0>(0, K.tt, K.relayout_blocks, 0, K.tiles, 0, BucketLists{0u, nullptr, nullptr, nullptr}, K.flags);
        const int st = launch_status();
        if (st != 1) return st;
    }
    c.tile_gather();
    return launch_status();
}

// K3g: the pixel -> (bin, weight) lists in HBM, then a gather that walks them
template <class T>
int launch_bwd_lists(const BwdLaunch<T>& c)
{
    const BwdDispatch::Lists& L = c.P.lists;
    const BwdWorkspace& ws = c.ws;
    const BucketLists bl = c.bucket_lists();
    // (1) the lists
    if (c.P.family == RROI_PLAN_BWD_BUCKETS) {
        // ONE launch: every pair into its pixel's bucket (or overflow chain) || the whole relayout
        c.template pairs_relayout<2>(L.pblocks, L.tt, L.bucket_blocks, 0, L.tiles, L.raw_bsum, bl, L.flags);
    } else {
        // count || first half of the relayout;  scan;  fill || second half
        c.template pairs_relayout<0>(L.pblocks, L.tt, L.count_blocks, 0, L.half, L.raw_bsum, bl, L.flags);
        hipLaunchKernelGGL(rroi_scan1_kernel, dim3(ws.scan_blocks), dim3(1024), 0, c.stream, ws.cnt, ws.off, ws.bsum,
                           ws.keys.keys);
        if (!L.raw_bsum) hipLaunchKernelGGL(rroi_scan2_kernel, dim3(1), dim3(1024), 0, c.stream, ws.bsum, ws.scan_blocks);
        c.template pairs_relayout<1>(L.pblocks, L.tt, L.fill_blocks, L.half, L.tiles, L.raw_bsum, bl, L.flags);
    }
    const int st = launch_status();
    if (st != 1) return st;
    // (2) gather: one thread group per key, no grid-stride
    if (c.P.family != RROI_PLAN_BWD_ORDERED) {
        c.list_gather();
        return launch_status();
    }
    // (2b) every list in bin order: the short ones in registers, the rest queued in the counters (which the
    // fill left at zero) for one workgroup each; then the in-order fp64 gather, in place
    unsigned* const queue = reinterpret_cast<unsigned*>(ws.cnt);
    hipLaunchKernelGGL(rroi_bwd_sort_lists_kernel, dim3(L.sort_lists_blocks), dim3(256), 0, c.stream, ws.off, ws.bsum, ws.pairs,
                       ws.keys.keys, ws.scan_blocks, L.raw_bsum, queue);
    hipLaunchKernelGGL(rroi_bwd_sort_queue_kernel, dim3(L.sort_queue_blocks), dim3(kSortQueueThreads), 0, c.stream, ws.off,
                       ws.bsum, ws.pairs, queue, ws.scan_blocks, L.raw_bsum);
    c.ordered_gather();
    return launch_status();
}

// rroi_bwd_tiled_kernel<VEC_LOAD>: the atomic scatter into the zeroed chunk-major scratch.  fp32 atomics: there is no 16-bit
// plan, and launch_backward has refused one
template <class T>
int launch_bwd_atomic(const BwdLaunch<T>& c)
{
    const Shape& S = c.S;
    const int pitch = row_pitch(S.width), ntiles = c.P.atomic.ntiles;
    const hipError_t e = hipMemsetAsync(c.ws.gcm, 0, (size_t)S.batch_size * S.nchunks() * S.height * pitch * kLineBytes, c.stream);
    if (e != hipSuccess) return status_of(e);
    if constexpr (BwdLaunch<T>::kF32)
        with_flag(c.P.atomic.vec4, [&](auto vec4) {
            hipLaunchKernelGGL(rroi_bwd_tiled_kernel<decltype(vec4)::value>, c.P.grid, dim3(kWave), 0, c.stream, c.top_diff,
                               c.ws.aff, c.ws.gcm, S.num_rois, S.channels, S.height, S.width, pitch, S.pooled_width, S.NB(),
                               S.batch_size, S.nchunks(), ntiles, make_fastdiv((unsigned)ntiles),
                               make_fastdiv((unsigned)S.pooled_width));
        });
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
    const size_t in_bytes = (size_t)S.batch_size * S.channels * (size_t)S.HW() * sizeof(T);
    const bool td_nhwc = P.td_nhwc, accumulate = P.accumulate;
    switch (P.family) {
    case RROI_PLAN_NONE:
        return accumulate ? 1 : status_of(hipMemsetAsync(bottom_diff, 0, in_bytes, stream));
    case RROI_PLAN_BWD_DIRECT:
        if constexpr (!kF32) {   // (fp32 atomics: no 16-bit plan)
            return 0;
        } else {
            const hipError_t e = hipMemsetAsync(bottom_diff, 0, in_bytes, stream);
            if (e != hipSuccess) return status_of(e);
            hipLaunchKernelGGL(rroi_bwd_direct_kernel, P.grid, dim3(256), 0, stream, top_diff, rois, bottom_diff, S.num_rois,
                               S.channels, S.height, S.width, S.pooled_height, S.pooled_width, spatial_scale, P.trig,
                               S.batch_size, P.direct.cslab);
            return launch_status();
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

    const bool buckets = P.family == RROI_PLAN_BWD_BUCKETS;
    const bool lists = buckets || P.family == RROI_PLAN_BWD_ORDERED || P.family == RROI_PLAN_BWD_LISTS;
    BwdLaunch<T> c{P, S, carve_bwd(workspace, S), list_addressing(S, td_nhwc), nullptr, top_diff, ragged, bottom_diff, stream};
    const BwdWorkspace& ws = c.ws;
    if (!workspace_ok(workspace) || workspace_bytes < ws.bytes) return 0;
    if (!kF32 && (P.family == RROI_PLAN_BWD_ATOMIC || td_nhwc || accumulate)) return 0;
    if (ragged && (td_nhwc || accumulate || !lists)) return 0;
    c.srcT = ws.tdT;
    if constexpr (kF32) c.srcT = td_nhwc ? top_diff : ws.tdT;

    // affine table; the list passes' pixel counters (K3g) are cleared by the same launch
    const BucketLists bl = c.bucket_lists();
    hipLaunchKernelGGL(rroi_affine_kernel, dim3(P.affine_blocks), dim3(256), 0, stream, rois, S.num_rois, S.pooled_height,
                       spatial_scale, P.trig, ws.aff, ws.cnt, lists ? ws.keys.keys : 0u, buckets ? bl.head : (int*)nullptr,
                       buckets ? bl.ovcnt : (unsigned*)nullptr);
    int st = launch_status();
    if (st != 1) return st;
    st = P.family == RROI_PLAN_BWD_INKERNEL ? launch_bwd_inkernel(c) : lists ? launch_bwd_lists(c) : launch_bwd_atomic(c);
    // (a gradient written in place needs no relayout back)
    if (st != 1 || P.dest != RROI_PLAN_DST_CHUNK_MAJOR) return st;
    c.cm_to_nchw();
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
