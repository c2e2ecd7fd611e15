/*
 * include/rroi_align_hip.h -- C-ABI of librroi_align_hip.so, the MI355X (gfx950)
 * implementation of the RoIRotate / rroi_align hot path of FOTS.pytorch.
 *
 * Plain pointers and sizes only; no torch types.  Every device pointer is
 * borrowed for the duration of the asynchronous launch; the library never
 * allocates, frees or synchronises.  `stream` is a hipStream_t passed as
 * void* (NULL = the null stream).  All citations below are relative to the
 * reference checkout (chenjun2hao/FOTS.pytorch).
 *
 * Return convention (extends rroi_align/src/rroi_align_cuda.c:23-26,43 and
 * rroi_align_kernel.cu:186): 1 = success, 0 = invalid argument, negative =
 * -(hipError_t) of a failed launch.  The reference's launchers call exit(-1)
 * on a launch error (kernel.cu:179-184); this library never exits.
 */
#ifndef RROI_ALIGN_HIP_H
#define RROI_ALIGN_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * 1. The reference's own launcher ABI, symbol for symbol.
 *    Replaces rroi_align/src/rroi_align_kernel.h:8-18 (implemented in the
 *    reference by rroi_align_kernel.cu:164-187 and :280-312), so the
 *    reference's glue rroi_align/src/rroi_align_cuda.c:37-41,80-84 links
 *    against this library unchanged (cudaStream_t -> hipStream_t as void*).
 *
 *    bottom_data : (B, C, H, W) fp32, contiguous NCHW
 *    bottom_rois : (R, 6) fp32 rows [batch_idx, cx, cy, h, w, angle_deg]
 *    top_data, con_idx_x, con_idx_y : (R, C, PH, PW) fp32.  Every element is
 *        written (zeros where the reference leaves its memset untouched), so
 *        the buffers need not be zeroed first; con_idx_* may be NULL.
 * ------------------------------------------------------------------------- */
int RROIAlignForwardLaucher(const float* bottom_data, const float spatial_scale,
                            const int num_rois, const int height, const int width,
                            const int channels, const int pooled_height, const int pooled_width,
                            const float* bottom_rois, float* top_data, float* con_idx_x,
                            float* con_idx_y, void* stream);

/*  top_diff : (R, C, PH, PW) fp32;  bottom_diff : (B, C, H, W) fp32: the gradient is
 *  ADDED to it, whatever the problem size, as the reference's atomicAdds do -- zero it
 *  first for the plain gradient (functions/rroi_align.py:35 does);
 *  con_idx_x/y : the tensors the forward wrote (read per element, as
 *  kernel.cu:232-233 does). */
int RROIAlignBackwardLaucher(const float* top_diff, const float spatial_scale,
                             const int batch_size, const int num_rois, const int height,
                             const int width, const int channels, const int pooled_height,
                             const int pooled_width, const float* bottom_rois,
                             float* bottom_diff, const float* con_idx_x, const float* con_idx_y,
                             void* stream);

/* The two launchers above carry no workspace argument: the library keeps one scratch buffer per (device, stream),
 * grown on demand and reused by later calls on that stream (no allocation per call; a call whose buffer exists only
 * enqueues kernels and can be captured into a HIP graph).  Calls on different streams do not serialise each other.
 * Lifetime: a buffer handed out while its stream was CAPTURING is part of that graph and from then on GRAPH-EXCLUSIVE:
 * never freed afterwards, never handed out again -- later eager calls on the stream get a buffer of their own, later
 * captures take stream-ordered memory their own graph owns -- so a captured launcher call stays replayable for the
 * life of the process, on any stream, concurrently with eager calls (replays of ONE graph must of course be ordered
 * among themselves, as for any graph that writes its own scratch).  To capture with memory the GRAPH owns from the
 * start, capture the first call on a stream that has no buffer yet (or one that is too small): that call allocates
 * inside the capture.  Further launcher calls inside the SAME capture reuse the buffer that capture pinned when it is
 * large enough (0.8.0; before, each took stream-ordered memory of its own).
 * Limits: the table has 64 entries; a pinned buffer keeps its entry for the life of the process, an unpinned one is
 * evicted least-recently-used first.  With every entry pinned (64 captures on 64 streams) a call that finds nothing
 * cached takes stream-ordered memory for that call alone (hipMallocAsync / hipFreeAsync around its launches): correct,
 * slower, and not silent -- rroi_align_launcher_scratch_stats() reports the table's state.
 * A thread that waits for another thread's enqueue on the SAME (device, stream) entry does so without the table lock:
 * calls on different streams never serialise each other.
 * This frees every buffer no graph holds (synchronously); they are re-created on demand.
 * Returns 1 / -hipError. */
int rroi_align_release_launcher_scratch(void);
/* State of the launcher scratch table: *in_use = entries that hold a buffer, *pinned = those a graph owns,
 * *capacity = 64, *transient_calls = launcher calls served by stream-ordered memory of their own so far (no entry to
 * cache in, or a capture that found no buffer large enough).  Any pointer may be NULL.  Returns 1. */
int rroi_align_launcher_scratch_stats(int* in_use, int* pinned, int* capacity, unsigned long long* transient_calls);

/* ------------------------------------------------------------------------- *
 * 2. The MI355X-native entry points used by the Python surface
 *    (rroi_align.functions.rroi_align.RRoiAlignFunction, replacing
 *    rroi_align/functions/rroi_align.py:13-40).  No con_idx tensors: the bin
 *    centres are a pure function of the rois and are recomputed in backward.
 * ------------------------------------------------------------------------- */

/* feature_layout */
#define RROI_LAYOUT_NCHW 0 /* (B, C, H, W) contiguous -- the reference contract */
#define RROI_LAYOUT_NHWC 1 /* (B, H, W, C) contiguous (torch channels_last storage) */

/* path */
#define RROI_PATH_AUTO 0   /* pick by problem size                                  */
#define RROI_PATH_DIRECT 1 /* one kernel, NCHW gather, no workspace (small R)       */
#define RROI_PATH_TILED 2  /* relayout to pixel-major + wave-tiled gather (large R) */
#define RROI_PATH_TILED_ATOMIC 3 /* backward only: the tiled scatter with fp32 atomics (the
                                    default tiled backward is an atomic-free gather)         */
#define RROI_PATH_TILED_LISTS 4  /* backward only: the gather over per-pixel lists built in HBM by
                                    count / scan / fill launches.  AUTO / TILED fall back to it where
                                    the memory cap leaves a bucket below the mean list, unless the
                                    in-kernel gather's rule (below) takes the problem         */
#define RROI_PATH_TILED_BUCKETS 6 /* backward only (round 3): the gather over per-pixel lists built in ONE pass --
                                    fixed-capacity buckets per pixel plus overflow chains: no count pass, no
                                    scan.  What AUTO / TILED run (the bucket grows with the density, 16 ..
                                    4096 entries, under a memory cap); any density is accepted when named    */
#define RROI_PATH_FUSED 7   /* forward only (round 5): ONE launch for few ROIs -- the tiled gather reading the NCHW map
                                    itself (four dword loads per tap instead of one 16-byte load from a relaid-out copy)
                                    and evaluating the affines itself: no prologue launch, no workspace (NULL / 0 is
                                    accepted).  NCHW features and crops only.  What AUTO runs between the direct kernel
                                    (a handful of ROIs) and the two-launch path                                     */
#define RROI_PATH_TILED_INKERNEL 5 /* backward only: the gather that finds each map tile's bins
                                    inside the kernel, no lists in HBM.  Round 2's choice for C <= 64;
                                    since round 3 AUTO / TILED reach it only where the buckets are not
                                    to be had (capped below the mean list, or 32-bit bucket indices
                                    exceeded) AND its own rule holds: at most two channel chunks per
                                    lane, or four with <= 8 bins per map pixel, or eight with <= 1, and
                                    R x B <= 8192.  Named, it runs wherever its 32-bit offsets hold   */

/* path flags (OR into `path`; round 5).
 * RROI_PATH_TRIG_FP32: the one library-dependent step of the arithmetic (rroi_align_kernel.cu:73-74, `cos(angle)` /
 * `sin(angle)` of a float) for THIS call.  Default (bit clear) = RROI_TRIG_DOUBLE: (float)cos((double)angle), the
 * recipe of the oracle -- bit-exact against it and against the reference's sources evaluated with a correctly rounded
 * cosine.  Bit set = RROI_TRIG_FP32: cosf / sinf of the device library, what the reference's own sources call when they
 * are built for this GPU -- bit-exact, every bin, against that build (oracle/_ref/librroi_ref_hip_nofma.so).  The two
 * differ in 15-17 bins per million, at rounding ties.  The recipe is a kernel argument: stream-ordered, capturable
 * into a HIP graph, independent per call -- pass the SAME bit to the backward of a forward (the Python surface keeps
 * it in the autograd context).  Rounds 3-4 had a per-device setter (rroi_align_set_trig_recipe_hip): removed in 0.7.0.
 * The reference-ABI launchers of section 1 have no `path`: they use RROI_TRIG_DOUBLE, or RROI_TRIG_FP32 when the
 * process was started with RROI_ALIGN_LAUNCHER_TRIG=fp32 in its environment (read once, at the first launcher call). */
#define RROI_PATH_TRIG_FP32 0x100
#define RROI_TRIG_DOUBLE 0
#define RROI_TRIG_FP32 1
/* The recipe the reference-ABI launchers run in this process (RROI_TRIG_DOUBLE / RROI_TRIG_FP32): the environment is
 * read once per process, by whichever comes first -- this call or the first launcher call -- so the answer is what every
 * launcher call of the process uses.  For a caller that computes a launcher call's gradient through the native entry
 * points (the Python glue under torch.use_deterministic_algorithms). */
int rroi_align_launcher_trig_recipe(void);
/* RROI_PATH_DETERMINISTIC (backward): the ORDERED plan, a gradient that does not change from run to run.
 * Every feature-gradient element (b, c, y, x) is the sum of the fp32 products w * g that reach it, added in DOUBLE from
 * +0.0 in statement order -- ROI n, pooled row ph, pooled column pw, tap lt / rt / rb / lb -- and rounded to fp32 once:
 * what the oracle's rroi_oracle_backward computes, bit for bit (NaN where it has NaN), whatever the layouts, the grid,
 * the CU count, the stream or a graph capture.  Masks and aliases are the reference's (kernel.cu:267-274, and the extra
 * 0 * g of two taps on one pixel).  A 16-bit call rounds that fp32 gradient of the widened top_diff once to its type.
 * Accepted with RROI_PATH_AUTO (| RROI_PATH_TRIG_FP32) from the native backward entry points and their plan queries,
 * every dtype and layout pair, wherever the call without the bit is accepted and the gather's 32-bit indices hold (the
 * rule 16-bit calls follow): plan RROI_PLAN_BWD_ORDERED for R >= 1, the zero fill for R = 0.  Refused (0) with an
 * explicit path and by RROI_CALLER_LAUNCHER; a 0.10.0 library refuses the bit itself, which is how a caller detects it.
 * The workspace is rroi_align_backward_workspace_bytes' (the exact lists' storage).  RROIAlignBackwardLaucher has no
 * `path`: it stays the reference's non-deterministic scatter order.
 * The forward needs no such flag: it writes every crop element once, with no atomics in its arithmetic (its ROI sort
 * only picks the workgroup that serves a ROI), so every forward plan is deterministic already.  The forward entry
 * points and rroi_align_forward_plan* keep refusing the bit as an unknown flag, as 0.10.0 did. */
#define RROI_PATH_DETERMINISTIC 0x200

/* Bytes of scratch the tiled path needs for this problem (0 for the direct
 * path).  The caller owns the scratch; its contents are dead after the call.
 * The workspace pointer must be a multiple of 256 bytes -- every sub-array the library carves out of it sits at an
 * offset rounded up to 256 -- and a plan that uses the workspace returns 0, before any launch, for one that is not
 * (as for NULL or fewer bytes than these queries report).  Beyond that the base address is free: the backward's size
 * already includes the two roundings to 4 KiB of the address it makes, whatever the base is.  A call writes nothing
 * outside [workspace, workspace + the queried bytes), whatever larger size it is told, and reads nothing of what the
 * workspace held before the call: it need not be cleared, and may hold anything.  The plans that take no workspace
 * (RROI_PATH_DIRECT, RROI_PATH_FUSED) accept any pointer and size, NULL / 0 included, and touch none of it. */
size_t rroi_align_forward_workspace_bytes(int batch_size, int channels, int height, int width,
                                          int num_rois, int feature_layout);
size_t rroi_align_backward_workspace_bytes(int batch_size, int channels, int height, int width,
                                           int num_rois, int pooled_height, int pooled_width);

/* Forward.  top_data (R, C, PH, PW) is fully written.  rois whose batch index
 * falls outside [0, batch_size) produce zeros (the reference reads out of
 * bounds there).  Returns 1 / 0 / -hipError. */
int rroi_align_forward_hip(const float* features, int feature_layout, float spatial_scale,
                           int batch_size, int num_rois, int height, int width, int channels,
                           int pooled_height, int pooled_width, const float* rois,
                           float* top_data, void* workspace, size_t workspace_bytes, int path,
                           void* stream);

/* The same with the layout of the crops stated: RROI_LAYOUT_NCHW (R, C, PH, PW) -- the reference
 * contract, what rroi_align_forward_hip writes -- or RROI_LAYOUT_NHWC = torch channels_last
 * storage (R, PH, PW, C), for a recognition head that runs in channels_last (MIOpen's preferred
 * layout): the first convolution then needs no 256 MiB relayout of its input.  Same values,
 * element for element.  Needs C % 4 == 0; tiled path only. */
int rroi_align_forward_layout_hip(const float* features, int feature_layout, int top_layout,
                                  float spatial_scale, int batch_size, int num_rois, int height,
                                  int width, int channels, int pooled_height, int pooled_width,
                                  const float* rois, float* top_data, void* workspace,
                                  size_t workspace_bytes, int path, void* stream);

/* The same call split into its launches, so a harness can bracket each kernel
 * with events on `stream`: RROI_STAGE_PROLOGUE = relayout + affine table,
 * RROI_STAGE_GATHER = the gather/blend/stream-out kernel (needs the workspace a
 * PROLOGUE call on the same arguments filled).  The direct path has one kernel,
 * run under RROI_STAGE_GATHER. */
#define RROI_STAGE_PROLOGUE 1
#define RROI_STAGE_GATHER 2
#define RROI_STAGE_ALL 3
int rroi_align_forward_stages_hip(const float* features, int feature_layout, float spatial_scale,
                                  int batch_size, int num_rois, int height, int width,
                                  int channels, int pooled_height, int pooled_width,
                                  const float* rois, float* top_data, void* workspace,
                                  size_t workspace_bytes, int path, int stages, void* stream);

/* Backward w.r.t. the features (kernel.cu:193-278 semantics, including its
 * asymmetric border tests :267-274).  bottom_diff (B, C, H, W) NCHW is fully
 * overwritten; it does not have to be zeroed. */
int rroi_align_backward_hip(const float* top_diff, float spatial_scale, int batch_size,
                            int num_rois, int height, int width, int channels,
                            int pooled_height, int pooled_width, const float* rois,
                            float* bottom_diff, void* workspace, size_t workspace_bytes, int path,
                            void* stream);

/* The same with the layouts stated.  top_diff_layout: RROI_LAYOUT_NCHW (R, C, PH, PW) as above, or
 * RROI_LAYOUT_NHWC = torch channels_last storage (R, PH, PW, C) -- what autograd hands over when
 * the recognition head runs in channels_last -- which the gather formulation consumes in place (no
 * relayout pass).  bottom_diff_layout: NCHW (B, C, H, W) as above, or NHWC storage (B, H, W, C),
 * written directly (no relayout back) for a channels_last backbone.  Either NHWC needs
 * C % 4 == 0 and path AUTO, TILED, TILED_LISTS, TILED_BUCKETS or TILED_INKERNEL. */
int rroi_align_backward_layout_hip(const float* top_diff, int top_diff_layout, int bottom_diff_layout,
                                   float spatial_scale, int batch_size, int num_rois, int height,
                                   int width, int channels, int pooled_height, int pooled_width,
                                   const float* rois, float* bottom_diff, void* workspace,
                                   size_t workspace_bytes, int path, void* stream);

/* Plan query (0.9.0): what a call with these arguments WOULD launch -- host only: it launches nothing, touches no
 * memory and needs no GPU (grids are sized for the current device's CU count, 256 where there is none).  The launches
 * above run the same plan (one decision function per direction), so the answer cannot disagree with what runs.
 * Arguments: those of rroi_align_forward_layout_hip / rroi_align_backward_layout_hip (path with its flag bits), and
 * `caller`: RROI_CALLER_NATIVE = those entry points; RROI_CALLER_LAUNCHER = RROIAlignForwardLaucher with con_idx NULL
 * / RROIAlignBackwardLaucher; RROI_CALLER_LAUNCHER_CON_IDX = RROIAlignForwardLaucher with con_idx (forward only).  A
 * launcher call has NCHW layouts and path RROI_PATH_AUTO (| RROI_PATH_TRIG_FP32); the forward launcher ignores
 * batch_size (its signature has none).  Returns 1 and fills *plan, or 0 exactly where the call would refuse its
 * (non-pointer) arguments -- a workspace of the queried size assumed. */
#define RROI_CALLER_NATIVE 0
#define RROI_CALLER_LAUNCHER 1
#define RROI_CALLER_LAUNCHER_CON_IDX 2
/* plan.family */
#define RROI_PLAN_NONE 0              /* no ROI: nothing launched (the native backward zeroes bottom_diff) */
#define RROI_PLAN_FWD_DIRECT_K2P 1    /* rroi_fwd_patch_kernel                                            */
#define RROI_PLAN_FWD_DIRECT_THREAD 2 /* rroi_fwd_direct_kernel, thread per bin (K2p does not apply)      */
#define RROI_PLAN_FWD_FUSED_STRIDED 3 /* one launch from the NCHW map, strided tiles                      */
#define RROI_PLAN_FWD_FUSED_SHIFT 4   /* one launch from the NCHW map, SHIFT tiles                        */
#define RROI_PLAN_FWD_TWO_LAUNCH 5    /* prologue (relayout + affines) + the gather of plan.kernel        */
#define RROI_PLAN_BWD_DIRECT 11       /* rroi_bwd_direct_kernel, atomics into NCHW                        */
#define RROI_PLAN_BWD_ATOMIC 12       /* rroi_bwd_tiled_kernel<plan.vec4>, atomics into the chunk-major copy */
#define RROI_PLAN_BWD_INKERNEL 13     /* rroi_bwd_tile_gather_kernel<plan.nk, NHWC>                       */
#define RROI_PLAN_BWD_LISTS 14        /* count / scan (+ rroi_scan2_kernel where !plan.raw_bsum) / fill + gather */
#define RROI_PLAN_BWD_BUCKETS 15      /* one-pass buckets of 1 << plan.kshift + overflow chains + gather  */
#define RROI_PLAN_BWD_LITERAL 16      /* the backward launcher's per-element kernel (reads con_idx)       */
#define RROI_PLAN_BWD_ORDERED 17      /* RROI_PATH_DETERMINISTIC: count / scan / fill, the lists sorted by bin, in-order fp64 gather */
/* plan.kernel: the gather instantiation of the fused / two-launch forward (-1: none) */
#define RROI_PLAN_KERNEL_STRIDED 0
#define RROI_PLAN_KERNEL_CHANNELS_LAST 1
#define RROI_PLAN_KERNEL_SHIFT 2
#define RROI_PLAN_KERNEL_STRIDED_MERGE 3
#define RROI_PLAN_KERNEL_SHIFT_LINES 4
/* plan.dest: where the backward's gradient goes */
#define RROI_PLAN_DST_NONE 0
#define RROI_PLAN_DST_CHUNK_MAJOR 1   /* scratch, then rroi_cm_to_nchw_kernel<plan.accumulate>            */
#define RROI_PLAN_DST_NCHW 2          /* NCHW bottom_diff written in place                                */
#define RROI_PLAN_DST_NCHW_ADD 3      /* NCHW bottom_diff added to in place                               */
#define RROI_PLAN_DST_NHWC 4          /* channels-last bottom_diff written in place                       */
typedef struct rroi_align_plan {
    int family;     /* RROI_PLAN_* */
    int kernel;     /* RROI_PLAN_KERNEL_*, -1 */
    int groups;     /* forward: XCD groups (1 = off) */
    int ntiles;     /* tiles per (roi, chunk) block of the tiled forward gather / the atomic backward; 0 */
    int grid_x;     /* grid of the plan's main kernel (the gather; the direct kernel) */
    int grid_y;
    int zero_copy;  /* channels-last features (forward) / top_diff (backward) consumed in place */
    int con_idx;    /* forward launcher: con_idx written */
    int nk;         /* in-kernel backward: channel chunks per lane (1, 2, 4, 8); 0 */
    int kshift;     /* buckets: log2 of the entries per bucket; 0 */
    int raw_bsum;   /* lists / buckets: 1 = consumers prefix-sum the scan blocks' totals, 0 = rroi_scan2_kernel; -1 */
    int gy;         /* list / bucket gather: channel passes in grid y (> 1: C > 128 on the in-place NCHW gather); 0 */
    int dest;       /* RROI_PLAN_DST_* */
    int accumulate; /* backward: added to bottom_diff */
    int vec4;       /* atomic backward: rroi_bwd_tiled_kernel<true> (PH * PW % 4 == 0) */
} rroi_align_plan;
int rroi_align_forward_plan(int feature_layout, int top_layout, int batch_size, int num_rois, int height, int width,
                            int channels, int pooled_height, int pooled_width, int path, int caller,
                            rroi_align_plan* plan);
int rroi_align_backward_plan(int top_diff_layout, int bottom_diff_layout, int batch_size, int num_rois, int height,
                             int width, int channels, int pooled_height, int pooled_width, int path, int caller,
                             rroi_align_plan* plan);

/* Half-precision I/O (0.10.0).  The element type of the caller's map and crops (forward) or top_diff and bottom_diff
 * (backward); `rois` are fp32 in every case (they carry the geometry).  Arithmetic: every element is widened exactly
 * to fp32, the geometry, taps and blend run unchanged in fp32 (the recipe above, `path`'s trig bit included), and
 * every result is rounded ONCE to the tensor's type, to nearest even (NaN stays NaN, -0.0 stays -0.0): a half forward
 * equals the fp32 forward of the widened map rounded to the type, bit for bit.  The backward sums every gradient
 * element in fp32 and rounds it once (no 16-bit atomics); bottom_diff is written, never added to.
 * What a 16-bit call may run:
 *   forward   features NCHW (no zero copy: repack channels-last features first), crops NCHW or NHWC; path AUTO,
 *             DIRECT or TILED -- RROI_PATH_FUSED is refused; native entry point only (the launchers of section 1 are
 *             fp32).  The two-launch path relays the map out to the same fp32 chunk-major copy as an fp32 call.
 *   backward  top_diff NCHW (repack a channels-last gradient first), bottom_diff NCHW or NHWC; path AUTO, TILED,
 *             TILED_LISTS, TILED_BUCKETS or TILED_INKERNEL -- RROI_PATH_DIRECT and RROI_PATH_TILED_ATOMIC (fp32
 *             atomics) are refused, and AUTO takes the gather TILED would take where an fp32 call would run DIRECT.
 *             A 16-bit backward is refused (0) where the gather's 32-bit indices do not hold: 4 x R x PH x PW >= 2^32
 *             pair slots, PH x PW x ceil(C / 32) x 128 >= 2^32 bytes of one ROI's gradient copy, or B x ceil(H / 4) x
 *             ceil(W / 8) x 32 >= 2^26 map keys (about 64 M map pixels) -- far beyond a training step; an fp32 call
 *             falls back to the atomic scatter there.
 * Workspace: a typed call needs no more than rroi_align_forward_workspace_bytes / rroi_align_backward_workspace_bytes
 * report for the same shape (the workspace is the same fp32 workspace whatever the dtype).
 * For RROI_DTYPE_FP32 the typed functions are the untyped ones: same plans, same kernels, same results. */
#define RROI_DTYPE_FP32 0
#define RROI_DTYPE_BF16 1
#define RROI_DTYPE_FP16 2
int rroi_align_forward_typed_hip(const void* features, int dtype, int feature_layout, int top_layout, float spatial_scale,
                                 int batch_size, int num_rois, int height, int width, int channels, int pooled_height,
                                 int pooled_width, const float* rois, void* top_data, void* workspace,
                                 size_t workspace_bytes, int path, void* stream);
int rroi_align_backward_typed_hip(const void* top_diff, int dtype, int top_diff_layout, int bottom_diff_layout,
                                  float spatial_scale, int batch_size, int num_rois, int height, int width, int channels,
                                  int pooled_height, int pooled_width, const float* rois, void* bottom_diff,
                                  void* workspace, size_t workspace_bytes, int path, void* stream);
/* The plan queries of a typed call (host only, as above).  RROI_DTYPE_FP32: exactly the untyped query's plan. */
int rroi_align_forward_plan_typed(int dtype, int feature_layout, int top_layout, int batch_size, int num_rois, int height,
                                  int width, int channels, int pooled_height, int pooled_width, int path, int caller,
                                  rroi_align_plan* plan);
int rroi_align_backward_plan_typed(int dtype, int top_diff_layout, int bottom_diff_layout, int batch_size, int num_rois,
                                   int height, int width, int channels, int pooled_height, int pooled_width, int path,
                                   int caller, rroi_align_plan* plan);

/* ------------------------------------------------------------------------- *
 * 2b. Bucketed RoIRotate: one pooled width PER ROI, one launch chain per call.
 *     Arrived after 0.10.0 under the same version string: a caller detects it by symbol.
 *
 *     RoIRotate is a variable-width operator -- a word keeps its aspect ratio -- but the calls of section 2 take one
 *     pooled_width, so a caller pools every ROI at the widest width of the batch and cuts its width buckets out afterwards.
 *     Here crop i is its own dense NCHW block (C, PH, W_i), found through a DEVICE table with one 16-byte row per ROI:
 *     its address and its pooled width.  Addresses are independent: the crops of one width usually form one contiguous
 *     (R_b, C, PH, W_b) tensor per bucket, each bucket an allocation of its own (autograd hands the backward one gradient
 *     tensor per bucket: they are consumed in place).  The value of element (c, ph, pw) of a crop depends on the ROI and
 *     on (ph, pw), never on the pooled width (kernel.cu:49-107), so crop i is, bit for bit, the first W_i columns of the
 *     same ROI pooled by the calls of section 2 at any width >= W_i.
 *
 *     Forward: EVERY element of every crop is written (masked bins are zeros; the crops need not be initialised) and
 *     NOTHING outside a crop's C * PH * W_i elements is.  Backward: the feature gradient (B, C, H, W), NCHW or NHWC, is
 *     fully overwritten; columns >= W_i do not exist.  Features and crops are NCHW, of element type `dtype` (RROI_DTYPE_*);
 *     rois are fp32.
 *     A row the host cannot check -- pooled_width < 1 or > max_pooled_width, or a NULL address -- is SKIPPED: nothing of
 *     that crop is read or written and it contributes nothing to the gradient; its neighbours are unaffected.
 *     Alignment: any crop address aligned to the element size gives correct results.  The caller STATES two facts about
 *     its table: `width_multiple`, a common divisor of all widths (1 says nothing), and `crop_alignment`, a power of two
 *     that divides every address in bytes (the element size says nothing).  The forward's fast form for many ROIs -- the
 *     prologue of the two-launch path followed by a ragged gather with 16-byte stores -- needs
 *     pooled_height * width_multiple % 16 == 0 and crop_alignment % 64 == 0; in that form a row that breaks the stated
 *     facts is skipped like a row with a bad width.  `sum_pooled_widths` (the sum over the table) is the call's real
 *     output size, by which RROI_PATH_AUTO chooses.
 *     Forward paths: RROI_PATH_AUTO; RROI_PATH_DIRECT = the ragged patch kernel (one launch, any widths, addresses and
 *     R); RROI_PATH_TILED = the ragged gather (refused where its contract does not hold); | RROI_PATH_TRIG_FP32.  AUTO
 *     takes the patch kernel for small outputs and wherever the gather's contract does not hold.  RROI_PATH_FUSED: 0.
 *     Backward paths: RROI_PATH_AUTO, RROI_PATH_TILED_LISTS, RROI_PATH_TILED_BUCKETS; | RROI_PATH_TRIG_FP32;
 *     RROI_PATH_AUTO | RROI_PATH_DETERMINISTIC = the ORDERED plan with the contract stated there (bit for bit the dense
 *     ORDERED gradient of the crops zero-padded to max_pooled_width).  Every other path returns 0; a ragged call is
 *     refused where the list gathers' 32-bit indices do not hold (the rule of 16-bit calls, above).
 *     Returns 1 / 0 / -hipError; every non-pointer argument is checked before any launch; a NULL pointer with
 *     num_rois > 0 returns 0; num_rois == 0 returns 1 (the backward zero-fills bottom_diff).  The calls only enqueue on
 *     `stream` and can be captured into a HIP graph.  Workspace: the sizes below (those of the dense calls at
 *     max_pooled_width); the patch kernel needs none (NULL / 0 accepted).  As in section 2 the workspace pointer must be
 *     a multiple of 256 bytes (0 otherwise, before any launch, from a plan that uses it); beyond that the base address
 *     is free, nothing outside the queried bytes is written and nothing the workspace held before is read.
 * ------------------------------------------------------------------------- */
typedef struct rroi_align_crop {
    void* data;       /* (C, PH, pooled_width) elements, contiguous */
    int pooled_width; /* 1 .. max_pooled_width */
    int reserved;     /* 0 */
} rroi_align_crop;    /* 16 bytes */
#define RROI_PLAN_KERNEL_STRIDED_RAGGED 5 /* plan.kernel of the bucketed two-launch forward */
size_t rroi_align_forward_bucketed_workspace_bytes(int batch_size, int channels, int height, int width, int num_rois);
size_t rroi_align_backward_bucketed_workspace_bytes(int batch_size, int channels, int height, int width, int num_rois,
                                                    int pooled_height, int max_pooled_width);
int rroi_align_forward_bucketed_hip(const void* features, int dtype, float spatial_scale, int batch_size, int num_rois,
                                    int height, int width, int channels, int pooled_height, int max_pooled_width,
                                    long long sum_pooled_widths, int width_multiple, int crop_alignment, const float* rois,
                                    const rroi_align_crop* crops, void* workspace, size_t workspace_bytes, int path,
                                    void* stream);
int rroi_align_backward_bucketed_hip(const rroi_align_crop* top_diffs, int dtype, int bottom_diff_layout, float spatial_scale,
                                     int batch_size, int num_rois, int height, int width, int channels, int pooled_height,
                                     int max_pooled_width, const float* rois, void* bottom_diff, void* workspace,
                                     size_t workspace_bytes, int path, void* stream);
/* Plan queries, host only as in section 2.  Forward: family RROI_PLAN_FWD_DIRECT_K2P (the ragged patch kernel) or
 * RROI_PLAN_FWD_TWO_LAUNCH with kernel RROI_PLAN_KERNEL_STRIDED_RAGGED, groups 1, ntiles = the widest crop's tiles (the
 * item space; a ROI has ceil(PH * W_i / 64) of them).  Backward: RROI_PLAN_BWD_LISTS / _BUCKETS / _ORDERED only. */
int rroi_align_forward_bucketed_plan(int dtype, int batch_size, int num_rois, int height, int width, int channels,
                                     int pooled_height, int max_pooled_width, long long sum_pooled_widths, int width_multiple,
                                     int crop_alignment, int path, rroi_align_plan* plan);
int rroi_align_backward_bucketed_plan(int dtype, int bottom_diff_layout, int batch_size, int num_rois, int height, int width,
                                      int channels, int pooled_height, int max_pooled_width, int path, rroi_align_plan* plan);

/* ------------------------------------------------------------------------- *
 * 3. The callers' ROI construction, on the device.
 *    quads (n, 8) fp32 [x0,y0,x1,y1,x2,y2,x3,y3] -> rois (n, 6) fp32 rows for the
 *    op, plus (optionally) each box's pooled width by the inference rule.
 *      mode 0 replaces tools/ocr_utils.py:133-150 (align_ocr, per detected box)
 *      mode 1 replaces src/ocr_process.py:196-206 (ground-truth quads in training;
 *             the random height jitter of :204 stays with the caller)
 *    batch_index (n) fp32 may be NULL (= 0).  target_gw (n) int32 may be NULL.
 * ------------------------------------------------------------------------- */
int rroi_align_quads_to_rois_hip(const float* quads, const float* batch_index, int n, int mode,
                                 int target_h, float* rois, int* target_gw, void* stream);

/* The training caller's side, src/ocr_process.py:196-219 and :259-263: ground-truth quads (n, 8)
 * -> rois (n, 6) with the reference's double-precision arithmetic, `height_jitter` (n) -- the
 * integer the caller draws with random.randint(-2, 2), :204; NULL = 0 -- added to h in double
 * before the row is rounded to fp32, and *max_ratio = max over the fp32 rows of w / h (NaN if any
 * ratio is NaN; -inf for n = 0): pooled_width = ceil(pooled_height * max_ratio), :260-263.  One
 * launch for the whole batch; a jitter that makes h <= 0 yields the degenerate rows the op handles
 * as the reference does (h < 0: zeros; h == 0: an infinite ratio, at which the reference's own
 * math.ceil raises). */
int rroi_align_gt_quads_to_rois_hip(const float* quads, const float* batch_index, const float* height_jitter,
                                    int n, float* rois, float* max_ratio, void* stream);

/* ------------------------------------------------------------------------- *
 * 4. Detection post-processing, replacing
 *    nms/adaptor.cpp:40-120 + nms/nms.h:116-215 (`nms.get_boxes`, nms/__init__.py:20-29).
 *
 *    rroi_rbox_decode_hip    device: every pixel of the score map `segm` (h, w) above
 *        `segm_thresh` -> one 64-byte candidate record, in raster order: int32 quad[8] in
 *        1/10000 px, float score, float rdist[4] (the pixel's four raw RBOX distances r[0..3]; the corner
 *        confidences expf(-r / 9) of adaptor.cpp:97-100 are formed by rroi_nms_merge_host with the C
 *        library's expf, as the reference does), int32 x, y, pad (adaptor.cpp:76-117).
 *        rbox (4, h, w) and angle (2, h, w) are CHANNELS-FIRST, as the network emits them
 *        (the reference transposes on the host first).  *count receives the number of passing
 *        pixels even when it exceeds `capacity` (records beyond it are dropped), for any `capacity` >= 0.
 *        One workgroup per 1024 pixels.  On a map of more than 262144 pixels a buffer of `capacity` >=
 *        h * w + ceil(h * w / 1024 / 16) records lets the library keep per-slab counts behind the h * w
 *        records it can fill (two short launches); a smaller buffer is served by the one-launch form, in
 *        which every workgroup counts the pixels before its slab itself (slower on such maps, same result).
 *    rroi_nms_merge_host     host (no GPU work): locality-aware merge with `iou_threshold`, then
 *        polygon NMS with `iou_threshold2` (the reference passes 0.4 and 0.2) over `num_candidates`
 *        records in host memory -> boxes (n, 9) fp32 [x0,y0,..,x3,y3 in px, score]; returns the
 *        number of boxes found (writes at most max_boxes), or -1 on an invalid argument.
 * ------------------------------------------------------------------------- */
/* Format of the 64-byte candidate record: 1 = {quad[8], score, probs[4], x, y, pad} (versions <= 0.5),
 * 2 = {quad[8], score, rdist[4], x, y, pad} (0.6.0 on: raw distances, confidences formed by rroi_nms_merge_host).
 * A consumer that reads records itself checks this constant against the library's rroi_nms_record_format(). */
#define RROI_NMS_RECORD_FORMAT 2
int rroi_nms_record_format(void);
int rroi_rbox_decode_hip(const float* segm, const float* rbox, const float* angle, int height, int width,
                         float segm_thresh, void* candidates, int capacity, int* count, void* stream);
int rroi_nms_merge_host(const void* candidates, int num_candidates, int width, int height, float iou_threshold,
                        float iou_threshold2, float* boxes, int max_boxes);
/* The maps of a 16-bit detector: `dtype` (RROI_DTYPE_*, section 2) is the element type of ALL THREE maps.  A bfloat16 /
 * float16 element is widened exactly to fp32 where it is loaded and everything after the load is the fp32 kernel's
 * arithmetic: count and records are byte for byte those of rroi_rbox_decode_hip on the widened maps (the record stays
 * RROI_NMS_RECORD_FORMAT 2: score and rdist[4] are the widened fp32 values; `score > segm_thresh` is decided on the
 * widened value), in both launch forms and for any capacity.  A 16-bit map needs 2-byte alignment only (image i of a
 * batch whose h * w is odd).  RROI_DTYPE_FP32 IS rroi_rbox_decode_hip; an unknown dtype returns 0 before any launch.
 * Arrived after 0.10.0 without a new version string: detect it by symbol (dlsym). */
int rroi_rbox_decode_typed_hip(int dtype, const void* segm, const void* rbox, const void* angle, int height, int width,
                               float segm_thresh, void* candidates, int capacity, int* count, void* stream);

/* Greedy CTC decode of the recognition logits computed from the crops: replaces the per-box
 * `labels_pred.max(1)` + Python loop of tools/ocr_utils.py:183-186 / src/utils.py:87-97
 * (strLabelConverter.decode, raw=False) for all boxes of an image in one launch.
 *   logits      (num_seqs, num_classes, num_steps) fp32, contiguous -- net.forward_ocr's layout
 *   lengths     (num_seqs) int32 valid time steps per sequence, or NULL (= num_steps)
 *   labels      (num_seqs, num_steps) int32 raw arg max per step, or NULL
 *   decoded     (num_seqs, num_steps) int32: label t is kept iff t < length, it is not the blank
 *               (0) and it differs from label t-1; kept labels first, then zeros
 *   decoded_len (num_seqs) int32 number of kept labels
 * arg max = first index of the largest value; NaN counts as largest (torch.max). */
int rroi_ctc_greedy_decode_hip(const float* logits, int num_seqs, int num_classes, int num_steps,
                               const int* lengths, int* labels, int* decoded, int* decoded_len,
                               void* stream);
/* ... of bfloat16 / float16 logits (`dtype`: RROI_DTYPE_*), the output of a head that runs in 16 bits: each element is
 * widened exactly where it is loaded, so labels, decoded and decoded_len are those of rroi_ctc_greedy_decode_hip on the
 * widened logits, ties and NaN included.  RROI_DTYPE_FP32 IS that call; an unknown dtype returns 0 before any launch.
 * Arrived after 0.10.0 without a new version string: detect it by symbol (dlsym). */
int rroi_ctc_greedy_decode_typed_hip(int dtype, const void* logits, int num_seqs, int num_classes, int num_steps,
                                     const int* lengths, int* labels, int* decoded, int* decoded_len, void* stream);

/* ------------------------------------------------------------------------- *
 * 5. The network's depthwise 3x3 convolution, replacing the stock convolution behind
 *    tools/models.py:70-102 (conv_dw_plain, conv_dw_in, conv_dw_res: `nn.Conv2d(c, c, 3, stride, 1, groups=c,
 *    bias=False)`) -- the depthwise halves of the separable blocks of layer3 / layer4 and of upconv1 / upconv2.
 *    Forward only; opt-in from Python (fots_e2e.native.use_native_depthwise).
 *
 *      x      (N, C, H, W)   contiguous NCHW, element type `dtype` (RROI_DTYPE_*)
 *      weight (C, 1, 3, 3)   contiguous, the same element type
 *      y      (N, C, Ho, Wo) Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1; EVERY element is written and
 *                            nothing else is
 *    padding 1, dilation 1, no bias, stride 1 or 2 on both axes.  Arithmetic, fixed so that results compare as bits:
 *      acc = +0.0 (double); for ky = 0, 1, 2: for kx = 0, 1, 2 (this order):
 *          acc = acc + (double)weight[c, 0, ky, kx] * (double)(inside the image ? x[n, c, oy * stride - 1 + ky,
 *                                                                                   ox * stride - 1 + kx] : +0.0)
 *      y[n, c, oy, ox] = (T)(float)acc
 *    -- a 16-bit element is widened exactly where it is loaded, the sum is rounded to fp32 once and (16-bit types)
 *    converted once more, to nearest even, NaN kept; a tap outside the image is weight * (+0.0), never skipped (NaN for
 *    a non-finite weight, as zero padding gives); fp32 subnormals are kept on input and output.
 *    Any element-aligned x, weight and y work (a view one element into an allocation is a legal argument).
 *    Returns 1 / 0 / -hipError.  0, before any launch: an unknown dtype, a stride other than 1 or 2, a dimension below
 *    1, a NULL pointer, N * C * H * W >= 2^31.  The call only enqueues one kernel on `stream`, allocates nothing and can
 *    be captured into a HIP graph.  Arrived after 0.10.0 under the same version string: detect it by symbol.
 * ------------------------------------------------------------------------- */
int rroi_depthwise3x3_forward_hip(int dtype, const void* x, const void* weight, void* y, int batch_size, int channels,
                                  int height, int width, int stride, void* stream);

/* ------------------------------------------------------------------------- *
 * 5b. The backward of the depthwise 3x3 convolution of section 5: the gradient of its input, bit-exact,
 *    and the gradient of its weight, deterministic.  Opt-in from Python (rroi_align.conv.depthwise3x3,
 *    fots_e2e.native_train.use_trainable_depthwise).
 *
 *      dy      (N, C, Ho, Wo)  contiguous NCHW, element type `dtype`: the gradient of the output; Ho, Wo as in section 5
 *      x       (N, C, H, W)    contiguous NCHW, the forward's input; read for dweight only
 *      weight  (C, 1, 3, 3)    the forward's; read for dx only
 *      dx      (N, C, H, W)    the same type, or NULL; EVERY element is written and nothing else is
 *      dweight (C, 1, 3, 3)    the same type, or NULL (not both NULL)
 *    batch_size, channels, height, width are x's, whichever outputs are wanted.  With dx NULL weight may be NULL; with
 *    dweight NULL x and the workspace may be.
 *
 *    dx, fixed so that results compare as bits (s = stride):
 *      acc = +0.0 (double); for ky = 2, 1, 0: for kx = 2, 1, 0 (this order: dy is visited in row-major order):
 *          if (iy + 1 - ky) % s == 0 and (ix + 1 - kx) % s == 0:   oy = (iy + 1 - ky) / s, ox = (ix + 1 - kx) / s
 *              acc = acc + (double)weight[c, 0, ky, kx] * (double)(0 <= oy < Ho and 0 <= ox < Wo ? dy[n, c, oy, ox] : +0.0)
 *      dx[n, c, iy, ix] = (T)(float)acc
 *    -- the rounding of section 5: to fp32 once, then one plain conversion.  A tap of the right parity whose dy lies
 *    outside is weight * (+0.0), never skipped, as the padding of section 5 is: a non-finite weight therefore gives NaN
 *    along the border -- the first and last row and column at stride 1; at stride 2 the last row where H is even and the
 *    last column where W is even -- where the mathematical gradient is finite.  A NaN or +-inf in dy reaches exactly the dx
 *    elements whose taps read it.
 *
 *    dweight, deterministic:
 *      dweight[c, 0, ky, kx] = sum over n, oy, ox of (double)dy[n, c, oy, ox] *
 *                              (double)(inside the image ? x[n, c, s * oy - 1 + ky, s * ox - 1 + kx] : +0.0)
 *    -- every product exact in double, every sum in double in an order that depends on the argument list alone (no
 *    atomics), no chain of additions longer than 8192 at any legal shape, one rounding from double to `dtype` (the 16-bit
 *    types through a float rounded to odd, as in sections 15 and 6c).  Two identical calls give identical bits.  A NaN
 *    or +-inf in a plane of dy or x stays in its channel's dweight.
 *    Two launches: `segments` workgroups per (n, c) plane -- a workgroup never mixes planes -- leave nine doubles each in
 *    the workspace, then one workgroup per channel adds its N * segments entries in (n, segment) order and rounds.
 *    Needs rroi_depthwise3x3_backward_workspace_bytes(N, C, H, W, stride) bytes, never 0 for a valid shape, at a
 *    256-byte-aligned address; the contents before and after the call mean nothing.  Where dweight is NULL the workspace
 *    is not needed: NULL / 0 is accepted and a buffer that is handed over is left alone.
 *
 *    Any element-aligned dy, x and dx work (a view one element into an allocation is a legal argument).
 *    Returns 1 / 0 / -hipError.  0, before any launch: everything section 5 refuses for (N, C, H, W, stride), a NULL dy, dx
 *    and dweight both NULL, dx without weight, dweight without x, dx overlapping dy (or x, where dweight is wanted too), and
 *    -- where dweight is wanted -- a NULL workspace, one that is not a multiple of 256, or workspace_bytes below the size
 *    query's answer.  The call only enqueues on `stream`, allocates nothing and can be captured into a HIP graph.
 *    Arrived after 0.10.0 under the same version string: detect it by symbol.
 * ------------------------------------------------------------------------- */
typedef struct rroi_depthwise_backward_plan_info {
    int dx_band;        /* dx rows per thread of the dx launch: 2, 4 or 8 times the stride */
    int dx_cols;        /* dx columns per thread: 4 (stride 1) / 8 (stride 2) */
    int dx_grid_x;      /* workgroups of the dx launch */
    int dw_band;        /* dy rows per thread of the partials launch */
    int segments;       /* workgroups per plane of the partials launch: nine doubles of workspace each */
    int dw_grid_x;      /* workgroups of the partials launch: N * C * segments (capped at 2^22; the finish has C) */
    int launches;       /* of a call that wants both gradients: 3 (dx alone 1, dweight alone 2) */
    int block;          /* threads per workgroup */
} rroi_depthwise_backward_plan_info;
int rroi_depthwise3x3_backward_hip(int dtype, const void* dy, const void* x, const void* weight, void* dx, void* dweight,
                                   int batch_size, int channels, int height, int width, int stride, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* host only; 0 for arguments the call would refuse */
size_t rroi_depthwise3x3_backward_workspace_bytes(int batch_size, int channels, int height, int width, int stride);
/* host only, no launch; 1, or 0 for arguments the call would refuse */
int rroi_depthwise3x3_backward_plan(int dtype, int batch_size, int channels, int height, int width, int stride,
                                    rroi_depthwise_backward_plan_info* plan);

/* ------------------------------------------------------------------------- *
 * 6. The network's InstanceNorm2d with the activation that follows it, replacing the stock
 *    `nn.InstanceNorm2d(c, eps, affine)` of tools/models.py (MIOpen's spatial batch norm in fp32, two ATen kernels in
 *    16 bits) and, optionally, the LeakyReLU / ReLU launch behind it.  Forward only, instance statistics only (never
 *    running statistics); opt-in from Python (fots_e2e.native.use_native_instancenorm).
 *
 *      x      (N, C, H, W)  contiguous NCHW, element type `dtype` (RROI_DTYPE_*)
 *      gamma, beta  (C)     the same element type, or BOTH NULL (= 1 and 0: affine=False)
 *      y      (N, C, H, W)  the same type; every element is written and nothing else is (beyond the workspace); x and y
 *                           must not overlap
 *      eps                  finite, > 0
 *      negative_slope       finite: 1.0 = no activation, 0.0 = ReLU, 0.01 = the network's LeakyReLU
 *
 *    Arithmetic per (n, c) plane of n = H * W elements, fixed so that two identical calls give identical bits:
 *      every element is widened exactly to double where it is loaded;  K = the plane's first element
 *      s1 = sum (x - K),  s2 = sum (x - K)^2      in double, in an order that depends on the argument list alone
 *                                                 (no atomics; the order changes with the form and with x mod 16 bytes)
 *      m = s1 / n,  mean = K + m,  var = s2 / n - m * m, negative -> 0 (a NaN stays),  a = gamma / sqrt(var + eps),
 *      b = beta - mean * a                        all in double, each operation rounded once (no contraction)
 *      v = (float)((double)x * a + b);  v = v < 0 ? v * negative_slope : v  (fp32);  y = (T)v
 *    -- one plain conversion to the tensor's type (nearest even, NaN kept).  A NaN or +-inf anywhere in a plane makes
 *    that whole plane NaN and touches no other plane; fp32 subnormals are kept on input and output.
 *    Any element-aligned x and y work (a view one element into an allocation is a legal argument).
 *
 *    Two forms, chosen by the library as a pure function of (dtype, N, C, H, W, CU count) -- rroi_instancenorm_plan
 *    reports the choice without a launch (256 CUs where there is no GPU):
 *      RROI_INORM_PLANE  one launch, one workgroup per plane; no workspace (NULL / 0 is accepted, a buffer that is
 *                        handed over is left alone)
 *      RROI_INORM_SPLIT  two launches for few large planes: `segments` workgroups per plane leave one {s1, s2} pair of
 *                        doubles each in the workspace, then every workgroup of the second launch adds its plane's pairs
 *                        in one fixed order and maps its segment.  Needs rroi_instancenorm_workspace_bytes(N, C, H, W)
 *                        bytes at a 256-byte-aligned address; the contents before and after the call mean nothing.
 *    Returns 1 / 0 / -hipError.  0, before any launch: an unknown dtype, a dimension below 1, N * C * H * W >= 2^31, a
 *    NULL x or y, exactly one of gamma / beta NULL, eps not finite or not > 0, negative_slope not finite, and -- for a
 *    plan that needs the workspace -- a NULL workspace, one that is not a multiple of 256, or workspace_bytes below
 *    the size query's answer.  The call only enqueues on `stream`, allocates nothing and can be captured into a HIP graph.
 *    Arrived after 0.10.0 under the same version string: detect it by symbol.
 * ------------------------------------------------------------------------- */
#define RROI_INORM_PLANE 1
#define RROI_INORM_SPLIT 2
typedef struct rroi_instancenorm_plan_info {
    int form;           /* RROI_INORM_PLANE / RROI_INORM_SPLIT */
    int launches;       /* 1 / 2 */
    int segments;       /* workgroups per plane (1 in the plane form) */
    int segment_elems;  /* elements per segment; the last segment takes what is left (H * W in the plane form) */
    int grid_x;         /* workgroups per launch: N * C * segments */
    int block;          /* threads per workgroup */
    int vector_elems;   /* elements per 16-byte access */
    int reserved;
} rroi_instancenorm_plan_info;
int rroi_instancenorm_forward_hip(int dtype, const void* x, const void* gamma, const void* beta, void* y, int batch_size,
                                  int channels, int height, int width, double eps, float negative_slope, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* host only; 0 where the plan needs no workspace (and for arguments the call would refuse) */
size_t rroi_instancenorm_workspace_bytes(int batch_size, int channels, int height, int width);
/* host only, no launch; 1, or 0 for arguments the call would refuse */
int rroi_instancenorm_plan(int dtype, int batch_size, int channels, int height, int width, rroi_instancenorm_plan_info* plan);

/* ------------------------------------------------------------------------- *
 * 6b. The InstanceNorm of section 6 with an epilogue fused in: the residual add in the tail of the
 *    network's residual blocks, or the concatenation cat(x, -x) in front of the stem's two norms (`CReLU_IN` of
 *    tools/models.py).  Forward only; opt-in from Python (fots_e2e.native.use_native_blocks).
 *
 *      x        (N, C, H, W)   as in section 6; `channels` is x's channel count in both modes
 *      residual (N, C, H, W)   the same type, or NULL
 *      mirror   0 / 1
 *      mirror = 0:  gamma, beta (C) or both NULL, y (N, C, H, W):
 *          v = (float)((double)x * a + b);  u = v + (float)residual  (fp32, rounded once);
 *          u = u < 0 ? u * negative_slope : u;  y = (T)u
 *        With residual = NULL this is the call of section 6.
 *      mirror = 1:  gamma, beta (2C) or both NULL, y (N, 2C, H, W), residual NULL:  y = what section 6 gives on
 *        cat(x, -x) along the channels, which is never materialised.  Source plane (n, j) is summed once, as in section 6;
 *        output plane (n, j) takes (K, s1, s2) with gamma[j], beta[j], and output plane (n, C + j) takes (-K, -s1, s2) --
 *        exactly the sums of the negated plane -- with gamma[C + j], beta[C + j].  The bits are those of the section 6
 *        call on the concatenated tensor whenever that call adds in the same order: the same form and segment length,
 *        and every plane of both tensors at the same offset from a 16-byte boundary.
 *    The statistics, their order and the workspace are those of section 6 for x's shape: rroi_instancenorm_plan and
 *    rroi_instancenorm_workspace_bytes called with (N, C, H, W) of x answer for this entry point too.  A NaN or +-inf in
 *    the residual affects its own element alone; one in a plane of x takes that plane and, under mirror, both its
 *    output planes.  y must not overlap x or residual.  Any element-aligned x, residual and y work.
 *
 *    Returns 1 / 0 / -hipError.  0, before any launch: everything section 6 refuses, a mirror other than 0 or 1,
 *    mirror = 1 with a non-NULL residual, mirror = 1 with N * 2C * H * W >= 2^31.  The call only enqueues on `stream`,
 *    allocates nothing and can be captured into a HIP graph.  Arrived after 0.10.0 under the same version string: detect
 *    it by symbol.
 * ------------------------------------------------------------------------- */
int rroi_instancenorm_fused_forward_hip(int dtype, const void* x, const void* gamma, const void* beta, const void* residual,
                                        void* y, int batch_size, int channels, int height, int width, int mirror, double eps,
                                        float negative_slope, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * 6c. The InstanceNorm of section 6 for training: a forward that also leaves every plane's statistics,
 *    and the backward that uses them.  Opt-in from Python (rroi_align.norm.instance_norm,
 *    fots_e2e.native_train.use_trainable_instancenorm).
 *
 *    rroi_instancenorm_forward_train_hip is the call of section 6 with one more output:
 *      stats  (N * C) pairs of doubles {mean, var}, 16-byte aligned: the plane's statistics exactly as the forward formed
 *             them, mean = K + m and var after the clamp
 *    y has the bits rroi_instancenorm_forward_hip gives for the same arguments; the plan and the workspace are those of
 *    section 6.  It refuses what section 6 refuses, and a NULL stats.
 *
 *    rroi_instancenorm_backward_hip:
 *      dy, x  (N, C, H, W)  contiguous NCHW, element type `dtype`: the gradient of the output, the forward's input
 *      stats  (N * C) pairs  what the training forward left for this x
 *      gamma, beta  (C)     the forward's, or BOTH NULL
 *      dx     (N, C, H, W)  the same type, or NULL (then dgamma must not be: the map pass is skipped)
 *      dgamma, dbeta  (C)   the same type, or BOTH NULL; they need gamma
 *      eps, negative_slope  the forward's
 *    Arithmetic per plane of n = H * W elements, all in double, each operation rounded once (no contraction):
 *      a = gamma / sqrt(var + eps),  b = beta - mean * a                 the forward's coefficients again
 *      v = (float)((double)x * a + b);  d = v > 0 ? 1 : negative_slope;  g = dy * d
 *                                    -- the sign decisions are the forward's own; torch's convention at 0
 *      rs = 1 / sqrt(var + eps);  xh = (x - mean) * rs
 *      t1 = sum g,  t2 = sum g * xh          in an order that depends on the argument list alone (no atomics; the
 *                                            order changes with the form and with x mod 16 bytes)
 *      dx = (T)(float)(A * ((g - t1 / n) - xh * (t2 / n))),  A = gamma * rs  (rs where gamma is NULL)
 *      dbeta[c] = sum over n of t1(n, c),  dgamma[c] = sum over n of t2(n, c),  in n order, each rounded once from double
 *      to `dtype` (the 16-bit types through a float rounded to odd, as in section 15)
 *    Two identical calls give identical bits.  A NaN or +-inf in a plane of x or dy stays in that plane's dx and in its
 *    channel's parameter gradients.  Any element-aligned dy, x and dx work; dx must not overlap x or dy.
 *
 *    Two forms by the rule of section 6 with the backward's own thresholds -- rroi_instancenorm_backward_plan reports the
 *    choice in the struct of section 6 (launches: of a call that wants every gradient; the parameter-gradient kernel is
 *    the last launch and is left out where dgamma is NULL):
 *      RROI_INORM_PLANE  one workgroup per plane: the two sums, then the map while the plane is in L2
 *      RROI_INORM_SPLIT  a partials launch, `segments` workgroups per plane leaving one {t1, t2} pair each, then an apply
 *                        launch in which every workgroup adds its plane's pairs in one fixed order and maps its segment
 *    The workspace -- rroi_instancenorm_backward_workspace_bytes(N, C, H, W) bytes, never 0 for a valid shape, at a
 *    256-byte-aligned address -- holds one {t1, t2} pair per plane for the parameter gradients and the split form's
 *    partials.  It is needed where dgamma is not NULL or the form is RROI_INORM_SPLIT; elsewhere NULL / 0 is accepted
 *    and a buffer that is handed over is left alone.  Its contents before and after the call mean nothing.
 *
 *    Returns 1 / 0 / -hipError.  0, before any launch: everything section 6 refuses (y's part read for dx), a NULL dy, x
 *    or stats, exactly one of dgamma / dbeta NULL, dx and dgamma both NULL, dgamma without gamma, dx overlapping x or dy,
 *    and -- where the workspace is needed -- a NULL workspace, one that is not a multiple of 256, or workspace_bytes
 *    below the size query's answer.  Both calls only enqueue on `stream`, allocate nothing and can be captured into a HIP
 *    graph.  Arrived after 0.10.0 under the same version string: detect them by symbol.
 * ------------------------------------------------------------------------- */
int rroi_instancenorm_forward_train_hip(int dtype, const void* x, const void* gamma, const void* beta, void* y, void* stats,
                                        int batch_size, int channels, int height, int width, double eps, float negative_slope,
                                        void* workspace, size_t workspace_bytes, void* stream);
int rroi_instancenorm_backward_hip(int dtype, const void* dy, const void* x, const void* stats, const void* gamma,
                                   const void* beta, void* dx, void* dgamma, void* dbeta, int batch_size, int channels,
                                   int height, int width, double eps, float negative_slope, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* host only; 0 for arguments the call would refuse */
size_t rroi_instancenorm_backward_workspace_bytes(int batch_size, int channels, int height, int width);
/* host only, no launch; 1, or 0 for arguments the call would refuse */
int rroi_instancenorm_backward_plan(int dtype, int batch_size, int channels, int height, int width,
                                    rroi_instancenorm_plan_info* plan);

/* ------------------------------------------------------------------------- *
 * 7. The network's detection heads and attention gate: a 1x1 convolution with bias from many channels to
 *    7 outputs (heads: `act` 1, `rbox` 4, `angle` 2 of tools/models.py) or to 1 (gate: `conv_attenton`), with the
 *    elementwise chain behind it -- three sigmoids, the scalings, the angle's normalisation -- in ONE launch that reads
 *    the map once.  Forward only; opt-in from Python (fots_e2e.native.use_native_heads).
 *
 *      x        (N, C, H, W)  contiguous NCHW, element type `dtype` (RROI_DTYPE_*)
 *      w_score  (1, C)   w_rbox (4, C)   w_angle (2, C)    contiguous, the same type: the memory of a (k, C, 1, 1) weight
 *      b_score  (1)      b_rbox (4)      b_angle (2)       the same type; a NULL bias is +0.0
 *      score    (N, 1, H, W)   rbox (N, 4, H, W)   angle (N, 2, H, W)   the same type; every element is written and
 *                             nothing else is; no output may overlap x
 *      gate:  w (1, C), b (1) or NULL, y (N, 1, H, W)
 *
 *    Arithmetic per pixel, fixed so that two identical calls give identical bits:
 *      every element of x and of the weights is widened exactly to double where it is loaded
 *      z_o = b_o + p_0 + p_1 + ... + p_{S-1}   added left to right;  p_k = the double sum, from +0.0 in channel order, of
 *            the exact products w[o][c] * x[c] over the k-th block of ceil(C / S) consecutive channels; S is
 *            rroi_heads_plan_info.channel_splits
 *      s_o = 1 / (1 + exp(-z_o))               in double, every operation rounded once (no contraction)
 *      heads:  score = s_0;  rbox_j = rbox_scale * s_{1+j};  a_i = 2 s_{5+i} - 1,  angle_i = a_i / sqrt(a_0 a_0 + a_1 a_1)
 *      gate:   y = s_0
 *      out = (T)(float)value
 *    -- one rounding to fp32 and one plain conversion to the tensor's type (nearest even, NaN kept), which is how a
 *    float64 tensor converts; fp32 subnormals are kept on input and output.  a_0 = a_1 = 0 gives NaN in both angle
 *    channels; a NaN or +-inf in a pixel's channel column affects that pixel alone; a zero weight times an inf is NaN (no
 *    channel is skipped).  No atomics: the order depends on the plan alone and the plan on (dtype, outputs, N, C, H, W,
 *    CU count) alone -- 256 CUs where there is no GPU.
 *    Any element-aligned x, weights and outputs work (a view one element into an allocation is a legal argument).
 *
 *    Returns 1 / 0 / -hipError.  0, before any launch: an unknown dtype, a dimension below 1, N * C * H * W >= 2^31, a
 *    NULL x, weight or output, an rbox_scale that is not finite, `outputs` other than 1 or 7 (plan query).  Each call
 *    enqueues one kernel on `stream`, uses no workspace, allocates nothing and can be captured into a HIP graph.
 *    Arrived after 0.10.0 under the same version string: detect it by symbol.
 * ------------------------------------------------------------------------- */
typedef struct rroi_heads_plan_info {
    int vector_elems;    /* V: consecutive pixels per lane (2 or 1) */
    int channel_splits;  /* S: waves per workgroup, each on its own block of channels (1, 2, 4, 8 or 16; at most 16 / V) */
    int tiles;           /* tiles of 64 * V pixels per image */
    int grid_x;          /* workgroups: N * tiles */
    int block;           /* threads per workgroup: 64 * S */
    int lds_bytes;       /* (S - 1) * outputs * V * 64 doubles */
    int channel_block;   /* ceil(C / S) */
    int reserved;
} rroi_heads_plan_info;
int rroi_heads_forward_hip(int dtype, const void* x, const void* w_score, const void* b_score, const void* w_rbox,
                           const void* b_rbox, const void* w_angle, const void* b_angle, void* score, void* rbox, void* angle,
                           int batch_size, int channels, int height, int width, double rbox_scale, void* stream);
int rroi_gate_forward_hip(int dtype, const void* x, const void* w, const void* b, void* y, int batch_size, int channels,
                          int height, int width, void* stream);
/* host only, no launch; 1, or 0 for arguments the call would refuse; outputs: 7 (heads) or 1 (gate) */
int rroi_heads_plan(int dtype, int outputs, int batch_size, int channels, int height, int width, rroi_heads_plan_info* plan);

/* ------------------------------------------------------------------------- *
 * 7b. The heads and the gate where a gradient is needed: a training forward that leaves what the backward
 *    needs, and a deterministic backward without atomics.  Opt-in from Python (rroi_align.heads.detection_heads /
 *    attention_gate, fots_e2e.native_train_heads.use_trainable_heads).  Tensors as in section 7, and
 *
 *      z        (N, 7 | 1, H, W)  DOUBLE, contiguous: the pre-activation sums z_o of section 7
 *      dscore (N, 1, H, W)  drbox (N, 4, H, W)  dangle (N, 2, H, W)  (gate: dy (N, 1, H, W))   element type `dtype`
 *      dx (N, C, H, W)   dw_* (k, C)   db_* (k)                                                element type `dtype`
 *
 *    rroi_heads_forward_train_hip / rroi_gate_forward_train_hip: the call of section 7 with one more output.  z holds
 *      z_o = b_o + p_0 + ... + p_{S-1} exactly as section 7 forms it, with the same plan; the other outputs have the bits
 *      of rroi_heads_forward_hip / rroi_gate_forward_hip.  One launch.  Refuses what section 7 refuses, and a NULL z.
 *
 *    rroi_heads_backward_hip / rroi_gate_backward_hip: each of dscore, drbox, dangle may be NULL, which means zero, not
 *      all of them (gate: dy is needed); each of dx, dw_*, db_* may be NULL and is then not computed, not all of them.
 *      Per pixel, in double, every operation rounded once except the fused multiply-adds named below:
 *        s_o = 1 / (1 + exp(-z_o));  g_0 = dscore;  g_{1+j} = rbox_scale * drbox_j
 *        a_i = 2 s_{5+i} - 1,  r = sqrt(a_0 a_0 + a_1 a_1),  u_i = a_i / r,  p = u_0 dangle_0 + u_1 dangle_1
 *        g_{5+i} = 2 (dangle_i - u_i p) / r;   dz_o = g_o * (s_o * (1 - s_o))        (gate: g_0 = dy, one output)
 *        dx_c = fma(w[6][c], dz_6, ... fma(w[0][c], dz_0, +0.0));   out = (T)(float)dx_c, as section 7 rounds
 *      r = 0 gives NaN in that pixel's dx column, as the stock chain's backward does; a non-finite value in a pixel
 *      affects that pixel's dx column and the parameter gradients alone; no channel and no output is skipped.
 *        dw[o][c] = sum over (n, pixel) of dz_o x[c],   db[o] = sum over (n, pixel) of dz_o
 *      in double, each term of dw entering by one fused multiply-add, in an order the plan alone fixes and without
 *      atomics: a lane adds its `vector_elems` pixels, the 64 lanes of a wave are added pairwise (lane l with l ^ 32,
 *      then ^ 16, ... ^ 1), a workgroup adds its `tiles_per_workgroup` tiles in tile order and leaves ONE partial row of
 *      k (C + 1) doubles -- dw [o][c], then db [o] -- in the workspace; a second launch adds the rows, four quarters of
 *      the rows each in row order and then the quarters in order, and rounds once, out = (T)(float)sum.  So a backward is
 *      two launches, and one where no parameter gradient is wanted.  The plan depends on (dtype, outputs, N, C, H, W, CU
 *      count) alone -- 256 CUs where there is no GPU -- so identical calls give identical bits at any addresses.
 *      The workspace: rroi_heads_backward_workspace_bytes(...) bytes at a 256-byte-aligned address where a dw or db is
 *      wanted; the partial rows never exceed four per CU, whatever N * H * W is.  Its contents before and after the call
 *      mean nothing.  Where no dw or db is wanted it is not needed: NULL / 0 is accepted.
 *
 *    Returns 1 / 0 / -hipError.  0, before any launch: everything section 7 refuses, k (C + 1) >= 2^31, a NULL x or z, a
 *    NULL weight while dx is wanted, no output gradient given, no output wanted, a workspace that is NULL, misaligned or
 *    too small while a dw or db is wanted, an output overlapping an input, another output or the workspace.  The calls
 *    only enqueue on `stream` and allocate nothing: they can be captured into a HIP graph.
 *    Arrived after 0.10.0 under the same version string: detect them by symbol.
 * ------------------------------------------------------------------------- */
typedef struct rroi_heads_backward_plan_info {
    int vector_elems;          /* V: consecutive pixels per lane (2 or 1) */
    int grid_x;                /* workgroups of the main launch */
    int partial_rows;          /* rows of k (C + 1) doubles in the workspace: one per workgroup */
    int tiles_per_workgroup;   /* tiles of 64 * V pixels a workgroup walks */
    int block;                 /* threads per workgroup: 256 */
    int lds_bytes;             /* of a main launch that leaves partial rows */
    int launches;              /* of a call that wants a dw or db: 2 (dx alone: 1) */
    int reserved;
    long long pixels_per_workgroup;   /* tiles_per_workgroup * 64 * V */
    long long workspace_bytes;        /* partial_rows * k * (C + 1) * 8 */
} rroi_heads_backward_plan_info;
int rroi_heads_forward_train_hip(int dtype, const void* x, const void* w_score, const void* b_score, const void* w_rbox,
                                 const void* b_rbox, const void* w_angle, const void* b_angle, void* score, void* rbox,
                                 void* angle, void* z, int batch_size, int channels, int height, int width, double rbox_scale,
                                 void* stream);
int rroi_gate_forward_train_hip(int dtype, const void* x, const void* w, const void* b, void* y, void* z, int batch_size,
                                int channels, int height, int width, void* stream);
int rroi_heads_backward_hip(int dtype, const void* dscore, const void* drbox, const void* dangle, const void* x, const void* z,
                            const void* w_score, const void* w_rbox, const void* w_angle, void* dx, void* dw_score,
                            void* db_score, void* dw_rbox, void* db_rbox, void* dw_angle, void* db_angle, int batch_size,
                            int channels, int height, int width, double rbox_scale, void* workspace, size_t workspace_bytes,
                            void* stream);
int rroi_gate_backward_hip(int dtype, const void* dy, const void* x, const void* z, const void* w, void* dx, void* dw, void* db,
                           int batch_size, int channels, int height, int width, void* workspace, size_t workspace_bytes,
                           void* stream);
/* host only; outputs: 7 (heads) or 1 (gate); 0 for arguments the call would refuse */
size_t rroi_heads_backward_workspace_bytes(int outputs, int batch_size, int channels, int height, int width);
/* host only, no launch; 1, or 0 for arguments the call would refuse */
int rroi_heads_backward_plan(int dtype, int outputs, int batch_size, int channels, int height, int width,
                             rroi_heads_backward_plan_info* plan);

/* ------------------------------------------------------------------------- *
 * 8. The gated merge of the network's feature merge: y = A + f * G in ONE launch, where A is `a` resized
 *    to f's size and G the one-channel `gate` resized likewise -- `up(a) + f * up(gate)` of tools/models.py:412-434.
 *    Forward only; opt-in from Python (fots_e2e.native.use_native_merge).
 *
 *      a      (N, C, a_h, a_w)      gate   (N, 1, g_h, g_w) or NULL: y = A + f (g_h, g_w are not read)
 *      f, y   (N, C, H, W)          all contiguous NCHW, one element type `dtype` (RROI_DTYPE_*)
 *    Every element of y is written and nothing else is; y may overlap no input.
 *
 *    Resize: bilinear, align_corners = true, in double.  Per axis s = (double)(in - 1) / (double)(out - 1), 0 where
 *    out == 1, computed on the host (rroi_merge_plan_info.*_scale_*);
 *      src = s * (double)dst;  i0 = min((int)src, in - 1);  i1 = min(i0 + 1, in - 1);  l1 = src - i0;  l0 = 1.0 - l1
 *      value = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)
 *    every multiply and add rounded separately to double in exactly that order (no contraction), every tap widened
 *    exactly to double where it is loaded, no tap skipped (a zero weight against an infinity is NaN).  A source whose
 *    size equals (H, W) on both axes is read as it is, with no interpolation arithmetic.
 *    Sum: p = (double)f * G;  z = A + p (no gate: z = A + (double)f);  out = (T)(float)z -- one rounding to fp32 and one
 *    plain conversion to the tensor's type, as in sections 6 and 7; fp32 subnormals are kept; a gate value outside [0, 1] is
 *    used as it is.  Nothing is transcendental and nothing is reduced across lanes: the bits depend on neither the plan nor
 *    an address, and a float64 restatement with separate multiplies and adds reproduces every element bit for bit.
 *    Any element-aligned a, gate, f and y work.
 *
 *    Returns 1 / 0 / -hipError.  0, before any launch: an unknown dtype, a dimension below 1 (g_h, g_w: with a gate),
 *    N * C * H * W >= 2^31, N * C * a_h * a_w >= 2^31, N * g_h * g_w >= 2^31, a NULL a, f or y, `gated` other than 0 or 1
 *    (plan query).  Each call enqueues one kernel on `stream`, uses no workspace, allocates nothing and can be captured
 *    into a HIP graph.  Arrived after 0.10.0 under the same version string: detect it by symbol.
 * ------------------------------------------------------------------------- */
typedef struct rroi_merge_plan_info {
    int vector_elems;    /* V: consecutive pixels per lane (4; 2 where a is resized) */
    int channel_groups;  /* K: workgroups per tile, each on its own block of channels */
    int tiles;           /* tiles of 256 * V pixels per image */
    int grid_x;          /* workgroups: N * K * tiles */
    int block;           /* threads per workgroup: 256 */
    int channel_block;   /* ceil(C / K) */
    int resize_a;        /* 1: a is interpolated; 0: it has f's size and is read as it is */
    int resize_gate;     /* likewise for the gate (0 without one) */
    double a_scale_y, a_scale_x, gate_scale_y, gate_scale_x;   /* s per axis (the gate's: 0 without one) */
} rroi_merge_plan_info;
int rroi_merge_forward_hip(int dtype, const void* a, int a_h, int a_w, const void* gate, int g_h, int g_w, const void* f,
                           void* y, int batch_size, int channels, int height, int width, void* stream);
/* host only, no launch; 1, or 0 for arguments the call would refuse; gated: 1 (g_h, g_w are the gate's size) or 0 */
int rroi_merge_plan(int dtype, int batch_size, int channels, int height, int width, int a_h, int a_w, int g_h, int g_w,
                    int gated, rroi_merge_plan_info* plan);

/* ------------------------------------------------------------------------- *
 * 8b. The backward of section 8's merge, the resize R of section 8 on its own, and its backward, all
 *    deterministic and free of atomics.  Opt-in from Python (rroi_align.merge.gated_merge / bilinear_resize,
 *    fots_e2e.native_train.use_trainable_merge).  R is section 8's resize with its scales, indices and weights; the
 *    forward is y = R_a a + f * (R_g gate).  All tensors contiguous NCHW of one element type `dtype`; any element-aligned
 *    address works.
 *
 *    rroi_resize_forward_hip:   x (N, C, in_height, in_width) -> y (N, C, height, width) = R x: section 8's `value`,
 *      rounded as its `out` is -- (T)(float)z -- so bit for bit what section 8 adds as A.  A source of y's size is copied
 *      as it is.  Every element of y is written and nothing else is.  One launch, no workspace.
 *
 *    rroi_resize_backward_hip:  dy (N, C, height, width) -> dx (N, C, in_height, in_width) = R^T dy, as a gather, the exact
 *      transpose of the forward's own index decisions: output row Y gives weight 1 - l1 to source row i0(Y) and l1 to
 *      i0(Y) + step(Y), step = min(i0 + 1, in - 1) - i0; columns likewise.  The rows that reach source row i are the
 *      contiguous range rroi_resize_footprint reports.  Per element, in double, every operation rounded separately:
 *          acc = +0.0;  for Y of the range, ascending:
 *              row = +0.0;  for X of the column range, ascending:  row = row + wx * (double)dy[n, c, Y, X]
 *              acc = acc + wy * row
 *      where step == 0 both weights meet in one element and are two terms, the first tap's and then the second's.  No tap
 *      of the range is skipped: a zero weight against an infinity is NaN, as in the forward.  dx = one rounding of acc from
 *      double to `dtype` (the 16-bit types through a float rounded to odd, as in sections 15, 6c and 5b).  EVERY element of
 *      dx is written, +0.0 where no output pixel reaches it, and nothing else is.  Sizes that agree: dx is dy's values.
 *      One launch, no workspace.
 *
 *    rroi_merge_backward_hip:   dy, f (N, C, H, W), gate (N, 1, g_h, g_w) or NULL -> df (N, C, H, W) and / or
 *      dgate (N, 1, g_h, g_w); either may be NULL, not both; dgate needs the gate.  (da needs no call: it is dy where a has
 *      f's size and rroi_resize_backward_hip of dy otherwise; without a gate df is dy.)
 *        df = (T)(float)((double)dy * G), G recomputed per pixel exactly as section 8 computes it (1 without a gate):
 *          bit for bit a float64 restatement.
 *        dgate = R_g^T S,  S[n, Y, X] = sum over c of (double)dy * (double)f (each product exact in double): first per
 *          block of `channel_block` consecutive channels, c ascending, into the workspace ([n][block][pixel], doubles),
 *          then the blocks ascending (a launch of its own where there is more than one, in place into block 0), then the
 *          gather of rroi_resize_backward_hip on those doubles (the identity where the gate has f's size), one rounding to
 *          `dtype`.  The blocks are a function of (N, C, H, W) alone -- never of the device -- so the bits are the same on
 *          every device and run.  Two or three launches (df alone: one).
 *      The workspace: rroi_merge_backward_workspace_bytes(...) bytes at a 256-byte-aligned address where dgate is wanted;
 *      its contents before and after the call mean nothing.  Where dgate is NULL it is not needed: NULL / 0 is accepted
 *      and a buffer that is handed over is left alone.
 *
 *    No chain of additions exceeds 8192 terms: channel blocks hold at most 2048 channels, and the host refuses more than
 *    4096 blocks and a resize in which more than 4096 output rows (columns) would meet in one source row (column) --
 *    judged by an upper bound: out where in == 1, else min(out, (long long)(2 / s) + 2); a 2x resize has 5.
 *
 *    Returns 1 / 0 / -hipError.  0, before any launch: an unknown dtype, a dimension below 1, a tensor of 2^31 elements or
 *    more, the chain limits above, a NULL input or output pointer (dy, f always; the gate where dgate is wanted; df and
 *    dgate both NULL), an output overlapping an input or the other output, and -- where dgate is wanted -- a NULL workspace,
 *    one that is not a multiple of 256, or workspace_bytes below the size query's answer.  Every call only enqueues on
 *    `stream`, allocates nothing and can be captured into a HIP graph.
 *    Arrived after 0.10.0 under the same version string: detect it by symbol.
 * ------------------------------------------------------------------------- */
typedef struct rroi_resize_backward_plan_info {
    int vector_elems;    /* dx elements per lane: 1 */
    int channel_groups;  /* K: workgroups per tile, each on its own block of channels (the bits do not depend on it) */
    int tiles;           /* tiles of 256 dx pixels per image */
    int grid_x;          /* workgroups: N * K * tiles */
    int block;           /* threads per workgroup: 256 */
    int channel_block;   /* ceil(C / K) */
    int identity;        /* 1: the sizes agree, dx is dy's values */
    int max_rows;        /* the upper bound of the output rows that meet in one source row (refused above 4096) */
    int max_cols;        /* likewise for columns */
    double scale_y, scale_x;
} rroi_resize_backward_plan_info;
typedef struct rroi_merge_backward_plan_info {
    int vector_elems;    /* V: consecutive pixels per lane of the first launch: 4 */
    int channel_groups;  /* channel blocks, a function of the shape alone */
    int tiles;           /* tiles of 256 * V pixels per image */
    int grid_x;          /* workgroups of the first launch: N * channel_groups * tiles */
    int block;           /* threads per workgroup: 256 */
    int channel_block;   /* channels per block: at most 2048, at least 32 in the last one where there are several */
    int gate_tiles;      /* tiles of 256 gate pixels per image of the dgate launch (0 without a gate) */
    int gate_grid_x;     /* its workgroups: N * gate_tiles */
    int resize_gate;     /* 1: the gate is interpolated; 0: it has f's size (or there is none) */
    int launches;        /* of a call that wants dgate: 2, 3 with more than one channel block (df alone, or no gate: 1) */
    long long workspace_bytes;   /* what dgate needs: N * channel_groups * H * W doubles, rounded up to 256 (0 without a gate) */
    double gate_scale_y, gate_scale_x;
} rroi_merge_backward_plan_info;
int rroi_resize_forward_hip(int dtype, const void* x, void* y, int batch_size, int channels, int in_height, int in_width,
                            int height, int width, void* stream);
int rroi_resize_backward_hip(int dtype, const void* dy, void* dx, int batch_size, int channels, int in_height, int in_width,
                             int height, int width, void* stream);
/* host only: the output indices [*lo, *hi) of an axis resized from `in` to `out` whose taps reach source index i (empty:
 * *lo == *hi); 1, or 0 for in or out below 1, i outside [0, in) or a NULL pointer */
int rroi_resize_footprint(int in, int out, int i, int* lo, int* hi);
/* host only, no launch; 1, or 0 for arguments the call would refuse */
int rroi_resize_backward_plan(int dtype, int batch_size, int channels, int in_height, int in_width, int height, int width,
                              rroi_resize_backward_plan_info* plan);
int rroi_merge_backward_hip(int dtype, const void* dy, const void* f, const void* gate, void* df, void* dgate, int batch_size,
                            int channels, int height, int width, int g_h, int g_w, void* workspace, size_t workspace_bytes,
                            void* stream);
/* host only; what dgate needs for a gate of (g_h, g_w); 0 for arguments the call would refuse */
size_t rroi_merge_backward_workspace_bytes(int dtype, int batch_size, int channels, int height, int width, int g_h, int g_w);
/* host only, no launch; 1, or 0 for arguments the call would refuse; gated: 1 (g_h, g_w are the gate's size) or 0 */
int rroi_merge_backward_plan(int dtype, int batch_size, int channels, int height, int width, int g_h, int g_w, int gated,
                             rroi_merge_backward_plan_info* plan);

/* ------------------------------------------------------------------------- *
 * 9. The network's dense 3x3 convolution on the matrix cores, bfloat16 / float16:
 *    y = act(conv2d(x, w, stride, padding = 1)) in ONE launch.  Forward only; opt-in from Python
 *    (fots_e2e.native.use_native_conv3x3).
 *
 *      x   (N, Cin, H, W)      w   (Cout, Cin, 3, 3)      y   (N, Cout, Ho, Wo),  Ho = (H - 1) / stride + 1, Wo likewise
 *    all contiguous NCHW of one 16-bit element type `dtype` (RROI_DTYPE_BF16 / RROI_DTYPE_FP16); stride 1 or 2; no bias,
 *    groups 1, dilation 1; any Cin >= 1 and Cout >= 1.  act(v) = v < 0 ? v * negative_slope : v in fp32: 1.0 is no
 *    activation, 0.0 a ReLU.  Every element of y is written and nothing else is; nothing outside x is read (the padding
 *    is a zero fill inside the kernel); y may overlap no input.  Any element-aligned x, w and y work.
 *
 *    Arithmetic: an implicit GEMM on v_mfma_f32_32x32x16_{bf16,f16} with fp32 accumulators; products of two 16-bit values
 *    are exact in fp32; K = (tap, cin) is summed in an order the plan fixes (no atomic, no split of K across workgroups),
 *    so repeated calls give the same bits; ONE rounding from fp32 to the tensor's type, after the activation.  Not
 *    bit-exact against another summation order: with ref the exact convolution and S that of |x| with |w|,
 *    |y - act(ref)| <= 9 Cin 2^-23 S + u |act(ref)| (+ 2^-25 in fp16's subnormal range), u = 2^-8 (bf16) / 2^-11 (fp16).
 *
 *    Returns 1 / 0 / -hipError.  0, before any launch: fp32 or an unknown dtype, a dimension below 1, a stride other than
 *    1 or 2, x, w or y of 2^31 elements or more, a NULL x, w or y, a non-finite negative_slope.  Each call enqueues one
 *    kernel on `stream`, uses no workspace, allocates nothing and can be captured into a HIP graph.  Arrived after 0.10.0
 *    under the same version string: detect it by symbol.
 * ------------------------------------------------------------------------- */
typedef struct rroi_conv3x3_plan_info {
    int tile_m;      /* output channels per workgroup: 32 */
    int tile_h;      /* output rows per workgroup: 4 (one per wave) */
    int tile_w;      /* output columns per workgroup: 32 */
    int k_chunk;     /* input channels staged through LDS at a time: 16 */
    int k_chunks;    /* ceil(Cin / k_chunk) */
    int m_tiles, y_tiles, x_tiles;   /* tiles per image along Cout, Ho and Wo */
    int grid_x;      /* workgroups: N * m_tiles * y_tiles * x_tiles */
    int block;       /* threads per workgroup: 256 */
    int lds_bytes;   /* the input tile with its halo + the chunk's weights */
    int out_h, out_w;
    int reserved;
} rroi_conv3x3_plan_info;
int rroi_conv3x3_forward_hip(int dtype, const void* x, const void* w, void* y, int batch_size, int in_channels,
                             int out_channels, int height, int width, int stride, float negative_slope, void* stream);
/* host only, no launch; 1, or 0 for arguments the call would refuse */
int rroi_conv3x3_plan(int dtype, int batch_size, int in_channels, int out_channels, int height, int width, int stride,
                      rroi_conv3x3_plan_info* plan);

/* ------------------------------------------------------------------------- *
 * 10. The recogniser's tail and pools, two kernels of one launch each.  Forward only; opt-in from Python
 *    (fots_e2e.native.use_native_recogniser).
 *
 *    A. The head -- `log_softmax(conv11(x).squeeze(2), dim=1)` of tools/models.py: a 1x1 convolution with bias to the K
 *    classes and the log-softmax over them, reading x once and writing y once.
 *
 *      x   (N, C, T)   the contiguous (N, C, 1, T) map      w   (K, C)      b   (K) or NULL (+0.0)      y   (N, K, T)
 *    all contiguous, of one element type `dtype` (RROI_DTYPE_*); any C >= 1 and T >= 1; 1 <= K <=
 *    RROI_OCR_HEAD_MAX_CLASSES.  Every element of y is written and nothing else is; y may overlap no input.
 *
 *    Arithmetic per column (n, t), the recipe of section 7, fixed so that two identical calls give identical bits:
 *      every element of x, w and b is widened exactly to double where it is loaded
 *      z_k = ((b_k + w[k][0] x[0]) + w[k][1] x[1]) + ...   in channel order; every product is exact in double
 *      m = max_j z_j;   s = ((0 + exp(z_0 - m)) + exp(z_1 - m)) + ...   in class order;   L = m + log(s)
 *      out = (T)(float)(z_k - L)
 *    -- every operation rounded once in double (no contraction), one rounding to fp32 and one plain conversion to the
 *    tensor's type (nearest even, NaN kept).  The logits are never rounded to 16 bits.  A NaN or +inf logit, or a column
 *    whose logits are all -inf, makes that column's K outputs NaN; a -inf logit beside finite ones gives -inf in its own
 *    class alone; no other column is affected.  A zero weight times an inf is NaN (no channel is skipped).  The order
 *    depends on nothing but (C, K): not on the plan, an address or the device.
 *    Any element-aligned x, w, b and y work.
 *
 *    B. Activation + (2,1) max-pool -- `F.max_pool2d(F.leaky_relu(x, s), (2, 1), stride=(2, 1))`, bit for bit:
 *      x   (N, C, H, W)      y   (N, C, H / 2, W)     contiguous NCHW of one element type; H >= 2; an odd last row is dropped
 *      a = (T)act((float)x[2i][j]),  c = (T)act((float)x[2i + 1][j]),  act(v) = v < 0 ? v * negative_slope : v  (fp32);
 *      y[i][j] = c where c > a or c is a NaN, a otherwise: a NaN in either element gives NaN, a tie (signed zeros
 *      included) keeps the upper row's element.  negative_slope = 1.0 is the plain pool.
 *    Every element of y is written and nothing else is; y may not overlap x.  Any element-aligned x and y work.
 *
 *    Both return 1 / 0 / -hipError.  0, before any launch: an unknown dtype, a dimension below 1 (B: H below 2), K above
 *    RROI_OCR_HEAD_MAX_CLASSES, x, w or y of 2^31 elements or more, a NULL x, w or y, (B) a non-finite negative_slope.
 *    Each call enqueues one kernel on `stream`, uses no workspace, no atomics and no cache of repacked parameters,
 *    allocates nothing and can be captured into a HIP graph.  Arrived after 0.10.0 under the same version string: detect
 *    it by symbol.
 * ------------------------------------------------------------------------- */
#define RROI_OCR_HEAD_MAX_CLASSES 128
typedef struct rroi_ocr_head_plan_info {
    int class_block;     /* classes per wave: 32 (8 per row of 16 lanes) */
    int waves;           /* S: waves per workgroup, ceil(K / class_block) */
    int tile_columns;    /* columns per workgroup: 16 */
    int tiles;           /* tiles per crop: ceil(T / tile_columns) */
    int grid_x;          /* workgroups: N * tiles */
    int block;           /* threads per workgroup: 64 * S */
    int lds_bytes;       /* max(64 S, 16 K) doubles */
    int max_classes;     /* RROI_OCR_HEAD_MAX_CLASSES */
} rroi_ocr_head_plan_info;
int rroi_ocr_head_forward_hip(int dtype, const void* x, const void* w, const void* b, void* y, int batch_size, int channels,
                              int classes, int steps, void* stream);
/* host only, no launch; 1, or 0 for arguments the call would refuse */
int rroi_ocr_head_plan(int dtype, int batch_size, int channels, int classes, int steps, rroi_ocr_head_plan_info* plan);
int rroi_act_maxpool2x1_forward_hip(int dtype, const void* x, void* y, int batch_size, int channels, int height, int width,
                                    float negative_slope, void* stream);

/* ------------------------------------------------------------------------- *
 * 11. The network's bias-free 1x1 convolutions on the matrix cores, bfloat16 / float16, with the BatchNorm of a shortcut
 *    folded in, in ONE launch.  Forward only; opt-in from Python (fots_e2e.native.use_native_conv1x1).
 *
 *      y[n,k,i,j] = act( s[k] * sum_c w[k,c] * x[n,c,S*i,S*j] + t[k] )
 *
 *      x   (N, Cin, H, W)      w   (Cout, Cin) -- the contiguous (Cout, Cin, 1, 1) weight      y   (N, Cout, Ho, Wo),
 *      Ho = (H - 1) / S + 1, Wo likewise, S = stride, 1 or 2
 *    all contiguous NCHW of one 16-bit element type `dtype` (RROI_DTYPE_BF16 / RROI_DTYPE_FP16); no bias, groups 1; any
 *    Cin >= 1 and Cout >= 1.  act(v) = v < 0 ? v * negative_slope : v in fp32: 1.0 is no activation, 0.0 a ReLU.
 *
 *    The norm: bn_mean and bn_var (Cout each, both or neither), bn_weight and bn_bias (Cout each, both or both NULL: 1
 *    and 0), of the tensors' type, and eps.  s = g / sqrt(var + eps), t = b - mean * s, computed in fp32 by every workgroup
 *    for its own channel rows: no cache of folded parameters, no workspace.  With all four NULL no norm is applied: s and t
 *    do not exist and the result is the bare fp32 sum, rounded once.  bn_weight and bn_bias without bn_mean and bn_var
 *    are refused.
 *
 *    Every element of y is written and nothing else is; nothing outside x, w and the vectors is read; y may overlap no
 *    input.  Any element-aligned x, w, y and vectors work (16-byte loads are decided per item inside the kernel).
 *
 *    Arithmetic: a GEMM per image on v_mfma_f32_32x32x16_{bf16,f16} with fp32 accumulators; products of two 16-bit values
 *    are exact in fp32; Cin is summed in an order the plan fixes (no atomic, no split of K across workgroups), so repeated
 *    calls give the same bits; s * sum + t as one fp32 multiply and one fp32 add; ONE rounding from fp32 to the tensor's
 *    type, after the activation.  With ref the exact sum, A that of |w| |x|, u = 2^-8 (bf16) / 2^-11 (fp16):
 *      no norm:  |y - act(ref)| <= Cin 2^-23 A + u |act(ref)| (+ 2^-25 in fp16's subnormal range)
 *      norm:     |y - act(z)| <= |s| Cin 2^-23 A + 2^-20 (|s| (A + |mean|) + |b|) + u |act(z)| (+ 2^-25),  z = s ref + t
 *
 *    Returns 1 / 0 / -hipError.  0, before any launch: fp32 or an unknown dtype, a dimension below 1, a stride other than
 *    1 or 2, x, w or y of 2^31 elements or more, a NULL x, w or y, a non-finite negative_slope, a non-finite or negative
 *    eps, bn_weight and bn_bias not both NULL or both given, bn_mean and bn_var likewise, an affine pair without
 *    statistics.  Each call enqueues one kernel on `stream`, allocates nothing and can be captured into a HIP graph.
 *    Arrived after 0.10.0 under the same version string: detect it by symbol.
 * ------------------------------------------------------------------------- */
typedef struct rroi_conv1x1_plan_info {
    int tile_m;      /* output channels per workgroup: 32 or 64 */
    int tile_p;      /* output pixels per workgroup, flat over the output plane: 128 (32 per wave) */
    int k_chunk;     /* input channels staged through LDS at a time: 64 */
    int k_chunks;    /* ceil(Cin / k_chunk) */
    int m_tiles, p_tiles;   /* tiles per image along Cout and along Ho * Wo */
    int grid_x;      /* workgroups: N * m_tiles * p_tiles */
    int block;       /* threads per workgroup: 256 */
    int lds_bytes;   /* the chunk's pixels and weights + the folded norm of the tile's channels */
    int out_h, out_w;
    int reserved;
} rroi_conv1x1_plan_info;
int rroi_conv1x1_forward_hip(int dtype, const void* x, const void* w, void* y, int batch_size, int in_channels,
                             int out_channels, int height, int width, int stride, float negative_slope,
                             const void* bn_weight, const void* bn_bias, const void* bn_mean, const void* bn_var, double eps,
                             void* stream);
/* host only, no launch; 1, or 0 for arguments the call would refuse */
int rroi_conv1x1_plan(int dtype, int batch_size, int in_channels, int out_channels, int height, int width, int stride,
                      rroi_conv1x1_plan_info* plan);

/* ------------------------------------------------------------------------- *
 * 12. The recogniser's (2,3) convolution on the matrix cores, bfloat16 / float16:
 *    y = act(conv2d(x, w, stride 1, padding (0, 1))) in ONE launch.  Forward only; opt-in from Python
 *    (fots_e2e.native_remainder.use_native_conv2x3).  Section 9's conventions.
 *
 *      x   (N, Cin, H, W), H >= 2      w   (Cout, Cin, 2, 3)      y   (N, Cout, H - 1, W)
 *    all contiguous NCHW of one 16-bit element type `dtype` (RROI_DTYPE_BF16 / RROI_DTYPE_FP16); no bias, groups 1,
 *    dilation 1; any Cin >= 1, Cout >= 1 and W >= 1.  act(v) = v < 0 ? v * negative_slope : v in fp32: 1.0 is no
 *    activation, 0.0 a ReLU.  Every element of y is written once and nothing else is; nothing outside x and w is read (the
 *    padding is a zero fill inside the kernel); y may overlap no input.  Any element-aligned x, w and y work.
 *
 *    Arithmetic: an implicit GEMM on v_mfma_f32_32x32x16_{bf16,f16} with fp32 accumulators; K = (ky, kx, cin) is summed in
 *    a fixed order (no atomic, no split of K), so repeated calls give the same bits; ONE rounding from fp32 to the tensor's
 *    type, after the activation.  With ref the exact convolution and S that of |x| with |w|,
 *    |y - act(ref)| <= 6 Cin 2^-23 S + u |act(ref)| (+ 2^-25 in fp16), u = 2^-8 (bf16) / 2^-11 (fp16).
 *
 *    Returns 1 / 0 / -hipError.  0, before any launch: fp32 or an unknown dtype, H < 2, another dimension below 1, x, w or
 *    y of 2^31 elements or more, a NULL x, w or y, a non-finite negative_slope.  Each call enqueues one kernel on
 *    `stream`, uses no workspace, allocates nothing and can be captured into a HIP graph.  Arrived after 0.10.0 under the
 *    same version string: detect it by symbol.
 * ------------------------------------------------------------------------- */
typedef struct rroi_conv2x3_plan_info {
    int tile_m;      /* output channels per workgroup: 32 */
    int tile_w;      /* output columns per item: 32 */
    int wave_items;  /* items (one output row x tile_w columns of one image) per workgroup, one per wave: 4 */
    int k_chunk;     /* input channels staged through LDS at a time: 32 */
    int k_chunks;    /* ceil(Cin / k_chunk) */
    int m_tiles;     /* ceil(Cout / tile_m) */
    int x_tiles;     /* ceil(W / tile_w) */
    int items;       /* N * (H - 1) * x_tiles */
    int grid_x;      /* workgroups: ceil(items / wave_items) * m_tiles */
    int block;       /* threads per workgroup: 256 */
    int lds_bytes;   /* the items' input tiles with their halo columns + the chunk's weights, rows padded by 8 elements */
    int out_h, out_w;
    int reserved;
} rroi_conv2x3_plan_info;
int rroi_conv2x3_forward_hip(int dtype, const void* x, const void* w, void* y, int batch_size, int in_channels,
                             int out_channels, int height, int width, float negative_slope, void* stream);
/* host only, no launch; 1, or 0 for arguments the call would refuse */
int rroi_conv2x3_plan(int dtype, int batch_size, int in_channels, int out_channels, int height, int width,
                      rroi_conv2x3_plan_info* plan);

/* ------------------------------------------------------------------------- *
 * 13. Bilinear resize + depthwise 3x3 convolution in ONE launch: y = depthwise3x3(U, w), stride 1,
 *    padding 1, where U is `a` resized to (out_height, out_width) and rounded to the tensors' type -- the resize in front
 *    of the network's `upconv1` / `upconv2` with the depthwise half of the block.  Forward only; opt-in from Python
 *    (fots_e2e.native_remainder.use_native_upconv).
 *
 *      a   (N, C, in_height, in_width)      w   (C, 1, 3, 3)      y   (N, C, out_height, out_width)
 *    all contiguous NCHW of one element type `dtype` (fp32, bf16 or fp16); any sizes >= 1 on both sides.
 *
 *    Arithmetic: U[n, c] = (T)(float) of section 8's resize (bilinear, align_corners = true, in double, the scale
 *    (in - 1) / (out - 1) computed on the host, 0 where out == 1, every operation rounded to double; a source that already
 *    has the target's size is read as it is), then section 5's recipe on those rounded values: a double accumulator, ky
 *    then kx ascending, a tap outside U is w * (+0.0) and is never skipped, the result (T)(float)acc.  So y is, bit for
 *    bit, what rroi_depthwise3x3_forward_hip gives on the rounded resized map; that map is never stored.
 *
 *    Returns 1 / 0 / -hipError.  0, before any launch: an unknown dtype, a dimension below 1, a or y of 2^31 elements or
 *    more, a NULL a, w or y.  Each call enqueues one kernel on `stream`, uses no workspace, allocates nothing, works for any
 *    element-aligned addresses and can be captured into a HIP graph.  Arrived after 0.10.0 under the same version string:
 *    detect it by symbol.
 * ------------------------------------------------------------------------- */
int rroi_up_depthwise3x3_forward_hip(int dtype, const void* a, const void* weight, void* y, int batch_size, int channels,
                                     int in_height, int in_width, int out_height, int out_width, void* stream);

/* ------------------------------------------------------------------------- *
 * 14. Native preprocessing: the uploaded bytes of a whole batch of images to the network's input tensor in
 *    ONE launch -- the half-pixel bilinear resize, `/ 128 - 1` and the rounding to the network's type that
 *    fots_e2e.pipeline.preprocess runs as a chain of stock operators per image.  Opt-in from Python
 *    (fots_e2e.pipeline.preprocess_batch, the pipeline's native_preprocess keyword).
 *
 *      src     one device buffer of bytes: the batch's images back to back, image n (H0_n, W0_n, 3) interleaved, the
 *              channel order kept as it is
 *      table   (N, 4) int32 on the device: {byte offset of image n in src, H0_n, W0_n, 0}.  Offsets need NO alignment
 *              (3 * H0 * W0 is rarely a multiple of 4) and the source sizes may differ from image to image.  The rows
 *              are TRUSTED, as ROI rows are: an offset or a size that points outside src is read out of bounds.
 *      y       (N, 3, out_height, out_width) contiguous NCHW of `dtype` (fp32, bf16 or fp16)
 *    Any sizes >= 1 on both sides.
 *
 *    Arithmetic -- the whole contract; every operation rounded to double, in this order.  Per axis with source extent n0
 *    and output extent n:  n0 == n: i0 = i1 = i, l = 0 (the source is read as it is);  otherwise
 *      s = max(0, (i + 0.5) * ((double)n0 / (double)n) - 0.5),  i0 = min((int)floor(s), n0 - 1),  i1 = min(i0 + 1, n0 - 1),
 *      l = s - i0.
 *    top = (1 - lx) * p[y0][x0] + lx * p[y0][x1], bot likewise on row y1, v = (1 - ly) * top + ly * bot,
 *    out = (T)(float)(v / 128.0 - 1.0) ((float) alone for fp32): F.interpolate(mode="bilinear", align_corners=False)
 *    followed by test.py:77-83's scaling, evaluated in double and rounded once.  Where no resize is needed the fp32
 *    result is bit for bit the stock chain's (p / 128 - 1 is exact).
 *
 *    Returns 1 / 0 / -hipError.  0, before any launch: an unknown dtype, batch_size < 0, out_height or out_width below 1,
 *    a y of 2^31 elements or more, a NULL src, table or y with batch_size > 0.  batch_size == 0 is 1 and launches nothing.
 *    Each call enqueues one kernel on `stream`, uses no workspace, allocates nothing and can be captured into a HIP graph.
 *    Any element-aligned y works: 16-byte stores are used where out_width is a multiple of columns_per_thread AND y is
 *    16-byte aligned, element stores otherwise; every element of y is written once and nothing else is.  Arrived after
 *    0.10.0 under the same version string: detect it by symbol.
 * ------------------------------------------------------------------------- */
typedef struct rroi_preprocess_plan_info {
    int grid_x;              /* workgroups: ceil(items / block); 0 for batch_size == 0 */
    int block;               /* threads per workgroup: 256, one item each */
    int columns_per_thread;  /* consecutive output columns of an item, all three channels: 16 bytes' worth, 4 (fp32) or 8 */
    int rows_per_thread;     /* consecutive output rows of an item: 1, 2 or 4 (grows while the grid keeps 1024 waves) */
    int strips;              /* ceil(out_width / columns_per_thread) */
    int bands;               /* ceil(out_height / rows_per_thread) */
    int items;               /* batch_size * bands * strips */
    int wide_store;          /* 1: out_width % columns_per_thread == 0, 16-byte stores for a 16-byte aligned y */
} rroi_preprocess_plan_info;
int rroi_preprocess_forward_hip(int dtype, const unsigned char* src, const int* table, void* y, int batch_size,
                                int out_height, int out_width, void* stream);
/* host only, no launch; 1, or 0 for arguments the call would refuse */
int rroi_preprocess_plan(int dtype, int batch_size, int out_height, int out_width, rroi_preprocess_plan_info* plan);

/* ------------------------------------------------------------------------- *
 * 15. The native CTC loss: the negative log-likelihood of every sequence and, where wanted, its UNSCALED
 *    gradient with respect to the log-probabilities, in ONE launch -- deterministic (no atomic, every sum in a fixed
 *    order: the same bits on every run), for fp32, bf16 and fp16 log-probabilities read where they lie.  Opt-in from
 *    Python (rroi_align.ctc.ctc_loss, fots_e2e.train.recognition_loss(native_ctc=True)).
 *
 *      log_probs        element (t, n, k) at log_probs[t * stride_t + n * stride_n + k * stride_k], t < steps, n < batch_size,
 *                       k < classes; any element strides (loads and stores coalesce where stride_t or stride_k is 1)
 *      targets          (batch_size, max_target_length) contiguous int32, row n holding target_lengths[n] labels
 *      input_lengths    (batch_size) int32 on the device, T_n
 *      target_lengths   (batch_size) int32 on the device, L_n
 *      nll              (batch_size) float32
 *      grad             NULL, or the gradient tensor with element strides of its own; every element (t, n, k) is written
 *                       exactly once, zeros included, so the caller neither clears it nor reads it before
 *      workspace        rroi_ctc_loss_workspace_bytes(...) bytes, 8-byte aligned (0 bytes: may be NULL)
 *
 *    Arithmetic -- the whole contract, every operation in double.  lp = log_probs widened exactly; l' = the target with
 *    blanks interleaved, S = 2 L + 1; lse(...) = m + log(sum of exp(x - m)), m the largest argument, -inf where m is:
 *      alpha_0(0) = lp[blank, 0], alpha_0(1) = lp[l_1, 0], -inf elsewhere
 *      alpha_t(s) = lp[l'_s, t] + lse(alpha_{t-1}(s), alpha_{t-1}(s-1), [alpha_{t-1}(s-2) if l'_s != blank and != l'_{s-2}])
 *      nll_n      = -lse(alpha_{T_n-1}(S-1), alpha_{T_n-1}(S-2)); T_n == 0: 0 if L_n == 0, else +inf
 *      beta the mirror image;  for t < T_n, with lp[k, t] and nll_n finite,
 *      grad[t, n, k] = exp(lp) - exp(lse_{s : l'_s = k}(alpha_t(s) + beta_t(s)) + nll_n - lp)
 *    -- torch.nn.functional.ctc_loss's gradient for grad_output = 1.  The gradient is 0 for t >= T_n, 0 where lp is -inf,
 *    and 0 for a sequence whose nll is +inf (torch leaves NaN in the last two cases).  nll is rounded to float32, the
 *    gradient once from double to `dtype`.  With zero_infinity an infinite nll is stored as 0.
 *    A sequence is INFEASIBLE -- nll +inf, gradient 0 -- where T_n is outside [0, steps], L_n outside
 *    [0, min(max_target_length, steps)], or one of its L_n labels outside [0, classes).  This is decided before anything is
 *    read through a length or a label: no contents of the three integer tensors make the call read or write out of bounds.
 *
 *    Returns 1 / 0 / -hipError.  0, before any launch: an unknown dtype, batch_size, steps or max_target_length below 0,
 *    classes below 1, blank outside [0, classes), a shape whose per-sequence arrays exceed the 64 KiB of LDS the kernel may
 *    use even at one step per chunk (60 * S_max + 8 * classes + 4 bytes, S_max = 2 * min(max_target_length, steps) + 1), a NULL log_probs, input_lengths, target_lengths
 *    or nll -- or targets with max_target_length > 0 -- with batch_size > 0, a workspace that is needed and NULL, short or
 *    not 8-byte aligned.  batch_size == 0 is 1 and launches nothing.  Each call enqueues one kernel on `stream`, allocates
 *    nothing and can be captured into a HIP graph.  Arrived after 0.10.0 under the same version string: detect it by symbol.
 * ------------------------------------------------------------------------- */
typedef struct rroi_ctc_loss_plan_info {
    int grid_x;              /* workgroups: one per sequence */
    int block;               /* threads per workgroup: 256; thread s owns position s of l' */
    int lds_bytes;           /* dynamic LDS of the launch, <= lds_limit */
    int lds_limit;           /* 65536 */
    int positions;           /* S_max = 2 * min(max_target_length, steps) + 1 */
    int chunk_steps;         /* time steps staged, and gradient rows stored, at a time: 16, halved while the chunk's arrays
                                (chunk_steps * (2 * positions + classes) doubles) exceed half of lds_limit */
    int stage_along_t;       /* 1: log_probs is staged with consecutive lanes along t (stride_t == 1, stride_k != 1); 0: along
                                positions / classes.  The gradient's stores choose likewise by the gradient's own strides. */
    int alpha_in_workspace;  /* with a gradient: 0 = every alpha and beta row is kept in LDS, 1 = in the workspace (2 * T * S_max
                                doubles per sequence did not fit); 0 without a gradient, which keeps two rows only */
} rroi_ctc_loss_plan_info;
int rroi_ctc_loss_forward_hip(int dtype, const void* log_probs, long long stride_t, long long stride_n, long long stride_k,
                              int batch_size, int classes, int steps, const int* targets, int max_target_length,
                              const int* input_lengths, const int* target_lengths, int blank, int zero_infinity, float* nll,
                              void* grad, long long grad_stride_t, long long grad_stride_n, long long grad_stride_k,
                              void* workspace, size_t workspace_bytes, void* stream);
/* host only, no launch; 1, or 0 for arguments the call would refuse.  want_grad: whether the call passes a gradient. */
int rroi_ctc_loss_plan(int dtype, int batch_size, int classes, int steps, int max_target_length, long long stride_t,
                       long long stride_k, int want_grad, rroi_ctc_loss_plan_info* plan);
/* host only: bytes of workspace the call needs (0: none; also 0 for arguments the call would refuse) */
size_t rroi_ctc_loss_workspace_bytes(int batch_size, int classes, int steps, int max_target_length, int want_grad);

/* ------------------------------------------------------------------------- *
 * 16. The native detection loss: the reference's ModelResNetSep2.loss -- a dice term on the score maps, a
 *    masked mean-squared error on the angle maps, an IoU term on the left and right halves of the boxes, on the 1/4 scale
 *    and on the 1/8 scale -- and its gradient with respect to the six predictions.  Forward is two launches (partial sums,
 *    finish), backward one; no host synchronisation, no atomic, every sum in a fixed order that depends on the shape alone:
 *    the same bits on every run and on every device.  Opt-in from Python (rroi_align.detection.detection_loss,
 *    fots_e2e.train.detection_loss(native=True)).
 *
 *      segm4, angle4, roi4   (N, 1, H, W), (N, 2, H, W), (N, 4, H, W) contiguous, of `dtype` (fp32, bf16, fp16)
 *      segm8, angle8, roi8   the same at (H8, W8), any H8, W8 >= 1; all NULL with height8 == width8 == 0 (a single scale)
 *      segm_gt, iou_mask, angle_gt   (N, H, W) contiguous float32
 *      roi_gt                (N, H, W, 4) contiguous float32 {top, bottom, left, right}, 16-byte aligned
 *      terms                 4 float32: {segm, angle, box, total}
 *      workspace             rroi_detection_loss_workspace_bytes(...) bytes, 8-byte aligned: grid_x slots of 10 doubles,
 *                            then the STATE of 20 doubles, which the backward call reads (pass workspace + 80 * grid_x bytes,
 *                            or a copy of those 160 bytes)
 *      grad_terms            4 float32 on the device: the gradient arriving at `terms`; read by the kernel, never by the host
 *      grad_*                the six gradients, shaped and typed like the predictions; every element is written exactly
 *                            once, zeros included, so the caller neither clears them nor reads them before
 *
 *    Arithmetic -- the whole contract, every operation in double, predictions widened exactly.  Per scale and pixel:
 *      1/4:  g = segm_gt, m = iou_mask, th = angle_gt, (d1, d2, d3, d4) = roi_gt, as they lie
 *      1/8:  each of the seven planes resized to (H8, W8), bilinear with align_corners = true by section 8's recipe --
 *            s = (in - 1) / (out - 1) (0 where out == 1), src = s * dst, i0 = min((int)src, in - 1), i1 = min(i0 + 1, in - 1),
 *            l1 = src - i0, l0 = 1 - l1, value = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11) -- and the four
 *            roi planes then halved; nothing resized is ever stored
 *      mask = g > 0.5 (of the double value);  p, (a0, a1), (r1, r2, r3, r4) the predictions
 *      I = sum (p m)(g m),  P = sum p m,  G = sum g m;                          dice = -(2 I + 1) / (P + G + 1)
 *      over mask: c = count, Ss = sum (a0 - sin th)^2, Sc = sum (a1 - cos th)^2;  angle = Ss / c + Sc / c
 *      over mask and d3 > 0:  X = min(d3, r3) (min(d1, r1) + min(d2, r2)),  U = (d1 + d2) d3 + (r1 + r2) r3 - X,
 *            Ll = sum -log((X + 1) / (U + 1)), nl = count;  likewise Lr, nr with d4, r4 over mask and d4 > 0
 *      box = Ll / nl + Lr / nr
 *      segm = dice4 + dice8, angle = angle4 + angle8, box = box4 + box8, total = segm + 2 angle + 0.5 box, to float32.
 *    A quotient whose count is 0 -- no pixel above 0.5, or none with d3 > 0 or d4 > 0 -- contributes 0 and a zero gradient
 *    (the reference gives NaN for an empty left or right selection).
 *    Summation order: thread t of workgroup b adds items (b' 256 ipt) + t, + 256, ... in ascending order (b' the workgroup's
 *    index within its scale); the workgroup's sum is a butterfly over each wave's 64 lanes (offsets 1, 2, ..., 32), then waves
 *    0..3 in ascending order; the finish adds the slots of a scale in ascending order.
 *    Gradient, for grad_terms = g: w_segm = g[0] + g[3], w_angle = g[1] + 2 g[3], w_box = g[2] + 0.5 g[3];
 *      d/dp = w_segm (m (2 I + 1) / (P + G + 1)^2 - g m m 2 / (P + G + 1))
 *      d/da0 = (2 w_angle / c)(a0 - sin th) on the mask, d/da1 with cos; 0 off it
 *      d/dr: from L = log(U + 1) - log(X + 1), with min's gradient going to the smaller side and a tie split in half
 *            (torch's rule), each half scaled by w_box / nl or w_box / nr; 0 off the mask
 *    each rounded once from double to `dtype` (the 16-bit types through a float rounded to odd, as in section 15).
 *    Nothing is indexed by a value read from a tensor: no contents of the ground truth take a kernel out of bounds.
 *
 *    Returns 1 / 0 / -hipError.  0, before any launch: an unknown dtype, batch_size, height or width below 1, height8 or
 *    width8 below 0 or only one of them 0, more than 2^30 pixels on a scale, a NULL tensor that the shape needs, roi_gt not
 *    16-byte aligned, a workspace that is NULL, short or not 8-byte aligned, a NULL or misaligned state or grad_terms.
 *    The calls allocate nothing and can be captured into a HIP graph.  Arrived after 0.10.0 under the same version string:
 *    detect it by symbol.
 * ------------------------------------------------------------------------- */
typedef struct rroi_detection_loss_plan_info {
    int grid_x;              /* workgroups of the partial-sum launch and of the backward launch: blocks_quarter + blocks_eighth */
    int block;               /* threads per workgroup: 256 */
    int items_per_thread;    /* 1 up to 4096 items (pixels of both scales), 2 up to 16384, 4 up to 262144, 8 beyond */
    int blocks_quarter;      /* ceil(N H W / (block * items_per_thread)): the workgroups of the 1/4 scale, which come first */
    int blocks_eighth;       /* ceil(N H8 W8 / (block * items_per_thread)); 0 for a single scale */
    int slot_doubles;        /* doubles a workgroup writes to its slot of the workspace: 10 */
    int state_doubles;       /* doubles of the state behind the slots: 20 */
    int finish_block;        /* threads of the one finishing workgroup: 64 */
} rroi_detection_loss_plan_info;
int rroi_detection_loss_forward_hip(int dtype, const void* segm4, const void* angle4, const void* roi4, const void* segm8,
                                    const void* angle8, const void* roi8, const float* segm_gt, const float* iou_mask,
                                    const float* angle_gt, const float* roi_gt, int batch_size, int height, int width, int height8,
                                    int width8, float* terms, void* workspace, size_t workspace_bytes, void* stream);
int rroi_detection_loss_backward_hip(int dtype, const void* angle4, const void* roi4, const void* angle8, const void* roi8,
                                     const float* segm_gt, const float* iou_mask, const float* angle_gt, const float* roi_gt,
                                     int batch_size, int height, int width, int height8, int width8, const double* state,
                                     const float* grad_terms, void* grad_segm4, void* grad_angle4, void* grad_roi4, void* grad_segm8,
                                     void* grad_angle8, void* grad_roi8, void* stream);
/* host only, no launch; 1, or 0 for arguments the calls would refuse.  A pure function of its arguments: never of the device. */
int rroi_detection_loss_plan(int dtype, int batch_size, int height, int width, int height8, int width8,
                             rroi_detection_loss_plan_info* plan);
/* host only: bytes of workspace the forward call needs, (10 * grid_x + 20) * 8; 0 for arguments the calls would refuse */
size_t rroi_detection_loss_workspace_bytes(int batch_size, int height, int width, int height8, int width8);

/* Bin centres only: geom (R, PH, PW, 2) = (bin_cx, bin_cy), 0 where the bin is
 * outside the ROI's pooled width (kernel.cu:86-107).  Diagnostic / test hook. */
int rroi_align_bin_centres_hip(float spatial_scale, int num_rois, int height, int width,
                               int pooled_height, int pooled_width, const float* rois,
                               float* geom, void* stream);
/* ... with the trig recipe stated (RROI_TRIG_DOUBLE / RROI_TRIG_FP32; the function above = RROI_TRIG_DOUBLE). */
int rroi_align_bin_centres_trig_hip(float spatial_scale, int num_rois, int height, int width,
                                    int pooled_height, int pooled_width, const float* rois,
                                    float* geom, int trig_recipe, void* stream);

/* (float)cos((double)x), (float)sin((double)x) of n angles given in degrees,
 * through the same device code the kernels use (test hook for the one
 * library-dependent step of the arithmetic recipe). out = (n, 2). */
int rroi_align_sincos_probe_hip(const float* angle_deg, int n, float* out, void* stream);

/* Measurement hook: fills out[0 .. num_floats) (16-byte aligned, a multiple of 4 floats) with values that differ
 * from store to store, one 16-byte plain store per thread.  bench.py times it on the output buffer as the ceiling
 * a write of non-zero, non-constant data reaches on the box (zeros are written faster on this chip). */
int rroi_align_write_probe_hip(float* out, size_t num_floats, void* stream);

/* DEPRECATED shims of the per-device setter / getter of versions 0.5-0.6 (removed in 0.7.0 without one, ADVICE r05;
 * they go away in 0.9): the recipe travels in `path` now.  set: 1 for RROI_TRIG_DOUBLE (what every call without the
 * RROI_PATH_TRIG_FP32 bit runs: nothing to do), 0 for RROI_TRIG_FP32 or anything else -- the library has no device-wide
 * state left to change, so the request is REFUSED rather than silently ignored; get: RROI_TRIG_DOUBLE. */
int rroi_align_set_trig_recipe_hip(int recipe);
int rroi_align_get_trig_recipe_hip(void);

/* Identification: "rroi_align_hip <version> gfx950" (0.7.0: per-call trig recipe, device-wide setter removed; 0.8.0: launcher scratch reused within a capture, table of 64, stats; 0.9.0: plan query; 0.10.0: bfloat16 / float16 tensors).
 * The typed callers' entry points (rroi_rbox_decode_typed_hip, rroi_ctc_greedy_decode_typed_hip) arrived after 0.10.0 under
 * the same version string: a caller detects them by symbol.  So did the bucketed calls of section 2b, the depthwise
 * convolution of section 5, the InstanceNorm of section 6, its fused epilogues of section 6b, its training calls of section 6c, the heads and gate of section 7, the gated merge
 * of section 8, the dense 3x3 convolution of section 9, the recogniser's head and activation + pool of section 10 and the 1x1
 * convolution of section 11, the calls of sections 12 to 16, and the backward calls of sections 5b and 8b. */
const char* rroi_align_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RROI_ALIGN_HIP_H */
