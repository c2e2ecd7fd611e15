// rroi_align_hip.hip -- RoIRotate (rroi_align) for MI355X / gfx950 (CDNA4).
//
// Written from scratch for wave64 / LDS / per-XCD-L2 hardware; it replaces the
// reference's CUDA kernels (rroi_align/src/rroi_align_kernel.cu:28-162 forward,
// :193-278 backward, launchers :164-187 / :280-312) behind the C-ABI declared in
// include/rroi_align_hip.h.  Build: -ffp-contract=off (the arithmetic recipe of
// the bin geometry is rounding-exact; see DESIGN.md "Arithmetic recipe").
//
// Design in one paragraph.  A bin's sample point depends on (roi, ph, pw) only,
// never on the channel, and its 4 taps are whole pixels.  The op is therefore a
// pixel gather replicated over C channels plus a 256 MiB streaming write.  In
// NCHW the channels of a pixel are H*W apart (one cache line per channel), so
// the hot path first relays the map out CHUNK-MAJOR: (B, C/32, H*W+1, 32) --
// 32 channels of a pixel are one 128-byte line, consecutive pixels of a chunk
// are consecutive lines (all L2 channels of an XCD are used evenly), and every
// (image, chunk) slice is one buffer descriptor, whose range check turns invalid
// taps into 0.0.  A workgroup (a gatherer and a storer wave) then owns a
// [32 channel] x [64 bin] output tile at a time: lanes = 8 bins x 8
// channel-quads fetch taps as 16-byte loads, blend in the reference's order,
// transpose through an LDS tile, and the tile streams out as full
// 256-byte row segments of the (R,C,PH,PW) tensor.  Channel chunk k is handled
// by blocks with blockIdx % nchunks == k, i.e. (8 chunks at C=256) by one XCD,
// whose 4 MiB L2 then holds exactly its 3.2 MB slice of the map.
//
// Files: this one holds the C-ABI (each entry point: argument checks, plan, NULL checks, launch); everything else is
// in parts that are included below, inside the anonymous namespace.  Device code: rroi_device_common.h (constants,
// geometry recipe, descriptor helpers), rroi_forward_kernels.h, rroi_backward_kernels.h, rroi_backward_tile_kernels.h,
// rroi_callers_kernels.h, rroi_nms_kernels.h (+ rroi_nms_host.h, host C++), rroi_depthwise_kernels.h (+ rroi_depthwise_host.h:
// the network's depthwise 3x3 convolution), rroi_instancenorm_kernels.h (+ rroi_instancenorm_host.h: its
// InstanceNorm2d with the activation behind it), rroi_heads_kernels.h (+ rroi_heads_host.h: its detection heads
// and attention gate), rroi_merge_kernels.h (+ rroi_merge_host.h: the gated merge of its feature merge,
// DESIGN 5.14), rroi_conv3x3_kernels.h (+ rroi_conv3x3_host.h: its dense 3x3 convolutions on the matrix cores, bfloat16 /
// float16), rroi_recogniser_kernels.h (+ rroi_recogniser_host.h: the recogniser's log-softmax head and its
// activation + (2,1) max-pool), rroi_conv1x1_kernels.h (+ rroi_conv1x1_host.h: its bias-free 1x1 convolutions on
// the matrix cores with the shortcut's BatchNorm folded in, bfloat16 / float16), rroi_conv2x3_kernels.h
// (+ rroi_conv2x3_host.h: the recogniser's (2,3) convolution on the matrix cores, bfloat16 / float16),
// rroi_updw_kernels.h (+ rroi_updw_host.h: the bilinear resize and the depthwise 3x3 behind it in one launch),
// rroi_preprocess_kernels.h (+ rroi_preprocess_host.h: uint8 images to the network's input tensor in one launch),
// rroi_ctc_loss_kernels.h (+ rroi_ctc_loss_host.h: the CTC loss and its unscaled gradient in one launch),
// rroi_detection_loss_kernels.h (+ rroi_detection_loss_host.h: the detection loss and its gradient),
// rroi_instancenorm_backward_kernels.h (+ rroi_instancenorm_backward_host.h: the InstanceNorm's training forward and its
// backward), rroi_depthwise_backward_kernels.h (+ rroi_depthwise_backward_host.h: the depthwise 3x3
// convolution's input and weight gradients), rroi_merge_backward_kernels.h (+ rroi_merge_backward_host.h: the
// gated merge's backward, the stand-alone resize and its backward), rroi_heads_backward_kernels.h
// (+ rroi_heads_backward_host.h: the heads' and the gate's training forward and their backward).
// Host side: rroi_host_plan.h (tuning table,
// Shape, limits, workspace carvers, the dispatch: what a call launches, down to every grid), rroi_host_scratch.h (the
// launchers' scratch), rroi_host_launch.h (the launches: one function per kernel template, run from the plan's fields).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

#include "rroi_align_hip.h"

#pragma clang fp contract(off)

namespace {

#include "rroi_device_common.h"
#include "rroi_forward_kernels.h"
#include "rroi_backward_kernels.h"
#include "rroi_backward_tile_kernels.h"
#include "rroi_callers_kernels.h"
#include "rroi_nms_kernels.h"
#include "rroi_nms_host.h"
#include "rroi_depthwise_kernels.h"
#include "rroi_instancenorm_kernels.h"
#include "rroi_heads_kernels.h"
#include "rroi_merge_kernels.h"
#include "rroi_conv3x3_kernels.h"
#include "rroi_recogniser_kernels.h"
#include "rroi_conv1x1_kernels.h"
#include "rroi_conv2x3_kernels.h"
#include "rroi_updw_kernels.h"
#include "rroi_preprocess_kernels.h"
#include "rroi_ctc_loss_kernels.h"
#include "rroi_detection_loss_kernels.h"
#include "rroi_instancenorm_backward_kernels.h"
#include "rroi_depthwise_backward_kernels.h"
#include "rroi_merge_backward_kernels.h"
#include "rroi_heads_backward_kernels.h"

#include "rroi_host_plan.h"
#include "rroi_host_scratch.h"
#include "rroi_host_launch.h"
#include "rroi_depthwise_host.h"
#include "rroi_instancenorm_host.h"
#include "rroi_heads_host.h"
#include "rroi_merge_host.h"
#include "rroi_conv3x3_host.h"
#include "rroi_recogniser_host.h"
#include "rroi_conv1x1_host.h"
#include "rroi_conv2x3_host.h"
#include "rroi_updw_host.h"
#include "rroi_preprocess_host.h"
#include "rroi_ctc_loss_host.h"
#include "rroi_detection_loss_host.h"
#include "rroi_instancenorm_backward_host.h"
#include "rroi_depthwise_backward_host.h"
#include "rroi_merge_backward_host.h"
#include "rroi_heads_backward_host.h"

}  // namespace

// ====================================================================================
extern "C" {

const char* rroi_align_hip_version(void) { return "rroi_align_hip 0.10.0 gfx950"; }

size_t rroi_align_forward_workspace_bytes(int batch_size, int channels, int height, int width,
                                          int num_rois, int feature_layout)
{
    if (batch_size <= 0 || channels <= 0 || height <= 0 || width <= 0 || num_rois < 0) return 0;
    return carve(nullptr, Shape{batch_size, num_rois, height, width, channels, 0, 0}, feature_layout).bytes;
}

size_t rroi_align_backward_workspace_bytes(int batch_size, int channels, int height, int width,
                                           int num_rois, int pooled_height, int pooled_width)
{
    if (batch_size <= 0 || channels <= 0 || height <= 0 || width <= 0 || num_rois < 0 ||
        pooled_height <= 0 || pooled_width <= 0)
        return 0;
    return carve_bwd(nullptr, Shape{batch_size, num_rois, height, width, channels, pooled_height, pooled_width}).bytes;
}

int rroi_align_forward_hip(const float* features, int feature_layout, float spatial_scale,
                           int batch_size, int num_rois, int height, int width, int channels,
                           int pooled_height, int pooled_width, const float* rois,
                           float* top_data, void* workspace, size_t workspace_bytes, int path,
                           void* stream_)
{
    return rroi_align_forward_stages_hip(features, feature_layout, spatial_scale, batch_size,
                                         num_rois, height, width, channels, pooled_height,
                                         pooled_width, rois, top_data, workspace, workspace_bytes,
                                         path, RROI_STAGE_ALL, stream_);
}

// every dense native forward: `dtype` names the element type of the map and the crops
static int forward_typed_impl(const void* features, int dtype, int feature_layout, int top_layout, float spatial_scale,
                              const Shape& S, const float* rois, void* top_data, void* workspace, size_t workspace_bytes,
                              int path, int stages, void* stream_)
{
    if ((stages & ~RROI_STAGE_ALL) || stages == 0) return 0;
    const FwdDispatch P = plan_forward(S, feature_layout, top_layout, path, RROI_CALLER_NATIVE, dtype);
    if (!P.status) return 0;
    if (P.family == RROI_PLAN_NONE) return 1;
    if (!features || !rois || !top_data) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_forward(P, static_cast<const T*>(features), rois, static_cast<T*>(top_data), nullptr, nullptr,
                              spatial_scale, workspace, workspace_bytes, stages, stream);
    });
}

int rroi_align_forward_stages_hip(const float* features, int feature_layout, float spatial_scale,
                                  int batch_size, int num_rois, int height, int width,
                                  int channels, int pooled_height, int pooled_width,
                                  const float* rois, float* top_data, void* workspace,
                                  size_t workspace_bytes, int path, int stages, void* stream_)
{
    const Shape S{batch_size, num_rois, height, width, channels, pooled_height, pooled_width};
    return forward_typed_impl(features, RROI_DTYPE_FP32, feature_layout, RROI_LAYOUT_NCHW, spatial_scale, S, rois, top_data,
                              workspace, workspace_bytes, path, stages, stream_);
}

int rroi_align_forward_layout_hip(const float* features, int feature_layout, int top_layout,
                                  float spatial_scale, int batch_size, int num_rois, int height,
                                  int width, int channels, int pooled_height, int pooled_width,
                                  const float* rois, float* top_data, void* workspace,
                                  size_t workspace_bytes, int path, void* stream_)
{
    const Shape S{batch_size, num_rois, height, width, channels, pooled_height, pooled_width};
    return forward_typed_impl(features, RROI_DTYPE_FP32, feature_layout, top_layout, spatial_scale, S, rois, top_data,
                              workspace, workspace_bytes, path, RROI_STAGE_ALL, stream_);
}

int rroi_align_forward_typed_hip(const void* features, int dtype, int feature_layout, int top_layout, float spatial_scale,
                                 int batch_size, int num_rois, int height, int width, int channels, int pooled_height,
                                 int pooled_width, const float* rois, void* top_data, void* workspace,
                                 size_t workspace_bytes, int path, void* stream_)
{
    const Shape S{batch_size, num_rois, height, width, channels, pooled_height, pooled_width};
    return forward_typed_impl(features, dtype, feature_layout, top_layout, spatial_scale, S, rois, top_data, workspace,
                              workspace_bytes, path, RROI_STAGE_ALL, stream_);
}

int rroi_align_backward_hip(const float* top_diff, float spatial_scale, int batch_size,
                            int num_rois, int height, int width, int channels,
                            int pooled_height, int pooled_width, const float* rois,
                            float* bottom_diff, void* workspace, size_t workspace_bytes, int path,
                            void* stream_)
{
    return rroi_align_backward_layout_hip(top_diff, RROI_LAYOUT_NCHW, RROI_LAYOUT_NCHW, spatial_scale,
                                          batch_size, num_rois, height, width, channels, pooled_height,
                                          pooled_width, rois, bottom_diff, workspace, workspace_bytes, path,
                                          stream_);
}

int rroi_align_backward_typed_hip(const void* top_diff, int dtype, int top_diff_layout, int bottom_diff_layout,
                                  float spatial_scale, int batch_size, int num_rois, int height, int width, int channels,
                                  int pooled_height, int pooled_width, const float* rois, void* bottom_diff,
                                  void* workspace, size_t workspace_bytes, int path, void* stream_)
{
    const Shape S{batch_size, num_rois, height, width, channels, pooled_height, pooled_width};
    const BwdDispatch P = plan_backward(S, top_diff_layout, bottom_diff_layout, path, RROI_CALLER_NATIVE, dtype);
    if (!P.status) return 0;
    if (!bottom_diff) return 0;
    if (P.family != RROI_PLAN_NONE && (!top_diff || !rois)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_backward(P, static_cast<const T*>(top_diff), rois, static_cast<T*>(bottom_diff), spatial_scale,
                               workspace, workspace_bytes, stream);
    });
}

int rroi_align_backward_layout_hip(const float* top_diff, int top_diff_layout, int bottom_diff_layout,
                                   float spatial_scale, int batch_size, int num_rois, int height,
                                   int width, int channels, int pooled_height, int pooled_width,
                                   const float* rois, float* bottom_diff, void* workspace,
                                   size_t workspace_bytes, int path, void* stream_)
{
    return rroi_align_backward_typed_hip(top_diff, RROI_DTYPE_FP32, top_diff_layout, bottom_diff_layout, spatial_scale,
                                         batch_size, num_rois, height, width, channels, pooled_height, pooled_width, rois,
                                         bottom_diff, workspace, workspace_bytes, path, stream_);
}

int rroi_align_bin_centres_hip(float spatial_scale, int num_rois, int height, int width,
                               int pooled_height, int pooled_width, const float* rois,
                               float* geom, void* stream_)
{
    return rroi_align_bin_centres_trig_hip(spatial_scale, num_rois, height, width, pooled_height, pooled_width, rois,
                                           geom, RROI_TRIG_DOUBLE, stream_);
}

int rroi_align_bin_centres_trig_hip(float spatial_scale, int num_rois, int height, int width,
                                    int pooled_height, int pooled_width, const float* rois,
                                    float* geom, int trig_recipe, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (trig_recipe != RROI_TRIG_DOUBLE && trig_recipe != RROI_TRIG_FP32) return 0;
    if (num_rois < 0 || height <= 0 || width <= 0 || pooled_height <= 0 || pooled_width <= 0)
        return 0;
    if (num_rois == 0) return 1;
    if (!rois || !geom) return 0;
    const long threads = (long)num_rois * pooled_height * pooled_width;
    hipLaunchKernelGGL(rroi_bin_centres_kernel, dim3(ceil_div(threads, 256)), dim3(256), 0, stream,
                       rois, geom, num_rois, height, width, pooled_height, pooled_width,
                       spatial_scale, trig_recipe);
    return launch_status();
}

int rroi_align_quads_to_rois_hip(const float* quads, const float* batch_index, int n, int mode,
                                 int target_h, float* rois, int* target_gw, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n < 0 || (mode != 0 && mode != 1) || target_h <= 0) return 0;
    if (n == 0) return 1;
    if (!quads || !rois) return 0;
    hipLaunchKernelGGL(rroi_quads_to_rois_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, stream, quads,
                       batch_index, n, mode, target_h, rois, target_gw);
    return launch_status();
}

int rroi_align_gt_quads_to_rois_hip(const float* quads, const float* batch_index, const float* height_jitter,
                                    int n, float* rois, float* max_ratio, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n < 0) return 0;
    if (!max_ratio || (n > 0 && (!quads || !rois))) return 0;
    hipLaunchKernelGGL(rroi_gt_quads_to_rois_kernel, dim3(1), dim3(256), 0, stream, quads, batch_index,
                       height_jitter, n, rois, max_ratio);
    return launch_status();
}

int rroi_rbox_decode_typed_hip(int dtype, const void* segm, const void* rbox, const void* angle, int height, int width,
                               float segm_thresh, void* candidates, int capacity, int* count, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!dtype_ok(dtype)) return 0;
    if (height <= 0 || width <= 0 || capacity < 0 || (long)height * width >= (1L << 30)) return 0;
    if (!segm || !rbox || !angle || !count || (capacity > 0 && !candidates)) return 0;
    // one decode call for maps of element type T (float: the kernels of every release; bf16_t / fp16_t: the typed ones)
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return rbox_decode_impl<T>(static_cast<const T*>(segm), static_cast<const T*>(rbox), static_cast<const T*>(angle),
                                   height, width, segm_thresh, candidates, capacity, count, stream);
    });
}

int rroi_rbox_decode_hip(const float* segm, const float* rbox, const float* angle, int height, int width,
                         float segm_thresh, void* candidates, int capacity, int* count, void* stream_)
{
    return rroi_rbox_decode_typed_hip(RROI_DTYPE_FP32, segm, rbox, angle, height, width, segm_thresh, candidates, capacity,
                                      count, stream_);
}

int rroi_nms_record_format(void) { return RROI_NMS_RECORD_FORMAT; }

int rroi_nms_merge_host(const void* candidates, int num_candidates, int width, int height, float iou_threshold,
                        float iou_threshold2, float* boxes, int max_boxes)
{
    if (num_candidates < 0 || width <= 0 || height <= 0 || max_boxes < 0) return -1;
    if (num_candidates > 0 && !candidates) return -1;
    const NmsCandidate* cand = static_cast<const NmsCandidate*>(candidates);
    for (int i = 0; i < num_candidates; ++i)
        if (cand[i].x < 0 || cand[i].x >= width || cand[i].y < 0 || cand[i].y >= height) return -1;
    const std::vector<NmsPoly> out = nms_merge(cand, num_candidates, width, height, iou_threshold, iou_threshold2);
    const int n = (int)out.size();
    for (int i = 0; i < n && i < max_boxes; ++i) {
        float* b = boxes + (size_t)i * 9;
        for (int v = 0; v < 4; ++v) {  // adaptor.cpp:14-31 (float of the integers), nms/__init__.py:15-16 (/ 10000)
            b[2 * v] = (float)out[(size_t)i].X[v] / 10000.0f;
            b[2 * v + 1] = (float)out[(size_t)i].Y[v] / 10000.0f;
        }
        b[8] = out[(size_t)i].score;
    }
    return n;
}

int rroi_ctc_greedy_decode_typed_hip(int dtype, const void* logits, int num_seqs, int num_classes, int num_steps,
                                     const int* lengths, int* labels, int* decoded, int* decoded_len, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!dtype_ok(dtype)) return 0;
    if (num_seqs < 0 || num_classes <= 0 || num_steps < 0) return 0;
    if ((long)num_seqs * num_classes * (long)num_steps >= (1L << 40)) return 0;
    if (num_seqs == 0) return 1;
    if (!decoded_len || (num_steps > 0 && (!logits || !decoded))) return 0;
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        if constexpr (std::is_same<T, float>::value)   // (the kernel of every release)
            hipLaunchKernelGGL(rroi_ctc_greedy_kernel, dim3(num_seqs), dim3(kWave), 0, stream, static_cast<const float*>(logits),
                               num_classes, num_steps, lengths, labels, decoded, decoded_len);
        else
            hipLaunchKernelGGL(rroi_ctc_greedy_typed_kernel<T>, dim3(num_seqs), dim3(kWave), 0, stream,
                               static_cast<const T*>(logits), num_classes, num_steps, lengths, labels, decoded, decoded_len);
        return launch_status();
    });
}

int rroi_ctc_greedy_decode_hip(const float* logits, int num_seqs, int num_classes, int num_steps,
                               const int* lengths, int* labels, int* decoded, int* decoded_len,
                               void* stream_)
{
    return rroi_ctc_greedy_decode_typed_hip(RROI_DTYPE_FP32, logits, num_seqs, num_classes, num_steps, lengths, labels,
                                            decoded, decoded_len, stream_);
}

int rroi_align_write_probe_hip(float* out, size_t num_floats, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!out || num_floats % 4 != 0 || reinterpret_cast<size_t>(out) % 16 != 0) return 0;
    const size_t n4 = num_floats / 4;
    if (n4 == 0) return 1;
    if ((n4 + 255) / 256 >= (1ull << 31)) return 0;
    hipLaunchKernelGGL(rroi_write_probe_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, out, n4);
    return launch_status();
}

int rroi_align_sincos_probe_hip(const float* angle_deg, int n, float* out, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n < 0) return 0;
    if (n == 0) return 1;
    if (!angle_deg || !out) return 0;
    hipLaunchKernelGGL(rroi_sincos_probe_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, stream,
                       angle_deg, n, out);
    return launch_status();
}

// The reference-ABI launchers have no `path` to carry the trig recipe: they use RROI_TRIG_DOUBLE, unless the process
// was started with RROI_ALIGN_LAUNCHER_TRIG=fp32 in its environment (read ONCE, at the first launcher call: a constant
// of the process, not a switch) -- for a drop-in user who wants every bin equal to the reference's own build for
// this GPU rather than to the correctly rounded recipe.
static int launcher_trig()
{
    static const int t = [] {
        const char* e = getenv("RROI_ALIGN_LAUNCHER_TRIG");
        return (e && (!strcmp(e, "fp32") || !strcmp(e, "1"))) ? RROI_TRIG_FP32 : RROI_TRIG_DOUBLE;
    }();
    return t;
}

// ---- the reference's launcher ABI (rroi_align_kernel.h:8-18) ------------------------
// The signatures carry no workspace (and the forward's no batch count), so the fast paths take
// their scratch from the library's per-(device, stream) buffers (launcher_scratch above: grown on
// demand, reused by later calls, pinned once a graph has captured them; no synchronisation).
// Small problems keep the one-kernel direct paths (no scratch).
int rroi_align_launcher_trig_recipe(void) { return launcher_trig(); }

int RROIAlignForwardLaucher(const float* bottom_data, const float spatial_scale,
                            const int num_rois, const int height, const int width,
                            const int channels, const int pooled_height, const int pooled_width,
                            const float* bottom_rois, float* top_data, float* con_idx_x,
                            float* con_idx_y, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Shape S{/*batch_size*/ 1, num_rois, height, width, channels, pooled_height, pooled_width};
    const FwdDispatch P = plan_forward(S, RROI_LAYOUT_NCHW, RROI_LAYOUT_NCHW, launcher_trig() ? RROI_PATH_TRIG_FP32 : 0,
                                       con_idx_x ? RROI_CALLER_LAUNCHER_CON_IDX : RROI_CALLER_LAUNCHER, RROI_DTYPE_FP32);
    if (!P.status) return 0;
    if (P.family == RROI_PLAN_NONE) return 1;
    if (!bottom_data || !bottom_rois || !top_data) return 0;
    if ((con_idx_x == nullptr) != (con_idx_y == nullptr)) return 0;
    if (P.family != RROI_PLAN_FWD_TWO_LAUNCH)   // the direct kernels (no scratch) write con_idx themselves
        return launch_forward(P, bottom_data, bottom_rois, top_data, con_idx_x, con_idx_y, spatial_scale, nullptr, 0,
                              RROI_STAGE_ALL, stream);
    // Tiled path for the ROIs of image 0 (every ROI, in inference and in the benchmark); the
    // signature does not say how many images `bottom_data` holds, so the ROIs of images >= 1 are
    // sampled from the NCHW tensor by one more block per ROI of the prologue launch (trusting the
    // index as the reference does; a block whose ROI is of image 0 reads the index and leaves) and
    // skipped by the gather: the same two launches as the native call.
    const size_t bytes = carve(nullptr, P.shape, RROI_LAYOUT_NCHW).bytes;
    ScratchLease lease = launcher_scratch(stream, bytes);
    void* const ws = lease.ptr;
    if (!ws) return status_of(lease.err);
    int st = launch_forward(P, bottom_data, bottom_rois, top_data, nullptr, nullptr, spatial_scale, ws, bytes, RROI_STAGE_ALL,
                            stream);
    if (st == 1 && P.con_idx) {
        hipLaunchKernelGGL(rroi_con_idx_kernel, P.dgrid, dim3(256), 0, stream, bottom_rois, con_idx_x, con_idx_y,
                           num_rois, channels, height, width, pooled_height, pooled_width, spatial_scale, P.trig,
                           P.cslab);
        st = launch_status();
    }
    const hipError_t e = lease.give_back(stream);   // (everything that uses the buffer is enqueued)
    return st != 1 ? st : status_of(e);
}

// con_idx_x / con_idx_y must be the tensors the forward wrote for the same rois (the reference
// re-reads the bin centres from them, kernel.cu:232-233): the fast path recomputes the centres from
// the rois instead of reading 2 x (R, C, PH, PW) floats back.  bottom_diff: the gradient is ADDED to it
// on every path, as the reference's atomicAdds do (kernel.cu:260-274; functions/rroi_align.py:35 hands
// over zeros) -- the result does not depend on which path the problem size selects.
int RROIAlignBackwardLaucher(const float* top_diff, const float spatial_scale,
                             const int batch_size, const int num_rois, const int height,
                             const int width, const int channels, const int pooled_height,
                             const int pooled_width, const float* bottom_rois,
                             float* bottom_diff, const float* con_idx_x, const float* con_idx_y,
                             void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Shape S{batch_size, num_rois, height, width, channels, pooled_height, pooled_width};
    const BwdDispatch P = plan_backward(S, RROI_LAYOUT_NCHW, RROI_LAYOUT_NCHW, launcher_trig() ? RROI_PATH_TRIG_FP32 : 0,
                                        RROI_CALLER_LAUNCHER, RROI_DTYPE_FP32);
    if (!P.status) return 0;
    if (P.family == RROI_PLAN_NONE) return 1;
    if (!top_diff || !bottom_rois || !bottom_diff || !con_idx_x || !con_idx_y) return 0;
    if (P.family != RROI_PLAN_BWD_LITERAL) {
        const size_t bytes = P.ws.bytes;
        ScratchLease lease = launcher_scratch(stream, bytes);
        void* const ws = lease.ptr;
        if (!ws) return status_of(lease.err);
        const int st = launch_backward(P, top_diff, bottom_rois, bottom_diff, spatial_scale, ws, bytes, stream);
        const hipError_t e = lease.give_back(stream);
        return st != 1 ? st : status_of(e);
    }
    const long nthreads = (long)num_rois * pooled_height * pooled_width * channels;
    hipLaunchKernelGGL(rroi_bwd_literal_kernel, P.grid, dim3(256), 0, stream,
                       top_diff, con_idx_x, con_idx_y, bottom_rois, bottom_diff, nthreads, channels,
                       height, width, pooled_height, pooled_width);
    return launch_status();
}

// ---- the plan query (section 2 of the header) ----------------------------------------
int rroi_align_forward_plan(int feature_layout, int top_layout, int batch_size, int num_rois, int height, int width,
                            int channels, int pooled_height, int pooled_width, int path, int caller,
                            rroi_align_plan* plan)
{
    return rroi_align_forward_plan_typed(RROI_DTYPE_FP32, feature_layout, top_layout, batch_size, num_rois, height, width,
                                         channels, pooled_height, pooled_width, path, caller, plan);
}

int rroi_align_forward_plan_typed(int dtype, int feature_layout, int top_layout, int batch_size, int num_rois, int height,
                                  int width, int channels, int pooled_height, int pooled_width, int path, int caller,
                                  rroi_align_plan* plan)
{
    const Shape S{batch_size, num_rois, height, width, channels, pooled_height, pooled_width};
    return report_plan(plan_forward(S, feature_layout, top_layout, path, caller, dtype), plan);
}

int rroi_align_backward_plan(int top_diff_layout, int bottom_diff_layout, int batch_size, int num_rois, int height,
                             int width, int channels, int pooled_height, int pooled_width, int path, int caller,
                             rroi_align_plan* plan)
{
    return rroi_align_backward_plan_typed(RROI_DTYPE_FP32, top_diff_layout, bottom_diff_layout, batch_size, num_rois, height,
                                          width, channels, pooled_height, pooled_width, path, caller, plan);
}

int rroi_align_backward_plan_typed(int dtype, int top_diff_layout, int bottom_diff_layout, int batch_size, int num_rois,
                                   int height, int width, int channels, int pooled_height, int pooled_width, int path,
                                   int caller, rroi_align_plan* plan)
{
    const Shape S{batch_size, num_rois, height, width, channels, pooled_height, pooled_width};
    return report_plan(plan_backward(S, top_diff_layout, bottom_diff_layout, path, caller, dtype), plan);
}

// ------------------------------------------------------------------------------------
// Bucketed RoIRotate (header section 2b): one pooled width per ROI, one launch chain per call.
// ------------------------------------------------------------------------------------
size_t rroi_align_forward_bucketed_workspace_bytes(int batch_size, int channels, int height, int width, int num_rois)
{
    return rroi_align_forward_workspace_bytes(batch_size, channels, height, width, num_rois, RROI_LAYOUT_NCHW);
}

size_t rroi_align_backward_bucketed_workspace_bytes(int batch_size, int channels, int height, int width, int num_rois,
                                                    int pooled_height, int max_pooled_width)
{
    return rroi_align_backward_workspace_bytes(batch_size, channels, height, width, num_rois, pooled_height, max_pooled_width);
}

int rroi_align_forward_bucketed_plan(int dtype, int batch_size, int num_rois, int height, int width, int channels,
                                     int pooled_height, int max_pooled_width, long long sum_pooled_widths, int width_multiple,
                                     int crop_alignment, int path, rroi_align_plan* plan)
{
    const Shape S{batch_size, num_rois, height, width, channels, pooled_height, max_pooled_width};
    return report_plan(plan_forward_bucketed(S, dtype, sum_pooled_widths, width_multiple, crop_alignment, path), plan);
}

int rroi_align_backward_bucketed_plan(int dtype, int bottom_diff_layout, int batch_size, int num_rois, int height, int width,
                                      int channels, int pooled_height, int max_pooled_width, int path, rroi_align_plan* plan)
{
    const Shape S{batch_size, num_rois, height, width, channels, pooled_height, max_pooled_width};
    return report_plan(plan_backward(S, RROI_LAYOUT_NCHW, bottom_diff_layout, path, RROI_CALLER_NATIVE, dtype, /*ragged*/ true), plan);
}

int rroi_align_forward_bucketed_hip(const void* features, int dtype, float spatial_scale, int batch_size, int num_rois,
                                    int height, int width, int channels, int pooled_height, int max_pooled_width,
                                    long long sum_pooled_widths, int width_multiple, int crop_alignment, const float* rois,
                                    const rroi_align_crop* crops, void* workspace, size_t workspace_bytes, int path,
                                    void* stream_)
{
    static_assert(sizeof(rroi_align_crop) == sizeof(CropRow), "the table's row");
    const Shape S{batch_size, num_rois, height, width, channels, pooled_height, max_pooled_width};
    const FwdDispatch P = plan_forward_bucketed(S, dtype, sum_pooled_widths, width_multiple, crop_alignment, path);
    if (!P.status) return 0;
    if (P.family == RROI_PLAN_NONE) return 1;
    if (!features || !rois || !crops) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    const CropRow* table = reinterpret_cast<const CropRow*>(crops);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_forward_bucketed(P, static_cast<const T*>(features), rois, table, spatial_scale, workspace, workspace_bytes,
                                       stream);
    });
}

int rroi_align_backward_bucketed_hip(const rroi_align_crop* top_diffs, int dtype, int bottom_diff_layout, float spatial_scale,
                                     int batch_size, int num_rois, int height, int width, int channels, int pooled_height,
                                     int max_pooled_width, const float* rois, void* bottom_diff, void* workspace,
                                     size_t workspace_bytes, int path, void* stream_)
{
    const Shape S{batch_size, num_rois, height, width, channels, pooled_height, max_pooled_width};
    const BwdDispatch P = plan_backward(S, RROI_LAYOUT_NCHW, bottom_diff_layout, path, RROI_CALLER_NATIVE, dtype, /*ragged*/ true);
    if (!P.status) return 0;
    if (!bottom_diff) return 0;
    if (P.family != RROI_PLAN_NONE && (!top_diffs || !rois)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    const CropRow* table = reinterpret_cast<const CropRow*>(top_diffs);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_backward(P, static_cast<const T*>(nullptr), rois, static_cast<T*>(bottom_diff), spatial_scale, workspace,
                               workspace_bytes, stream, table);
    });
}

// ------------------------------------------------------------------------------------
// Depthwise 3x3 convolution of the network (header section 5): one launch, no workspace.
// ------------------------------------------------------------------------------------
int rroi_depthwise3x3_forward_hip(int dtype, const void* x, const void* weight, void* y, int batch_size, int channels,
                                  int height, int width, int stride, void* stream_)
{
    if (!depthwise_shape_ok(dtype, batch_size, channels, height, width, stride)) return 0;
    if (!x || !weight || !y) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_depthwise3x3(static_cast<const T*>(x), static_cast<const T*>(weight), static_cast<T*>(y), batch_size,
                                   channels, height, width, stride, stream);
    });
}

// The backward of that convolution (header section 5b): one launch for dx, two and a workspace for dweight.
size_t rroi_depthwise3x3_backward_workspace_bytes(int batch_size, int channels, int height, int width, int stride)
{
    return plan_depthwise_backward(RROI_DTYPE_FP32, batch_size, channels, height, width, stride).ws_bytes;   // no dtype in the rule
}

int rroi_depthwise3x3_backward_plan(int dtype, int batch_size, int channels, int height, int width, int stride,
                                    rroi_depthwise_backward_plan_info* plan)
{
    const DwBwdPlan P = plan_depthwise_backward(dtype, batch_size, channels, height, width, stride);
    if (!P.status || !plan) return 0;
    // launches: of a call that wants both gradients (dx alone is one, dweight alone two)
    *plan = rroi_depthwise_backward_plan_info{P.band * stride, kDwCols * stride, (int)P.dx_grid, P.band, (int)P.nseg,
                                              (int)P.dw_grid, 3, kDwThreads};
    return 1;
}

int rroi_depthwise3x3_backward_hip(int dtype, const void* dy, const void* x, const void* weight, void* dx, void* dweight,
                                   int batch_size, int channels, int height, int width, int stride, void* workspace,
                                   size_t workspace_bytes, void* stream_)
{
    const DwBwdPlan P = plan_depthwise_backward(dtype, batch_size, channels, height, width, stride);
    if (!P.status) return 0;
    if (!dy || (!dx && !dweight) || (dx && !weight) || (dweight && !x)) return 0;
    if (dx) {
        const size_t esize = dtype == RROI_DTYPE_FP32 ? 4 : 2;
        const size_t out_bytes = (size_t)P.planes * height * width * esize, dy_bytes = (size_t)P.planes * P.Ho * P.Wo * esize;
        const char *o = static_cast<const char*>(dx), *g = static_cast<const char*>(dy), *i = static_cast<const char*>(x);
        if (o < g + dy_bytes && g < o + out_bytes) return 0;
        if (dweight && o < i + out_bytes && i < o + out_bytes) return 0;   // (x is read only for dweight)
    }
    if (dweight && (!workspace_ok(workspace) || workspace_bytes < P.ws_bytes)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_depthwise3x3_backward(P, static_cast<const T*>(dy), static_cast<const T*>(x), static_cast<const T*>(weight),
                                            static_cast<T*>(dx), static_cast<T*>(dweight), batch_size, channels, height, width,
                                            stride, workspace, stream);
    });
}

// ------------------------------------------------------------------------------------
// InstanceNorm2d of the network with its activation (header section 6): one launch, or two and a workspace.
// ------------------------------------------------------------------------------------
size_t rroi_instancenorm_workspace_bytes(int batch_size, int channels, int height, int width)
{
    size_t bytes = 0;   // the size query has no dtype: what the largest of the three plans needs (today they are one)
    for (const int dtype : {RROI_DTYPE_FP32, RROI_DTYPE_BF16, RROI_DTYPE_FP16})
        bytes = std::max(bytes, plan_instancenorm(dtype, batch_size, channels, height, width, num_cus()).ws_bytes);
    return bytes;
}

int rroi_instancenorm_plan(int dtype, int batch_size, int channels, int height, int width, rroi_instancenorm_plan_info* plan)
{
    const InormPlan P = plan_instancenorm(dtype, batch_size, channels, height, width, num_cus());
    if (!P.status || !plan) return 0;
    *plan = rroi_instancenorm_plan_info{P.form, P.form == RROI_INORM_SPLIT ? 2 : 1, (int)P.nseg, (int)P.seg, (int)P.grid,
                                        kInThreads, dtype == RROI_DTYPE_FP32 ? 4 : 8, 0};
    return 1;
}

int rroi_instancenorm_forward_hip(int dtype, const void* x, const void* gamma, const void* beta, void* y, int batch_size,
                                  int channels, int height, int width, double eps, float negative_slope, void* workspace,
                                  size_t workspace_bytes, void* stream_)
{
    const InormPlan P = plan_instancenorm(dtype, batch_size, channels, height, width, num_cus());
    if (!P.status) return 0;
    if (!x || !y || (gamma == nullptr) != (beta == nullptr)) return 0;
    if (!std::isfinite(eps) || !(eps > 0.0) || !std::isfinite(negative_slope)) return 0;
    if (P.ws_bytes &&
        (!workspace_ok(workspace) || workspace_bytes < rroi_instancenorm_workspace_bytes(batch_size, channels, height, width)))
        return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_instancenorm(P, static_cast<const T*>(x), static_cast<const T*>(gamma), static_cast<const T*>(beta),
                                   static_cast<T*>(y), (unsigned)channels, eps, negative_slope, workspace, stream);
    });
}

// The same norm with an epilogue fused in (header section 6b): the residual add of a block's tail, or the
// stem's cat(x, -x) in front of it.  The plan is the plain call's for x's shape; neither a residual nor the mirror is
// the plain call.
int rroi_instancenorm_fused_forward_hip(int dtype, const void* x, const void* gamma, const void* beta, const void* residual,
                                        void* y, int batch_size, int channels, int height, int width, int mirror, double eps,
                                        float negative_slope, void* workspace, size_t workspace_bytes, void* stream_)
{
    if (mirror != 0 && mirror != 1) return 0;
    if (mirror && residual) return 0;
    if (!mirror && !residual)
        return rroi_instancenorm_forward_hip(dtype, x, gamma, beta, y, batch_size, channels, height, width, eps, negative_slope,
                                             workspace, workspace_bytes, stream_);
    const InormPlan P = plan_instancenorm(dtype, batch_size, channels, height, width, num_cus());
    if (!P.status) return 0;
    if (mirror && 2LL * batch_size * channels * height * width >= (1LL << 31)) return 0;   // y's elements (x's are < 2^31)
    if (!x || !y || (gamma == nullptr) != (beta == nullptr)) return 0;
    if (!std::isfinite(eps) || !(eps > 0.0) || !std::isfinite(negative_slope)) return 0;
    if (P.ws_bytes &&
        (!workspace_ok(workspace) || workspace_bytes < rroi_instancenorm_workspace_bytes(batch_size, channels, height, width)))
        return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        const T *xt = static_cast<const T*>(x), *g = static_cast<const T*>(gamma), *bt = static_cast<const T*>(beta);
        if (mirror)
            return launch_instancenorm_fused<T, kInMirror>(P, xt, g, bt, static_cast<const T*>(nullptr), static_cast<T*>(y),
                                                           (unsigned)channels, eps, negative_slope, workspace, stream);
        return launch_instancenorm_fused<T, kInResidual>(P, xt, g, bt, static_cast<const T*>(residual), static_cast<T*>(y),
                                                         (unsigned)channels, eps, negative_slope, workspace, stream);
    });
}

// The training twin of the plain call (header section 6c): the same y, and the {mean, var} of every plane.
int rroi_instancenorm_forward_train_hip(int dtype, const void* x, const void* gamma, const void* beta, void* y, void* stats,
                                        int batch_size, int channels, int height, int width, double eps, float negative_slope,
                                        void* workspace, size_t workspace_bytes, void* stream_)
{
    const InormPlan P = plan_instancenorm(dtype, batch_size, channels, height, width, num_cus());
    if (!P.status) return 0;
    if (!x || !y || !stats || (gamma == nullptr) != (beta == nullptr)) return 0;
    if (!std::isfinite(eps) || !(eps > 0.0) || !std::isfinite(negative_slope)) return 0;
    if (P.ws_bytes &&
        (!workspace_ok(workspace) || workspace_bytes < rroi_instancenorm_workspace_bytes(batch_size, channels, height, width)))
        return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_instancenorm_train(P, static_cast<const T*>(x), static_cast<const T*>(gamma), static_cast<const T*>(beta),
                                         static_cast<T*>(y), static_cast<double2*>(stats), (unsigned)channels, eps,
                                         negative_slope, workspace, stream);
    });
}

size_t rroi_instancenorm_backward_workspace_bytes(int batch_size, int channels, int height, int width)
{
    size_t bytes = 0;   // no dtype, as the forward's query: what the largest of the three plans needs (today they are one)
    for (const int dtype : {RROI_DTYPE_FP32, RROI_DTYPE_BF16, RROI_DTYPE_FP16})
        bytes = std::max(bytes, plan_instancenorm_backward(dtype, batch_size, channels, height, width, num_cus()).ws_bytes);
    return bytes;
}

int rroi_instancenorm_backward_plan(int dtype, int batch_size, int channels, int height, int width,
                                    rroi_instancenorm_plan_info* plan)
{
    const InormPlan P = plan_instancenorm_backward(dtype, batch_size, channels, height, width, num_cus()).P;
    if (!P.status || !plan) return 0;
    // launches: of a call that wants every gradient (the parameter-gradient kernel is the last; one fewer without it)
    *plan = rroi_instancenorm_plan_info{P.form, P.form == RROI_INORM_SPLIT ? 3 : 2, (int)P.nseg, (int)P.seg, (int)P.grid,
                                        kInThreads, dtype == RROI_DTYPE_FP32 ? 4 : 8, 0};
    return 1;
}

int rroi_instancenorm_backward_hip(int dtype, const void* dy, const void* x, const void* stats, const void* gamma,
                                   const void* beta, void* dx, void* dgamma, void* dbeta, int batch_size, int channels,
                                   int height, int width, double eps, float negative_slope, void* workspace,
                                   size_t workspace_bytes, void* stream_)
{
    const InormBwdPlan B = plan_instancenorm_backward(dtype, batch_size, channels, height, width, num_cus());
    if (!B.P.status) return 0;
    if (!dy || !x || !stats || (gamma == nullptr) != (beta == nullptr) || (dgamma == nullptr) != (dbeta == nullptr)) return 0;
    if (!dx && !dgamma) return 0;
    if (dgamma && !gamma) return 0;
    if (!std::isfinite(eps) || !(eps > 0.0) || !std::isfinite(negative_slope)) return 0;
    if (dx) {
        const size_t bytes = (size_t)B.P.planes * B.P.n * (dtype == RROI_DTYPE_FP32 ? 4 : 2);
        const char* o = static_cast<const char*>(dx);
        for (const void* in : {x, dy}) {
            const char* i = static_cast<const char*>(in);
            if (o < i + bytes && i < o + bytes) return 0;
        }
    }
    if ((dgamma || B.P.form == RROI_INORM_SPLIT) &&
        (!workspace_ok(workspace) ||
         workspace_bytes < rroi_instancenorm_backward_workspace_bytes(batch_size, channels, height, width)))
        return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_instancenorm_backward(B, static_cast<const T*>(dy), static_cast<const T*>(x),
                                            static_cast<const double2*>(stats), static_cast<const T*>(gamma),
                                            static_cast<const T*>(beta), static_cast<T*>(dx), static_cast<T*>(dgamma),
                                            static_cast<T*>(dbeta), (unsigned)batch_size, (unsigned)channels, eps,
                                            negative_slope, workspace, stream);
    });
}

// ------------------------------------------------------------------------------------
// Detection heads and attention gate of the network (header section 7): one launch, no workspace.
// ------------------------------------------------------------------------------------
int rroi_heads_plan(int dtype, int outputs, int batch_size, int channels, int height, int width, rroi_heads_plan_info* plan)
{
    const HeadsPlan P = plan_heads(dtype, outputs, batch_size, channels, height, width, num_cus());
    if (!P.status || !plan) return 0;
    *plan = rroi_heads_plan_info{P.V, P.S, (int)P.tiles, (int)P.grid, P.S * 64, (int)P.lds_bytes, (int)P.cb, 0};
    return 1;
}

static int heads_impl(const HeadsPlan& P, int dtype, const void* x, const void* w_score, const void* b_score,
                      const void* w_rbox, const void* b_rbox, const void* w_angle, const void* b_angle, void* score, void* rbox,
                      void* angle, int channels, double rbox_scale, void* stream_)
{
    if (!P.status) return 0;
    if (!x || !w_score || !w_rbox || !w_angle || !score || !rbox || !angle) return 0;
    if (!std::isfinite(rbox_scale)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_pointwise<T, 7, kPwEpiHeads>(
            P, static_cast<const T*>(x), static_cast<const T*>(w_score), static_cast<const T*>(b_score),
            static_cast<const T*>(w_rbox), static_cast<const T*>(b_rbox), static_cast<const T*>(w_angle),
            static_cast<const T*>(b_angle), static_cast<T*>(score), static_cast<T*>(rbox), static_cast<T*>(angle),
            (unsigned)channels, rbox_scale, stream);
    });
}

int rroi_heads_forward_hip(int dtype, const void* x, const void* w_score, const void* b_score, const void* w_rbox,
                           const void* b_rbox, const void* w_angle, const void* b_angle, void* score, void* rbox, void* angle,
                           int batch_size, int channels, int height, int width, double rbox_scale, void* stream)
{
    return heads_impl(plan_heads(dtype, 7, batch_size, channels, height, width, num_cus()), dtype, x, w_score, b_score, w_rbox,
                      b_rbox, w_angle, b_angle, score, rbox, angle, channels, rbox_scale, stream);
}

#ifdef RROI_HEADS_MEASURE
// Measurement build only (`make heads-forms`; not declared in the header, not in the shipped library): the heads with V
// and S forced, for the comparison of the plan rule against its neighbours (tools/heads_bench.py --forms).
// *v_used / *s_used report what ran after the caps of plan_heads.
int rroi_heads_forward_forced_hip(int dtype, const void* x, const void* w_score, const void* b_score, const void* w_rbox,
                                  const void* b_rbox, const void* w_angle, const void* b_angle, void* score, void* rbox,
                                  void* angle, int batch_size, int channels, int height, int width, double rbox_scale,
                                  int force_v, int force_s, int* v_used, int* s_used, void* stream)
{
    const HeadsPlan P = plan_heads(dtype, 7, batch_size, channels, height, width, num_cus(), force_v, force_s);
    if (v_used) *v_used = P.V;
    if (s_used) *s_used = P.S;
    return heads_impl(P, dtype, x, w_score, b_score, w_rbox, b_rbox, w_angle, b_angle, score, rbox, angle, channels, rbox_scale,
                      stream);
}
#endif

int rroi_gate_forward_hip(int dtype, const void* x, const void* w, const void* b, void* y, int batch_size, int channels,
                          int height, int width, void* stream_)
{
    const HeadsPlan P = plan_heads(dtype, 1, batch_size, channels, height, width, num_cus());
    if (!P.status) return 0;
    if (!x || !w || !y) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_pointwise<T, 1, kPwEpiSigmoid>(P, static_cast<const T*>(x), static_cast<const T*>(w),
                                                     static_cast<const T*>(b), static_cast<const T*>(nullptr),
                                                     static_cast<const T*>(nullptr), static_cast<const T*>(nullptr),
                                                     static_cast<const T*>(nullptr), static_cast<T*>(y), static_cast<T*>(nullptr),
                                                     static_cast<T*>(nullptr), (unsigned)channels, 1.0, stream);
    });
}

// Their training forward and backward (header section 7b): the forward with z as one more output, and a
// backward of one launch for dx, two and a workspace where a parameter gradient is wanted.
int rroi_heads_forward_train_hip(int dtype, const void* x, const void* w_score, const void* b_score, const void* w_rbox,
                                 const void* b_rbox, const void* w_angle, const void* b_angle, void* score, void* rbox,
                                 void* angle, void* z, int batch_size, int channels, int height, int width, double rbox_scale,
                                 void* stream_)
{
    const HeadsPlan P = plan_heads(dtype, 7, batch_size, channels, height, width, num_cus());
    if (!P.status) return 0;
    if (!x || !w_score || !w_rbox || !w_angle || !score || !rbox || !angle || !z) return 0;
    if (!std::isfinite(rbox_scale)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_pointwise_train<T, 7, kPwEpiHeads>(
            P, static_cast<const T*>(x), static_cast<const T*>(w_score), static_cast<const T*>(b_score),
            static_cast<const T*>(w_rbox), static_cast<const T*>(b_rbox), static_cast<const T*>(w_angle),
            static_cast<const T*>(b_angle), static_cast<T*>(score), static_cast<T*>(rbox), static_cast<T*>(angle),
            static_cast<double*>(z), (unsigned)channels, rbox_scale, stream);
    });
}

int rroi_gate_forward_train_hip(int dtype, const void* x, const void* w, const void* b, void* y, void* z, int batch_size,
                                int channels, int height, int width, void* stream_)
{
    const HeadsPlan P = plan_heads(dtype, 1, batch_size, channels, height, width, num_cus());
    if (!P.status) return 0;
    if (!x || !w || !y || !z) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        const T* none = nullptr;
        return launch_pointwise_train<T, 1, kPwEpiSigmoid>(P, static_cast<const T*>(x), static_cast<const T*>(w),
                                                           static_cast<const T*>(b), none, none, none, none, static_cast<T*>(y),
                                                           static_cast<T*>(nullptr), static_cast<T*>(nullptr),
                                                           static_cast<double*>(z), (unsigned)channels, 1.0, stream);
    });
}

int rroi_heads_backward_plan(int dtype, int outputs, int batch_size, int channels, int height, int width,
                             rroi_heads_backward_plan_info* plan)
{
    const HeadsBwdPlan P = plan_heads_backward(dtype, outputs, batch_size, channels, height, width, num_cus());
    if (!P.status || !plan) return 0;
    // launches: of a call that wants a parameter gradient (dx alone is one)
    *plan = rroi_heads_backward_plan_info{P.V, (int)P.rows, (int)P.rows, (int)P.tpw, kHbThreads, (int)P.lds_bytes, 2, 0,
                                          (long long)P.tpw * 64 * P.V, (long long)P.ws_bytes};
    return 1;
}

size_t rroi_heads_backward_workspace_bytes(int outputs, int batch_size, int channels, int height, int width)
{
    return plan_heads_backward(RROI_DTYPE_FP32, outputs, batch_size, channels, height, width, num_cus()).ws_bytes;   // no dtype in the rule
}

// an argument's memory; NULL overlaps nothing
struct HbSpan { const void* p; size_t bytes; };

static int heads_backward_impl(int dtype, int outputs, const void* g0, const void* g1, const void* g2, const void* x,
                               const void* z, const void* w0, const void* w1, const void* w2, void* dx, void* const (&dwb)[6],
                               int batch_size, int channels, int height, int width, double rbox_scale, void* workspace,
                               size_t workspace_bytes, void* stream_)
{
    const HeadsBwdPlan P = plan_heads_backward(dtype, outputs, batch_size, channels, height, width, num_cus());
    if (!P.status || !std::isfinite(rbox_scale)) return 0;
    const bool heads = outputs == 7;
    if (!x || !z || (!g0 && !g1 && !g2)) return 0;
    bool params = false;
    for (const void* p : dwb) params = params || p;
    if (!dx && !params) return 0;
    if (dx && (!w0 || (heads && (!w1 || !w2)))) return 0;
    if (params && (!workspace_ok(workspace) || workspace_bytes < P.ws_bytes)) return 0;
    const size_t esize = dtype_bytes(dtype), px = (size_t)batch_size * P.hw, C = (size_t)channels;
    const HbSpan ins[] = {{g0, px * esize}, {g1, 4 * px * esize}, {g2, 2 * px * esize}, {x, px * C * esize},
                          {z, px * outputs * sizeof(double)}, {w0, C * esize}, {w1, 4 * C * esize}, {w2, 2 * C * esize}};
    const HbSpan outs[] = {{dx, px * C * esize}, {dwb[0], C * esize}, {dwb[1], esize}, {dwb[2], 4 * C * esize},
                           {dwb[3], 4 * esize}, {dwb[4], 2 * C * esize}, {dwb[5], 2 * esize},
                           {params ? workspace : nullptr, P.ws_bytes}};
    for (size_t a = 0; a < sizeof(outs) / sizeof(outs[0]); ++a) {
        for (const HbSpan& in : ins)
            if (bytes_overlap(outs[a].p, outs[a].bytes, in.p, in.bytes)) return 0;
        for (size_t b = a + 1; b < sizeof(outs) / sizeof(outs[0]); ++b)
            if (bytes_overlap(outs[a].p, outs[a].bytes, outs[b].p, outs[b].bytes)) return 0;
    }
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        const auto in = [](const void* p) { return static_cast<const T*>(p); };
        const auto out = [](void* p) { return static_cast<T*>(p); };
        if (heads)
            return launch_heads_backward<T, 7>(P, in(g0), in(g1), in(g2), in(x), static_cast<const double*>(z), in(w0), in(w1),
                                               in(w2), out(dx), out(dwb[0]), out(dwb[1]), out(dwb[2]), out(dwb[3]), out(dwb[4]),
                                               out(dwb[5]), (unsigned)channels, rbox_scale, workspace, stream);
        return launch_heads_backward<T, 1>(P, in(g0), in(nullptr), in(nullptr), in(x), static_cast<const double*>(z), in(w0),
                                           in(nullptr), in(nullptr), out(dx), out(dwb[0]), out(dwb[1]), out(nullptr),
                                           out(nullptr), out(nullptr), out(nullptr), (unsigned)channels, 1.0, workspace, stream);
    });
}

int rroi_heads_backward_hip(int dtype, const void* dscore, const void* drbox, const void* dangle, const void* x, const void* z,
                            const void* w_score, const void* w_rbox, const void* w_angle, void* dx, void* dw_score,
                            void* db_score, void* dw_rbox, void* db_rbox, void* dw_angle, void* db_angle, int batch_size,
                            int channels, int height, int width, double rbox_scale, void* workspace, size_t workspace_bytes,
                            void* stream)
{
    void* const dwb[6] = {dw_score, db_score, dw_rbox, db_rbox, dw_angle, db_angle};
    return heads_backward_impl(dtype, 7, dscore, drbox, dangle, x, z, w_score, w_rbox, w_angle, dx, dwb, batch_size, channels,
                               height, width, rbox_scale, workspace, workspace_bytes, stream);
}

int rroi_gate_backward_hip(int dtype, const void* dy, const void* x, const void* z, const void* w, void* dx, void* dw, void* db,
                           int batch_size, int channels, int height, int width, void* workspace, size_t workspace_bytes,
                           void* stream)
{
    void* const dwb[6] = {dw, db, nullptr, nullptr, nullptr, nullptr};
    return heads_backward_impl(dtype, 1, dy, nullptr, nullptr, x, z, w, nullptr, nullptr, dx, dwb, batch_size, channels, height,
                               width, 1.0, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------
// Gated merge of the network's feature merge (header section 8): y = A + f * G, one launch, no workspace.
// ------------------------------------------------------------------------------------
int rroi_merge_plan(int dtype, int batch_size, int channels, int height, int width, int a_h, int a_w, int g_h, int g_w,
                    int gated, rroi_merge_plan_info* plan)
{
    const MergePlan P = plan_merge(dtype, batch_size, channels, height, width, a_h, a_w, g_h, g_w, gated, num_cus());
    if (!P.status || !plan) return 0;
    *plan = rroi_merge_plan_info{P.V, P.K, (int)P.tiles, (int)P.grid, kMgThreads, (int)P.cb, P.resize_a ? 1 : 0,
                                 P.resize_g ? 1 : 0, P.A.sy, P.A.sx, P.G.sy, P.G.sx};
    return 1;
}

static int merge_impl(const MergePlan& P, int dtype, const void* a, const void* gate, const void* f, void* y, int channels,
                      int width, void* stream_)
{
    if (!P.status) return 0;
    if (!a || !f || !y) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_merge(P, static_cast<const T*>(a), static_cast<const T*>(gate), static_cast<const T*>(f),
                            static_cast<T*>(y), (unsigned)channels, (unsigned)width, stream);
    });
}

int rroi_merge_forward_hip(int dtype, const void* a, int a_h, int a_w, const void* gate, int g_h, int g_w, const void* f,
                           void* y, int batch_size, int channels, int height, int width, void* stream)
{
    return merge_impl(plan_merge(dtype, batch_size, channels, height, width, a_h, a_w, g_h, g_w, gate ? 1 : 0, num_cus()), dtype,
                      a, gate, f, y, channels, width, stream);
}

#ifdef RROI_MERGE_MEASURE
// Measurement build only (`make merge-forms`; not declared in the header, not in the shipped library): the merge with V
// and K forced, for the comparison of the plan rule against its neighbours (tools/merge_bench.py --forms).
// *v_used / *k_used report what ran.
int rroi_merge_forward_forced_hip(int dtype, const void* a, int a_h, int a_w, const void* gate, int g_h, int g_w,
                                  const void* f, void* y, int batch_size, int channels, int height, int width, int force_v,
                                  int force_k, int* v_used, int* k_used, void* stream)
{
    const MergePlan P = plan_merge(dtype, batch_size, channels, height, width, a_h, a_w, g_h, g_w, gate ? 1 : 0, num_cus(),
                                   force_v, force_k);
    if (v_used) *v_used = P.V;
    if (k_used) *k_used = P.K;
    return merge_impl(P, dtype, a, gate, f, y, channels, width, stream);
}
#endif

// ------------------------------------------------------------------------------------
// The stand-alone resize, its backward and the merge's backward (header section 8b): one launch each, two or
// three and a workspace where dgate is wanted.
// ------------------------------------------------------------------------------------
int rroi_resize_footprint(int in, int out, int i, int* lo, int* hi)
{
    if (in < 1 || out < 1 || i < 0 || i >= in || !lo || !hi) return 0;
    rs_footprint(merge_scale(in, out), in, out, i, lo, hi);
    return 1;
}

int rroi_resize_forward_hip(int dtype, const void* x, void* y, int batch_size, int channels, int in_height, int in_width,
                            int height, int width, void* stream_)
{
    const MergePlan P = plan_merge(dtype, batch_size, channels, height, width, in_height, in_width, 1, 1, 0, num_cus());
    if (!P.status || !x || !y) return 0;
    const size_t esize = dtype == RROI_DTYPE_FP32 ? 4 : 2, planes = (size_t)batch_size * channels;
    if (bytes_overlap(y, planes * height * width * esize, x, planes * in_height * in_width * esize)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_resize(P, static_cast<const T*>(x), static_cast<T*>(y), (unsigned)channels, (unsigned)width, stream);
    });
}

int rroi_resize_backward_plan(int dtype, int batch_size, int channels, int in_height, int in_width, int height, int width,
                              rroi_resize_backward_plan_info* plan)
{
    const ResizeBwdPlan P = plan_resize_backward(dtype, batch_size, channels, in_height, in_width, height, width, num_cus());
    if (!P.status || !plan) return 0;
    *plan = rroi_resize_backward_plan_info{1, P.K, (int)P.tiles, (int)P.grid, kMgThreads, (int)P.cb, P.ident ? 1 : 0,
                                           P.max_rows, P.max_cols, P.sy, P.sx};
    return 1;
}

int rroi_resize_backward_hip(int dtype, const void* dy, void* dx, int batch_size, int channels, int in_height, int in_width,
                             int height, int width, void* stream_)
{
    const ResizeBwdPlan P = plan_resize_backward(dtype, batch_size, channels, in_height, in_width, height, width, num_cus());
    if (!P.status || !dy || !dx) return 0;
    const size_t esize = dtype == RROI_DTYPE_FP32 ? 4 : 2, planes = (size_t)batch_size * channels;
    if (bytes_overlap(dx, planes * in_height * in_width * esize, dy, planes * height * width * esize)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_resize_backward(P, static_cast<const T*>(dy), static_cast<T*>(dx), (unsigned)channels, in_height, in_width,
                                      height, width, stream);
    });
}

size_t rroi_merge_backward_workspace_bytes(int dtype, int batch_size, int channels, int height, int width, int g_h, int g_w)
{
    return plan_merge_backward(dtype, batch_size, channels, height, width, g_h, g_w, 1).ws_bytes;
}

int rroi_merge_backward_plan(int dtype, int batch_size, int channels, int height, int width, int g_h, int g_w, int gated,
                             rroi_merge_backward_plan_info* plan)
{
    const MergeBwdPlan P = plan_merge_backward(dtype, batch_size, channels, height, width, g_h, g_w, gated);
    if (!P.status || !plan) return 0;
    // launches: of a call that wants dgate (df alone is one; the blocks' sum is a launch of its own where there are several)
    *plan = rroi_merge_backward_plan_info{P.V, P.K, (int)P.tiles, (int)P.grid, kMgThreads, (int)P.cb, (int)P.gtiles,
                                          (int)P.ggrid, P.resize_g ? 1 : 0, P.gated ? (P.K > 1 ? 3 : 2) : 1, (long long)P.ws_bytes,
                                          P.G.sy, P.G.sx};
    return 1;
}

int rroi_merge_backward_hip(int dtype, const void* dy, const void* f, const void* gate, void* df, void* dgate, int batch_size,
                            int channels, int height, int width, int g_h, int g_w, void* workspace, size_t workspace_bytes,
                            void* stream_)
{
    const MergeBwdPlan P = plan_merge_backward(dtype, batch_size, channels, height, width, g_h, g_w, gate ? 1 : 0);
    if (!P.status) return 0;
    if (!dy || !f || (!df && !dgate) || (dgate && !gate)) return 0;
    const size_t esize = dtype == RROI_DTYPE_FP32 ? 4 : 2;
    const size_t map_bytes = (size_t)batch_size * channels * P.hw * esize, gate_bytes = (size_t)batch_size * P.ghw * esize;
    for (const void* in : {dy, f}) {
        if (bytes_overlap(df, map_bytes, in, map_bytes) || bytes_overlap(dgate, gate_bytes, in, map_bytes)) return 0;
    }
    if (bytes_overlap(df, map_bytes, gate, gate_bytes) || bytes_overlap(dgate, gate_bytes, gate, gate_bytes) ||
        bytes_overlap(df, map_bytes, dgate, gate_bytes))
        return 0;
    if (dgate && (!workspace_ok(workspace) || workspace_bytes < P.ws_bytes)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_merge_backward(P, static_cast<const T*>(dy), static_cast<const T*>(f), static_cast<const T*>(gate),
                                     static_cast<T*>(df), static_cast<T*>(dgate), (unsigned)channels, height, width, workspace,
                                     stream);
    });
}

// ------------------------------------------------------------------------------------
// Dense 3x3 convolution on the matrix cores, bfloat16 / float16 (header section 9): one launch, no workspace.
// ------------------------------------------------------------------------------------
int rroi_conv3x3_plan(int dtype, int batch_size, int in_channels, int out_channels, int height, int width, int stride,
                      rroi_conv3x3_plan_info* plan)
{
    const ConvPlan P = plan_conv3x3(dtype, batch_size, in_channels, out_channels, height, width, stride);
    if (!P.status || !plan) return 0;
    *plan = rroi_conv3x3_plan_info{32 * P.MT, 4 * P.NT, kCvTileW, P.KC, (int)P.k_chunks, (int)P.m_tiles, (int)P.y_tiles,
                                   (int)P.x_tiles, (int)P.grid, kCvThreads, P.lds_bytes, P.Ho, P.Wo, 0};
    return 1;
}

static int conv3x3_impl(const ConvPlan& P, int dtype, const void* x, const void* w, void* y, int in_channels, int out_channels,
                        int height, int width, int stride, float negative_slope, void* stream_)
{
    if (!P.status) return 0;
    if (!x || !w || !y) return 0;
    if (!std::isfinite(negative_slope)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (dtype == RROI_DTYPE_BF16)
        return launch_conv3x3(P, static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(w), static_cast<bf16_t*>(y),
                              (unsigned)in_channels, (unsigned)out_channels, (unsigned)height, (unsigned)width, stride,
                              negative_slope, stream);
    return launch_conv3x3(P, static_cast<const fp16_t*>(x), static_cast<const fp16_t*>(w), static_cast<fp16_t*>(y),
                          (unsigned)in_channels, (unsigned)out_channels, (unsigned)height, (unsigned)width, stride,
                          negative_slope, stream);
}

int rroi_conv3x3_forward_hip(int dtype, const void* x, const void* w, void* y, int batch_size, int in_channels,
                             int out_channels, int height, int width, int stride, float negative_slope, void* stream)
{
    return conv3x3_impl(plan_conv3x3(dtype, batch_size, in_channels, out_channels, height, width, stride), dtype, x,
                        w, y, in_channels, out_channels, height, width, stride, negative_slope, stream);
}

#ifdef RROI_CONV3X3_MEASURE
// Measurement build only (`make conv-forms`; not declared in the header, not in the shipped library): the convolution with
// the tile shape (32 * force_mt channels, 4 * force_nt rows) and the K chunk forced, for the comparison of the plan rule
// against its neighbours (tools/conv3x3_bench.py --forms).  *used = {MT, NT, KC} that ran.
int rroi_conv3x3_forward_forced_hip(int dtype, const void* x, const void* w, void* y, int batch_size, int in_channels,
                                    int out_channels, int height, int width, int stride, float negative_slope, int force_mt,
                                    int force_nt, int force_kc, int* used, void* stream)
{
    const ConvPlan P = plan_conv3x3(dtype, batch_size, in_channels, out_channels, height, width, stride, force_mt,
                                    force_nt, force_kc);
    if (used) used[0] = P.MT, used[1] = P.NT, used[2] = P.KC;
    return conv3x3_impl(P, dtype, x, w, y, in_channels, out_channels, height, width, stride, negative_slope, stream);
}
#endif

// ------------------------------------------------------------------------------------
// The recogniser's head and its activation + (2,1) max-pool (header section 10): one launch each, no workspace.
// ------------------------------------------------------------------------------------
int rroi_ocr_head_plan(int dtype, int batch_size, int channels, int classes, int steps, rroi_ocr_head_plan_info* plan)
{
    const OcrHeadPlan P = plan_ocr_head(dtype, batch_size, channels, classes, steps);
    if (!P.status || !plan) return 0;
    *plan = rroi_ocr_head_plan_info{kOhClasses, P.S, kOhCols, (int)P.tiles, (int)P.grid, P.S * 64, (int)P.lds_bytes,
                                    kOhMaxClasses};
    return 1;
}

int rroi_ocr_head_forward_hip(int dtype, const void* x, const void* w, const void* b, void* y, int batch_size, int channels,
                              int classes, int steps, void* stream_)
{
    const OcrHeadPlan P = plan_ocr_head(dtype, batch_size, channels, classes, steps);
    if (!P.status) return 0;
    if (!x || !w || !y) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_ocr_head(P, static_cast<const T*>(x), static_cast<const T*>(w), static_cast<const T*>(b),
                               static_cast<T*>(y), (unsigned)channels, (unsigned)classes, (unsigned)steps, stream);
    });
}

int rroi_act_maxpool2x1_forward_hip(int dtype, const void* x, void* y, int batch_size, int channels, int height, int width,
                                    float negative_slope, void* stream_)
{
    const ActPoolPlan P = plan_act_pool(dtype, batch_size, channels, height, width);
    if (!P.status) return 0;
    if (!x || !y) return 0;
    if (!std::isfinite(negative_slope)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_act_pool(P, static_cast<const T*>(x), static_cast<T*>(y), (unsigned)height, (unsigned)width,
                               negative_slope, stream);
    });
}

// ------------------------------------------------------------------------------------
// 1x1 convolution on the matrix cores with an optional folded BatchNorm, bfloat16 / float16 (header section 11):
// one launch, no workspace, no cache of folded parameters.
// ------------------------------------------------------------------------------------
int rroi_conv1x1_plan(int dtype, int batch_size, int in_channels, int out_channels, int height, int width, int stride,
                      rroi_conv1x1_plan_info* plan)
{
    const Conv1x1Plan P = plan_conv1x1(dtype, batch_size, in_channels, out_channels, height, width, stride);
    if (!P.status || !plan) return 0;
    *plan = rroi_conv1x1_plan_info{32 * P.MT, kC1Pixels, kC1Chunk, (int)P.k_chunks, (int)P.m_tiles, (int)P.p_tiles,
                                   (int)P.grid, kC1Threads, P.lds_bytes, P.Ho, P.Wo, 0};
    return 1;
}

static int conv1x1_impl(const Conv1x1Plan& P, int dtype, const void* x, const void* w, void* y, int in_channels,
                        int out_channels, int height, int width, int stride, float negative_slope, const void* bn_weight,
                        const void* bn_bias, const void* bn_mean, const void* bn_var, double eps, void* stream_)
{
    if (!P.status) return 0;
    if (!x || !w || !y) return 0;
    if (!std::isfinite(negative_slope) || !std::isfinite(eps) || eps < 0.0) return 0;
    if ((bn_weight == nullptr) != (bn_bias == nullptr) || (bn_mean == nullptr) != (bn_var == nullptr)) return 0;
    if (bn_weight && !bn_mean) return 0;     // an affine pair without statistics is no norm
    const Conv1x1Norm bn{bn_weight, bn_bias, bn_mean, bn_var, (float)eps};
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (dtype == RROI_DTYPE_BF16)
        return launch_conv1x1(P, static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(w), static_cast<bf16_t*>(y), bn,
                              (unsigned)in_channels, (unsigned)out_channels, (unsigned)height, (unsigned)width, stride,
                              negative_slope, stream);
    return launch_conv1x1(P, static_cast<const fp16_t*>(x), static_cast<const fp16_t*>(w), static_cast<fp16_t*>(y), bn,
                          (unsigned)in_channels, (unsigned)out_channels, (unsigned)height, (unsigned)width, stride,
                          negative_slope, stream);
}

int rroi_conv1x1_forward_hip(int dtype, const void* x, const void* w, void* y, int batch_size, int in_channels,
                             int out_channels, int height, int width, int stride, float negative_slope,
                             const void* bn_weight, const void* bn_bias, const void* bn_mean, const void* bn_var, double eps,
                             void* stream)
{
    return conv1x1_impl(plan_conv1x1(dtype, batch_size, in_channels, out_channels, height, width, stride), dtype, x, w, y,
                        in_channels, out_channels, height, width, stride, negative_slope, bn_weight, bn_bias, bn_mean, bn_var,
                        eps, stream);
}

#ifdef RROI_CONV1X1_MEASURE
// Measurement build only (`make conv1x1-forms`; not declared in the header, not in the shipped library): the convolution
// with 32 * force_mt output channels per workgroup, for the comparison of the plan rule against its neighbour
// (tools/conv1x1_bench.py --forms).  *mt_used = the MT that ran.
int rroi_conv1x1_forward_forced_hip(int dtype, const void* x, const void* w, void* y, int batch_size, int in_channels,
                                    int out_channels, int height, int width, int stride, float negative_slope,
                                    const void* bn_weight, const void* bn_bias, const void* bn_mean, const void* bn_var,
                                    double eps, int force_mt, int* mt_used, void* stream)
{
    const Conv1x1Plan P = plan_conv1x1(dtype, batch_size, in_channels, out_channels, height, width, stride, force_mt);
    if (mt_used) *mt_used = P.MT;
    return conv1x1_impl(P, dtype, x, w, y, in_channels, out_channels, height, width, stride, negative_slope, bn_weight,
                        bn_bias, bn_mean, bn_var, eps, stream);
}
#endif

// ------------------------------------------------------------------------------------
// The recogniser's (2,3) convolution on the matrix cores, bfloat16 / float16 (header section 12): one launch,
// no workspace.
// ------------------------------------------------------------------------------------
int rroi_conv2x3_plan(int dtype, int batch_size, int in_channels, int out_channels, int height, int width,
                      rroi_conv2x3_plan_info* plan)
{
    const Conv2x3Plan P = plan_conv2x3(dtype, batch_size, in_channels, out_channels, height, width);
    if (!P.status || !plan) return 0;
    *plan = rroi_conv2x3_plan_info{32, kC2TileW, kC2Items, kC2KC, (int)P.k_chunks, (int)P.m_tiles, (int)P.x_tiles,
                                   (int)P.items, (int)P.grid, kC2Threads, kC2LdsBytes, P.Ho, width, 0};
    return 1;
}

int rroi_conv2x3_forward_hip(int dtype, const void* x, const void* w, void* y, int batch_size, int in_channels,
                             int out_channels, int height, int width, float negative_slope, void* stream_)
{
    const Conv2x3Plan P = plan_conv2x3(dtype, batch_size, in_channels, out_channels, height, width);
    if (!P.status) return 0;
    if (!x || !w || !y) return 0;
    if (!std::isfinite(negative_slope)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (dtype == RROI_DTYPE_BF16)
        return launch_conv2x3(P, static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(w), static_cast<bf16_t*>(y),
                              (unsigned)in_channels, (unsigned)out_channels, (unsigned)height, (unsigned)width,
                              negative_slope, stream);
    return launch_conv2x3(P, static_cast<const fp16_t*>(x), static_cast<const fp16_t*>(w), static_cast<fp16_t*>(y),
                          (unsigned)in_channels, (unsigned)out_channels, (unsigned)height, (unsigned)width, negative_slope,
                          stream);
}

// ------------------------------------------------------------------------------------
// Bilinear resize + depthwise 3x3 convolution (header section 13): one launch, no workspace.
// ------------------------------------------------------------------------------------
int rroi_up_depthwise3x3_forward_hip(int dtype, const void* a, const void* weight, void* y, int batch_size, int channels,
                                     int in_height, int in_width, int out_height, int out_width, void* stream_)
{
    if (!updw_shape_ok(dtype, batch_size, channels, in_height, in_width, out_height, out_width)) return 0;
    if (!a || !weight || !y) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_updw(static_cast<const T*>(a), static_cast<const T*>(weight), static_cast<T*>(y), batch_size, channels,
                           in_height, in_width, out_height, out_width, stream);
    });
}

// ------------------------------------------------------------------------------------
// Native preprocessing (header section 14): uint8 images to the network's input, one launch, no workspace.
// ------------------------------------------------------------------------------------
int rroi_preprocess_plan(int dtype, int batch_size, int out_height, int out_width, rroi_preprocess_plan_info* plan)
{
    const PreprocessPlan P = plan_preprocess(dtype, batch_size, out_height, out_width);
    if (!P.status || !plan) return 0;
    *plan = rroi_preprocess_plan_info{(int)P.grid, kPpThreads, P.V, P.band, (int)P.nstrips, (int)P.nbands, (int)P.items, P.wide};
    return 1;
}

int rroi_preprocess_forward_hip(int dtype, const unsigned char* src, const int* table, void* y, int batch_size,
                                int out_height, int out_width, void* stream_)
{
    const PreprocessPlan P = plan_preprocess(dtype, batch_size, out_height, out_width);
    if (!P.status) return 0;
    if (batch_size == 0) return 1;
    if (!src || !table || !y) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_preprocess(P, src, table, static_cast<T*>(y), out_height, out_width, stream);
    });
}

// ------------------------------------------------------------------------------------
// The native CTC loss (header section 15): every sequence's nll and the unscaled gradient in one launch.
// ------------------------------------------------------------------------------------
int rroi_ctc_loss_plan(int dtype, int batch_size, int classes, int steps, int max_target_length, long long stride_t,
                       long long stride_k, int want_grad, rroi_ctc_loss_plan_info* plan)
{
    const CtcPlan P = plan_ctc_loss(dtype, batch_size, classes, steps, max_target_length, stride_t, stride_k, want_grad);
    if (!P.status || !plan) return 0;
    *plan = rroi_ctc_loss_plan_info{(int)P.grid, kCtcThreads, (int)P.lds_bytes, (int)kCtcLdsLimit, P.smax, P.chunk, P.along_t,
                                    P.workspace_bytes != 0};
    return 1;
}

size_t rroi_ctc_loss_workspace_bytes(int batch_size, int classes, int steps, int max_target_length, int want_grad)
{
    return plan_ctc_loss(RROI_DTYPE_FP32, batch_size, classes, steps, max_target_length, 0, 1, want_grad).workspace_bytes;
}

int rroi_ctc_loss_forward_hip(int dtype, const void* log_probs, long long stride_t, long long stride_n, long long stride_k,
                              int batch_size, int classes, int steps, const int* targets, int max_target_length,
                              const int* input_lengths, const int* target_lengths, int blank, int zero_infinity, float* nll,
                              void* grad, long long grad_stride_t, long long grad_stride_n, long long grad_stride_k,
                              void* workspace, size_t workspace_bytes, void* stream_)
{
    const CtcPlan P = plan_ctc_loss(dtype, batch_size, classes, steps, max_target_length, stride_t, stride_k, grad != nullptr);
    if (!P.status || blank < 0 || blank >= classes) return 0;
    if (batch_size == 0) return 1;
    if (!log_probs || !input_lengths || !target_lengths || !nll || (max_target_length > 0 && !targets)) return 0;
    if (P.workspace_bytes && (!workspace || workspace_bytes < P.workspace_bytes || reinterpret_cast<size_t>(workspace) % 8)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        return launch_ctc_loss(P, static_cast<const T*>(log_probs), CtcStrides{stride_t, stride_n, stride_k}, classes, steps, targets,
                               max_target_length, input_lengths, target_lengths, blank, zero_infinity, nll, static_cast<T*>(grad),
                               CtcStrides{grad_stride_t, grad_stride_n, grad_stride_k}, workspace, stream);
    });
}

// ------------------------------------------------------------------------------------
// The native detection loss (header section 16): two launches forward (partial sums, finish), one backward.
// ------------------------------------------------------------------------------------
int rroi_detection_loss_plan(int dtype, int batch_size, int height, int width, int height8, int width8,
                             rroi_detection_loss_plan_info* plan)
{
    const DlPlan P = plan_detection_loss(dtype, batch_size, height, width, height8, width8);
    if (!P.status || !plan) return 0;
    *plan = rroi_detection_loss_plan_info{(int)P.grid, kDlThreads, P.S.ipt, (int)P.S.blocks4, (int)P.S.blocks8, kDlSums, 2 * kDlSums,
                                          kDlFinishThreads};
    return 1;
}

size_t rroi_detection_loss_workspace_bytes(int batch_size, int height, int width, int height8, int width8)
{
    return plan_detection_loss(RROI_DTYPE_FP32, batch_size, height, width, height8, width8).workspace_bytes;
}

int rroi_detection_loss_forward_hip(int dtype, const void* segm4, const void* angle4, const void* roi4, const void* segm8,
                                    const void* angle8, const void* roi8, const float* segm_gt, const float* iou_mask,
                                    const float* angle_gt, const float* roi_gt, int batch_size, int height, int width, int height8,
                                    int width8, float* terms, void* workspace, size_t workspace_bytes, void* stream_)
{
    const DlPlan P = plan_detection_loss(dtype, batch_size, height, width, height8, width8);
    if (!P.status) return 0;
    if (!segm4 || !angle4 || !roi4 || !segm_gt || !iou_mask || !angle_gt || !roi_gt || !terms) return 0;
    if (height8 && (!segm8 || !angle8 || !roi8)) return 0;
    if (!dl_aligned(roi_gt, 16)) return 0;                                        // read four channels at a time
    if (!workspace || workspace_bytes < P.workspace_bytes || !dl_aligned(workspace, 8)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        const DlPreds<T> p4{static_cast<const T*>(segm4), static_cast<const T*>(angle4), static_cast<const T*>(roi4)};
        const DlPreds<T> p8{static_cast<const T*>(segm8), static_cast<const T*>(angle8), static_cast<const T*>(roi8)};
        return launch_detection_loss_forward(P, p4, p8, DlTruth{segm_gt, iou_mask, angle_gt, roi_gt}, terms, workspace, stream);
    });
}

int rroi_detection_loss_backward_hip(int dtype, const void* angle4, const void* roi4, const void* angle8, const void* roi8,
                                     const float* segm_gt, const float* iou_mask, const float* angle_gt, const float* roi_gt,
                                     int batch_size, int height, int width, int height8, int width8, const double* state,
                                     const float* grad_terms, void* grad_segm4, void* grad_angle4, void* grad_roi4, void* grad_segm8,
                                     void* grad_angle8, void* grad_roi8, void* stream_)
{
    const DlPlan P = plan_detection_loss(dtype, batch_size, height, width, height8, width8);
    if (!P.status) return 0;
    if (!angle4 || !roi4 || !segm_gt || !iou_mask || !angle_gt || !roi_gt || !grad_segm4 || !grad_angle4 || !grad_roi4) return 0;
    if (height8 && (!angle8 || !roi8 || !grad_segm8 || !grad_angle8 || !grad_roi8)) return 0;
    if (!dl_aligned(roi_gt, 16)) return 0;
    if (!state || !dl_aligned(state, 8) || !grad_terms || !dl_aligned(grad_terms, 4)) return 0;
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    return with_dtype(dtype, [&](auto tag) {
        typedef decltype(tag) T;
        const DlPreds<T> p4{nullptr, static_cast<const T*>(angle4), static_cast<const T*>(roi4)};
        const DlPreds<T> p8{nullptr, static_cast<const T*>(angle8), static_cast<const T*>(roi8)};
        const DlGrads<T> g4{static_cast<T*>(grad_segm4), static_cast<T*>(grad_angle4), static_cast<T*>(grad_roi4)};
        const DlGrads<T> g8{static_cast<T*>(grad_segm8), static_cast<T*>(grad_angle8), static_cast<T*>(grad_roi8)};
        return launch_detection_loss_backward(P, p4, p8, DlTruth{segm_gt, iou_mask, angle_gt, roi_gt}, state, grad_terms, g4, g8, stream);
    });
}

int rroi_align_set_trig_recipe_hip(int recipe) { return recipe == RROI_TRIG_DOUBLE ? 1 : 0; }   // deprecated shim, see the header
int rroi_align_get_trig_recipe_hip(void) { return RROI_TRIG_DOUBLE; }

int rroi_align_launcher_scratch_stats(int* in_use, int* pinned, int* capacity, unsigned long long* transient_calls)
{
    std::lock_guard<std::mutex> table(g_table_mutex);
    int u = 0, p = 0;
    for (const LauncherArena& a : g_arenas) {
        u += a.used ? 1 : 0;
        p += a.used && a.pinned ? 1 : 0;
    }
    if (in_use) *in_use = u;
    if (pinned) *pinned = p;
    if (capacity) *capacity = kMaxArenas;
    if (transient_calls) *transient_calls = g_transient_calls.load(std::memory_order_relaxed);
    return 1;
}

int rroi_align_release_launcher_scratch(void)
{
    std::unique_lock<std::mutex> table(g_table_mutex);
    int cur = 0;
    (void)hipGetDevice(&cur);
    hipError_t e = hipSuccess;
    for (int i = 0; i < kMaxArenas; ++i) {
        LauncherArena& a = g_arenas[i];
        if (!a.used || a.pinned) continue;   // pinned: a graph replays with this address, it lives as long as the process
        std::unique_lock<std::mutex> mine(a.in_use, std::try_to_lock);
        if (!mine.owns_lock()) {   // a call is enqueuing on it: wait without the table lock, then look at the entry again
            table.unlock();
            { std::lock_guard<std::mutex> wait(a.in_use); }
            table.lock();
            --i;
            continue;
        }
        (void)hipSetDevice(a.device);
        const hipError_t ei = hipFree(a.ptr);  // synchronous: the buffers' streams may be gone
        if (ei != hipSuccess) e = ei;
        a.used = false;
        a.ptr = nullptr;
        a.bytes = 0;
    }
    (void)hipSetDevice(cur);
    return status_of(e);
}

}  // extern "C"
