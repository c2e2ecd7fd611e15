// rroi_detection_loss_kernels.h -- the detection loss (dice, angle and IoU terms on both scales) and its gradient, DESIGN 5.23
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_ctc_loss_kernels.h, whose ctc_widen / ctc_narrow it uses); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// The contract is include/rroi_align_hip.h section 16.  Per scale (1/4: the ground truth as it lies; 1/8: the seven
// ground-truth planes resized inside the kernel with 5.14's recipe, never stored) and per pixel, everything in double:
//     g = segm_gt, m = iou_mask, mask = g > 0.5, (d1, d2, d3, d4) = roi_gt (halved on 1/8), th = angle_gt
//     dice    I += p g m m,  P += p m,  G += g m
//     angle   mask:  c += 1,  Ss += (a0 - sin th)^2,  Sc += (a1 - cos th)^2
//     box     mask and d3 > 0:  nl += 1,  Ll += log((U + 1) / (X + 1))   with the left half's intersection X and union U
//             mask and d4 > 0:  nr += 1,  Lr += ...                      the right half's
// Ten sums per scale.  The item space is the N H W pixels of 1/4 followed by the N H8 W8 pixels of 1/8; a workgroup of 256
// threads owns 256 * ipt consecutive items of ONE scale (the 1/4 workgroups come first), thread t the items t, t + 256, ...
//
//   partial   each thread adds its items in ascending order; the workgroup's ten sums are a fixed tree -- an xor butterfly
//           over the 64 lanes of a wave (cross-lane moves), then the four waves' results from LDS in ascending order -- and go
//           to the workgroup's slot of the workspace.
//   finish    one workgroup: thread k adds sum k of its scale's slots in ascending order, writes the twenty totals (the
//           state the backward reads) and the four float32 terms.
//   backward  the same item space: a thread recomputes its pixel's ground truth and box geometry, reads five coefficients
//           that thread 0 derived from the state and g, and stores all seven gradient values of the pixel, zeros included.
// No atomic, no ticket, no order that depends on scheduling or on the device: a second run gives the same bits.
// Nothing is indexed by a value read from memory, so no contents of the tensors take a kernel out of bounds.
// ------------------------------------------------------------------------------------
constexpr int kDlThreads = 256;
constexpr int kDlSums = 10;             // per scale
constexpr int kDlFinishThreads = 64;
enum { DL_I = 0, DL_P, DL_G, DL_C, DL_SS, DL_SC, DL_NL, DL_LL, DL_NR, DL_LR };

struct DlShape {
    int N, H, W, H8, W8;          // H8 == 0: single scale
    double sy, sx;                // (H - 1) / (H8 - 1), (W - 1) / (W8 - 1); 0 where the 1/8 side is 1
    unsigned blocks4, blocks8;    // workgroups of each scale
    int ipt;                      // items per thread
};

template <class T>
struct DlPreds { const T *s, *a, *r; };      // (N, 1, h, w), (N, 2, h, w), (N, 4, h, w) of one scale
template <class T>
struct DlGrads { T *s, *a, *r; };
struct DlTruth { const float *segm, *mask, *angle, *roi; };   // (N, H, W) x 3, (N, H, W, 4)

struct DlPixel {
    double g, m, th, d1, d2, d3, d4;
};

__device__ __forceinline__ DlPixel dl_tap(const DlTruth& gt, size_t at)
{
    const float4 d = *reinterpret_cast<const float4*>(gt.roi + 4 * at);
    return {(double)gt.segm[at], (double)gt.mask[at], (double)gt.angle[at], (double)d.x, (double)d.y, (double)d.z, (double)d.w};
}

__device__ __forceinline__ double dl_blend(double v00, double v01, double v10, double v11, double lx1, double ly1)
{
    const double lx0 = 1.0 - lx1, ly0 = 1.0 - ly1;
    const double top = lx0 * v00 + lx1 * v01;
    const double bot = lx0 * v10 + lx1 * v11;
    return ly0 * top + ly1 * bot;
}

// the ground truth of item `i` (< N h w) of a scale: as it lies on 1/4, resized on 1/8 (roi_gt halved after the blend)
__device__ __forceinline__ DlPixel dl_truth(const DlTruth& gt, const DlShape& S, bool eighth, unsigned i)
{
    if (!eighth) return dl_tap(gt, (size_t)i);
    const unsigned hw8 = (unsigned)S.H8 * (unsigned)S.W8;
    const unsigned n = i / hw8, rest = i % hw8, y = rest / (unsigned)S.W8, x = rest % (unsigned)S.W8;
    const MgAxis ay = mg_axis(S.sy, y, S.H), ax = mg_axis(S.sx, x, S.W);
    const size_t at = ((size_t)n * S.H + ay.i0) * S.W + ax.i0;
    const size_t dx = (size_t)ax.step, dy = (size_t)ay.step * S.W;
    const DlPixel a = dl_tap(gt, at), b = dl_tap(gt, at + dx), c = dl_tap(gt, at + dy), d = dl_tap(gt, at + dy + dx);
    DlPixel p;
    p.g = dl_blend(a.g, b.g, c.g, d.g, ax.l1, ay.l1);
    p.m = dl_blend(a.m, b.m, c.m, d.m, ax.l1, ay.l1);
    p.th = dl_blend(a.th, b.th, c.th, d.th, ax.l1, ay.l1);
    p.d1 = dl_blend(a.d1, b.d1, c.d1, d.d1, ax.l1, ay.l1) * 0.5;
    p.d2 = dl_blend(a.d2, b.d2, c.d2, d.d2, ax.l1, ay.l1) * 0.5;
    p.d3 = dl_blend(a.d3, b.d3, c.d3, d.d3, ax.l1, ay.l1) * 0.5;
    p.d4 = dl_blend(a.d4, b.d4, c.d4, d.d4, ax.l1, ay.l1) * 0.5;
    return p;
}

// one half of the box term: the ground truth's and the prediction's (top, bottom, side)
struct DlHalf { double x, u; };       // intersection and union
__device__ __forceinline__ DlHalf dl_half(double g1, double g2, double gs, double p1, double p2, double ps)
{
    const double area_g = (g1 + g2) * gs, area_p = (p1 + p2) * ps;
    const double w = fmin(gs, ps), h = fmin(g1, p1) + fmin(g2, p2);
    const double x = w * h;
    return {x, area_g + area_p - x};
}
// torch's rule for min(gt, pred): the gradient goes to the smaller side, a tie is split in half
__device__ __forceinline__ double dl_min_share(double gt, double pred) { return pred < gt ? 1.0 : pred == gt ? 0.5 : 0.0; }

// which scale a workgroup works on, its first item, and the scale's geometry
struct DlWhere {
    bool eighth;
    unsigned first, items, hw;       // first item of the workgroup, items and pixels per image of the scale
};
__device__ __forceinline__ DlWhere dl_where(const DlShape& S)
{
    DlWhere w;
    w.eighth = blockIdx.x >= S.blocks4;
    w.hw = w.eighth ? (unsigned)S.H8 * (unsigned)S.W8 : (unsigned)S.H * (unsigned)S.W;
    w.items = (unsigned)S.N * w.hw;
    w.first = (w.eighth ? blockIdx.x - S.blocks4 : blockIdx.x) * (unsigned)(kDlThreads * S.ipt);
    return w;
}

// ---- forward, launch A: grid blocks4 + blocks8, 256 threads; slot b of `slots` gets workgroup b's ten sums
template <class T>
__global__ __launch_bounds__(kDlThreads) void rroi_detection_loss_partial_kernel(DlPreds<T> p4, DlPreds<T> p8, DlTruth gt, DlShape S,
                                                                                  double* __restrict__ slots)
{
    __shared__ double lds[kDlThreads / 64][kDlSums];
    const DlWhere w = dl_where(S);
    const DlPreds<T> p = w.eighth ? p8 : p4;
    double s[kDlSums];
#pragma unroll
    for (int k = 0; k < kDlSums; ++k) s[k] = 0.0;
    for (int j = 0; j < S.ipt; ++j) {
        const unsigned i = w.first + (unsigned)j * kDlThreads + threadIdx.x;
        if (i >= w.items) break;
        const DlPixel t = dl_truth(gt, S, w.eighth, i);
        const unsigned n = i / w.hw, px = i % w.hw;
        const double ps = ctc_widen(p.s[i]);
        s[DL_I] += ps * t.m * (t.g * t.m);
        s[DL_P] += ps * t.m;
        s[DL_G] += t.g * t.m;
        if (t.g > 0.5) {
            const size_t ab = (size_t)n * 2 * w.hw + px, rb = (size_t)n * 4 * w.hw + px;
            const double es = ctc_widen(p.a[ab]) - sin(t.th), ec = ctc_widen(p.a[ab + w.hw]) - cos(t.th);
            s[DL_C] += 1.0;
            s[DL_SS] += es * es;
            s[DL_SC] += ec * ec;
            const double r1 = ctc_widen(p.r[rb]), r2 = ctc_widen(p.r[rb + w.hw]);
            if (t.d3 > 0.0) {
                const DlHalf h = dl_half(t.d1, t.d2, t.d3, r1, r2, ctc_widen(p.r[rb + 2 * (size_t)w.hw]));
                s[DL_NL] += 1.0;
                s[DL_LL] += -log((h.x + 1.0) / (h.u + 1.0));
            }
            if (t.d4 > 0.0) {
                const DlHalf h = dl_half(t.d1, t.d2, t.d4, r1, r2, ctc_widen(p.r[rb + 3 * (size_t)w.hw]));
                s[DL_NR] += 1.0;
                s[DL_LR] += -log((h.x + 1.0) / (h.u + 1.0));
            }
        }
    }
    // the fixed tree: a butterfly over the wave's 64 lanes (every lane ends with the same bits), then the waves in order
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
#pragma unroll
        for (int k = 0; k < kDlSums; ++k) s[k] += __shfl_xor(s[k], off, 64);
    if ((threadIdx.x & 63u) == 0)
#pragma unroll
        for (int k = 0; k < kDlSums; ++k) lds[threadIdx.x >> 6][k] = s[k];
    __syncthreads();
    if (threadIdx.x < kDlSums) {
        double r = lds[0][threadIdx.x];
        for (int wv = 1; wv < kDlThreads / 64; ++wv) r += lds[wv][threadIdx.x];
        slots[(size_t)blockIdx.x * kDlSums + threadIdx.x] = r;
    }
}

// the three terms of one scale from its ten totals; an empty selection contributes 0
__device__ __forceinline__ void dl_terms(const double* t, double& segm, double& angle, double& box)
{
    segm += -((2.0 * t[DL_I] + 1.0) / (t[DL_P] + t[DL_G] + 1.0));
    if (t[DL_C] > 0.0) angle += t[DL_SS] / t[DL_C] + t[DL_SC] / t[DL_C];
    if (t[DL_NL] > 0.0) box += t[DL_LL] / t[DL_NL];
    if (t[DL_NR] > 0.0) box += t[DL_LR] / t[DL_NR];
}

// ---- forward, launch B: one workgroup of 64; state[0..10) the 1/4 totals, [10..20) the 1/8 totals (0 for a single scale)
__global__ __launch_bounds__(kDlFinishThreads) void rroi_detection_loss_finish_kernel(const double* __restrict__ slots, unsigned blocks4,
                                                                                       unsigned blocks8, double* __restrict__ state,
                                                                                       float* __restrict__ terms)
{
    __shared__ double tot[2 * kDlSums];
    const unsigned t = threadIdx.x;
    if (t < 2 * kDlSums) {
        const unsigned k = t % kDlSums;
        const unsigned b0 = t < kDlSums ? 0 : blocks4, b1 = t < kDlSums ? blocks4 : blocks4 + blocks8;
        double r = 0.0;
        for (unsigned b = b0; b < b1; ++b) r += slots[(size_t)b * kDlSums + k];
        tot[t] = r;
        state[t] = r;
    }
    __syncthreads();
    if (t == 0) {
        double segm = 0.0, angle = 0.0, box = 0.0;
        dl_terms(tot, segm, angle, box);
        if (blocks8) dl_terms(tot + kDlSums, segm, angle, box);
        terms[0] = (float)segm;
        terms[1] = (float)angle;
        terms[2] = (float)box;
        terms[3] = (float)(segm + 2.0 * angle + 0.5 * box);
    }
}

// ---- backward: the grid of launch A.  gw: the four float32 weights of the terms, on the device.
// Per scale five coefficients: grad_s = m cs1 - g m m cs2;  grad_a = ca (a - sin | cos);  the box halves scaled by cl, cr.
template <class T>
__global__ __launch_bounds__(kDlThreads) void rroi_detection_loss_backward_kernel(DlPreds<T> p4, DlPreds<T> p8, DlTruth gt, DlShape S,
                                                                                   const double* __restrict__ state,
                                                                                   const float* __restrict__ gw, DlGrads<T> g4, DlGrads<T> g8)
{
    __shared__ double coef[5];
    const DlWhere w = dl_where(S);
    if (threadIdx.x == 0) {
        const double* t = state + (w.eighth ? kDlSums : 0);
        const double g0 = (double)gw[0], g1 = (double)gw[1], g2 = (double)gw[2], g3 = (double)gw[3];
        const double w_segm = g0 + g3, w_angle = g1 + 2.0 * g3, w_box = g2 + 0.5 * g3;
        const double den = t[DL_P] + t[DL_G] + 1.0;
        coef[0] = w_segm * ((2.0 * t[DL_I] + 1.0) / (den * den));
        coef[1] = w_segm * (2.0 / den);
        coef[2] = t[DL_C] > 0.0 ? w_angle * 2.0 / t[DL_C] : 0.0;
        coef[3] = t[DL_NL] > 0.0 ? w_box / t[DL_NL] : 0.0;
        coef[4] = t[DL_NR] > 0.0 ? w_box / t[DL_NR] : 0.0;
    }
    __syncthreads();
    const double cs1 = coef[0], cs2 = coef[1], ca = coef[2], cl = coef[3], cr = coef[4];
    const DlPreds<T> p = w.eighth ? p8 : p4;
    const DlGrads<T> g = w.eighth ? g8 : g4;
    for (int j = 0; j < S.ipt; ++j) {
        const unsigned i = w.first + (unsigned)j * kDlThreads + threadIdx.x;
        if (i >= w.items) break;
        const DlPixel t = dl_truth(gt, S, w.eighth, i);
        const unsigned n = i / w.hw, px = i % w.hw;
        const size_t ab = (size_t)n * 2 * w.hw + px, rb = (size_t)n * 4 * w.hw + px;
        ctc_narrow(t.m * cs1 - t.g * t.m * t.m * cs2, g.s + i);
        double ga0 = 0.0, ga1 = 0.0, gr1 = 0.0, gr2 = 0.0, gr3 = 0.0, gr4 = 0.0;
        if (t.g > 0.5) {
            ga0 = ca * (ctc_widen(p.a[ab]) - sin(t.th));
            ga1 = ca * (ctc_widen(p.a[ab + w.hw]) - cos(t.th));
            const double r1 = ctc_widen(p.r[rb]), r2 = ctc_widen(p.r[rb + w.hw]);
            const double m1 = dl_min_share(t.d1, r1), m2 = dl_min_share(t.d2, r2);
            if (t.d3 > 0.0) {
                // L = log(U + 1) - log(X + 1), U = A_gt + A_pred - X:  dL = dA_pred / (U + 1) - dX (1 / (U + 1) + 1 / (X + 1))
                const double r3 = ctc_widen(p.r[rb + 2 * (size_t)w.hw]);
                const DlHalf h = dl_half(t.d1, t.d2, t.d3, r1, r2, r3);
                const double iu = 1.0 / (h.u + 1.0), ix = iu + 1.0 / (h.x + 1.0);
                const double wd = fmin(t.d3, r3), ht = fmin(t.d1, r1) + fmin(t.d2, r2);
                gr1 += cl * (r3 * iu - wd * m1 * ix);
                gr2 += cl * (r3 * iu - wd * m2 * ix);
                gr3 = cl * ((r1 + r2) * iu - ht * dl_min_share(t.d3, r3) * ix);
            }
            if (t.d4 > 0.0) {
                const double r4 = ctc_widen(p.r[rb + 3 * (size_t)w.hw]);
                const DlHalf h = dl_half(t.d1, t.d2, t.d4, r1, r2, r4);
                const double iu = 1.0 / (h.u + 1.0), ix = iu + 1.0 / (h.x + 1.0);
                const double wd = fmin(t.d4, r4), ht = fmin(t.d1, r1) + fmin(t.d2, r2);
                gr1 += cr * (r4 * iu - wd * m1 * ix);
                gr2 += cr * (r4 * iu - wd * m2 * ix);
                gr4 = cr * ((r1 + r2) * iu - ht * dl_min_share(t.d4, r4) * ix);
            }
        }
        ctc_narrow(ga0, g.a + ab);
        ctc_narrow(ga1, g.a + ab + w.hw);
        ctc_narrow(gr1, g.r + rb);
        ctc_narrow(gr2, g.r + rb + w.hw);
        ctc_narrow(gr3, g.r + rb + 2 * (size_t)w.hw);
        ctc_narrow(gr4, g.r + rb + 3 * (size_t)w.hw);
    }
}
