// rroi_instancenorm_backward_kernels.h -- the training forward and the backward of InstanceNorm2d with its activation,
// DESIGN 5.24.  Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_instancenorm_kernels.h, whose streaming helpers and block sum it uses, and rroi_ctc_loss_kernels.h, whose
// ctc_narrow rounds a double once to T); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// Training forward (header section 6c): the kernels of section 6 with one more output, the plane's {mean, var} as the
// forward formed them -- mean = K + m, var after the clamp -- one pair of doubles per plane.  y is computed by the very
// device functions of rroi_inorm_plane_kernel / rroi_inorm_apply_kernel in the same order: the same bits.
//   rroi_inorm_train_plane_kernel   plane form
//   rroi_inorm_train_apply_kernel   split form, launch 2 (launch 1 is rroi_inorm_stats_kernel as it stands); the
//                                   workgroup of a plane's first segment stores the pair
//
// Backward, per (n, c) plane of n elements, everything in double and each operation rounded once:
//     a = gamma / sqrt(var + eps), b = beta - mean a          the forward's own coefficients, from the saved pair
//     v = (float)(x a + b);  d = v > 0 ? 1 : slope;  g = dy d        (the sign decisions are the forward's)
//     rs = 1 / sqrt(var + eps);  xh = (x - mean) rs
//     t1 = sum g,  t2 = sum g xh
//     dx = (T)(float)(A ((g - t1 / n) - xh (t2 / n))),  A = gamma rs
//     dbeta[c] = sum over n of t1(n, c),  dgamma[c] = sum over n of t2(n, c), each rounded once to T
// The structure is the forward's: pass 1 streams x and dy following x's address (dy by vectors where it shares that
// alignment, by elements otherwise), pass 2 follows dx's address (vector stores) and loads x and dy each by vectors
// where it shares dx's alignment.  Lanes add in address order, waves by the butterfly, the four waves through LDS in
// wave order (in_block_sum): no atomic anywhere, the same arguments give the same bits.
//   rroi_inorm_bwd_plane_kernel     one workgroup per plane: pass 1, pass 2 (the plane is still in L2); {t1, t2} to
//                                   `plane_sums` where parameter gradients are wanted; dx == NULL skips pass 2
//   rroi_inorm_bwd_partial_kernel   split form, launch 1: workgroup (plane, segment) leaves {t1, t2} of its segment
//   rroi_inorm_bwd_apply_kernel     split form, launch 2: lane t takes pair t of its plane, the block sum combines them
//                                   (the same bits in every workgroup of the plane), then the workgroup maps its segment
//   rroi_inorm_bwd_param_kernel     lane c adds the N plane pairs of channel c in n order and stores dgamma[c], dbeta[c]
// The launch boundary is the only synchronisation between workgroups.
// ------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(kInThreads) void rroi_inorm_train_plane_kernel(
    const T* __restrict__ x, const T* __restrict__ gamma, const T* __restrict__ beta, T* __restrict__ y,
    double2* __restrict__ stats, unsigned C, unsigned n, unsigned planes, double eps, float slope)
{
    __shared__ double lds[2 * kInThreads / 64];
    for (unsigned plane = blockIdx.x; plane < planes; plane += gridDim.x) {
        const T* xp = x + (size_t)plane * n;
        const double K = (double)to_f32(xp[0]);
        const InSums s = in_block_sum(in_accumulate<T>(xp, n, K), lds);
        double mean, var, a, b;
        in_moments(s, K, n, mean, var);
        in_affine<T>(mean, var, gamma, beta, plane % C, eps, a, b);
        if (threadIdx.x == 0) stats[plane] = double2{mean, var};
        in_map<T>(xp, y + (size_t)plane * n, n, a, b, slope);
        __syncthreads();               // the next plane's sums reuse lds
    }
}

template <class T>
__global__ __launch_bounds__(kInThreads) void rroi_inorm_train_apply_kernel(
    const T* __restrict__ x, const T* __restrict__ gamma, const T* __restrict__ beta, T* __restrict__ y,
    double2* __restrict__ stats, const double2* __restrict__ pairs, unsigned C, unsigned n, unsigned seg, unsigned nseg,
    double eps, float slope)
{
    __shared__ double lds[2 * kInThreads / 64];
    const unsigned plane = blockIdx.x / nseg, lo = (blockIdx.x % nseg) * seg;
    const T* xp = x + (size_t)plane * n;
    const double K = (double)to_f32(xp[0]);
    InSums p{0.0, 0.0};                // as in rroi_inorm_apply_kernel: lane t holds pair t, the others +0.0
    if (threadIdx.x < nseg) {
        const double2 v = pairs[(size_t)plane * nseg + threadIdx.x];
        p = InSums{v.x, v.y};
    }
    const InSums s = in_block_sum(p, lds);
    double mean, var, a, b;
    in_moments(s, K, n, mean, var);
    in_affine<T>(mean, var, gamma, beta, plane % C, eps, a, b);
    if (lo == 0 && threadIdx.x == 0) stats[plane] = double2{mean, var};
    in_map<T>(xp + lo, y + (size_t)plane * n + lo, min(seg, n - lo), a, b, slope);
}

// ------------------------------------------------------------------------------------
// Backward.
// ------------------------------------------------------------------------------------
struct InbPlane {                  // what a plane's elements need of its statistics and parameters
    double a, b;                   // the forward's coefficients
    double mean, rs;               // xh = (x - mean) rs
    double A;                      // gamma rs (rs without affine: gamma = 1.0 exactly)
    double slope;                  // (double)negative_slope
};

template <class T>
__device__ __forceinline__ InbPlane inb_plane(double2 st, const T* gamma, const T* beta, unsigned c, double eps, float slope)
{
    InbPlane k;
    in_affine<T>(st.x, st.y, gamma, beta, c, eps, k.a, k.b);
    k.mean = st.x;
    k.rs = 1.0 / sqrt(st.y + eps);
    k.A = (gamma ? (double)to_f32(gamma[c]) : 1.0) * k.rs;
    k.slope = (double)slope;
    return k;
}

// g = dy d and xh of one element
template <class T>
__device__ __forceinline__ void inb_terms(T xe, T de, const InbPlane& k, double& g, double& xh)
{
    const double xd = (double)to_f32(xe);
    const float v = (float)(xd * k.a + k.b);
    g = (double)to_f32(de) * (v > 0.0f ? 1.0 : k.slope);
    xh = (xd - k.mean) * k.rs;
}

template <class T>
__device__ __forceinline__ void inb_add(InSums& s, T xe, T de, const InbPlane& k)
{
    double g, xh;
    inb_terms<T>(xe, de, k, g, xh);
    s.s1 += g;
    s.s2 += g * xh;
}

// this lane's share of {sum g, sum g xh} over [0, m): the walk of in_accumulate along x's address; dy by vectors where
// it shares x's alignment.  A lane meets its elements in the same order either way.
template <class T>
__device__ __forceinline__ InSums inb_accumulate(const T* __restrict__ xp, const T* __restrict__ dp, unsigned m,
                                                 const InbPlane& k)
{
    typedef typename InVec<T>::type vt;
    constexpr unsigned VW = InVec<T>::N;
    InSums s{0.0, 0.0};
    const unsigned t = threadIdx.x;
    const unsigned head = in_head(xp, m), nv = (m - head) / VW, done = head + nv * VW;
    if (t < head) inb_add<T>(s, xp[t], dp[t], k);
    const vt* xv = reinterpret_cast<const vt*>(xp + head);
    const T* di = dp + head;
    const bool dvec = (reinterpret_cast<size_t>(di) & 15u) == 0;
    unsigned v = t;
    if (dvec) {
        const vt* dv = reinterpret_cast<const vt*>(di);
        for (; v + (kInUnroll - 1) * kInThreads < nv; v += kInUnroll * kInThreads) {
            vt e[kInUnroll], d[kInUnroll];
#pragma unroll
            for (int u = 0; u < kInUnroll; ++u) {
                e[u] = xv[v + u * kInThreads];
                d[u] = dv[v + u * kInThreads];
            }
#pragma unroll
            for (int u = 0; u < kInUnroll; ++u)
#pragma unroll
                for (unsigned j = 0; j < VW; ++j) inb_add<T>(s, e[u][j], d[u][j], k);
        }
    }
    for (; v < nv; v += kInThreads) {
        const vt e = xv[v];
        const vt d = in_load<T>(di, v, dvec);
#pragma unroll
        for (unsigned j = 0; j < VW; ++j) inb_add<T>(s, e[j], d[j], k);
    }
    if (t < m - done) inb_add<T>(s, xp[done + t], dp[done + t], k);
    return s;
}

template <class T>
__device__ __forceinline__ T inb_dx1(T xe, T de, const InbPlane& k, double m1, double m2)
{
    double g, xh;
    inb_terms<T>(xe, de, k, g, xh);
    return from_f32<T>((float)(k.A * ((g - m1) - xh * m2)));
}

// dx[i] over [0, m), m1 = t1 / n and m2 = t2 / n: vector stores follow dx's address; x and dy are each loaded by vectors
// where they share it, decided for each alone
template <class T>
__device__ __forceinline__ void inb_map(const T* __restrict__ xp, const T* __restrict__ dp, T* __restrict__ op, unsigned m,
                                        const InbPlane& k, double m1, double m2)
{
    typedef typename InVec<T>::type vt;
    constexpr unsigned VW = InVec<T>::N;
    const unsigned t = threadIdx.x;
    const unsigned head = in_head(op, m), nv = (m - head) / VW, done = head + nv * VW;
    if (t < head) op[t] = inb_dx1<T>(xp[t], dp[t], k, m1, m2);
    const T* xi = xp + head;
    const T* di = dp + head;
    vt* ov = reinterpret_cast<vt*>(op + head);
    const bool xvec = (reinterpret_cast<size_t>(xi) & 15u) == 0, dvec = (reinterpret_cast<size_t>(di) & 15u) == 0;
    unsigned v = t;
    if (xvec && dvec) {
        const vt* xv = reinterpret_cast<const vt*>(xi);
        const vt* dv = reinterpret_cast<const vt*>(di);
        for (; v + (kInUnroll - 1) * kInThreads < nv; v += kInUnroll * kInThreads) {
            vt e[kInUnroll], d[kInUnroll];
#pragma unroll
            for (int u = 0; u < kInUnroll; ++u) {
                e[u] = xv[v + u * kInThreads];
                d[u] = dv[v + u * kInThreads];
            }
#pragma unroll
            for (int u = 0; u < kInUnroll; ++u) {
#pragma unroll
                for (unsigned j = 0; j < VW; ++j) e[u][j] = inb_dx1<T>(e[u][j], d[u][j], k, m1, m2);
                ov[v + u * kInThreads] = e[u];
            }
        }
    }
    for (; v < nv; v += kInThreads) {
        vt e = in_load<T>(xi, v, xvec);
        const vt d = in_load<T>(di, v, dvec);
#pragma unroll
        for (unsigned j = 0; j < VW; ++j) e[j] = inb_dx1<T>(e[j], d[j], k, m1, m2);
        ov[v] = e;
    }
    if (t < m - done) op[done + t] = inb_dx1<T>(xp[done + t], dp[done + t], k, m1, m2);
}

// grid: min(planes, kInMaxPlaneGrid) workgroups; a workgroup takes planes blockIdx.x, + gridDim.x, ...
template <class T>
__global__ __launch_bounds__(kInThreads) void rroi_inorm_bwd_plane_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, const double2* __restrict__ stats, const T* __restrict__ gamma,
    const T* __restrict__ beta, T* __restrict__ dx, double2* __restrict__ plane_sums, unsigned C, unsigned n, unsigned planes,
    double eps, float slope)
{
    __shared__ double lds[2 * kInThreads / 64];
    for (unsigned plane = blockIdx.x; plane < planes; plane += gridDim.x) {
        const size_t at = (size_t)plane * n;
        const InbPlane k = inb_plane<T>(stats[plane], gamma, beta, plane % C, eps, slope);
        const InSums s = in_block_sum(inb_accumulate<T>(x + at, dy + at, n, k), lds);
        if (plane_sums && threadIdx.x == 0) plane_sums[plane] = double2{s.s1, s.s2};
        if (dx) inb_map<T>(x + at, dy + at, dx + at, n, k, s.s1 / (double)n, s.s2 / (double)n);
        __syncthreads();               // the next plane's sums reuse lds
    }
}

// grid: planes * nseg workgroups, segment fastest, as rroi_inorm_stats_kernel
template <class T>
__global__ __launch_bounds__(kInThreads) void rroi_inorm_bwd_partial_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, const double2* __restrict__ stats, const T* __restrict__ gamma,
    const T* __restrict__ beta, double2* __restrict__ pairs, unsigned C, unsigned n, unsigned seg, unsigned nseg, double eps,
    float slope)
{
    __shared__ double lds[2 * kInThreads / 64];
    const unsigned plane = blockIdx.x / nseg, lo = (blockIdx.x % nseg) * seg;
    const size_t at = (size_t)plane * n + lo;
    const InbPlane k = inb_plane<T>(stats[plane], gamma, beta, plane % C, eps, slope);
    const InSums s = in_block_sum(inb_accumulate<T>(x + at, dy + at, min(seg, n - lo), k), lds);
    if (threadIdx.x == 0) pairs[blockIdx.x] = double2{s.s1, s.s2};   // one 16-byte vector store
}

template <class T>
__global__ __launch_bounds__(kInThreads) void rroi_inorm_bwd_apply_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, const double2* __restrict__ stats, const T* __restrict__ gamma,
    const T* __restrict__ beta, T* __restrict__ dx, const double2* __restrict__ pairs, double2* __restrict__ plane_sums,
    unsigned C, unsigned n, unsigned seg, unsigned nseg, double eps, float slope)
{
    __shared__ double lds[2 * kInThreads / 64];
    const unsigned plane = blockIdx.x / nseg, lo = (blockIdx.x % nseg) * seg;
    InSums p{0.0, 0.0};                // nseg <= kInThreads: lane t holds pair t, the others +0.0
    if (threadIdx.x < nseg) {
        const double2 v = pairs[(size_t)plane * nseg + threadIdx.x];
        p = InSums{v.x, v.y};
    }
    const InSums s = in_block_sum(p, lds);
    if (plane_sums && lo == 0 && threadIdx.x == 0) plane_sums[plane] = double2{s.s1, s.s2};
    if (!dx) return;
    const size_t at = (size_t)plane * n + lo;
    const InbPlane k = inb_plane<T>(stats[plane], gamma, beta, plane % C, eps, slope);
    inb_map<T>(x + at, dy + at, dx + at, min(seg, n - lo), k, s.s1 / (double)n, s.s2 / (double)n);
}

// grid: ceil(C / kInThreads) workgroups, one lane per channel
template <class T>
__global__ __launch_bounds__(kInThreads) void rroi_inorm_bwd_param_kernel(const double2* __restrict__ plane_sums,
                                                                          T* __restrict__ dgamma, T* __restrict__ dbeta,
                                                                          unsigned N, unsigned C)
{
    const unsigned c = blockIdx.x * kInThreads + threadIdx.x;
    if (c >= C) return;
    double t1 = 0.0, t2 = 0.0;
    for (unsigned i = 0; i < N; ++i) {
        const double2 p = plane_sums[(size_t)i * C + c];
        t1 += p.x;
        t2 += p.y;
    }
    ctc_narrow(t1, dbeta + c);
    ctc_narrow(t2, dgamma + c);
}
