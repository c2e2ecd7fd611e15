// rroi_instancenorm_kernels.h -- InstanceNorm2d with the activation that follows it, DESIGN 5.11
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_device_common.h); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// The InstanceNorms of the network (tools/models.py of the reference: `nn.InstanceNorm2d(c, eps=1e-5, affine=...)`), per
// (n, c) plane of n = H * W elements, with the arithmetic of header section 6:
//     K = (double)x[0];  s1 = sum (x - K), s2 = sum (x - K)^2  in double
//     m = s1 / n, mean = K + m, var = s2 / n - m * m (negative -> 0), a = gamma / sqrt(var + eps), b = beta - mean * a
//     v = (float)((double)x * a + b);  v = v < 0 ? v * slope : v;  y = (T)v
// The shift by K keeps the single-pass variance from cancelling where |mean| >> std (DESIGN 5.11 has the counts).
//
// Both passes stream a run of elements the same way (in_accumulate, in_map): up to 16 / sizeof(T) - 1 single elements up
// to the first 16-byte boundary, 16-byte vectors strided over the workgroup's 256 lanes, single elements behind the last
// whole vector.  A plane starts (n * C + c) * H * W elements into the tensor, so with an odd H * W, a 16-bit type or a view
// the boundary moves from plane to plane; pass 1 follows x's address and pass 2 follows y's (vector stores), loading x
// by vectors where it shares y's alignment -- two whole allocations always do -- and by elements otherwise.
//
// Sums: a lane adds its elements in address order, the 64 lanes of a wave are combined by a butterfly (every lane
// computes the same bits: the two operands of each step are swapped between partners and IEEE addition commutes), the
// four waves through LDS in wave order.  No atomics anywhere: the same arguments give the same bits.
//
//   rroi_inorm_plane_kernel   one workgroup per plane: pass 1, coefficients, pass 2 (the plane is still in L2)
//   rroi_inorm_stats_kernel   split form, launch 1: workgroup (plane, segment) leaves {s1, s2} of its segment in the workspace
//   rroi_inorm_apply_kernel   split form, launch 2: lane t takes pair t of its plane, the same block sum combines them (the
//                             same bits in every workgroup of the plane), then the workgroup maps its segment
// The launch boundary is the only synchronisation between workgroups.
// ------------------------------------------------------------------------------------
constexpr int kInThreads = 256;
constexpr int kInUnroll = 4;      // vector loads in flight per lane
constexpr unsigned kInMaxPlaneGrid = 1u << 20;   // plane form: more planes than this are walked by a grid of this size

template <class T>
struct InVec {                    // 16 bytes of T
    static constexpr unsigned N = 16 / sizeof(T);
    typedef T type __attribute__((ext_vector_type(16 / sizeof(T))));
};

struct InSums {
    double s1, s2;
};

// elements of p[0 .. m) in front of the first 16-byte boundary (all of them where there is none)
template <class T>
__device__ __forceinline__ unsigned in_head(const T* p, unsigned m)
{
    const unsigned h = ((16u - (unsigned)(reinterpret_cast<size_t>(p) & 15u)) & 15u) / (unsigned)sizeof(T);
    return h < m ? h : m;
}

template <class T>
__device__ __forceinline__ void in_add(InSums& s, T e, double K)
{
    const double d = (double)to_f32(e) - K;
    s.s1 += d;
    s.s2 += d * d;
}

// this lane's share of sum (p[i] - K), sum (p[i] - K)^2 over p[0 .. m)
template <class T>
__device__ __forceinline__ InSums in_accumulate(const T* __restrict__ p, unsigned m, double K)
{
    typedef typename InVec<T>::type vt;
    constexpr unsigned VW = InVec<T>::N;
    InSums s{0.0, 0.0};
    const unsigned t = threadIdx.x;
    const unsigned head = in_head(p, m), nv = (m - head) / VW, done = head + nv * VW;
    if (t < head) in_add(s, p[t], K);
    const vt* pv = reinterpret_cast<const vt*>(p + head);
    unsigned v = t;
    for (; v + (kInUnroll - 1) * kInThreads < nv; v += kInUnroll * kInThreads) {
        vt r[kInUnroll];
#pragma unroll
        for (int k = 0; k < kInUnroll; ++k) r[k] = pv[v + k * kInThreads];
#pragma unroll
        for (int k = 0; k < kInUnroll; ++k)
#pragma unroll
            for (unsigned j = 0; j < VW; ++j) in_add<T>(s, r[k][j], K);
    }
    for (; v < nv; v += kInThreads) {
        const vt r = pv[v];
#pragma unroll
        for (unsigned j = 0; j < VW; ++j) in_add<T>(s, r[j], K);
    }
    if (t < m - done) in_add(s, p[done + t], K);
    return s;
}

// the workgroup's sum, the same bits in every lane; lds: 8 doubles
__device__ __forceinline__ InSums in_block_sum(InSums s, double* lds)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        s.s1 += __shfl_xor(s.s1, off, 64);
        s.s2 += __shfl_xor(s.s2, off, 64);
    }
    const unsigned wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        lds[2 * wave] = s.s1;
        lds[2 * wave + 1] = s.s2;
    }
    __syncthreads();
    InSums r{lds[0], lds[1]};
#pragma unroll
    for (int w = 1; w < kInThreads / 64; ++w) {
        r.s1 += lds[2 * w];
        r.s2 += lds[2 * w + 1];
    }
    return r;
}

// the plane's mean and (clamped) variance from its shifted sums
__device__ __forceinline__ void in_moments(InSums s, double K, unsigned n, double& mean, double& var)
{
    const double m = s.s1 / (double)n;
    mean = K + m;
    var = s.s2 / (double)n - m * m;
    if (var < 0.0) var = 0.0;          // a comparison, not fmax: a NaN stays a NaN and takes the plane with it
}

// a and b of a plane of channel c from its mean and variance (the backward forms them again, from the saved pair)
template <class T>
__device__ __forceinline__ void in_affine(double mean, double var, const T* gamma, const T* beta, unsigned c, double eps,
                                          double& a, double& b)
{
    const double g = gamma ? (double)to_f32(gamma[c]) : 1.0, bt = gamma ? (double)to_f32(beta[c]) : 0.0;
    a = g / sqrt(var + eps);
    b = bt - mean * a;
}

template <class T>
__device__ __forceinline__ void in_coefficients(InSums s, double K, unsigned n, const T* gamma, const T* beta, unsigned c,
                                                double eps, double& a, double& b)
{
    double mean, var;
    in_moments(s, K, n, mean, var);
    in_affine<T>(mean, var, gamma, beta, c, eps, a, b);
}

template <class T>
__device__ __forceinline__ T in_map1(T e, double a, double b, float slope)
{
    float v = (float)((double)to_f32(e) * a + b);
    v = v < 0.0f ? v * slope : v;
    return from_f32<T>(v);
}

// y[i] = map(x[i]) over [0, m): vector stores follow y's address
template <class T>
__device__ __forceinline__ void in_map(const T* __restrict__ xp, T* __restrict__ yp, unsigned m, double a, double b, float slope)
{
    typedef typename InVec<T>::type vt;
    constexpr unsigned VW = InVec<T>::N;
    const unsigned t = threadIdx.x;
    const unsigned head = in_head(yp, m), nv = (m - head) / VW, done = head + nv * VW;
    if (t < head) yp[t] = in_map1(xp[t], a, b, slope);
    const T* xi = xp + head;
    vt* yv = reinterpret_cast<vt*>(yp + head);
    if ((reinterpret_cast<size_t>(xi) & 15u) == 0) {
        const vt* xv = reinterpret_cast<const vt*>(xi);
        unsigned v = t;
        for (; v + (kInUnroll - 1) * kInThreads < nv; v += kInUnroll * kInThreads) {
            vt r[kInUnroll];
#pragma unroll
            for (int k = 0; k < kInUnroll; ++k) r[k] = xv[v + k * kInThreads];
#pragma unroll
            for (int k = 0; k < kInUnroll; ++k) {
#pragma unroll
                for (unsigned j = 0; j < VW; ++j) r[k][j] = in_map1<T>(r[k][j], a, b, slope);
                yv[v + k * kInThreads] = r[k];
            }
        }
        for (; v < nv; v += kInThreads) {
            vt r = xv[v];
#pragma unroll
            for (unsigned j = 0; j < VW; ++j) r[j] = in_map1<T>(r[j], a, b, slope);
            yv[v] = r;
        }
    } else {
        for (unsigned v = t; v < nv; v += kInThreads) {
            vt r;
#pragma unroll
            for (unsigned j = 0; j < VW; ++j) r[j] = in_map1<T>(xi[(size_t)v * VW + j], a, b, slope);
            yv[v] = r;
        }
    }
    if (t < m - done) yp[done + t] = in_map1(xp[done + t], a, b, slope);
}

// grid: min(planes, kInMaxPlaneGrid) workgroups; a workgroup takes planes blockIdx.x, + gridDim.x, ...
template <class T>
__global__ __launch_bounds__(kInThreads) void rroi_inorm_plane_kernel(
    const T* __restrict__ x, const T* __restrict__ gamma, const T* __restrict__ beta, T* __restrict__ y, unsigned C, unsigned n,
    unsigned planes, double eps, float slope)
{
    __shared__ double lds[2 * kInThreads / 64];
    for (unsigned plane = blockIdx.x; plane < planes; plane += gridDim.x) {
        const T* xp = x + (size_t)plane * n;
        const double K = (double)to_f32(xp[0]);
        const InSums s = in_block_sum(in_accumulate<T>(xp, n, K), lds);
        double a, b;
        in_coefficients<T>(s, K, n, gamma, beta, plane % C, eps, a, b);
        in_map<T>(xp, y + (size_t)plane * n, n, a, b, slope);
        __syncthreads();               // the next plane's sums reuse lds
    }
}

// grid: planes * nseg workgroups, segment fastest.  Segment s of a plane is its elements [s * seg, min((s + 1) * seg, n)).
template <class T>
__global__ __launch_bounds__(kInThreads) void rroi_inorm_stats_kernel(const T* __restrict__ x, double2* __restrict__ pairs,
                                                                      unsigned n, unsigned seg, unsigned nseg)
{
    __shared__ double lds[2 * kInThreads / 64];
    const unsigned plane = blockIdx.x / nseg, lo = (blockIdx.x % nseg) * seg;
    const T* xp = x + (size_t)plane * n;
    const double K = (double)to_f32(xp[0]);
    const InSums s = in_block_sum(in_accumulate<T>(xp + lo, min(seg, n - lo), K), lds);
    if (threadIdx.x == 0) pairs[blockIdx.x] = double2{s.s1, s.s2};   // one 16-byte vector store
}

template <class T>
__global__ __launch_bounds__(kInThreads) void rroi_inorm_apply_kernel(
    const T* __restrict__ x, const T* __restrict__ gamma, const T* __restrict__ beta, T* __restrict__ y,
    const double2* __restrict__ pairs, unsigned C, unsigned n, unsigned seg, unsigned nseg, double eps, float slope)
{
    __shared__ double lds[2 * kInThreads / 64];
    const unsigned plane = blockIdx.x / nseg, lo = (blockIdx.x % nseg) * seg;
    const T* xp = x + (size_t)plane * n;
    const double K = (double)to_f32(xp[0]);
    InSums p{0.0, 0.0};                // nseg <= kInThreads (plan_instancenorm): lane t holds pair t, the others +0.0
    if (threadIdx.x < nseg) {
        const double2 v = pairs[(size_t)plane * nseg + threadIdx.x];
        p = InSums{v.x, v.y};
    }
    const InSums s = in_block_sum(p, lds);
    double a, b;
    in_coefficients<T>(s, K, n, gamma, beta, plane % C, eps, a, b);
    in_map<T>(xp + lo, y + (size_t)plane * n + lo, min(seg, n - lo), a, b, slope);
}

// ------------------------------------------------------------------------------------
// Fused epilogues (header section 6b).  Pass 1 and the pair combination are the ones above, unchanged -- the
// statistics depend on x alone -- and only the map differs:
//   kInResidual   y = act((float)(x a + b) + (float)r), the sum in fp32 and rounded once: the tail of a residual block
//   kInMirror     a source plane (n, j) of x (N, C, H, W) gives planes (n, j) and (n, C + j) of y (N, 2C, H, W), the
//                 InstanceNorm of cat(x, -x) without the concatenation: with K' = -K the negated half has s1' = -s1 and
//                 s2' = s2 exactly, so it needs no sums of its own, and (-x) a' + b' = x (-a') + b' exactly, so its map
//                 is the plain one with the negated coefficient.  The grid runs over SOURCE planes.
//   rroi_inorm_fused_plane_kernel   plane form
//   rroi_inorm_fused_apply_kernel   split form, launch 2 (launch 1 is rroi_inorm_stats_kernel as it stands)
// ------------------------------------------------------------------------------------
constexpr int kInResidual = 0;
constexpr int kInMirror = 1;

// vector v of p[0 ..): one 16-byte load where `vec` (p is on a 16-byte boundary), element loads otherwise
template <class T>
__device__ __forceinline__ typename InVec<T>::type in_load(const T* __restrict__ p, unsigned v, bool vec)
{
    typedef typename InVec<T>::type vt;
    constexpr unsigned VW = InVec<T>::N;
    if (vec) return reinterpret_cast<const vt*>(p)[v];
    vt r;
#pragma unroll
    for (unsigned j = 0; j < VW; ++j) r[j] = p[(size_t)v * VW + j];
    return r;
}

template <class T>
__device__ __forceinline__ T in_map_res1(T e, T res, double a, double b, float slope)
{
    const float v = (float)((double)to_f32(e) * a + b);
    float u = v + to_f32(res);
    u = u < 0.0f ? u * slope : u;
    return from_f32<T>(u);
}

// y[i] = act(map(x[i]) + r[i]) over [0, m): vector stores follow y's address; x and r are each loaded by vectors where
// they share y's alignment, decided for each alone
template <class T>
__device__ __forceinline__ void in_map_residual(const T* __restrict__ xp, const T* __restrict__ rp, T* __restrict__ yp,
                                                unsigned m, double a, double b, float slope)
{
    typedef typename InVec<T>::type vt;
    constexpr unsigned VW = InVec<T>::N;
    const unsigned t = threadIdx.x;
    const unsigned head = in_head(yp, m), nv = (m - head) / VW, done = head + nv * VW;
    if (t < head) yp[t] = in_map_res1(xp[t], rp[t], a, b, slope);
    const T* xi = xp + head;
    const T* ri = rp + head;
    vt* yv = reinterpret_cast<vt*>(yp + head);
    const bool xvec = (reinterpret_cast<size_t>(xi) & 15u) == 0, rvec = (reinterpret_cast<size_t>(ri) & 15u) == 0;
    if (xvec && rvec) {
        const vt* xv = reinterpret_cast<const vt*>(xi);
        const vt* rv = reinterpret_cast<const vt*>(ri);
        unsigned v = t;
        for (; v + (kInUnroll - 1) * kInThreads < nv; v += kInUnroll * kInThreads) {
            vt e[kInUnroll], r[kInUnroll];
#pragma unroll
            for (int k = 0; k < kInUnroll; ++k) {
                e[k] = xv[v + k * kInThreads];
                r[k] = rv[v + k * kInThreads];
            }
#pragma unroll
            for (int k = 0; k < kInUnroll; ++k) {
#pragma unroll
                for (unsigned j = 0; j < VW; ++j) e[k][j] = in_map_res1<T>(e[k][j], r[k][j], a, b, slope);
                yv[v + k * kInThreads] = e[k];
            }
        }
        for (; v < nv; v += kInThreads) {
            vt e = xv[v];
            const vt r = rv[v];
#pragma unroll
            for (unsigned j = 0; j < VW; ++j) e[j] = in_map_res1<T>(e[j], r[j], a, b, slope);
            yv[v] = e;
        }
    } else {
        for (unsigned v = t; v < nv; v += kInThreads) {
            vt e = in_load<T>(xi, v, xvec);
            const vt r = in_load<T>(ri, v, rvec);
#pragma unroll
            for (unsigned j = 0; j < VW; ++j) e[j] = in_map_res1<T>(e[j], r[j], a, b, slope);
            yv[v] = e;
        }
    }
    if (t < m - done) yp[done + t] = in_map_res1(xp[done + t], rp[done + t], a, b, slope);
}

// y0[i] = map(x[i]; a0, b0), y1[i] = map(x[i]; a1, b1) over [0, m).  Where y0 and y1 share their alignment, one walk
// that follows it: every x vector is loaded once and stored twice.  Otherwise two plain maps, the second read from L2.
template <class T>
__device__ __forceinline__ void in_map_mirror(const T* __restrict__ xp, T* __restrict__ y0, T* __restrict__ y1, unsigned m,
                                              double a0, double b0, double a1, double b1, float slope)
{
    typedef typename InVec<T>::type vt;
    constexpr unsigned VW = InVec<T>::N;
    if (((reinterpret_cast<size_t>(y0) ^ reinterpret_cast<size_t>(y1)) & 15u) != 0) {
        in_map<T>(xp, y0, m, a0, b0, slope);
        in_map<T>(xp, y1, m, a1, b1, slope);
        return;
    }
    const unsigned t = threadIdx.x;
    const unsigned head = in_head(y0, m), nv = (m - head) / VW, done = head + nv * VW;
    if (t < head) {
        const T e = xp[t];
        y0[t] = in_map1(e, a0, b0, slope);
        y1[t] = in_map1(e, a1, b1, slope);
    }
    const T* xi = xp + head;
    vt* yv0 = reinterpret_cast<vt*>(y0 + head);
    vt* yv1 = reinterpret_cast<vt*>(y1 + head);
    const bool xvec = (reinterpret_cast<size_t>(xi) & 15u) == 0;
    unsigned v = t;
    if (xvec) {
        const vt* xv = reinterpret_cast<const vt*>(xi);
        for (; v + (kInUnroll - 1) * kInThreads < nv; v += kInUnroll * kInThreads) {
            vt e[kInUnroll];
#pragma unroll
            for (int k = 0; k < kInUnroll; ++k) e[k] = xv[v + k * kInThreads];
#pragma unroll
            for (int k = 0; k < kInUnroll; ++k) {
                vt o0, o1;
#pragma unroll
                for (unsigned j = 0; j < VW; ++j) {
                    o0[j] = in_map1<T>(e[k][j], a0, b0, slope);
                    o1[j] = in_map1<T>(e[k][j], a1, b1, slope);
                }
                yv0[v + k * kInThreads] = o0;
                yv1[v + k * kInThreads] = o1;
            }
        }
    }
    for (; v < nv; v += kInThreads) {
        const vt e = in_load<T>(xi, v, xvec);
        vt o0, o1;
#pragma unroll
        for (unsigned j = 0; j < VW; ++j) {
            o0[j] = in_map1<T>(e[j], a0, b0, slope);
            o1[j] = in_map1<T>(e[j], a1, b1, slope);
        }
        yv0[v] = o0;
        yv1[v] = o1;
    }
    if (t < m - done) {
        const T e = xp[done + t];
        y0[done + t] = in_map1(e, a0, b0, slope);
        y1[done + t] = in_map1(e, a1, b1, slope);
    }
}

// The coefficients of source plane `plane` from its sums, then the map of its elements [lo, lo + m).  `C` is x's channel
// count; under kInMirror gamma and beta hold 2C values and y has 2C channels.
template <class T, int MODE>
__device__ __forceinline__ void in_fused_finish(InSums s, double K, const T* __restrict__ xp, const T* __restrict__ gamma,
                                                const T* __restrict__ beta, const T* __restrict__ r, T* __restrict__ y,
                                                unsigned C, unsigned n, unsigned plane, unsigned lo, unsigned m, double eps,
                                                float slope)
{
    const unsigned c = plane % C;
    double a, b;
    in_coefficients<T>(s, K, n, gamma, beta, c, eps, a, b);
    if constexpr (MODE == kInResidual) {
        const size_t at = (size_t)plane * n + lo;
        in_map_residual<T>(xp + lo, r + at, y + at, m, a, b, slope);
    } else {
        double a1, b1;                 // the plane of -x: K' = -K, s1' = -s1, s2' = s2, and (-x) a1 + b1 = x (-a1) + b1
        in_coefficients<T>(InSums{-s.s1, s.s2}, -K, n, gamma, beta, C + c, eps, a1, b1);
        T* y0 = y + ((size_t)(plane / C) * 2 * C + c) * n + lo;
        in_map_mirror<T>(xp + lo, y0, y0 + (size_t)C * n, m, a, b, -a1, b1, slope);
    }
}

// grid: as rroi_inorm_plane_kernel, over the planes of x
template <class T, int MODE>
__global__ __launch_bounds__(kInThreads) void rroi_inorm_fused_plane_kernel(
    const T* __restrict__ x, const T* __restrict__ gamma, const T* __restrict__ beta, const T* __restrict__ r,
    T* __restrict__ y, unsigned C, unsigned n, unsigned planes, double eps, float slope)
{
    __shared__ double lds[2 * kInThreads / 64];
    for (unsigned plane = blockIdx.x; plane < planes; plane += gridDim.x) {
        const T* xp = x + (size_t)plane * n;
        const double K = (double)to_f32(xp[0]);
        const InSums s = in_block_sum(in_accumulate<T>(xp, n, K), lds);
        in_fused_finish<T, MODE>(s, K, xp, gamma, beta, r, y, C, n, plane, 0, n, eps, slope);
        __syncthreads();               // the next plane's sums reuse lds
    }
}

// grid: as rroi_inorm_apply_kernel, over the planes of x; `pairs` is what rroi_inorm_stats_kernel left
template <class T, int MODE>
__global__ __launch_bounds__(kInThreads) void rroi_inorm_fused_apply_kernel(
    const T* __restrict__ x, const T* __restrict__ gamma, const T* __restrict__ beta, const T* __restrict__ r,
    T* __restrict__ y, const double2* __restrict__ pairs, unsigned C, unsigned n, unsigned seg, unsigned nseg, double eps,
    float slope)
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
    in_fused_finish<T, MODE>(s, K, xp, gamma, beta, r, y, C, n, plane, lo, min(seg, n - lo), eps, slope);
}
