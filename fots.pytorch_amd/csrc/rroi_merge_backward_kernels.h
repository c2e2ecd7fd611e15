// rroi_merge_backward_kernels.h -- the backward of the gated merge and the stand-alone bilinear resize with its backward,
// DESIGN 5.26.  Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_merge_kernels.h, whose mg_axis / mg_blend / MgSource it uses as they are, rroi_heads_kernels.h (pw_load / pw_store)
// and rroi_ctc_loss_kernels.h, whose ctc_narrow rounds a double once to T); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// R is the resize of header section 8 (bilinear, align_corners = true, in double), y = R_a a + f * (R_g gate) the forward.
//   rroi_resize_kernel            y = R x, the merge kernel's scheme and arithmetic without f and the gate: z = mg_blend,
//       out = (T)(float)z.  A source of the output's size is copied element by element.
//   rroi_resize_backward_kernel   dx = R^T dy as a GATHER: a lane owns one dx element (i, j) of a tile of 256 consecutive
//       pixels of one image and walks a block of channels.  Output row Y reaches source row i where i0(Y) == i (weight
//       1 - l1) or i0(Y) + step(Y) == i (weight l1); i0 is monotone in Y, so these rows are the contiguous range
//       [first Y with i0 >= i - 1, first Y with i0 > i) (rs_footprint: an estimate from i / s, corrected by evaluating
//       i0 itself).  Columns likewise.  The sum, in double, every operation rounded separately:
//           acc = +0.0;  for Y ascending:  row = +0.0;  for X ascending:  row = row + wx * dy[Y, X]  (where step == 0 both
//           weights meet in one element: the first tap's term, then the second's);  acc = acc + wy * row  (likewise)
//       then ONE rounding to T (ctc_narrow).  No tap of the range is skipped -- a zero weight against an infinity is NaN, as
//       in the forward -- and an element no output pixel reaches is +0.0.  The column weights of up to kRsTaps taps are
//       computed once per lane and kept in registers (a 2x resize has at most five) and a row's kRsTaps loads are issued
//       together, columns past the range clamped into the row; a longer range recomputes the weights per row.
//   rroi_merge_backward_kernel    the forward's tile / channel-block scheme, V = 4: G recomputed per pixel as the forward
//       does; df = (T)(float)((double)dy * G); S = S + (double)dy * (double)f over the block's channels ascending (the
//       product of two widened values is exact in double), the lane's S stored to workspace[n][block][pixel].
//   rroi_merge_blocksum_kernel    the blocks' maps summed per pixel, ascending, in place into block 0 (launched where K > 1):
//       a tap of the gather then costs one load, not K.
//   rroi_merge_dgate_kernel       dgate = R_g^T (that sum) by the same gather; where the gate has f's size the gather is the
//       identity.
// No atomic, nothing crosses a lane: the bits depend on the shape alone.
// Longest chain of additions: kMgbMaxBlock (S) / kMgbMaxBlocks (blocks) / 2 * kRsMaxFootprint (a row or a column of the
// gather): the host refuses what would exceed 8192.
// ------------------------------------------------------------------------------------
constexpr int kRsTaps = 6;
constexpr int kRsMaxFootprint = 4096;   // contributing rows (columns) of one source row (column): 2 terms each
constexpr int kMgbMaxBlock = 2048;      // channels per block of the merge backward
constexpr int kMgbMaxBlocks = 4096;

// mg_axis's first tap for both sides of the launch: the same multiply, truncation and clamp
__host__ __device__ inline int rs_i0(double s, int dst, int in)
{
    const double src = s * (double)dst;
    const int i0 = (int)src;
    return i0 < in - 1 ? i0 : in - 1;
}

// the first dst in [0, out] with i0(dst) >= t (out where there is none)
__host__ __device__ inline int rs_first(double s, int in, int out, int t)
{
    if (t <= 0) return 0;
    if (t > in - 1 || s == 0.0) return out;        // i0 never exceeds in - 1; scale 0: i0 == 0 everywhere
    const double e = (double)t / s;
    int d = e >= (double)out ? out : (int)e;
    while (d > 0 && rs_i0(s, d - 1, in) >= t) --d;
    while (d < out && rs_i0(s, d, in) < t) ++d;
    return d;
}

// the output indices whose taps reach source index i: [lo, hi)
__host__ __device__ inline void rs_footprint(double s, int in, int out, int i, int* lo, int* hi)
{
    *lo = rs_first(s, in, out, i - 1);
    *hi = rs_first(s, in, out, i + 1);
}

// what output index `ax` gives source index i: the first term's weight, and whether a second (wb) follows
__device__ __forceinline__ bool rs_weights(const MgAxis& ax, int i, double* wa, double* wb)
{
    const bool first = ax.i0 == i, second = ax.i0 + ax.step == i;
    *wa = first ? 1.0 - ax.l1 : ax.l1;
    *wb = ax.l1;
    return first && second;
}

struct RsCols {
    int lo, n;
    unsigned dup;      // bit t: tap t adds a second term
    double wa[kRsTaps], wb[kRsTaps];
};

// the gather of one element (i, j); tap(Y, X) is the gathered map's value as a double
template <class Tap>
__device__ __forceinline__ double rs_gather(const Tap& tap, const RsCols& cx, int ylo, int yhi, int i, int j, double sy,
                                            double sx, int h, int w, int W)
{
    double acc = 0.0;
    for (int Y = ylo; Y < yhi; ++Y) {
        double row = 0.0;
        if (cx.n <= kRsTaps) {
            // all kRsTaps loads are issued before the first is used: a column past the range is clamped into the row (it is
            // loaded and not used), so no load waits for a branch
            double v[kRsTaps];
#pragma unroll
            for (int t = 0; t < kRsTaps; ++t) v[t] = tap(Y, min(cx.lo + t, W - 1));
#pragma unroll
            for (int t = 0; t < kRsTaps; ++t)
                if (t < cx.n) {
                    row = row + cx.wa[t] * v[t];
                    if (cx.dup >> t & 1u) row = row + cx.wb[t] * v[t];
                }
        } else {
            for (int X = cx.lo; X < cx.lo + cx.n; ++X) {
                double wa, wb;
                const bool dup = rs_weights(mg_axis(sx, (unsigned)X, w), j, &wa, &wb);
                const double v = tap(Y, X);
                row = row + wa * v;
                if (dup) row = row + wb * v;
            }
        }
        double wa, wb;
        const bool dup = rs_weights(mg_axis(sy, (unsigned)Y, h), i, &wa, &wb);
        acc = acc + wa * row;
        if (dup) acc = acc + wb * row;
    }
    return acc;
}

__device__ __forceinline__ RsCols rs_cols(double sx, int w, int W, int j)
{
    RsCols c;
    int hi;
    rs_footprint(sx, w, W, j, &c.lo, &hi);
    c.n = hi - c.lo;
    c.dup = 0;
#pragma unroll
    for (int t = 0; t < kRsTaps; ++t) {
        c.wa[t] = c.wb[t] = 0.0;
        if (t < c.n && c.n <= kRsTaps)
            if (rs_weights(mg_axis(sx, (unsigned)(c.lo + t), w), j, &c.wa[t], &c.wb[t])) c.dup |= 1u << t;
    }
    return c;
}

// ------------------------------------------------------------------------------------
// y = R x.  grid: N * K * tiles workgroups of 256 threads, as rroi_merge_kernel.  UP: x is (N, C, A.h, A.w) and is resized
// to (H, W); else it has y's shape.
// ------------------------------------------------------------------------------------
template <class T, int V, bool UP>
__global__ __launch_bounds__(kMgThreads) void rroi_resize_kernel(const T* __restrict__ x, T* __restrict__ y, unsigned C,
                                                                 unsigned W, unsigned HW, unsigned tiles, unsigned K, unsigned cb,
                                                                 MgSource A)
{
    const unsigned n = blockIdx.x / (tiles * K), rest = blockIdx.x % (tiles * K);
    const unsigned grp = rest / tiles, tile = rest % tiles;
    const unsigned px = (tile * kMgThreads + threadIdx.x) * V;
    const int left = px < HW ? (int)min(HW - px, (unsigned)V) : 0;
    const unsigned c0 = grp * cb, c1 = min(c0 + cb, C);
    unsigned aoff[V], astep[V];
    double alx1[V], aly1[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        aoff[j] = astep[j] = 0;
        alx1[j] = aly1[j] = 0.0;
        if (UP && j < left) {
            const unsigned p = px + j, Y = p / W, X = p - Y * W;
            const MgAxis ay = mg_axis(A.sy, Y, A.h), ax = mg_axis(A.sx, X, A.w);
            aoff[j] = (unsigned)ay.i0 * (unsigned)A.w + (unsigned)ax.i0;
            astep[j] = (unsigned)(ay.step << 1 | ax.step);
            alx1[j] = ax.l1;
            aly1[j] = ay.l1;
        }
    }
    const size_t aplane = UP ? (size_t)A.h * A.w : (size_t)HW;
    const T* xp = x + (size_t)n * C * aplane + (UP ? 0 : px);
    T* yp = y + ((size_t)n * C * HW + px);
    for (unsigned c = c0; c < c1; ++c) {
        double z[V];
        if constexpr (UP) {
#pragma unroll
            for (int j = 0; j < V; ++j)
                z[j] = j < left ? mg_blend(xp + ((size_t)c * aplane + aoff[j]), (int)(astep[j] & 1u),
                                           (int)(astep[j] >> 1) * A.w, alx1[j], aly1[j])
                                : 0.0;
        } else {
            T r[V];
            pw_load<T, V>(xp + (size_t)c * HW, left, r);
#pragma unroll
            for (int j = 0; j < V; ++j) z[j] = (double)to_f32(r[j]);
        }
        pw_store<T, V>(yp + (size_t)c * HW, left, z);
    }
}

// ------------------------------------------------------------------------------------
// dx = R^T dy.  grid: N * K * tiles workgroups of 256 threads (tile fastest), tiles of 256 dx pixels.  dy is (N, C, H, W),
// dx (N, C, h, w); ident: the sizes agree and dx is dy's values.
// ------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(kMgThreads) void rroi_resize_backward_kernel(const T* __restrict__ dy, T* __restrict__ dx,
                                                                          unsigned C, int h, int w, int H, int W, unsigned hw,
                                                                          unsigned tiles, unsigned K, unsigned cb, double sy,
                                                                          double sx, int ident)
{
    const unsigned n = blockIdx.x / (tiles * K), rest = blockIdx.x % (tiles * K);
    const unsigned grp = rest / tiles, tile = rest % tiles;
    const unsigned p = tile * kMgThreads + threadIdx.x;
    if (p >= hw) return;
    const unsigned c0 = grp * cb, c1 = min(c0 + cb, C);
    T* op = dx + ((size_t)n * C * hw + p);
    if (ident) {
        const T* gp = dy + ((size_t)n * C * hw + p);
        for (unsigned c = c0; c < c1; ++c) op[(size_t)c * hw] = gp[(size_t)c * hw];
        return;
    }
    const int i = (int)(p / (unsigned)w), j = (int)(p - (unsigned)i * (unsigned)w);
    int ylo, yhi;
    rs_footprint(sy, h, H, i, &ylo, &yhi);
    const RsCols cx = rs_cols(sx, w, W, j);
    const size_t plane = (size_t)H * W;
    for (unsigned c = c0; c < c1; ++c) {
        const T* gp = dy + ((size_t)n * C + c) * plane;
        const auto tap = [&](int Y, int X) { return (double)to_f32(gp[(size_t)Y * W + X]); };
        ctc_narrow(rs_gather(tap, cx, ylo, yhi, i, j, sy, sx, h, w, W), op + (size_t)c * hw);
    }
}

// ------------------------------------------------------------------------------------
// The merge backward's first launch.  grid and decomposition as rroi_merge_kernel; DF: df is stored; DG: the per-pixel sums
// of dy * f go to ws[(n * K + block) * HW + pixel].  gate NULL: G = 1.
// ------------------------------------------------------------------------------------
template <class T, int V, bool DF, bool DG>
__global__ __launch_bounds__(kMgThreads) void rroi_merge_backward_kernel(
    const T* __restrict__ dy, const T* __restrict__ f, const T* __restrict__ gate, T* __restrict__ df, double* __restrict__ ws,
    unsigned C, unsigned W, unsigned HW, unsigned tiles, unsigned K, unsigned cb, MgSource Gs, int g_resize)
{
    const unsigned n = blockIdx.x / (tiles * K), rest = blockIdx.x % (tiles * K);
    const unsigned grp = rest / tiles, tile = rest % tiles;
    const unsigned px = (tile * kMgThreads + threadIdx.x) * V;
    const int left = px < HW ? (int)min(HW - px, (unsigned)V) : 0;
    const unsigned c0 = grp * cb, c1 = min(c0 + cb, C);

    double G[V], S[V];
    const T* gp = gate ? gate + (size_t)n * ((size_t)Gs.h * Gs.w) : nullptr;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        G[j] = 1.0;
        S[j] = 0.0;
        if (DF && gp && j < left) {
            const unsigned p = px + j, Y = p / W, X = p - Y * W;
            if (g_resize) {
                const MgAxis gy = mg_axis(Gs.sy, Y, Gs.h), gx = mg_axis(Gs.sx, X, Gs.w);
                G[j] = mg_blend(gp + ((size_t)gy.i0 * Gs.w + gx.i0), gx.step, gy.step * Gs.w, gx.l1, gy.l1);
            } else {
                G[j] = (double)to_f32(gp[p]);
            }
        }
    }
    const T* dyp = dy + ((size_t)n * C * HW + px);
    const T* fp = f + ((size_t)n * C * HW + px);
    T* dfp = DF ? df + ((size_t)n * C * HW + px) : nullptr;
    for (unsigned c = c0; c < c1; c += kMgChunk) {
        T dr[kMgChunk][V];
        T fr[kMgChunk][V];
#pragma unroll
        for (int k = 0; k < kMgChunk; ++k)
            if (c + k < c1) {
                pw_load<T, V>(dyp + (size_t)(c + k) * HW, left, dr[k]);
                if constexpr (DG) pw_load<T, V>(fp + (size_t)(c + k) * HW, left, fr[k]);
            }
#pragma unroll
        for (int k = 0; k < kMgChunk; ++k)
            if (c + k < c1) {
                double z[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const double d = (double)to_f32(dr[k][j]);
                    z[j] = d * G[j];
                    if constexpr (DG) {
                        const double t = d * (double)to_f32(fr[k][j]);
                        S[j] = S[j] + t;
                    }
                }
                if constexpr (DF) pw_store<T, V>(dfp + (size_t)(c + k) * HW, left, z);
            }
    }
    if constexpr (DG) {
        double* sp = ws + (((size_t)n * K + grp) * HW + px);
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (j < left) sp[j] = S[j];
    }
}

// ------------------------------------------------------------------------------------
// The blocks' maps summed in place, ascending, into block 0: ws[n][0][p] = ws[n][0][p] + ws[n][1][p] + ...  A thread owns
// one pixel of one image and touches nothing else.  grid: ceil(N * HW / 256) workgroups.  Launched where K > 1.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMgThreads) void rroi_merge_blocksum_kernel(double* __restrict__ ws, unsigned K, unsigned HW,
                                                                         unsigned total)
{
    const unsigned idx = blockIdx.x * kMgThreads + threadIdx.x;      // n * HW + p < 2^31
    if (idx >= total) return;
    double* q = ws + ((size_t)(idx / HW) * K * HW + idx % HW);
    double t = q[0];
    for (unsigned b = 1; b < K; ++b) t = t + q[(size_t)b * HW];
    q[0] = t;
}

// ------------------------------------------------------------------------------------
// dgate = R_g^T S, S the summed map in block 0 of each image's K blocks.  grid: N * tiles workgroups, tiles of 256 gate pixels.
// ------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(kMgThreads) void rroi_merge_dgate_kernel(const double* __restrict__ ws, T* __restrict__ dgate,
                                                                      unsigned K, int gh, int gw, int H, int W, unsigned ghw,
                                                                      unsigned HW, unsigned tiles, double sy, double sx, int ident)
{
    const unsigned n = blockIdx.x / tiles, p = (blockIdx.x % tiles) * kMgThreads + threadIdx.x;
    if (p >= ghw) return;
    const double* base = ws + (size_t)n * K * HW;
    const auto tap = [&](int Y, int X) { return base[(size_t)Y * W + X]; };
    T* out = dgate + ((size_t)n * ghw + p);
    if (ident) {
        ctc_narrow(base[p], out);       // (ghw == HW)
        return;
    }
    const int i = (int)(p / (unsigned)gw), j = (int)(p - (unsigned)i * (unsigned)gw);
    int ylo, yhi;
    rs_footprint(sy, gh, H, i, &ylo, &yhi);
    const RsCols cx = rs_cols(sx, gw, W, j);
    ctc_narrow(rs_gather(tap, cx, ylo, yhi, i, j, sy, sx, gh, gw, W), out);
}
