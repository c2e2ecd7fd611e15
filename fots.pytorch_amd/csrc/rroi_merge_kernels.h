// rroi_merge_kernels.h -- the gated merge of the network's feature merge in one launch, DESIGN 5.14
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_heads_kernels.h, whose pw_load / pw_store it uses); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// y = A + f * G over an NCHW map, with the arithmetic of header section 8: A is `a` resized to f's (H, W), G the
// one-channel `gate` resized likewise (no gate: y = A + f).  The resize is bilinear with align_corners = true, in double:
//     src = s * (double)dst,  i0 = min((int)src, in - 1),  i1 = min(i0 + 1, in - 1),  l1 = src - i0,  l0 = 1.0 - l1
//     value = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)      every operation rounded to double
//     z = A + (double)f * G;  out = (T)(float)z
// s comes from the host ((in - 1) / (out - 1) in double, 0 where out == 1).  A source of f's size is read as it is.  No tap
// is skipped (0 * inf = NaN, as the stock resize gives).  Nothing is transcendental and nothing crosses a lane: the bits
// depend on neither the plan nor an address.
//
// A streaming kernel.  A workgroup of 256 lanes owns a tile of 256 * V consecutive pixels (flat Y * W + X) of one image
// and one block of cb consecutive channels; lane l owns pixels l * V .. l * V + V - 1 of the tile.  Once per tile a lane
// computes, for each of its pixels, G (one double kept) and -- UP: `a` is smaller or larger than f -- the offset of a's
// first tap, the steps to the other three and the two weights.  It then walks its channels kMgChunk at a time: the loads
// of a chunk are issued before the first is used.  f (and `a` where it has f's size) is read, and y stored, as one
// V-element vector where the address allows and the V pixels exist, single elements otherwise: a plane starts
// (n * C + c) * H * W elements into the tensor, so the alignment is decided per channel (pw_load / pw_store).  UP: the
// four taps of `a` are single-element loads through the cache (a is the small map).  Plain stores: the next launch reads y.
// Every access is guarded by the lane's count of existing pixels.
// ------------------------------------------------------------------------------------
constexpr int kMgThreads = 256;
constexpr int kMgChunk = 4;           // channels per step where `a` has f's size: 2 * kMgChunk vector loads in flight per lane

struct MgAxis {
    int i0, step;      // the first tap, and 1 where the second is another element (0 at the source's last row / column)
    double l1;         // the second tap's weight; the first's is 1.0 - l1
};

__device__ __forceinline__ MgAxis mg_axis(double s, unsigned dst, int in)
{
    const double src = s * (double)dst;
    const int i0 = min((int)src, in - 1);
    return {i0, min(i0 + 1, in - 1) - i0, src - (double)i0};
}

// the four taps at p[0], p[dx], p[dy], p[dy + dx], blended in the header's order
template <class T>
__device__ __forceinline__ double mg_blend(const T* __restrict__ p, int dx, int dy, double lx1, double ly1)
{
    const double v00 = (double)to_f32(p[0]), v01 = (double)to_f32(p[dx]);
    const double v10 = (double)to_f32(p[dy]), v11 = (double)to_f32(p[dy + dx]);
    const double lx0 = 1.0 - lx1, ly0 = 1.0 - ly1;
    const double top = lx0 * v00 + lx1 * v01;
    const double bot = lx0 * v10 + lx1 * v11;
    return ly0 * top + ly1 * bot;
}

struct MgSource {      // a resized source: its size and the two scales ((in - 1) / (out - 1), or 0), from the plan
    int h, w;
    double sy, sx;
};

// grid: N * K * tiles workgroups (tile fastest, then the channel block) of 256 threads.
// UP: a is (N, C, A.h, A.w) and is resized; else it has f's shape.  gate: (N, 1, Gs.h, Gs.w) or NULL; g_resize: whether
// its size differs from (H, W).
template <class T, int V, bool UP>
__global__ __launch_bounds__(kMgThreads) void rroi_merge_kernel(
    const T* __restrict__ a, const T* __restrict__ gate, const T* __restrict__ f, T* __restrict__ y, unsigned C, unsigned W,
    unsigned HW, unsigned tiles, unsigned K, unsigned cb, MgSource A, MgSource Gs, int g_resize)
{
    constexpr int CH = UP ? (V >= 8 ? 1 : 2) : kMgChunk;   // UP holds 4 * V taps per channel: fewer channels in flight
    const unsigned n = blockIdx.x / (tiles * K), rest = blockIdx.x % (tiles * K);
    const unsigned grp = rest / tiles, tile = rest % tiles;
    const unsigned px = (tile * kMgThreads + threadIdx.x) * V;             // < HW + 256 * V
    const int left = px < HW ? (int)min(HW - px, (unsigned)V) : 0;       // this lane's pixels that exist
    const unsigned c0 = grp * cb, c1 = min(c0 + cb, C);                    // plan_merge: c0 < C for every block

    double G[V];
    unsigned aoff[V], astep[V];       // UP: the first tap's offset in a plane of a; the steps to the others (bit 0: x, 1: y)
    double alx1[V], aly1[V];
    const bool gated = gate != nullptr;
    const T* gp = gated ? gate + (size_t)n * ((size_t)Gs.h * Gs.w) : nullptr;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        G[j] = 0.0;
        aoff[j] = astep[j] = 0;
        alx1[j] = aly1[j] = 0.0;
        if (j < left) {
            const unsigned p = px + j, Y = p / W, X = p - Y * W;
            if (gated) {
                if (g_resize) {
                    const MgAxis gy = mg_axis(Gs.sy, Y, Gs.h), gx = mg_axis(Gs.sx, X, Gs.w);
                    G[j] = mg_blend(gp + ((size_t)gy.i0 * Gs.w + gx.i0), gx.step, gy.step * Gs.w, gx.l1, gy.l1);
                } else {
                    G[j] = (double)to_f32(gp[p]);
                }
            }
            if constexpr (UP) {
                const MgAxis ay = mg_axis(A.sy, Y, A.h), ax = mg_axis(A.sx, X, A.w);
                aoff[j] = (unsigned)ay.i0 * (unsigned)A.w + (unsigned)ax.i0;   // < a_h * a_w < 2^31
                astep[j] = (unsigned)(ay.step << 1 | ax.step);
                alx1[j] = ax.l1;
                aly1[j] = ay.l1;
            }
        }
    }

    const T* fp = f + ((size_t)n * C * HW + px);
    T* yp = y + ((size_t)n * C * HW + px);
    const size_t aplane = UP ? (size_t)A.h * A.w : (size_t)HW;
    const T* ap = a + (size_t)n * C * aplane + (UP ? 0 : px);

    for (unsigned c = c0; c < c1; c += CH) {
        T fr[CH][V];
        T ar[CH][V];
#pragma unroll
        for (int k = 0; k < CH; ++k)
            if (c + k < c1) {
                pw_load<T, V>(fp + (size_t)(c + k) * HW, left, fr[k]);
                if constexpr (!UP) pw_load<T, V>(ap + (size_t)(c + k) * HW, left, ar[k]);
            }
#pragma unroll
        for (int k = 0; k < CH; ++k)
            if (c + k < c1) {
                double z[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    double Ad = 0.0;
                    if constexpr (UP) {
                        if (j < left)
                            Ad = mg_blend(ap + ((size_t)(c + k) * aplane + aoff[j]), (int)(astep[j] & 1u),
                                          (int)(astep[j] >> 1) * A.w, alx1[j], aly1[j]);
                    } else {
                        Ad = (double)to_f32(ar[k][j]);
                    }
                    const double fd = (double)to_f32(fr[k][j]);
                    const double p = gated ? fd * G[j] : fd;
                    z[j] = Ad + p;
                }
                pw_store<T, V>(yp + (size_t)(c + k) * HW, left, z);
            }
    }
}
