// rroi_heads_backward_kernels.h -- the training forward and the backward of the detection heads and the attention gate,
// DESIGN 5.27 (header section 7b).
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_heads_kernels.h, whose loads, stores and weight broadcast it uses); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// The training forward: rroi_pointwise_kernel (rroi_heads_kernels.h) statement for statement, with one more store -- the
// sums z_o as they stand in front of the sigmoid go to `z` (N, NOUT, H, W) in double -- so score, rbox, angle and y have
// the forward's bits.  A kernel of its own, so that the forward's code stays what was measured: change both together.
// ------------------------------------------------------------------------------------
template <class T, int NOUT, int EPI, int V>
__global__ __launch_bounds__(kPwMaxWaves / V * 64) void rroi_pointwise_train_kernel(
    const T* __restrict__ x, const T* __restrict__ w0, const T* __restrict__ b0, const T* __restrict__ w1,
    const T* __restrict__ b1, const T* __restrict__ w2, const T* __restrict__ b2, T* __restrict__ y0, T* __restrict__ y1,
    T* __restrict__ y2, double* __restrict__ z, unsigned C, unsigned HW, unsigned tiles, unsigned cb, double rbox_scale)
{
    static_assert(NOUT * kPwChunk <= 64, "one weight of a chunk per lane");
    static_assert((NOUT == 7 && EPI == kPwEpiHeads) || (NOUT == 1 && EPI == kPwEpiSigmoid), "heads or gate");
    extern __shared__ double pw_partials[];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), S = blockDim.x >> 6;
    const unsigned n = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const unsigned px = (tile * 64u + lane) * V;           // < HW + 64 * V
    const int left = px < HW ? (int)min(HW - px, (unsigned)V) : 0;   // this lane's pixels that exist
    const unsigned c0 = wave * cb, c1 = min(c0 + cb, C);   // plan_heads: c0 < C for every wave
    const T* xp = x + ((size_t)n * C * HW + px);

    // lane o * kPwChunk + k carries w[o][c + k] of the current chunk
    const unsigned wo = lane / kPwChunk, wk = lane % kPwChunk;
    const T* wrow = nullptr;
    if (wo < (unsigned)NOUT) wrow = wo == 0 ? w0 : wo < 5 ? w1 + (size_t)(wo - 1) * C : w2 + (size_t)(wo - 5) * C;

    double acc[NOUT][V];
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
        for (int j = 0; j < V; ++j) acc[o][j] = 0.0;
    unsigned c = c0;
    for (; c + kPwChunk <= c1; c += kPwChunk)
        pw_chunk<T, NOUT, V, true>(xp + (size_t)c * HW, wrow ? wrow + c : nullptr, HW, kPwChunk, left, wk, acc);
    if (c < c1) pw_chunk<T, NOUT, V, false>(xp + (size_t)c * HW, wrow ? wrow + c : nullptr, HW, c1 - c, left, wk, acc);

    if (wave != 0) {
#pragma unroll
        for (int o = 0; o < NOUT; ++o)
#pragma unroll
            for (int j = 0; j < V; ++j) pw_partials[(((wave - 1) * NOUT + o) * V + j) * 64 + lane] = acc[o][j];
    }
    __syncthreads();
    if (wave != 0) return;

    double s[NOUT][V];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
        const T* bp = o == 0 ? b0 : o < 5 ? b1 : b2;
        const double b = bp ? (double)to_f32(bp[o == 0 ? 0 : o < 5 ? o - 1 : o - 5]) : 0.0;
#pragma unroll
        for (int j = 0; j < V; ++j) s[o][j] = b + acc[o][j];
    }
    for (unsigned k = 1; k < S; ++k)
#pragma unroll
        for (int o = 0; o < NOUT; ++o)
#pragma unroll
            for (int j = 0; j < V; ++j) s[o][j] += pw_partials[(((k - 1) * NOUT + o) * V + j) * 64 + lane];
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (j < left) z[((size_t)n * NOUT + o) * HW + px + j] = s[o][j];   // the one addition to the forward
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
        for (int j = 0; j < V; ++j) s[o][j] = pw_sigmoid(s[o][j]);

    pw_store<T, V>(y0 + ((size_t)n * HW + px), left, s[0]);
    if constexpr (EPI == kPwEpiHeads) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int j = 0; j < V; ++j) s[1 + q][j] = rbox_scale * s[1 + q][j];
            pw_store<T, V>(y1 + (((size_t)n * 4 + q) * HW + px), left, s[1 + q]);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const double a0 = 2.0 * s[5][j] - 1.0, a1 = 2.0 * s[6][j] - 1.0;
            const double r = sqrt(a0 * a0 + a1 * a1);      // 0 / 0 = NaN where both vanish, as the stock chain gives
            s[5][j] = a0 / r;
            s[6][j] = a1 / r;
        }
        pw_store<T, V>(y2 + (((size_t)n * 2 + 0) * HW + px), left, s[5]);
        pw_store<T, V>(y2 + (((size_t)n * 2 + 1) * HW + px), left, s[6]);
    }
}

// ------------------------------------------------------------------------------------
// The backward, with the arithmetic of header section 7b, all in double:
//     s_o = 1 / (1 + exp(-z_o));  g_0 = dscore, g_{1+j} = rbox_scale * drbox_j,
//     a_i = 2 s_{5+i} - 1, r = sqrt(a_0 a_0 + a_1 a_1), u_i = a_i / r, g_{5+i} = 2 (dangle_i - u_i (u_0 dangle_0 + u_1 dangle_1)) / r
//     dz_o = g_o * (s_o * (1 - s_o));   dx_c = fma(w[6][c], dz_6, ... fma(w[0][c], dz_0, +0.0));   out = (T)(float)value
//     dw[o][c] = sum over pixels of dz_o x[c],  db[o] = sum over pixels of dz_o, in the order written out below.
//
// A workgroup is kHbWaves waves on one tile of 64 * V consecutive pixels of one image at a time; lane l owns pixels
// l * V .. l * V + V - 1 of the tile, as in the forward, and every wave forms those pixels' dz for itself (NOUT exps per
// pixel against C * NOUT fma).  Wave k owns the channels [k * cb, (k + 1) * cb) of the current pass, cb a multiple of
// kPwChunk, and walks them kPwChunk at a time: kPwChunk loads of x per lane, the weights wave-uniform through pw_bcast as
// in the forward, NOUT * V fma and one store per channel for dx, and NOUT * V fma into the lane's partials of dw --
// kPwChunk * 8 values, value k * 8 + o the sum over the lane's V pixels of dz_o x[c + k] (o >= NOUT: +0.0).
// Those values are then summed over the 64 lanes by halving (hb_fold): lanes l and l ^ 32 exchange one half of their
// values each and keep the sum of the other, then l ^ 16 with a quarter, and so on; after log2(values) steps lane l holds
// the wave's sum of value l alone (the gate's 8 values: of value l >> 3, after three more plain exchanges).  63 exchanges
// for 56 sums, where a wave reduction per value would be 336.
// The lane adds its value onto its own LDS cell [wave][chunk of the pass][lane], so a workgroup may walk many tiles -- of
// several images -- before it writes: at the end of a pass every cell goes to the workgroup's row of the workspace
// ([o][c] for o < NOUT, then db[o]: NOUT * (C + 1) doubles).  db is a lane-private sum over the tiles in wave 0, reduced
// once per workgroup.  A pass is at most kHbWaves * kHbPassBlock channels (the LDS it takes); more channels are further
// passes over the same tiles.  No atomics, no hand-off between workgroups, and no wave reads another wave's cells.
//
// The sums' order, which the plan alone fixes: within a lane over its V pixels; over the lanes as hb_fold pairs them;
// over the workgroup's tiles in tile order; over the workgroups' rows in rroi_heads_backward_finish_kernel.
// ------------------------------------------------------------------------------------
constexpr int kHbWaves = 4;
constexpr int kHbThreads = kHbWaves * 64;
constexpr unsigned kHbPassBlock = 128;    // channels per wave and pass: kHbWaves * (128 / kPwChunk) * 64 doubles = 32 KiB of LDS
constexpr int kHbFinishParts = 4;         // of the finish launch

__device__ __forceinline__ double hb_xor(double v, int mask) { return __shfl_xor(v, mask, 64); }

// v[0 .. M): per-lane values -> v[0]: the sum over the wave's lanes of the value the lane ends up with (see above)
template <int M, int MASK>
__device__ __forceinline__ void hb_fold(double* v, unsigned lane)
{
    if constexpr (MASK >= 1) {
        if constexpr (M > 1) {
            constexpr int H = M / 2;
            const bool up = (lane & (unsigned)MASK) != 0;
#pragma unroll
            for (int i = 0; i < H; ++i) {
                const double lo = v[i], hi = v[i + H];
                v[i] = (up ? hi : lo) + hb_xor(up ? lo : hi, MASK);
            }
            hb_fold<H, MASK / 2>(v, lane);
        } else {
            v[0] = v[0] + hb_xor(v[0], MASK);
            hb_fold<1, MASK / 2>(v, lane);
        }
    }
}

// dz of the lane's V pixels of tile (n, tile): +0.0 for a pixel behind the plane's end
template <class T, int NOUT, int V>
__device__ __forceinline__ void hb_dz(const double* __restrict__ z, const T* __restrict__ g0, const T* __restrict__ g1,
                                      const T* __restrict__ g2, unsigned n, unsigned px, int left, unsigned HW,
                                      double rbox_scale, double (&dz)[NOUT][V])
{
#pragma unroll
    for (int j = 0; j < V; ++j) {
        if (j >= left) {
#pragma unroll
            for (int o = 0; o < NOUT; ++o) dz[o][j] = 0.0;
            continue;
        }
        double s[NOUT], g[NOUT];
#pragma unroll
        for (int o = 0; o < NOUT; ++o) s[o] = pw_sigmoid(z[((size_t)n * NOUT + o) * HW + px + j]);
        g[0] = g0 ? (double)to_f32(g0[(size_t)n * HW + px + j]) : 0.0;
        if constexpr (NOUT == 7) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                g[1 + q] = rbox_scale * (g1 ? (double)to_f32(g1[((size_t)n * 4 + q) * HW + px + j]) : 0.0);
            const double d0 = g2 ? (double)to_f32(g2[((size_t)n * 2 + 0) * HW + px + j]) : 0.0;
            const double d1 = g2 ? (double)to_f32(g2[((size_t)n * 2 + 1) * HW + px + j]) : 0.0;
            const double a0 = 2.0 * s[5] - 1.0, a1 = 2.0 * s[6] - 1.0;
            const double r = sqrt(a0 * a0 + a1 * a1);      // 0: NaN in both, as the stock chain's backward gives
            const double u0 = a0 / r, u1 = a1 / r;
            const double p = u0 * d0 + u1 * d1;
            g[5] = 2.0 * (d0 - u0 * p) / r;
            g[6] = 2.0 * (d1 - u1 * p) / r;
        }
#pragma unroll
        for (int o = 0; o < NOUT; ++o) dz[o][j] = g[o] * (s[o] * (1.0 - s[o]));
    }
}

// grid: `rows` workgroups of kHbThreads; workgroup b walks tiles [b * tpw, min((b + 1) * tpw, N * tiles)), tile index
// n * tiles + tile.  dynamic LDS: kHbWaves * (min(cb, kHbPassBlock) / kPwChunk) * 64 doubles where `partials` is given, else 0.
// g0 / g1 / g2: dscore, drbox, dangle (gate: dy, -, -), each or NULL (zero).  dx or NULL; partials (the workspace) or NULL.
template <class T, int NOUT, int V>
__global__ __launch_bounds__(kHbThreads) void rroi_heads_backward_kernel(
    const T* __restrict__ g0, const T* __restrict__ g1, const T* __restrict__ g2, const T* __restrict__ x,
    const double* __restrict__ z, const T* __restrict__ w0, const T* __restrict__ w1, const T* __restrict__ w2,
    T* __restrict__ dx, double* __restrict__ partials, unsigned C, unsigned HW, unsigned tiles, unsigned total_tiles,
    unsigned tpw, unsigned cb, double rbox_scale)
{
    static_assert(NOUT == 7 || NOUT == 1, "heads or gate");
    constexpr int NP = NOUT == 7 ? 8 : 1;                  // a channel's slots among the folded values
    constexpr int M = kPwChunk * NP;
    extern __shared__ double hb_cells[];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned t0 = blockIdx.x * tpw, t1 = min(t0 + tpw, total_tiles);
    const unsigned pass_cb = min(cb, kHbPassBlock), pass_chunks = pass_cb / kPwChunk;
    double* cells = hb_cells + (size_t)wave * pass_chunks * 64;
    double* row = partials ? partials + (size_t)blockIdx.x * NOUT * (C + 1) : nullptr;

    // lane o * kPwChunk + k carries w[o][c + k] of the current chunk, as in the forward
    const unsigned wo = lane / kPwChunk, wk = lane % kPwChunk;
    const T* wrow = nullptr;
    if (wo < (unsigned)NOUT && w0) wrow = wo == 0 ? w0 : wo < 5 ? w1 + (size_t)(wo - 1) * C : w2 + (size_t)(wo - 5) * C;
    // the cell of lane l is channel l >> 3 of its chunk and output l & 7
    const unsigned ck = lane >> 3, co = lane & 7u;

    double db[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) db[o] = 0.0;

    for (unsigned base = 0; base < cb; base += pass_cb) {
        // this wave's channels of this pass; possibly none (c0 >= c1)
        const unsigned c0 = min(wave * cb + base, C), c1 = min(min(c0 + pass_cb, wave * cb + cb), C);
        if (row)
            for (unsigned q = 0; q < pass_chunks; ++q) cells[q * 64 + lane] = 0.0;
        for (unsigned t = t0; t < t1; ++t) {
            const unsigned n = t / tiles, tile = t % tiles;
            const unsigned px = (tile * 64u + lane) * V;
            const int left = px < HW ? (int)min(HW - px, (unsigned)V) : 0;
            double dz[NOUT][V];
            hb_dz<T, NOUT, V>(z, g0, g1, g2, n, px, left, HW, rbox_scale, dz);
            if (row && wave == 0 && base == 0) {
#pragma unroll
                for (int o = 0; o < NOUT; ++o)
#pragma unroll
                    for (int j = 0; j < V; ++j) db[o] += dz[o][j];
            }
            const T* xp = x + ((size_t)n * C * HW + px);
            T* dxp = dx ? dx + ((size_t)n * C * HW + px) : nullptr;
            for (unsigned c = c0, q = 0; c < c1; c += kPwChunk, ++q) {
                const unsigned m = min(c1 - c, (unsigned)kPwChunk);
                T r[kPwChunk][V];
                const T* xc = xp + (size_t)c * HW;         // the chunk's first plane; stepped by HW per channel
                T* dxc = dxp ? dxp + (size_t)c * HW : nullptr;
#pragma unroll
                for (int k = 0; k < kPwChunk; ++k) {
                    if ((unsigned)k < m) {
                        pw_load<T, V>(xc, left, r[k]);
                        xc += HW;
                    } else {
#pragma unroll
                        for (int j = 0; j < V; ++j) r[k][j] = (T)0.0f;
                    }
                }
                if (dxc) {
                    const double wl = (wrow && wk < m) ? (double)to_f32(wrow[c + wk]) : 0.0;
#pragma unroll
                    for (int k = 0; k < kPwChunk; ++k)
                        if ((unsigned)k < m) {
                            double acc[V];
#pragma unroll
                            for (int j = 0; j < V; ++j) acc[j] = 0.0;
#pragma unroll
                            for (int o = 0; o < NOUT; ++o) {
                                const double wd = pw_bcast(wl, o * kPwChunk + k);
#pragma unroll
                                for (int j = 0; j < V; ++j) acc[j] = __builtin_fma(wd, dz[o][j], acc[j]);
                            }
                            pw_store<T, V>(dxc, left, acc);
                            dxc += HW;
                        }
                }
                if (row) {
                    double v[M];
#pragma unroll
                    for (int k = 0; k < kPwChunk; ++k)
#pragma unroll
                        for (int o = 0; o < NP; ++o) {
                            double a = 0.0;
                            if (o < NOUT) {
#pragma unroll
                                for (int j = 0; j < V; ++j) a = __builtin_fma(dz[o < NOUT ? o : 0][j], (double)to_f32(r[k][j]), a);
                            }
                            v[k * NP + o] = a;
                        }
                    hb_fold<M, 32>(v, lane);
                    cells[q * 64 + lane] += v[0];
                }
            }
        }
        if (row && co < (unsigned)NOUT) {
            for (unsigned c = c0 + ck, q = 0; c < c1; c += kPwChunk, ++q) row[(size_t)co * C + c] = cells[q * 64 + lane];
        }
    }
    if (row && wave == 0) {
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            double v = db[o];
            hb_fold<1, 32>(&v, lane);
            if (lane == 0) row[(size_t)NOUT * C + o] = v;
        }
    }
}

// Entry e of a row is dw[o][c] (e = o * C + c) or db[o] (e = NOUT * C + o).  Thread (e, part q) adds the rows
// [q * per, min((q + 1) * per, rows)), per = ceil(rows / kHbFinishParts), in row order from +0.0; the parts are then added
// in part order, rounded once and stored -- where the output is wanted.
// grid: ceil(NOUT * (C + 1) / 64) workgroups of 64 * kHbFinishParts threads.
template <class T, int NOUT>
__global__ __launch_bounds__(64 * kHbFinishParts) void rroi_heads_backward_finish_kernel(
    const double* __restrict__ partials, T* __restrict__ dw0, T* __restrict__ db0, T* __restrict__ dw1, T* __restrict__ db1,
    T* __restrict__ dw2, T* __restrict__ db2, unsigned C, unsigned rows)
{
    __shared__ double parts[kHbFinishParts][64];
    const unsigned E = (unsigned)NOUT * (C + 1), e = blockIdx.x * 64u + (threadIdx.x & 63u), q = threadIdx.x >> 6;
    const unsigned per = (rows + kHbFinishParts - 1) / kHbFinishParts;
    double sum = 0.0;
    if (e < E) {
        const unsigned r1 = min((q + 1) * per, rows);
        for (unsigned r = q * per; r < r1; ++r) sum += partials[(size_t)r * E + e];
    }
    parts[q][threadIdx.x & 63u] = sum;
    __syncthreads();
    if (q != 0 || e >= E) return;
#pragma unroll
    for (int k = 1; k < kHbFinishParts; ++k) sum += parts[k][threadIdx.x];
    T* out;
    if (e < (unsigned)NOUT * C) {
        const unsigned o = e / C, c = e % C;
        out = o == 0 ? (dw0 ? dw0 + c : nullptr) : o < 5 ? (dw1 ? dw1 + (size_t)(o - 1) * C + c : nullptr)
                                                         : (dw2 ? dw2 + (size_t)(o - 5) * C + c : nullptr);
    } else {
        const unsigned o = e - (unsigned)NOUT * C;
        out = o == 0 ? (db0 ? db0 : nullptr) : o < 5 ? (db1 ? db1 + (o - 1) : nullptr) : (db2 ? db2 + (o - 5) : nullptr);
    }
    if (out) *out = from_f32<T>((float)sum);
}
