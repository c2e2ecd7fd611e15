// rroi_ctc_loss_kernels.h -- the CTC loss of every sequence and its unscaled gradient in one launch, DESIGN 5.22
// Part of the single translation unit rroi_align_hip.hip (included inside its anonymous namespace after
// rroi_device_common.h, whose bf16_t / fp16_t it uses); not a standalone header.
#pragma once

// ------------------------------------------------------------------------------------
// The contract is include/rroi_align_hip.h section 15.  lp = the input widened exactly to double, l' = the target with
// blanks interleaved (S = 2 L + 1), every operation in double:
//     alpha_0(0) = lp[blank, 0], alpha_0(1) = lp[l_1, 0], -inf elsewhere
//     alpha_t(s) = lp[l'_s, t] + lse(alpha_{t-1}(s), alpha_{t-1}(s-1), [alpha_{t-1}(s-2) if l'_s != blank, != l'_{s-2}])
//     nll        = -lse(alpha_{Tn-1}(S-1), alpha_{Tn-1}(S-2)),  beta the mirror image
//     grad[t, k] = exp(lp) - exp(lse_{s: l'_s = k}(alpha_t(s) + beta_t(s)) + nll - lp)     (t < Tn, lp and nll finite)
//
// One workgroup of 256 threads owns one sequence.  Time is cut into chunks of TC steps.
//   recurrences   With a gradient, the two recurrences run AT THE SAME TIME: in step i the lower half of the workgroup takes
//           alpha at t = i (thread s owns position s; positions past 128 go round) and the upper half beta at t = Tn - 1 - i,
//           one barrier per step for both, so the serial chain is Tn steps long, not 2 Tn.  Each side reads its previous
//           row from a two-row LDS buffer and keeps every row -- in LDS where 2 S_max T doubles fit beside the rest, else in
//           the caller's workspace, which only the combine below reads.  lp[l'_s, t] of a chunk's steps is staged to LDS in
//           one round of loads per chunk (both sides' chunks together), so a step never waits on memory.  Without a
//           gradient only alpha runs and only two rows are kept.
//   combine   per chunk of TC steps, fully parallel: the class sums of each step are taken IN A FIXED ORDER -- the odd
//           positions of one class are a chain in ascending s (built once per sequence), walked by one thread per (step,
//           chain); the positions that hold the blank are walked in ascending s by one thread per step.  No atomic anywhere
//           and no order that depends on scheduling, so a second run gives the same bits.
//   store     the chunk's (TC, K) tile of class sums becomes gradient elements, written along whichever of t or k is
//           contiguous in the gradient tensor; steps at or past Tn, classes with lp = -inf and sequences whose nll is
//           infinite get zeros.  Every element of the gradient is written exactly once.
//
// A sequence is infeasible -- nll = +inf, gradient 0 -- where Tn is outside [0, T], L is outside [0, min(L_max, T)] or a
// label is outside [0, K); this is decided before anything is read through a label or a length, so no contents of the
// integer tensors make the kernel read or write out of bounds.
// ------------------------------------------------------------------------------------
constexpr int kCtcThreads = 256;
constexpr int kCtcHalf = kCtcThreads / 2;

struct CtcStrides { long long t, n, k; };

__device__ __forceinline__ double ctc_ninf() { return -__builtin_huge_val(); }

__device__ __forceinline__ double ctc_widen(float v) { return (double)v; }
__device__ __forceinline__ double ctc_widen(bf16_t v) { return (double)(float)v; }
__device__ __forceinline__ double ctc_widen(fp16_t v) { return (double)(float)v; }

// double -> T, rounded once: fp32 directly; the 16-bit types through a float rounded TO ODD, whose second rounding (to
// nearest even, 13 or 16 bits shorter) then lands where a single rounding of the double would.
__device__ __forceinline__ float ctc_to_f32_odd(double d)
{
    float f = (float)d;
    const double back = (double)f;
    if (back != d && back - back == 0.0) {                 // inexact and finite
        unsigned u = __float_as_uint(f);
        if (fabs(back) > fabs(d)) u -= 1u;                 // back towards zero: the truncation
        f = __uint_as_float(u | 1u);
    }
    return f;
}
__device__ __forceinline__ void ctc_narrow(double d, float* p) { *p = (float)d; }
__device__ __forceinline__ void ctc_narrow(double d, bf16_t* p) { *p = (bf16_t)ctc_to_f32_odd(d); }
__device__ __forceinline__ void ctc_narrow(double d, fp16_t* p) { *p = (fp16_t)ctc_to_f32_odd(d); }

// log(exp(a) + exp(b) + exp(c)) = m + log(1 + exp(x - m) + exp(y - m)), m the largest and x <= y the other two (the
// largest term is exactly 1 and costs no exp); -inf where all three are
__device__ __forceinline__ double ctc_lse3(double a, double b, double c)
{
    const double lo = fmin(a, b), hi = fmax(a, b);
    const double m = fmax(hi, c), mid = fmin(hi, c);
    if (m == ctc_ninf()) return m;
    return m + log(1.0 + (exp(lo - m) + exp(mid - m)));
}

// lp[l'_s, t] of the steps t = tfirst + dir * tc, tc < nt, to dst[tc][s]; `threads` threads starting at `first` take part
template <class T>
__device__ __forceinline__ void ctc_stage(double* __restrict__ dst, const T* __restrict__ lpn, CtcStrides ls, const int* lab, int S,
                                          int Smax, int tfirst, int dir, int nt, bool along_t, int first, int threads)
{
    for (int i = (int)threadIdx.x - first; i < nt * S; i += threads) {
        const int tc = along_t ? i % nt : i / S, s = along_t ? i / nt : i % S;
        dst[tc * Smax + s] = ctc_widen(lpn[(long long)(tfirst + dir * tc) * ls.t + (long long)lab[s] * ls.k]);
    }
}

template <class T>
__global__ __launch_bounds__(kCtcThreads) void rroi_ctc_loss_kernel(
    const T* __restrict__ lp, CtcStrides ls, int K, int Tmax, const int* __restrict__ targets, int Lmax,
    const int* __restrict__ in_len, const int* __restrict__ tgt_len, int blank, int zero_infinity,
    float* __restrict__ nll_out, T* __restrict__ grad, CtcStrides gs, double* __restrict__ rows_ws, int rows_in_lds, int TC)
{
    extern __shared__ double ctc_lds[];
    const int n = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int Lcap = Lmax < Tmax ? Lmax : Tmax;
    const int Smax = 2 * Lcap + 1;
    // LDS: doubles first, then ints
    double* arow = ctc_lds;                          // [2][Smax]   alpha's previous and current row
    double* brow = arow + 2 * (size_t)Smax;          // [2][Smax]   beta's
    double* lpa = brow + 2 * (size_t)Smax;           // [TC][Smax]  lp[l'_s, t] of alpha's chunk
    double* lpb = lpa + (size_t)TC * Smax;           // [TC][Smax]  ... of beta's chunk
    double* tile = lpb + (size_t)TC * Smax;          // [TC][K]     the class sums of a chunk
    double* rows_lds = tile + (size_t)TC * K;        // [2][Tmax][Smax] every alpha and beta row, where they fit
    int* lab = reinterpret_cast<int*>(rows_lds + (rows_in_lds && grad ? 2 * (size_t)Tmax * Smax : 0));   // [Smax] l'_s
    int* nxt = lab + Smax;                           // [Smax] odd s: the next position of the same class, -1 at the end
    int* own = nxt + Smax;                           // [Smax] odd s: 1 where no earlier position has the class
    int* bad_label = own + Smax;                     // [1]    a label of this sequence is outside [0, K)
    double* alpha = rows_in_lds ? rows_lds : rows_ws + (size_t)n * 2 * Tmax * Smax;
    double* beta = alpha + (size_t)Tmax * Smax;

    const int Tn = in_len[n], L = tgt_len[n];
    const bool lengths_ok = Tn >= 0 && Tn <= Tmax && L >= 0 && L <= Lcap;
    const int S = lengths_ok ? 2 * L + 1 : 1;
    if (tid == 0) *bad_label = 0;
    __syncthreads();
    if (lengths_ok)
        for (int s = tid; s < S; s += kCtcThreads) {
            int c = blank;
            if (s & 1) {
                c = targets[(size_t)n * Lmax + (s >> 1)];
                if (c < 0 || c >= K) { *bad_label = 1; c = blank; }
            }
            lab[s] = c;
        }
    __syncthreads();                                 // publishes lab and the flag
    const bool feasible = lengths_ok && !*bad_label;

    const T* lpn = lp + (long long)n * ls.n;
    T* gn = grad ? grad + (long long)n * gs.n : nullptr;
    const bool g_along_t = gs.t == 1 && gs.k != 1, l_along_t = ls.t == 1 && ls.k != 1;
    // who does what in a step: with a gradient the lower half alpha and the upper half beta, else everybody alpha
    const bool both = grad != nullptr;
    const int side_threads = both ? kCtcHalf : kCtcThreads;
    const bool on_beta = both && tid >= kCtcHalf;
    const int stid = on_beta ? tid - kCtcHalf : tid;

    double nll = __builtin_huge_val();
    if (feasible) {
        // the chains of equal classes over the odd positions, ascending
        if (grad)
            for (int s = tid; s < S; s += kCtcThreads) {
                int nx = -1, first = 1;
                if (s & 1) {
                    const int c = lab[s];
                    for (int q = s + 2; q < S; q += 2)
                        if (lab[q] == c) { nx = q; break; }
                    for (int q = 1; q < s; q += 2)
                        if (lab[q] == c) { first = 0; break; }
                }
                nxt[s] = nx;
                own[s] = first;
            }
        // ---- alpha forwards and, with a gradient, beta backwards at the same time
        for (int i0 = 0; i0 < Tn; i0 += TC) {
            const int nt = Tn - i0 < TC ? Tn - i0 : TC;
            if (!on_beta) ctc_stage(lpa, lpn, ls, lab, S, Smax, i0, 1, nt, l_along_t, 0, side_threads);
            else ctc_stage(lpb, lpn, ls, lab, S, Smax, Tn - 1 - i0, -1, nt, l_along_t, kCtcHalf, side_threads);
            __syncthreads();
            for (int tc = 0; tc < nt; ++tc) {
                const int i = i0 + tc;
                if (!on_beta) {
                    const int t = i;
                    const double* prev = arow + ((i + 1) & 1) * Smax;
                    double* cur = arow + (i & 1) * Smax;
                    for (int s = stid; s < S; s += side_threads) {
                        double a;
                        if (i == 0) {
                            a = s < 2 ? lpa[tc * Smax + s] : ctc_ninf();
                        } else {
                            const double a1 = s >= 1 ? prev[s - 1] : ctc_ninf();
                            const double a2 = s >= 2 && lab[s] != blank && lab[s] != lab[s - 2] ? prev[s - 2] : ctc_ninf();
                            a = lpa[tc * Smax + s] + ctc_lse3(prev[s], a1, a2);
                        }
                        cur[s] = a;
                        if (grad) alpha[(size_t)t * Smax + s] = a;
                    }
                } else {
                    const int t = Tn - 1 - i;
                    const double* next = brow + ((i + 1) & 1) * Smax;
                    double* cur = brow + (i & 1) * Smax;
                    for (int s = stid; s < S; s += side_threads) {
                        double b;
                        if (i == 0) {
                            b = s >= S - 2 ? lpb[tc * Smax + s] : ctc_ninf();
                        } else {
                            const double b1 = s + 1 < S ? next[s + 1] : ctc_ninf();
                            const double b2 = s + 2 < S && lab[s] != blank && lab[s] != lab[s + 2] ? next[s + 2] : ctc_ninf();
                            b = lpb[tc * Smax + s] + ctc_lse3(next[s], b1, b2);
                        }
                        cur[s] = b;
                        beta[(size_t)t * Smax + s] = b;
                    }
                }
                __syncthreads();
            }
        }
        if (Tn == 0) {
            nll = L == 0 ? 0.0 : __builtin_huge_val();
        } else {
            const double* last = arow + ((Tn - 1) & 1) * Smax;
            nll = -ctc_lse3(last[S - 1], S >= 2 ? last[S - 2] : ctc_ninf(), ctc_ninf());
        }
    }
    const bool finite = nll < __builtin_huge_val();
    if (tid == 0) nll_out[n] = finite || !zero_infinity ? (float)nll : 0.0f;
    if (!grad) return;

    // ---- the class sums and the gradient, a chunk of steps at a time; chunks at or past Tn store zeros only.  The rows a
    // thread reads here were written by other threads: behind the last step's barrier, which orders LDS and (within a
    // workgroup) global memory alike.
    const int Tlive = feasible && finite ? Tn : 0;
    for (int t0 = 0; t0 < Tmax; t0 += TC) {
        const int ntile = Tmax - t0 < TC ? Tmax - t0 : TC;                        // steps of this chunk that exist
        const int nt = Tlive - t0 < TC ? (Tlive - t0 > 0 ? Tlive - t0 : 0) : TC;  // ... that are below Tn
        if (nt > 0) {
            for (int i = tid; i < nt * K; i += kCtcThreads) tile[i] = ctc_ninf();
            __syncthreads();
            // one thread per (step, position that starts a chain); the blank's positions: one thread per step, from the
            // other end of the workgroup so that the two kinds of item share few waves
            for (int i = tid; i < nt * S; i += kCtcThreads) {
                const int tc = i / S, s = i % S;
                if (!(s & 1) || !own[s] || lab[s] == blank) continue;
                const double* at = alpha + (size_t)(t0 + tc) * Smax;
                const double* bt = beta + (size_t)(t0 + tc) * Smax;
                double v = at[s] + bt[s];
                if (nxt[s] >= 0) {
                    double m = v;
                    for (int q = nxt[s]; q >= 0; q = nxt[q]) m = fmax(m, at[q] + bt[q]);
                    if (m == ctc_ninf()) {
                        v = m;
                    } else {
                        double sum = 0.0;
                        for (int q = s; q >= 0; q = nxt[q]) sum += exp((at[q] + bt[q]) - m);
                        v = m + log(sum);
                    }
                }
                tile[tc * K + lab[s]] = v;
            }
            for (int tc = kCtcThreads - 1 - tid; tc < nt; tc += kCtcThreads) {
                const double* at = alpha + (size_t)(t0 + tc) * Smax;
                const double* bt = beta + (size_t)(t0 + tc) * Smax;
                double m = ctc_ninf();
                for (int s = 0; s < S; ++s)
                    if (lab[s] == blank) m = fmax(m, at[s] + bt[s]);
                double v = m;
                if (m != ctc_ninf()) {
                    double sum = 0.0;
                    for (int s = 0; s < S; ++s)
                        if (lab[s] == blank) sum += exp((at[s] + bt[s]) - m);
                    v = m + log(sum);
                }
                tile[tc * K + blank] = v;
            }
            __syncthreads();
        }
        for (int i = tid; i < ntile * K; i += kCtcThreads) {
            const int tc = g_along_t ? i % ntile : i / K, k = g_along_t ? i / ntile : i % K;
            const int t = t0 + tc;
            double g = 0.0;
            if (tc < nt) {
                const double v = ctc_widen(lpn[(long long)t * ls.t + (long long)k * ls.k]);
                if (v != ctc_ninf()) {
                    g = exp(v);
                    const double c = tile[tc * K + k];
                    if (c != ctc_ninf()) g -= exp(c + nll - v);          // a class outside the target: nothing to subtract
                }
            }
            ctc_narrow(g, gn + (long long)t * gs.t + (long long)k * gs.k);
        }
        __syncthreads();       // the tile is free for the next chunk
    }
}
