// rroi_host_plan.h -- host side, part 1 of 3: what a call launches.  The tuning table, a call's Shape and its limits, the
// grids, both workspace carvers, AUTO's rules and the dispatch (plan_forward / plan_backward / plan_forward_bucketed) with
// its report as an rroi_align_plan.  Every number of a launch that depends on the CU count or on the tuning table -- every
// grid, every block count, every flag word -- is computed here, once, by the planner of the family that launches it, and
// carried by the plan.  Nothing in this file launches or touches memory; num_cus() is its only HIP call.
// Included by rroi_align_hip.hip inside its anonymous namespace, after the device headers.
#pragma once

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// CU count per device ordinal (a process may drive several GPUs, one per thread or per call):
// grids are sized for the device that is current at the call.
constexpr int kMaxDevices = 64;
std::atomic<int> g_cus[kMaxDevices];

int num_cus()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
    int cus = g_cus[dev].load(std::memory_order_relaxed);
    if (cus > 0) return cus;
    cus = 256;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) cus = p.multiProcessorCount;
    g_cus[dev].store(cus, std::memory_order_relaxed);
    return cus;
}

// Launch-shape constants of the shipped configuration.  The product reads them as compile-time constants.  The tools'
// exploration build (tools/rroi_align_hip_explore.hip: kbench, build_explore.sh) includes rroi_align_hip.hip with
// RROI_TUNING_QUALIFIER defined empty -- a mutable struct -- and adds its rroi_align_debug_set_* setters BEHIND the
// include: nothing of it is in this file or in the product library.
struct Tuning {
    int row_pad = -1;             // chunk-major row pitch: -1 = W | 1 (see row_pitch)
    int waves_per_cu = 12;        // the backward's one-wave atomic scatter (rroi_bwd_tiled_kernel): 12.4 KB of LDS each
    // rroi_fwd_split_kernel: 62-64 VGPRs under __launch_bounds__(128, 6) and 12.1 KB of LDS (10 granules of 1280 B)
    // -> 12 workgroups per CU; a larger grid would run its surplus as a second round
    int split_wgs_per_cu = 12;
    int fwd_shift = 1;            // 1: crops with PH * PW % 16 != 0 take the SHIFT forms where they pay; 2: always; 0: never
    int shift_wgs_per_cu = 0;     // > 0 overrides the SHIFT kernels' workgroups per CU
    int fwd_dbg = 0;              // ablations: 1 = skip output stores, 2 = all taps out of range, 256 = free first item
    int prologue_blocks_per_cu = 3;
    int fwd_patch = 1;            // the direct path = K2p (round 5: shared geometry, row pairs as 8-byte loads); 0: rounds 1-4's thread-per-bin kernel
    int fwd_patch_waves = 4096;   // ... channel slabs sized for about this many waves ...
    int fwd_patch_cwave = 8;      // ... of at most this many channels each
    int fwd_fused = 1;            // AUTO may take the one-launch gather from the NCHW map for few ROIs (round 5)
    double fwd_fused_min_elems = 1.5e6;   // ... from this many output elements up (below: the direct kernel) ...
    int fwd_fused_min_channels = 128;     // ... and this many channels
    double fwd_tiled_min_elems = 3.8e6;   // ... and the two-launch path from this many up
    int fwd_shift_lines = 1;      // 1: line-aligned windows for rows that are not whole sectors beyond 320 MB of crops (round 5); 0: never; 2: always
    int shift_lines_wgs_per_cu = 10;
    int fwd_merge = 1;            // rows that are not whole sectors under XCD groups: strided tiles + plain stores where it pays (round 5); 0: SHIFT always; 2: always
    int fwd_groups = 1;           // XCD groups for nchunks in {1, 2} (round 5; XcdGroups in rroi_forward_kernels.h); 0: off
    int fwd_groups_min_rois = 64; // ... from this many ROIs up
    int bwd_buckets = 1;          // one-pass pixel lists (round 3); 0: count / scan / fill as in rounds 1-2
    int bwd_pair_aggregate = 1;       // bucket slots reserved per wave through LDS (round 5); 0: one atomic per pair
    int bwd_pair_blocks_per_cu = 0;   // 0: 256 / C, clamped to 2 .. 4 (see plan_backward)
    int bwd_tile_run = 2;         // the in-place NCHW gather: 2^v neighbouring key tiles per XCD turn
    int bwd_skip_dead = 1;        // the relayout of top_diff leaves out the bins that enter no list (round 4)
    int bwd_nchw_direct = 16;     // the list gather stores an NCHW bottom_diff itself (round 4): always for C <= 128, up to this
                                  // many bins per map pixel beyond; 0: never
};
#ifndef RROI_TUNING_QUALIFIER
#define RROI_TUNING_QUALIFIER constexpr
#endif
RROI_TUNING_QUALIFIER Tuning g_tune{};
// store policy of the backward's top_diff relayout (round 2 sweep, four runs: write-through (sc1) 163.4-165.9 us per
// call, streaming (nt) 166.8-168.8, plain 166.2-169.2): write-through leaves no dirty lines for the end of the launch
// to flush.  Non-temporal LOADS in the gather: +16 us.
constexpr int kBwdRelayoutAux = 16;

// Row pitch (pixels = 128-byte lines) of the chunk-major copy: W plus a pad that makes the
// pitch odd, so that the lines of vertically adjacent pixels differ in their low address
// bits and spread over the L2 channels.
int row_pitch(int width)
{
    if (g_tune.row_pad >= 0) return width + g_tune.row_pad;
    return width | 1;
}

// The shape of one call.  Every extern "C" entry point builds it once from its named arguments; everything behind the entry
// points takes it whole, and a plan (FwdDispatch / BwdDispatch) carries the Shape it was made for.  The bucketed calls:
// pooled_width is the call's largest width.
struct Shape {
    int batch_size, num_rois, height, width, channels, pooled_height, pooled_width;
    int NB() const { return pooled_height * pooled_width; }       // bins of a crop
    int HW() const { return height * width; }                     // pixels of a map
    int nchunks() const { return (channels + kChunk - 1) / kChunk; }
};

// lcm(nchunks, 8): a grid that is a multiple of it keeps block -> chunk -> XCD stable
inline long lcm8(int nchunks)
{
    long unit = nchunks;
    while (unit % 8) unit += nchunks;
    return unit;
}

bool shape_ok(const Shape& S)
{
    if (S.batch_size <= 0 || S.num_rois < 0 || S.height <= 0 || S.width <= 0 || S.channels <= 0 ||
        S.pooled_height <= 0 || S.pooled_width <= 0)
        return false;
    // tap offsets inside a slice are 32-bit BYTE offsets; the image stride is a 32-bit float count
    const long nchunks = S.nchunks();
    const long slice_px = (long)S.height * (S.width + 16) + 1;
    // tap offsets: < kQuadOOB = 2^30, so that (offset or kOOB) + (quad offset or kQuadOOB) never wraps
    if (slice_px * kLineBytes >= (1L << 30)) return false;                          // chunk-major
    if ((long)S.height * S.width * S.channels * 4 >= (1L << 30)) return false;      // channels-last
    if ((long)kChunk * S.pooled_height * S.pooled_width * 4 >= (1L << 31)) return false; // one output block
    if (slice_px * kChunk * nchunks >= (1L << 32)) return false;                    // img_stride
    if ((long)S.pooled_height * S.pooled_width >= (1L << 31)) return false;
    return true;
}

// grid for the tiled kernels: `per_cu` workgroups per CU (default: the 12 that 12.4 KB of LDS per workgroup admit; LDS is granted in 1280-byte granules, and a grid larger than the resident set would run its surplus
// blocks as a second, mostly empty round) and a multiple of lcm(nchunks, 8) so that blockIdx % nchunks is also
// stable per XCD.
int tiled_grid(long items, int nchunks, int per_cu = 0)
{
    long want = items * nchunks;
    const long cap = (long)num_cus() * (per_cu > 0 ? per_cu : g_tune.waves_per_cu);
    if (want > cap) want = cap;
    const long unit = lcm8(nchunks);
    long g = (want + unit - 1) / unit * unit;
    if (g < nchunks) g = nchunks;
    return (int)g;
}

// Blocks of a top_diff relayout over `tiles` tiles: one per pixel range (a block takes all chunks of its range), at most 8
// resident blocks per CU.
inline long relayout_blocks(long tiles, int nchunks)
{
    const long cap = (long)num_cus() * 8;
    return tiles / nchunks <= cap ? tiles / nchunks : cap;
}

void direct_grid(const Shape& S, dim3& grid, int& cslab)
{
    const int channels = S.channels;
    const long threads = (long)S.num_rois * S.NB();
    const int bx = ceil_div(threads, 256);
    // enough blocks to fill the chip a few times over, but keep slabs >= 4 channels
    int slabs = 1;
    const long target = (long)num_cus() * 8;
    while ((long)bx * slabs < target && channels / (slabs * 2) >= 4) slabs *= 2;
    cslab = ceil_div(channels, slabs);
    grid = dim3(bx, ceil_div(channels, cslab), 1);
}

// K2p, the direct path (rroi_fwd_patch_kernel): workgroup = (ROI, patch of up to 64 bins, four channel slabs of `cw` channels).
struct PatchPlan {
    int prows = 4, pcols = 16, npx = 0, npatches = 0, cw = 0;
    dim3 grid;
};
// Returns false where the form does not apply (the caller falls back to rounds 1-4's thread-per-bin kernel).
bool plan_patch_forward(const Shape& S, PatchPlan& p)
{
    const int num_rois = S.num_rois, channels = S.channels, pooled_height = S.pooled_height, pooled_width = S.pooled_width;
    const long NB = (long)pooled_height * pooled_width;
    if (!g_tune.fwd_patch || S.width < 2 || (long)num_rois * NB >= (1L << 30)) return false;
    // patch shape: rows x columns <= 64 with the fewest patches for this pooled size (ties: the wider rows -- longer store
    // runs); 11 x 96 -> 4 x 16 (18 patches), 11 x 83 -> 3 x 21 (16 instead of 18), 8 x 64 -> 4 x 16
    int prows = 4, pcols = 16;
    {
        long best = -1;
        // (at least three rows where the pooled height has them: a 1 x 64 or 2 x 32 patch is a long thin line of the map --
        // 11 x 128 with 1 x 64 patches: 11.0 us where 4 x 16 takes 8.6, although it needs two patches fewer)
        for (int r = std::min(3, pooled_height); r <= 8 && r <= pooled_height; ++r) {
            const int c = std::min(pooled_width, 64 / r);
            const long np = (long)ceil_div(pooled_height, r) * ceil_div(pooled_width, c);
            if (best < 0 || np < best || (np == best && c > pcols)) {
                best = np;
                prows = r;
                pcols = c;
            }
        }
    }
    const int npx = ceil_div(pooled_width, pcols), npatches = ceil_div(pooled_height, prows) * npx;
    long slabs = ceil_div((long)g_tune.fwd_patch_waves, (long)num_rois * npatches);
    if (slabs < 1) slabs = 1;
    int cw = (ceil_div(channels, slabs) + 3) / 4 * 4;
    if (cw > g_tune.fwd_patch_cwave) cw = g_tune.fwd_patch_cwave;
    const dim3 pgrid((unsigned)((long)num_rois * npatches), (unsigned)ceil_div(channels, 4 * cw), 1);
    if (pgrid.y > 65535u) return false;
    // (tools/patch_sweep.py: 2-8 K waves, 8-32 channels per wave, 4 or 8 in flight -- all within 0.3 us)
    p.prows = prows;
    p.pcols = pcols;
    p.npx = npx;
    p.npatches = npatches;
    p.cw = cw;
    p.grid = pgrid;
    return true;
}

FastDiv make_fastdiv(unsigned d)
{
    unsigned l = 0;
    while ((1ull << l) < d) ++l;
    FastDiv f;
    f.m = (unsigned)((((1ull << l) - d) << 32) / d + 1);
    f.sh1 = l < 1 ? l : 1;
    f.sh2 = l > 0 ? l - 1 : 0;
    return f;
}

PatchMap make_patch_map(int pooled_height, int pooled_width)
{
    unsigned pr = 1;   // rows of a patch: the largest power of two <= min(PH, 8)
    while (pr * 2 <= (unsigned)pooled_height && pr * 2 <= 8u) pr *= 2;
    PatchMap pm;
    pm.pc_shift = 0;
    while ((64u >> pm.pc_shift) > pr) ++pm.pc_shift;   // 64 / pr columns
    const unsigned pc = 1u << pm.pc_shift;
    const unsigned npy = ((unsigned)pooled_height + pr - 1) / pr;
    pm.npx = ((unsigned)pooled_width + pc - 1) / pc;
    pm.lanes_per_roi = npy * pm.npx * 64u;
    pm.div_roi = make_fastdiv(pm.lanes_per_roi);
    pm.div_npx = make_fastdiv(pm.npx);
    return pm;
}

// A caller's workspace: not NULL and a multiple of 256 bytes -- every sub-array of carve / carve_bwd sits at an
// align_up(..., 256) offset from it and is indexed as 16-byte vectors and 128-byte lines.  Beyond that the base address is
// free (carve_bwd's two roundings to 4 KiB of the address are in its size).
inline bool workspace_ok(const void* ws) { return ws && (reinterpret_cast<uintptr_t>(ws) & 255u) == 0; }

struct Workspace {
    Affine* aff;
    int* sort_rank;    // XCD groups: the counting sort's scratch and ...
    int* sort_order;   // ... its result, ROI index by sorted position (R ints each)
    float* cm;
    size_t cm_bytes;
    size_t bytes;
};

// XCD groups (XcdGroups, rroi_forward_kernels.h): G = 8 / nchunks groups per chunk for one or two chunks (C <= 64)
// and enough ROIs; else one group, the mapping of rounds 1-4
int forward_groups(int num_rois, int nchunks)
{
    // measured (tools/groups_ab.py, profiles/r05_groups_ab.txt; us per call, one group / G groups): C = 64, two
    // 120 x 160 maps, 11 x 96: R = 512 38.3 / 33.3, R = 128 19.0 / 15.2, R = 32 12.0 / 12.4 (the sort's block is the last of
    // its launch to finish: few ROIs keep one group); C = 128 (G = 2, a 3.3 MB slice per XCD already): 33.4 / 33.5
    // the same with the cheap sort (r05_groups_ab2.txt): R = 512 38.2 / 32.1 (11 x 83: 39.3 / 32.9, 11 x 100: 42.0 / 35.3), R = 64
    // 14.3 / 12.7, R = 32 12.0 / 12.1; eight 160 x 160 maps, R = 512, 11 x 100: 57.3 / 47.3.  ROIs bunched in a third of
    // one image: +0.5 us.  Crops beyond the 256 MB memory-side cache: with the HALF-line windows of the SHIFT form the sorted
    // order scattered a moment's half lines over the whole tensor (R = 2048, 11 x 100, 577 MB: 260 / 289) and the first
    // version kept one group there; stores of whole lines gain more beyond the cache than anywhere (tools/big_crops_probe.py,
    // profiles/r05_big_crops.txt: rows of whole sectors, eight 160 x 160 maps, R = 2048, 11 x 96, 528 MB: 152.7 / 117.9; the
    // line-aligned windows that such sizes now take, 11 x 100: 192-208 / 167, 11 x 83: 173-185 / 145-151) -- a (roi, chunk)
    // block's 135 KB leave one XCD together -- and between 256 and 320 MB the groups bring the merging form with them
    // (tools/shift_lines_threshold.py: 267 MB 80-86 / 66-67, 275 MB 73-85 / 73-75, eight maps 118-123 / 112): no size limit.
    if (!g_tune.fwd_groups || (nchunks != 1 && nchunks != 2)) return 1;
    const int G = 8 / nchunks;
    return num_rois >= g_tune.fwd_groups_min_rois ? G : 1;
}

// [affine table | sort rank | sort order | chunk-major copy (B, nchunks, HW+1, 32)]; the copy is absent when
// channels-last features with C % 4 == 0 are consumed in place.
Workspace carve(void* ws, const Shape& S, int layout)
{
    Workspace w;
    const size_t R = S.num_rois > 0 ? S.num_rois : 1;
    const size_t aff_bytes = align_up(R * sizeof(Affine), 256);
    const size_t sort_bytes = align_up(R * sizeof(int), 256);   // x 2: rank, order
    const size_t nchunks = S.nchunks();
    w.cm_bytes = layout == RROI_LAYOUT_NHWC
                     ? 0
                     : align_up((size_t)S.batch_size * nchunks * ((size_t)S.height * row_pitch(S.width) + 1) * kLineBytes, 256);
    w.aff = reinterpret_cast<Affine*>(ws);
    w.sort_rank = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + aff_bytes);
    w.sort_order = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + aff_bytes + sort_bytes);
    w.cm = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + aff_bytes + 2 * sort_bytes);
    w.bytes = aff_bytes + 2 * sort_bytes + w.cm_bytes;
    return w;
}

// backward: [affine | chunk-major gradient | pixel counters | pixel offsets | pairs |
//            top_diff relaid out to (R, NB, nchunks * 32)]
struct BwdWorkspace {
    Affine* aff;
    float* gcm;
    int* cnt;
    unsigned* off;
    unsigned* bsum;
    uint2* pairs;
    float* tdT;
    KeyLayout keys;
    unsigned scan_blocks;
    size_t gcm_bytes, cnt_bytes;
    size_t bytes;
    bool gather_ok;  // the gather formulation's 32-bit indices hold for this problem
    // one-pass lists (round 3): per-pixel buckets of 1 << kshift pairs in `pairs`, the overflow array behind
    // them, the chains' heads in `off`, the overflow counter in `bsum`
    bool bucket_ok, bucket_pref;
    unsigned kshift;
    uint4* ov;
};

BwdWorkspace carve_bwd(void* ws, const Shape& S)
{
    BwdWorkspace w;
    const int batch_size = S.batch_size, height = S.height, width = S.width, NB = S.NB();
    const size_t nchunks = S.nchunks();
    const size_t R = S.num_rois > 0 ? S.num_rois : 1;
    w.keys.Wt = (unsigned)((width + 7) / 8);
    w.keys.Ht = (unsigned)((height + 3) / 4);
    const size_t nkeys = (size_t)batch_size * w.keys.Ht * w.keys.Wt * 32;
    w.keys.keys = (unsigned)nkeys;
    w.scan_blocks = (unsigned)((nkeys + 1 + kScanBlock - 1) / kScanBlock);
    const size_t aff_bytes = align_up(R * sizeof(Affine), 256);
    w.gcm_bytes = align_up((size_t)batch_size * nchunks * height * row_pitch(width) * kLineBytes, 256);
    w.cnt_bytes = align_up(nkeys * sizeof(int), 256);
    const size_t off_bytes = align_up((nkeys + 1) * sizeof(unsigned), 256);
    const size_t bsum_bytes = align_up((size_t)w.scan_blocks * sizeof(unsigned), 256);
    // bucket capacity: ~3x the average list (about 2 pairs per bin over the map's pixels), a power of two from 16
    // up -- as far as the buckets stay within max(64 MB, twice the exact lists' bytes): only the entries in use are
    // ever read, a large bucket costs address space, not bandwidth.  Where that cap leaves the bucket below the
    // AVERAGE list, most of a list would live in the (slow) chains and AUTO / TILED keep count / scan / fill.
    const double avg = 2.0 * (double)R * NB / ((double)batch_size * height * width);
    const size_t bucket_cap = std::max<size_t>((size_t)64 << 20, 2 * 4 * R * NB * sizeof(uint2));
    w.kshift = 4;
    while ((1u << w.kshift) < 3.0 * avg && w.kshift < 12 && (nkeys << (w.kshift + 1)) * sizeof(uint2) <= bucket_cap)
        ++w.kshift;
    w.bucket_pref = (double)(1u << w.kshift) >= avg;
    w.bucket_ok = (nkeys << w.kshift) < (1ull << 32) && 4 * R * NB < (1ull << 31);
    const size_t bucket_bytes = w.bucket_ok ? align_up((nkeys << w.kshift) * sizeof(uint2), 256) : 0;
    const size_t ov_bytes = w.bucket_ok ? align_up(4 * R * NB * sizeof(uint4), 256) : 0;
    const size_t pair_bytes = std::max(align_up(4 * R * NB * sizeof(uint2), 256), bucket_bytes + ov_bytes);
    const size_t td_bytes = align_up(R * (size_t)NB * nchunks * kLineBytes, 256);   // (R, NB, nchunks * 32)
    // pair slots, top_diff line indices and keys are 32-bit; the gather launches one thread group per key
    // ... and its thread index (key * lanes-per-pixel, at most 64) and block index are 32-bit too
    w.gather_ok = 4 * R * NB < (1ull << 32) && R * (size_t)NB < (1ull << 32) &&
                  (size_t)NB * nchunks * kLineBytes < (1ull << 32) && nkeys * 64 < (1ull << 32) && nkeys < (1ull << 31);
    char* b = reinterpret_cast<char*>(ws);
    w.aff = reinterpret_cast<Affine*>(b);
    b += aff_bytes;
    w.gcm = reinterpret_cast<float*>(b);
    b += w.gcm_bytes;
    w.cnt = reinterpret_cast<int*>(b);
    b += w.cnt_bytes;
    w.off = reinterpret_cast<unsigned*>(b);
    b += off_bytes;
    w.bsum = reinterpret_cast<unsigned*>(b);
    b += bsum_bytes;
    // the big arrays start on 4 KiB boundaries of the ADDRESS: a bin's run of the pixel-major copy (nchunks x 128 B) then
    // never straddles a page, whatever the small arrays in front add up to (round 5, tools/experiments/
    // r05_clean_workspace_backward: with the copy 256 B further on configs[2]'s list launch took 84 us instead of 74;
    // page-aligned the call is 2 us faster than round 4's layout)
    auto page_up = [](char* p) { return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(p) + 4095u) & ~(uintptr_t)4095u); };
    b = page_up(b);
    w.pairs = reinterpret_cast<uint2*>(b);
    w.ov = reinterpret_cast<uint4*>(b + bucket_bytes);
    b = page_up(b + pair_bytes);
    w.tdT = reinterpret_cast<float*>(b);
    b += td_bytes;
    // (+ 2 x 4 KiB: the two roundings, whatever the caller's base address is)
    w.bytes = aff_bytes + w.gcm_bytes +
              (w.gather_ok ? w.cnt_bytes + off_bytes + bsum_bytes + pair_bytes + td_bytes + 8192 : 0);
    return w;
}

// AUTO.  The tiled paths have a fixed cost (forward: two launches; backward: three) plus a term in the size of the
// whole map (relayout; the backward also visits every pixel); the direct paths cost per output element, the
// backward's with four float atomics.
// Measured crossovers (MI355X; forward: round 5, tools/fused_probe.py, us per call between events, direct = K2p):
//   forward   C=64 two 120x160 maps 11x96:  R=32 direct 8.8 / tiled 12.1,  R=48 12.7 / 13.4,  R=64 13.5 / 13.0,  R=128 21.9 / 14.9
//             C=256 160x160 8x64:  R=8 direct 6.1 / fused 7.3 / tiled 13.9,  R=16 11.5 / 9.7 / 14.4,  R=32 22.1 / 16.0 / 15.5
//   (rounds 1-4, tools/crossover.py, wall time per call:)
//   backward  C=256:  R=4 direct 59 / tiled 43,   R=32 448 / 50,   R=512 7145 / 195
//             C=64:   R=4 direct 15 / tiled 34,   R=16 105 / 39,   R=512 1745 / 113
bool pick_tiled_fwd(const Shape& S)
{
    const double out_elems = (double)S.num_rois * S.channels * S.NB();
    const double map_elems = (double)S.batch_size * S.channels * S.height * S.width;
    return out_elems >= g_tune.fwd_tiled_min_elems && out_elems >= map_elems / 4;
}
// Below the two-launch path's crossover: the one-launch gather from the NCHW map (RROI_PATH_FUSED) or the direct path's
// patch kernel (K2p)?  Measured (tools/fused_probe.py, profiles/r05_fused_probe.txt; us per call, K2p / fused / two-launch):
//   C = 64, two 120 x 160 maps, 11 x 96:  R = 8  4.9 / 6.4 / 10.9,  16  7.3 / 7.9 / 11.0,  32  8.9 / 11.7 / 12.1,  64  12.7 / 17.9 / 13.0
//   C = 128, 160 x 160, 8 x 64:           R = 32  10.9 / 8.2 / 11.5
//   C = 256, 160 x 160, 8 x 64:           R = 8  6.5 / 7.4 / 13.9,  16  11.6 / 9.7 / 14.4,  32  21.0 / 16.1 / 15.5
// Both one-launch forms pay per output element (K2p three vector-memory instructions and ~16 VALU per 64 bin-channels, the
// fused form four dword loads per tap but one 16-byte store and one blend per FOUR channels) and meet at ~1.5 M elements;
// the fused form wins from there up to the two-launch crossover WHEN THERE ARE CHANNELS TO AMORTISE ITS ITEMS OVER: C >= 128.
// At the reference's own C = 64 K2p stays ahead up to the two-launch path (profiles/r05_small_r_forward.md).
bool pick_fused_fwd(const Shape& S)
{
    const double out_elems = (double)S.num_rois * S.channels * S.NB();
    return g_tune.fwd_fused && S.channels >= g_tune.fwd_fused_min_channels && out_elems >= g_tune.fwd_fused_min_elems;
}
bool pick_tiled_bwd(const Shape& S)
{
    const double out_elems = (double)S.num_rois * S.channels * S.NB();
    const double map_elems = (double)S.batch_size * S.channels * S.height * S.width;
    // the scatter's cost is the memset of the map plus its atomics: with the one-pass lists (round 3) the gather
    // wins from ~0.2 M gradient elements up (one 64 x 176 x 320 map, R = 4, 0.27 M: 26-27 us whatever the draw, the
    // scatter 18.6 or 41.4 depending on how the four ROIs overlap), and below that wherever the map alone is 8 M
    // elements (eight 64 x 160 x 160 maps, R = 4: 41.7 against 48.0 us); tools/crossover.py, tools/bucket_ab.py
    // ... unless the map dwarfs the gradient: the gather path moves the whole map three times (chunk-major gradient
    // written, read back, written as NCHW), the scatter once (its memset), and the scatter's atomics cost ~110 us
    // per million gradient elements (R = 16, C = 256: 250 us for 2.1 M)
    if (2.0 * map_elems * 4.0 / 7.0e6 > 110.0 * out_elems / 1.0e6 - 21.0 && map_elems >= 32.0e6) return false;
    return out_elems >= 0.2e6 || map_elems >= 8.0e6;
}

// ------------------------------------------------------------------------------------
// Which instantiation of rroi_fwd_split_kernel gathers a problem, with what grid and flags.
// ------------------------------------------------------------------------------------
enum class FwdKernel {
    kStrided,        // every n-th (roi, tile) item per workgroup, 16-byte stores: crops whose rows are whole sectors
    kChannelsLast,   // channels-last crops (R, PH, PW, C)
    kShift,          // SHIFT: overlapped tiles, sector-aligned store windows -- crops whose rows are not whole sectors
    kStridedMerge,   // strided tiles on rows that are not whole sectors, plain stores: the XCD's L2 merges the partial sectors (XCD groups only)
    kShiftLines,     // SHIFT == 2: line-aligned windows (32 own bins of 64 gathered) -- such crops beyond the memory-side cache
    kStridedRagged,  // the bucketed call's gather (launch_forward_bucketed): strided tiles of the widest crop, one width per ROI
};
// a plan reports its kernel as the enumerator's value
static_assert((int)FwdKernel::kStrided == RROI_PLAN_KERNEL_STRIDED && (int)FwdKernel::kShiftLines == RROI_PLAN_KERNEL_SHIFT_LINES &&
              (int)FwdKernel::kStridedRagged == RROI_PLAN_KERNEL_STRIDED_RAGGED, "rroi_align_plan.kernel");
struct ForwardPlan {
    FwdKernel kernel;
    int grid;
    int ntiles;   // tiles per (roi, chunk) block: ceil(NB / 64), SHIFT: ceil(NB / 48)
    int dbg;      // the kernel's flag word (see its header comment)
};

constexpr int kShiftWgsPerCu = 12;   // the SHIFT instantiation: <= 80 VGPRs under __launch_bounds__(128, 6), 12.4 KB of LDS
constexpr int kShiftOwnBins = kTileBins - 16;   // bins a SHIFT tile advances by (it gathers 64: kOwnBins in the kernel)

// allow_lines = false: the one-launch NCHW_SRC form has no SHIFT == 2 instantiation -- rows that are not whole sectors
// take kShift there at any size (the plan used to return kShiftLines beyond 320 MB, which the fused launch
// then ran as SHIFT = 0 on a grid sized for 32-bin tiles)
// elem_bytes: bytes of one crop element (4, or 2 for bfloat16 / float16 crops).  The two rules below that stand for BYTES
// of crops (the merging form from 48 MB, the line-aligned windows beyond the 320 MB memory-side cache) use it: 16-bit crops
// reach them at twice the elements.  Every other size rule of the dispatch counts ELEMENTS (or the fp32 workspace's bytes).
ForwardPlan plan_forward_gather(const Shape& S, bool out_nhwc, bool launcher_rest, int groups = 1,
                                size_t map_bytes_per_xcd = 0, bool allow_lines = true, size_t elem_bytes = sizeof(float))
{
    const int num_rois = S.num_rois, channels = S.channels, NB = S.NB(), nchunks = S.nchunks();
    const int base_dbg = (g_tune.fwd_dbg & ~0xe0) | (launcher_rest ? 32 : 0);   // bits 5-7 are the host's
    const int ntiles = ceil_div(NB, kTileBins);
    if (out_nhwc)   // (91 VGPRs -> five waves per SIMD: 10 workgroups per CU are resident, and no more are launched)
        return {FwdKernel::kChannelsLast, tiled_grid((long)num_rois * ntiles, nchunks, 10), ntiles, g_tune.fwd_dbg & ~0xe0};
    // Crops whose rows are not whole 64-byte sectors (PH * PW % 16 != 0) take the SHIFT form: sector-aligned store windows
    // over OVERLAPPED tiles (a tile advances by 48 bins and gathers 64, rroi_forward_kernels.h), items dealt every n-th
    // like the strided form's.  It costs 4 / 3 of the gather work per byte and was never slower than the strided items on
    // such crops, from R = 8 to R = 2048 (tools/align_probe.py, profiles/r04_align_probe.txt: R = 32, C = 64, 11 x 83: 6.6
    // against 9.4 us; R = 128, 11 x 100: 13.7 against 16.5; R = 512, 11 x 83: 40 against 209)
    // Round 5: beyond the 256 MB memory-side cache a half line reaches HBM as a half line -- the SHIFT
    // form's store stream ALONE runs at 3.1 TB/s there (tools/big_crops_ablate.py).  SHIFT == 2 stores whole LINES: a tile
    // advances by 32 bins and gathers 64 (twice the gather work per byte instead of 4 / 3).  tools/shift_lines_ab.py,
    // profiles/r05_shift_lines.txt (us per call, SHIFT / lines): eight 160 x 160 maps, C = 64, R = 2048, 11 x 100 (550 MB) 255 / 191;
    // two 120 x 160 maps, 11 x 83: R = 2048 (456 MB) 172 / 141, R = 4096 (913 MB) 358 / 272; C = 256, 11 x 50, R = 1024 (550 MB)
    // 251 / 176; 11 x 100, R = 600 (645 MB) 215 / 183.  Around the cache's size it is a draw or worse (267-275 MB: 80 / 87,
    // 73 / 87, 104 / 93, 76 / 83; 322-334 MB: 105 / 97, 112 / 108): from 320 MB up.
    if (allow_lines && NB % 16 != 0 && (g_tune.fwd_shift_lines == 2 ||
                         (g_tune.fwd_shift_lines == 1 && (size_t)num_rois * channels * NB * elem_bytes > ((size_t)320 << 20)))) {   // bytes
        const int nt = ceil_div(NB, kTileBins - 32);
        return {FwdKernel::kShiftLines, tiled_grid((long)num_rois * nt, nchunks, g_tune.shift_lines_wgs_per_cu), nt, base_dbg};
    }
    // Round 5, with XCD groups: ALL tiles of a (roi, chunk) block go through ONE XCD at about the same time, so the partial
    // sectors that strided tiles leave at their ends on rows that are not whole sectors meet in that XCD's L2 -- if the
    // stores are plain (write-back) instead of streamed.  Then such crops need no SHIFT form (4 / 3 of the items): strided
    // tiles, 16-byte stores at dword alignment, a row's last <= 3 dwords in its last tile (WAUX = 0 in the kernel).
    // tools/merge_ab.py, profiles/r05_merge_ab.txt (us per call, SHIFT / merging): C = 64, two 120 x 160 maps, R = 512: 11 x 83
    // 32.9 / 30.1, 11 x 84 32.2 / 29.6, 11 x 91 34.5 / 33.0, 11 x 100 35.4 / 34.8; C = 32 20.9 / 19.9.  It needs the L2 room:
    // R = 128 15.7 / 15.6, R = 64 12.5 / 13.1, eight 160 x 160 maps (6.6 MB of map per XCD) 47.1 / 49.8 -- so: XCD groups, at
    // least 48 MB of crops, at most 2 MB of the chunk-major copy per XCD.
    if (g_tune.fwd_merge && groups > 1 && NB % 16 != 0 && (g_tune.fwd_merge > 1 ||
        ((size_t)num_rois * channels * NB * elem_bytes >= ((size_t)48 << 20) && map_bytes_per_xcd <= ((size_t)2 << 20))))   // bytes
        return {FwdKernel::kStridedMerge, tiled_grid((long)num_rois * ntiles, nchunks, g_tune.split_wgs_per_cu), ntiles, base_dbg};
    if (NB % 4 != 0 || (g_tune.fwd_shift && (NB % 16 != 0 || g_tune.fwd_shift == 2))) {   // (rows of dwords: always)
        const int wpc = g_tune.shift_wgs_per_cu > 0 ? g_tune.shift_wgs_per_cu : kShiftWgsPerCu;
        const int nt = ceil_div(NB, kShiftOwnBins);
        return {FwdKernel::kShift, tiled_grid((long)num_rois * nt, nchunks, wpc), nt, base_dbg};
    }
    return {FwdKernel::kStrided, tiled_grid((long)num_rois * ntiles, nchunks, g_tune.split_wgs_per_cu), ntiles, base_dbg};
}

// ------------------------------------------------------------------------------------
// The dispatch.  One function per direction decides what a call launches, down to every grid; the launches
// (rroi_host_launch.h) run its fields and the plan query (rroi_align_forward_plan / rroi_align_backward_plan) reports
// them, so the two cannot disagree.  Host only: no launch, no memory touched (the backward's workspace is carved at
// address 0 for its sizes).
// ------------------------------------------------------------------------------------
bool caller_ok(int caller, bool con_idx_allowed)
{
    return caller == RROI_CALLER_NATIVE || caller == RROI_CALLER_LAUNCHER ||
           (con_idx_allowed && caller == RROI_CALLER_LAUNCHER_CON_IDX);
}

inline bool dtype_ok(int dtype) { return dtype == RROI_DTYPE_FP32 || dtype == RROI_DTYPE_BF16 || dtype == RROI_DTYPE_FP16; }
inline size_t dtype_bytes(int dtype) { return dtype == RROI_DTYPE_FP32 ? 4 : 2; }

// The forward prologue launch (rroi_prologue_kernel): [relayout blocks | affine blocks | the ROI sort's block (XCD groups) |
// the launcher's rest blocks, one per ROI].
struct ProloguePlan {
    int ptiles = 0;            // pixel tiles of one (image, chunk) slice
    int relayout_tiles = 0;    // ... in all (0: channels-last features consumed in place)
    int relayout_blocks = 0, aff_blocks = 0, sort_blocks = 0, rest_blocks = 0;
    int grid() const { return relayout_blocks + aff_blocks + sort_blocks + rest_blocks; }
};
ProloguePlan plan_prologue(const Shape& S, bool zero_copy, int groups, bool launcher_rest)
{
    const int nchunks = S.nchunks();
    ProloguePlan p;
    p.ptiles = ceil_div(S.HW(), kRelayoutPx);
    p.relayout_tiles = zero_copy ? 0 : p.ptiles * nchunks * S.batch_size;
    // ~3 resident blocks per CU, each streaming several tiles with the next tile prefetched
    int relayout_blocks = p.relayout_tiles;
    if (groups > 1) relayout_blocks = (relayout_blocks + 7) / 8 * 8;   // whole XCD rounds (a block without a tile leaves)
    if (relayout_blocks > num_cus() * g_tune.prologue_blocks_per_cu) {
        relayout_blocks = num_cus() * g_tune.prologue_blocks_per_cu;
        const long unit = lcm8(nchunks);   // keeps block -> chunk -> XCD stable
        if (relayout_blocks >= unit) relayout_blocks = (int)(relayout_blocks / unit * unit);
    }
    p.relayout_blocks = relayout_blocks;
    p.aff_blocks = ceil_div(S.num_rois, 256);
    p.sort_blocks = groups > 1 ? 1 : 0;
    p.rest_blocks = launcher_rest ? S.num_rois : 0;
    return p;
}

struct FwdDispatch {
    int status = 0;                  // 1: the call launches this plan; 0: it refuses its arguments
    Shape shape{};                   // what the plan was made for, and what its launch runs on (the launcher's: batch 1)
    int family = RROI_PLAN_NONE;
    int trig = RROI_TRIG_DOUBLE;
    bool launcher = false;           // the reference-ABI launcher: ROIs of images >= 1 by the prologue (launcher_rest) ...
    bool con_idx = false;            // ... and con_idx written
    bool out_nhwc = false, zero_copy = false;
    int groups = 1;
    ProloguePlan prologue;           // two-launch
    ForwardPlan gather{FwdKernel::kStrided, 0, 0, 0};   // fused / two-launch
    PatchPlan patch;                 // K2p
    dim3 dgrid;                      // thread-per-bin kernel; the launcher's con_idx kernel
    int cslab = 0;
    int direct_batch() const { return launcher ? -1 : shape.batch_size; }   // (the launcher's signature has no batch count)
};

// dtype (0.10.0): the element type of the map and the crops.  A 16-bit call is native-only, reads NCHW
// features, and never takes the one-launch NCHW_SRC form; where an fp32 AUTO call would take it, a 16-bit call runs K2p.
FwdDispatch plan_forward(const Shape& shape, int feature_layout, int top_layout, int path, int caller, int dtype)
{
    FwdDispatch P;
    P.shape = shape;
    const Shape& S = P.shape;
    if (!caller_ok(caller, true) || !dtype_ok(dtype)) return P;
    const bool half = dtype != RROI_DTYPE_FP32;
    if (half && (caller != RROI_CALLER_NATIVE || feature_layout != RROI_LAYOUT_NCHW ||
                 (path & 0xff) == RROI_PATH_FUSED))
        return P;
    // unknown flag bits (RROI_PATH_DETERMINISTIC among them: a backward flag -- the forward is deterministic as it is)
    if (path & ~(0xff | RROI_PATH_TRIG_FP32)) return P;
    P.trig = (path & RROI_PATH_TRIG_FP32) ? RROI_TRIG_FP32 : RROI_TRIG_DOUBLE;
    path &= 0xff;
    P.launcher = caller != RROI_CALLER_NATIVE;
    P.con_idx = caller == RROI_CALLER_LAUNCHER_CON_IDX;
    if (P.launcher) {
        // the launcher's signature: NCHW in and out, no path, no batch count -- the tiled path knows image 0 only
        if (feature_layout != RROI_LAYOUT_NCHW || top_layout != RROI_LAYOUT_NCHW || path != RROI_PATH_AUTO) return P;
        P.shape.batch_size = 1;
        if (!shape_ok(S)) return P;
        P.status = 1;
        if (S.num_rois == 0) return P;
        direct_grid(S, P.dgrid, P.cslab);
        if (!pick_tiled_fwd(S)) {
            P.family = plan_patch_forward(S, P.patch) ? RROI_PLAN_FWD_DIRECT_K2P : RROI_PLAN_FWD_DIRECT_THREAD;
            return P;
        }
        P.status = 0;
        path = RROI_PATH_TILED;
    }
    if (top_layout != RROI_LAYOUT_NCHW && top_layout != RROI_LAYOUT_NHWC) return P;
    P.out_nhwc = top_layout == RROI_LAYOUT_NHWC;
    // channels-last crops are written by the tiled kernel only: 16-byte channel quads
    if (P.out_nhwc && (S.channels % 4 != 0 || path == RROI_PATH_DIRECT ||
                       (long)S.pooled_height * S.pooled_width * S.channels * 4 >= (1L << 31)))
        return P;
    if (!shape_ok(S)) return P;
    if (feature_layout != RROI_LAYOUT_NCHW && feature_layout != RROI_LAYOUT_NHWC) return P;
    if (path != RROI_PATH_AUTO && path != RROI_PATH_DIRECT && path != RROI_PATH_TILED && path != RROI_PATH_FUSED) return P;
    if (S.num_rois == 0) {
        P.status = 1;
        return P;
    }

    bool tiled;
    if (P.out_nhwc)
        tiled = true;
    else if (path == RROI_PATH_AUTO)
        tiled = feature_layout == RROI_LAYOUT_NHWC || pick_tiled_fwd(S);
    else
        tiled = path == RROI_PATH_TILED;
    // the one-launch form for few ROIs (the gather reading the NCHW map itself): NCHW in, NCHW out, not for the launcher,
    // fp32 only.  A 16-bit call in its range stays on the direct path (K2p), which was never slower than the two-launch
    // path there (tools/half_bench.py, profiles/half_precision.md; us per call, bf16 K2p / two-launch, back-to-back calls
    // from Python): C = 256, 160 x 160, 8 x 64, R = 12 15.1 / 19.0, 16 15.0 / 18.7, 24 15.3 / 19.1, 28 15.5 / 19.2;
    // C = 128, 11 x 50, R = 24 15.4 / 18.9, 32 14.7 / 18.6, 48 15.6 / 18.2 (fp32 AUTO, fused: 16.2 ... 34.2)
    const bool fused = !half && !P.launcher && !P.out_nhwc && feature_layout == RROI_LAYOUT_NCHW &&
                       (path == RROI_PATH_FUSED || (path == RROI_PATH_AUTO && !tiled && pick_fused_fwd(S)));
    if (path == RROI_PATH_FUSED && !fused) return P;
    if (fused) {
        P.gather = plan_forward_gather(S, false, false, 1, 0, /*allow_lines*/ false);
        if (P.gather.kernel != FwdKernel::kShift && P.gather.kernel != FwdKernel::kStrided) return P;   // the two forms NCHW_SRC has
        if ((long)S.num_rois * P.gather.ntiles >= (1L << 31)) return P;
        P.family = P.gather.kernel == FwdKernel::kShift ? RROI_PLAN_FWD_FUSED_SHIFT : RROI_PLAN_FWD_FUSED_STRIDED;
        P.status = 1;
        return P;
    }
    if (!tiled) {
        if (feature_layout != RROI_LAYOUT_NCHW) return P;  // direct path reads NCHW only
        if (plan_patch_forward(S, P.patch)) {
            P.family = RROI_PLAN_FWD_DIRECT_K2P;
        } else {
            P.family = RROI_PLAN_FWD_DIRECT_THREAD;
            direct_grid(S, P.dgrid, P.cslab);
        }
        P.status = 1;
        return P;
    }
    if (feature_layout == RROI_LAYOUT_NHWC && S.channels % 4 != 0) return P;  // repack to NCHW first
    P.zero_copy = feature_layout == RROI_LAYOUT_NHWC;
    P.groups = P.launcher ? 1 : forward_groups(S.num_rois, S.nchunks());
    P.prologue = plan_prologue(S, P.zero_copy, P.groups, P.launcher);
    const size_t map_bytes_per_xcd = P.zero_copy ? (size_t)S.batch_size * S.height * S.width * S.channels * 4 / 8
                                                 : carve(nullptr, S, feature_layout).cm_bytes / 8;
    P.gather = plan_forward_gather(S, P.out_nhwc, P.launcher, P.groups, map_bytes_per_xcd, true, dtype_bytes(dtype));
    if ((long)S.num_rois * P.gather.ntiles >= (1L << 31)) return P;
    P.family = RROI_PLAN_FWD_TWO_LAUNCH;
    P.status = 1;
    return P;
}

struct BwdDispatch {
    int status = 0;                  // 1: the call launches this plan; 0: it refuses its arguments
    Shape shape{};                   // what the plan was made for, and what its launch runs on
    int family = RROI_PLAN_NONE;
    int trig = RROI_TRIG_DOUBLE;
    int dest = RROI_PLAN_DST_NONE;
    bool td_nhwc = false, accumulate = false;
    BwdWorkspace ws{};               // carved at address 0: sizes, key layout, bucket shift
    dim3 grid;                       // the main kernel's
    int affine_blocks = 0;           // every tiled family: the affine table's launch, which also clears the lists' pixel counters
    struct Direct {
        int cslab = 0;
    } direct;
    struct Atomic {
        int ntiles = 0;
        bool vec4 = false;           // rroi_bwd_tiled_kernel<true> (NB % 4 == 0)
    } atomic;
    struct InKernel {
        int nk = 0;
        int tt = 0;                  // top_diff relayout tiles per (roi, chunk) ...
        long tiles = 0;              // ... and in all
        long relayout_blocks = 0;    // the relayout of top_diff (0: consumed in place)
        int flags = 0;               // ... its flag word: bit 0 dead bins are not copied
    } inkernel;
    struct Lists {                   // LISTS, BUCKETS and ORDERED
        int raw_bsum = -1;
        int pblocks = 0;             // pair blocks in front of each relayout launch ...
        int flags = 0;               // ... their flag word: bit 0 dead bins are not copied, bit 1 reservations aggregated per wave
        int tt = 0;                  // top_diff relayout tiles per (roi, chunk) ...
        long tiles = 0, half = 0;    // ... in all; the count launch's share
        long count_blocks = 0, fill_blocks = 0, bucket_blocks = 0;   // relayout blocks of the count, fill and bucket launches
        unsigned sub_shift = 0, gy = 0, tile_run = 0;
        int sort_lists_blocks = 0, sort_queue_blocks = 0;   // ORDERED's two sort launches
    } lists;
};

// accumulate (the reference-ABI launcher, tiled NCHW paths only): bottom_diff += gradient instead of = gradient
// AUTO / TILED choose among the gathers; LISTS and INKERNEL name one
static inline bool gather_choice_is_open(int path)
{
    return path != RROI_PATH_TILED_LISTS && path != RROI_PATH_TILED_INKERNEL;
}

// dtype (0.10.0): the element type of top_diff and bottom_diff.  A 16-bit call is native-only, reads an
// NCHW top_diff, and runs one of the three gathers (never the fp32-atomic DIRECT / ATOMIC forms): AUTO takes the gather
// TILED would take, and a problem no gather can index is refused.
// RROI_PATH_DETERMINISTIC: native AUTO calls only; every R >= 1 runs ORDERED -- the exact lists, sorted,
// and the in-order fp64 gather, written in place in either layout -- where the gather can index the problem.
// ragged (the bucketed call): pooled_width is the call's largest width; the gradient crops are NCHW, the
// caller is native, and the plan is one of the list gathers -- LISTS (named), BUCKETS (named, or where AUTO prefers them),
// ORDERED (RROI_PATH_DETERMINISTIC) -- whatever the size: the in-kernel gather and the fp32-atomic forms have no ragged
// form, so AUTO never returns them and every other path is refused.
BwdDispatch plan_backward(const Shape& S, int top_diff_layout, int bottom_diff_layout, int path, int caller, int dtype,
                          bool ragged = false)
{
    BwdDispatch P;
    P.shape = S;
    const int batch_size = S.batch_size, num_rois = S.num_rois, channels = S.channels;
    if (!caller_ok(caller, false) || !dtype_ok(dtype)) return P;
    if (ragged) {
        const int named = path & 0xff;
        if (caller != RROI_CALLER_NATIVE || top_diff_layout != RROI_LAYOUT_NCHW ||
            (named != RROI_PATH_AUTO && named != RROI_PATH_TILED_LISTS && named != RROI_PATH_TILED_BUCKETS))
            return P;
    }
    const bool half = dtype != RROI_DTYPE_FP32;
    if (half && (caller != RROI_CALLER_NATIVE || top_diff_layout != RROI_LAYOUT_NCHW ||
                 (path & 0xff) == RROI_PATH_DIRECT || (path & 0xff) == RROI_PATH_TILED_ATOMIC))
        return P;
    if (path & ~(0xff | RROI_PATH_TRIG_FP32 | RROI_PATH_DETERMINISTIC)) return P;   // unknown flag bits
    const bool ordered = (path & RROI_PATH_DETERMINISTIC) != 0;
    if (ordered && (caller != RROI_CALLER_NATIVE || (path & 0xff) != RROI_PATH_AUTO)) return P;
    P.trig = (path & RROI_PATH_TRIG_FP32) ? RROI_TRIG_FP32 : RROI_TRIG_DOUBLE;
    path &= 0xff;
    if (caller == RROI_CALLER_LAUNCHER) {
        if (top_diff_layout != RROI_LAYOUT_NCHW || bottom_diff_layout != RROI_LAYOUT_NCHW || path != RROI_PATH_AUTO) return P;
        if (!shape_ok(S)) return P;
        P.accumulate = true;
        P.status = 1;
        if (num_rois == 0) return P;   // nothing to add
        if (!pick_tiled_bwd(S)) {
            P.family = RROI_PLAN_BWD_LITERAL;
            P.dest = RROI_PLAN_DST_NCHW_ADD;
            const long nthreads = (long)num_rois * S.pooled_height * S.pooled_width * channels;
            long blocks = (nthreads + 255) / 256;
            const long cap = (long)num_cus() * 32;
            if (blocks > cap) blocks = cap;
            P.grid = dim3((unsigned)blocks);
            return P;
        }
        P.status = 0;
        path = RROI_PATH_TILED;
    }
    if (top_diff_layout != RROI_LAYOUT_NCHW && top_diff_layout != RROI_LAYOUT_NHWC) return P;
    if (bottom_diff_layout != RROI_LAYOUT_NCHW && bottom_diff_layout != RROI_LAYOUT_NHWC) return P;
    const bool td_nhwc = top_diff_layout == RROI_LAYOUT_NHWC, bd_nhwc = bottom_diff_layout == RROI_LAYOUT_NHWC;
    P.td_nhwc = td_nhwc;
    // channels-last tensors are read / written in place by the gather formulation only
    if ((td_nhwc || bd_nhwc) &&
        (channels % 4 != 0 || path == RROI_PATH_DIRECT || path == RROI_PATH_TILED_ATOMIC))
        return P;
    if (!shape_ok(S)) return P;
    if (path != RROI_PATH_AUTO && path != RROI_PATH_DIRECT && path != RROI_PATH_TILED &&
        path != RROI_PATH_TILED_ATOMIC && path != RROI_PATH_TILED_LISTS && path != RROI_PATH_TILED_INKERNEL &&
        path != RROI_PATH_TILED_BUCKETS)
        return P;
    if (num_rois == 0) {   // bottom_diff zeroed
        P.status = 1;
        return P;
    }
    const int NB = S.NB(), HW = S.HW();
    const bool accumulate = P.accumulate;
    const bool tiled = ragged || ordered || half || td_nhwc || bd_nhwc ||
                       (path == RROI_PATH_AUTO ? pick_tiled_bwd(S) : path != RROI_PATH_DIRECT);
    if (accumulate && (!tiled || bd_nhwc)) return P;
    const int nchunks = S.nchunks();
    if (!tiled) {
        direct_grid(S, P.grid, P.direct.cslab);
        P.family = RROI_PLAN_BWD_DIRECT;
        P.dest = RROI_PLAN_DST_NCHW;
        P.status = 1;
        return P;
    }

    const BwdWorkspace ws = carve_bwd(nullptr, S);
    P.ws = ws;
    if ((td_nhwc || bd_nhwc) && (!ws.gather_ok || (size_t)num_rois * NB >= (1ull << 32))) return P;
    if (half && !ws.gather_ok) return P;   // (the atomic scatter, an fp32 call's fallback, has no 16-bit form)
    if (ordered && !ws.gather_ok) return P;   // (... nor an ordered one)
    if (ragged && !ws.gather_ok) return P;    // (... nor a ragged one)
    const bool gather = path != RROI_PATH_TILED_ATOMIC && ws.gather_ok;
    // Two gathers.  K3t builds the pixel lists inside the gather kernel (rroi_backward_tile_kernels.h), K3g
    // with count / scan / fill launches in HBM.  Measured (tools/crossover.py, MI355X, us per call,
    // K3t / K3g): C = 64, 176x320 map, 11x96: R = 4 26 / 33, 32 31 / 37, 128 41 / 49, 512 88 / 98;  C = 64,
    // 8 images of 160x160, 11x100: 45 / 51, 54 / 54, 68 / 72, 133 / 148;  C = 256, 160x160, 8x64: 39 / 39,
    // 43 / 40, 77 / 62, 201 / 168 -- K3t's serial work per tile is hidden when a lane carries two
    // channel chunks, not when it carries eight.  K3t addresses its source with 32-bit byte offsets.
    const size_t src_bytes = td_nhwc ? (size_t)num_rois * NB * channels * 4
                                     : (size_t)num_rois * NB * nchunks * kLineBytes;
    const bool inkernel_ok = src_bytes < (1ull << 32);
    if (path == RROI_PATH_TILED_INKERNEL && !(gather && inkernel_ok)) return P;
    // ... with four chunks per lane (C <= 128) it still wins where the lists are short: C = 128, 160x160,
    // 8x64: R = 32 33 / 42, 128 48 / 48, 512 101 / 93;  C = 96, 176x320, 11x96: 38 / 45, 56 / 61, 114 / 122
    const bool short_lists = (double)num_rois * NB <= 8.0 * (double)batch_size * HW;   // bins per map pixel
    // every map tile's workgroup scans ALL the ROIs (in batches of 256): O(tiles x R), measured up to R = 512
    // and 8 images -- beyond that the lists in HBM, whose cost does not grow that way, are the safe choice
    const bool scan_ok = (double)num_rois * batch_size <= 8192.0;
    // round 3 (profiles/r03_crossover.txt): up to 256 channels it also wins while there is at most one bin per map
    // pixel -- C = 256, 160 x 160, 8 x 64: R = 4 45.9 / 52.8, 16 49.5 / 52.5, 32 49.7 / 53.7, 64 56.9 / 57.4, 128 78.3 / 65.5
    const bool very_short = (double)num_rois * NB <= 1.0 * (double)batch_size * HW;
    const bool prefer_inkernel = scan_ok && (nchunks <= 2 || (nchunks <= 4 && short_lists) || (nchunks <= 8 && very_short));
    if (path == RROI_PATH_TILED_BUCKETS && !(gather && ws.bucket_ok)) return P;
    // Round 3: the lists in HBM built in ONE pass over the bins (fixed buckets of 2^kshift entries per pixel plus
    // overflow chains, rroi_backward_kernels.h) instead of count / scan / fill.  Measured (tools/crossover.py,
    // tools/bucket_ab.py, profiles/r03_crossover_buckets.txt; us per call, buckets / exact lists / K3t): cfg3 129 /
    // 144 / 179;  C = 256 R = 16 37 / 53 / 48;  C = 64 176x320 R = 128 40 / 48 / 43;  8 images of 160x160 R = 64
    // 49 / 61 / 61 -- they win wherever the bucket holds at least the average list (128 entries per pixel in buckets
    // of 128: 74 / 89 / 164) and lose where most of a list lives in the chains (512 per pixel in buckets of 128:
    // 200 / 128 / 318): the bucket grows with the density as far as carve_bwd's cap lets it, bucket_pref says if
    // that was far enough.
    const bool buckets = !ordered && gather && ws.bucket_ok && gather_choice_is_open(path) &&
                         (path == RROI_PATH_TILED_BUCKETS || (ws.bucket_pref && g_tune.bwd_buckets));
    const bool lists = ragged || ordered || buckets || path == RROI_PATH_TILED_LISTS || !inkernel_ok ||
                       (path != RROI_PATH_TILED_INKERNEL && !prefer_inkernel);
    const int tt = ceil_div(NB, kRelayoutPx);
    unsigned nzero = 0;   // pixel counters that the affine launch clears
    if (gather && !lists) {
        // K3t: relayout of top_diff (one launch, masked bins skipped), then the tile gather
        P.family = RROI_PLAN_BWD_INKERNEL;
        BwdDispatch::InKernel& K = P.inkernel;
        K.tt = tt;
        if (!td_nhwc) {
            K.tiles = (long)K.tt * nchunks * num_rois;
            if (K.tiles >= (1L << 31)) return P;
            K.relayout_blocks = relayout_blocks(K.tiles, nchunks);
        }
        K.flags = g_tune.bwd_skip_dead;
        K.nk = nchunks > 4 ? 8 : nchunks > 2 ? 4 : nchunks > 1 ? 2 : 1;
        // 16-bit calls: at most four chunks per lane (two passes beyond 128 channels) -- the eight-chunk instantiation
        // spills to scratch (as the fp32 one does), and a 16-bit instantiation of it is not built
        if (half && K.nk > 4) K.nk = 4;
        const unsigned ntiles = ws.keys.keys / 32u;
        const unsigned per_xcd = (ntiles + 7u) / 8u;
        P.grid = dim3(per_xcd * 8u);
        P.dest = bd_nhwc ? RROI_PLAN_DST_NHWC : RROI_PLAN_DST_CHUNK_MAJOR;
    } else if (gather) {
        // (1) pixel -> (bin, weight) lists: count, scan, fill -- or buckets in one pass
        P.family = ordered ? RROI_PLAN_BWD_ORDERED : buckets ? RROI_PLAN_BWD_BUCKETS : RROI_PLAN_BWD_LISTS;
        BwdDispatch::Lists& L = P.lists;
        L.tt = tt;
        nzero = ws.keys.keys;
        // few scan blocks: every consumer block prefix-sums their totals itself (no second scan launch)
        L.raw_bsum = ws.scan_blocks <= kInlineScanBlocks ? 1 : 0;
        // one pair block per CU, looping over the bins: the pair passes need outstanding atomics,
        // not CU slots -- more blocks only take residency from the relayout (207 -> 197 us per call)
        const PatchMap dnb = make_patch_map(S.pooled_height, S.pooled_width);
        if ((long)num_rois * dnb.lanes_per_roi >= (1L << 32)) return P;
        int pblocks = ceil_div((long)num_rois * dnb.lanes_per_roi, 256);
        {
            // pair blocks per CU.  A pair wave walks a chain of returning atomics (~2.5 us per patch of 64 bins under
            // load), so its launch time is patches per wave x that; the relayout it shares the launch with takes
            // bytes / bandwidth.  One block per CU hides the pairs behind the relayout of 256 channels (round 2); with
            // FEWER channels the same bins bring a quarter of the bytes and the pair pass set the launch (R = 512, C = 64,
            // 11 x 96: 58 us where the relayout alone takes 30): blocks per CU ~ 256 / C.
            // (tools/pair_blocks_ab.py, profiles/r05_pair_blocks_ab2.txt: with the wave-aggregated reservations, us per call at 1 / 2
            // / 4 / 8 blocks per CU -- C = 64, R = 512, 11 x 96: 90.6 / 73.0 / 67.0 / 68.8 (round 4: 84.3); C = 128: 66.5 / 58.9 /
            // 59.7 / 59.7; configs[2]: 104.4 / 103.3 / 103.6 / 103.5)
            int per_cu = g_tune.bwd_pair_blocks_per_cu;
            if (per_cu <= 0) per_cu = std::min(4, std::max(2, 256 / std::max(channels, 1)));
            // channels-last gradients need no relayout: the pair blocks have the launch to themselves (CL=1 tools/pair_blocks_ab.py,
            // profiles/r05_pair_blocks_ab_cl.txt: C = 64, R = 512 45.3 / 41.4 us at 4 / 8 per CU, round 4: 64.0; configs[2] 52.8 / 49.0, 51.3)
            if (g_tune.bwd_pair_blocks_per_cu <= 0 && td_nhwc) per_cu = 8;
            const long cap = (long)num_cus() * per_cu;
            if (pblocks > cap) pblocks = (int)cap;
        }
        L.pblocks = pblocks;
        // the bucket slots reserved per WAVE through a table in LDS (pairs_reserve_wave) -- where a wave has several
        // patches to walk; with one patch per wave the table's set-up is pure latency (R = 32, C = 64: +0.8 us)
        const bool aggregate = g_tune.bwd_pair_aggregate && (long)num_rois * (dnb.lanes_per_roi / 64) > 8L * num_cus();
        L.flags = (g_tune.bwd_skip_dead ? 1 : 0) | (aggregate ? 2 : 0);
        // count || first half of the relayout;  scan;  fill || second half.  The relayout is the
        // forward's, with R "images" of PH x PW "pixels" and the masked bins skipped:
        // top_diff (R, C, NB) -> (R, NB, nchunks * 32)
        L.tiles = td_nhwc ? 0 : (long)L.tt * nchunks * num_rois;  // nothing to relay out
        if (L.tiles >= (1L << 31)) return P;
        const long unit = nchunks;  // a block takes all chunks of a pixel range: whole ranges per launch
        L.half = (L.tiles / 2 + unit - 1) / unit * unit < L.tiles ? (L.tiles / 2 + unit - 1) / unit * unit : L.tiles;
        // buckets: ONE launch, every pair into its pixel's bucket (or overflow chain) || the whole relayout
        L.bucket_blocks = relayout_blocks(L.tiles, nchunks);
        L.count_blocks = relayout_blocks(L.half, nchunks);
        L.fill_blocks = relayout_blocks(L.tiles - L.half, nchunks);
        // (3) gather: one thread group per key, no grid-stride
        unsigned sub_shift = 3;  // 8 lanes = one chunk
        while ((1u << sub_shift) < 8u * (unsigned)nchunks && sub_shift < 6) ++sub_shift;
        // NCHW bottom_diff written in place (round 4; tools/bwd_nchw_ab.py, profiles/r04_bwd_nchw_ab.txt): a workgroup
        // needs whole rows (8 pixels) of a key tile, i.e. at most 32 lanes per pixel -- wider pixels (C > 128) deal
        // their passes of four chunks to blockIdx.y, which walks every list once per pass: that pays while the lists
        // are short (cfg3, 10 bins per map pixel: 125.6 -> 117.5 us; 20 per pixel: 274 -> 283), so C > 128 keeps the
        // scratch form beyond 16 bins per pixel.  C <= 128 gains at every density measured: R = 512, C = 64 / 128
        // 76.0 -> 71.9 / 76.5 -> 71.2, R = 16...32 36.8 -> 29.0 / 24.3 -> 17.9 (the relayout launch was a fifth of
        // those calls), 84 bins per pixel 159 -> 153.
        // (ORDERED: always in place -- its gather has no chunk-major form)
        const bool nchw_direct = !bd_nhwc && (ordered || (g_tune.bwd_nchw_direct != 0 &&
                                 (nchunks <= 4 || (double)num_rois * NB <= (double)g_tune.bwd_nchw_direct * (double)batch_size * HW)));
        unsigned gy = 1;
        if (nchw_direct && sub_shift == 6) {
            sub_shift = 5;
            gy = (unsigned)ceil_div(nchunks, 4);
        }
        const unsigned groups_per_block = 256u >> sub_shift;
        // whole groups of 8 key tiles (the kernel deals the tiles of a group to the 8 XCDs)
        const long wg_per_tile = 32 / groups_per_block;  // 1, 2, 4 or 8
        const unsigned tile_run = nchw_direct ? (unsigned)g_tune.bwd_tile_run : 0u;
        const long gblocks = ceil_div(ceil_div((long)ws.keys.keys, 32L), 8L << tile_run) * (8L << tile_run) * wg_per_tile;
        L.sub_shift = sub_shift;
        L.gy = gy;
        L.tile_run = tile_run;
        // ORDERED's sorts: four lists per workgroup in registers; the queue of long lists drained by four workgroups per CU
        L.sort_lists_blocks = ceil_div((long)ws.keys.keys, 4L);
        L.sort_queue_blocks = num_cus() * 4;
        P.grid = dim3((unsigned)gblocks, gy);
        P.dest = bd_nhwc ? RROI_PLAN_DST_NHWC
                         : nchw_direct ? (accumulate ? RROI_PLAN_DST_NCHW_ADD : RROI_PLAN_DST_NCHW) : RROI_PLAN_DST_CHUNK_MAJOR;
    } else {
        P.family = RROI_PLAN_BWD_ATOMIC;
        P.atomic.ntiles = ceil_div(NB, kTileBins);
        if ((long)num_rois * P.atomic.ntiles >= (1L << 31)) return P;
        P.grid = dim3(tiled_grid((long)num_rois * P.atomic.ntiles, nchunks));
        P.atomic.vec4 = NB % 4 == 0;
        P.dest = RROI_PLAN_DST_CHUNK_MAJOR;
    }
    {
        // affine table; the list passes' pixel counters (K3g) are cleared by the same launch
        int ablocks = ceil_div(num_rois, 256);
        const int zblocks = nzero ? (int)std::min<long>(ceil_div((long)nzero, 1024), 2L * num_cus()) : 0;
        if (zblocks > ablocks) ablocks = zblocks;
        P.affine_blocks = ablocks;
    }
    P.status = 1;
    return P;
}

// What a bucketed forward launches.  The host cannot see the table, so the choice goes by what the caller states:
// the sum of the widths (the call's real output size), a common divisor of the widths and the crops' alignment.
FwdDispatch plan_forward_bucketed(const Shape& S, int dtype, long long sum_pooled_widths, int width_multiple,
                                  int crop_alignment, int path)
{
    FwdDispatch P;
    P.shape = S;
    const int num_rois = S.num_rois, channels = S.channels, pooled_height = S.pooled_height, max_pooled_width = S.pooled_width;
    if (!dtype_ok(dtype)) return P;
    if (path & ~(0xff | RROI_PATH_TRIG_FP32)) return P;
    P.trig = (path & RROI_PATH_TRIG_FP32) ? RROI_TRIG_FP32 : RROI_TRIG_DOUBLE;
    path &= 0xff;
    if (path != RROI_PATH_AUTO && path != RROI_PATH_DIRECT && path != RROI_PATH_TILED) return P;
    if (!shape_ok(S)) return P;
    if (width_multiple < 1 || crop_alignment < 1 || sum_pooled_widths < 0) return P;
    if (num_rois == 0) {
        P.status = 1;
        return P;
    }
    if (sum_pooled_widths < num_rois || sum_pooled_widths > (long long)num_rois * max_pooled_width) return P;
    // the ragged gather's contract: every crop's rows are whole 64-byte sectors and every crop starts on one
    const bool fast_ok = ((long long)pooled_height * width_multiple) % 16 == 0 && crop_alignment % 64 == 0;
    const double out_elems = (double)channels * pooled_height * (double)sum_pooled_widths;
    const double map_elems = (double)S.batch_size * channels * S.height * S.width;
    const bool tiled = path == RROI_PATH_TILED ||
                       (path == RROI_PATH_AUTO && fast_ok && out_elems >= g_tune.fwd_tiled_min_elems && out_elems >= map_elems / 4);
    if (tiled && !fast_ok) return P;
    if (!tiled) {
        // the ragged patch kernel, at any R: the floor for every width set and address (no thread-per-bin form)
        if (!plan_patch_forward(S, P.patch)) return P;
        P.family = RROI_PLAN_FWD_DIRECT_K2P;
        P.status = 1;
        return P;
    }
    const int ntiles = ceil_div((long)pooled_height * max_pooled_width, kTileBins);   // the item space: ROI x tiles of the widest
    if ((long)num_rois * ntiles >= (1L << 31)) return P;
    // ... of which about ceil(PH * W_i / 64) per ROI exist: the grid is sized for those
    const long items = std::min<long>((long)num_rois * ntiles,
                                      (long)(((long long)pooled_height * sum_pooled_widths + kTileBins - 1) / kTileBins) + num_rois);
    // reported as RROI_PLAN_KERNEL_STRIDED_RAGGED, one XCD group
    P.gather = {FwdKernel::kStridedRagged, tiled_grid(items, S.nchunks(), g_tune.split_wgs_per_cu), ntiles, g_tune.fwd_dbg & ~0xe0};
    P.groups = 1;
    P.prologue = plan_prologue(S, false, P.groups, false);   // (the dense prologue, unchanged: one group, no launcher)
    P.family = RROI_PLAN_FWD_TWO_LAUNCH;
    P.status = 1;
    return P;
}

// ------------------------------------------------------------------------------------
// What the plan queries report: one conversion per direction, shared by the dense and the bucketed query.  A field the
// plan does not use reports its "none" value (rroi_align_plan in the header).
// ------------------------------------------------------------------------------------
rroi_align_plan to_plan(const FwdDispatch& P)
{
    const bool none = P.family == RROI_PLAN_NONE;
    const bool gathers = P.family == RROI_PLAN_FWD_FUSED_STRIDED || P.family == RROI_PLAN_FWD_FUSED_SHIFT ||
                         P.family == RROI_PLAN_FWD_TWO_LAUNCH;
    const dim3 grid = gathers ? dim3(P.gather.grid)
                      : P.family == RROI_PLAN_FWD_DIRECT_K2P ? P.patch.grid
                      : P.family == RROI_PLAN_FWD_DIRECT_THREAD ? P.dgrid : dim3(0, 0, 0);
    rroi_align_plan out;
    out.family = P.family;
    out.kernel = gathers ? (int)P.gather.kernel : -1;
    out.groups = none ? 0 : P.groups;
    out.ntiles = gathers ? P.gather.ntiles : 0;
    out.grid_x = (int)grid.x;
    out.grid_y = (int)grid.y;
    out.zero_copy = P.zero_copy;
    out.con_idx = P.con_idx && !none;
    out.nk = 0;
    out.kshift = 0;
    out.raw_bsum = -1;
    out.gy = 0;
    out.dest = RROI_PLAN_DST_NONE;
    out.accumulate = false;
    out.vec4 = false;
    return out;
}

rroi_align_plan to_plan(const BwdDispatch& P)
{
    const bool none = P.family == RROI_PLAN_NONE;
    const bool lists = P.family == RROI_PLAN_BWD_LISTS || P.family == RROI_PLAN_BWD_BUCKETS ||
                       P.family == RROI_PLAN_BWD_ORDERED;
    rroi_align_plan out;
    out.family = P.family;
    out.kernel = -1;
    out.groups = 0;
    out.ntiles = P.family == RROI_PLAN_BWD_ATOMIC ? P.atomic.ntiles : 0;
    out.grid_x = none ? 0 : (int)P.grid.x;
    out.grid_y = none ? 0 : (int)P.grid.y;
    out.zero_copy = P.td_nhwc && !none;
    out.con_idx = false;
    out.nk = P.inkernel.nk;
    out.kshift = P.family == RROI_PLAN_BWD_BUCKETS ? (int)P.ws.kshift : 0;
    out.raw_bsum = lists ? P.lists.raw_bsum : -1;
    out.gy = lists ? (int)P.lists.gy : 0;
    out.dest = P.dest;
    out.accumulate = P.accumulate && !none;
    out.vec4 = P.atomic.vec4;
    return out;
}

// A plan query's answer: 0 where the call would refuse its arguments (or `plan` is NULL), else 1 and the report.
template <class Dispatch>
int report_plan(const Dispatch& P, rroi_align_plan* plan)
{
    if (!plan || !P.status) return 0;
    *plan = to_plan(P);
    return 1;
}
