// The H-form block scans, written once for the three families of ldpc_hosd.hip (ldpc_hosd_*, (128,64)), ldpc_hosdx.h
// (ldpc_hosdx_*, any shape with k, n - k <= 64) and ldpc_hosdw.h (ldpc_hosdw_*, k up to 127, an H with redundant rows): the
// choice between the two forms of the search, the per-thread-run scan, the ticketed work-item scan, the search's results,
// the sliding kernel (group rule, window decisions, results), and the padded ascending sort of the any-shape front ends.
// Included from ldpc_hosd.hip before the families.  A family is a traits struct FAM with
//   Lds<RUNS>                         its LDS plan (HSearchLds / HSearchXLds / HSearchWLds), which also picks its hosd_apply
//   cost(L, lo, hi, sh)               the metric of a discrepancy
//   setup(L, sh, in, f, truth, lo, hi)  the per-frame set-up: LUTs, columns, keys reset, the order-0 discrepancy, L.truth
//   kPosBits, pos(v)                  the width of a TEP position in the packed LDS table, and what a position is reduced to
// and sh is what its kernels know of the code: compile-time constants (HShape128) or the kernel's n, m (HShapeNM).
// The three search kernels declare their __shared__ object and call hosd_search_body.  The three sliding kernels are one
// text, the macro HOSD_SLIDING_KERNEL below: as a function template called from a thin kernel, even the unchanged text of the
// kernels it replaced compiles to other code, and the any-shape sliding kernel then measured 0.3-0.7 % slower.
// The form selection is a probe that returns a flag plus a staging step: as one function with an early return it compiled to
// 200 instructions more per run-form kernel.
#pragma once

#include "ldpc_wave.h"
#include "ldpc_hosd_limits.h"   // kHosdMaxBlocks, kSlideMaxWin

namespace ldpc {

constexpr int kHosdLdsTeps = 2304;     // a TEP table up to this size (256 threads x 9) of weight <= 2 in <= kHosdRunBlocks blocks is kept in LDS,
constexpr int kHosdRunBlocks = 128;    // two bytes per TEP, and scanned in per-thread runs (the reference's order-2 paths: 2081 TEPs, 28 blocks)
constexpr int kHosdChunk = 256;        // larger tables: TEPs per work item (a block larger than this is split)
constexpr int kSlideGroupTeps = 256;   // default group: consecutive blocks until the group holds one TEP per thread

struct HShape128 {                     // (128,64): the shape is compile-time constants
    static constexpr int n = 128, m = 64, nb = 16, words = 2;
};
struct HShapeNM {                      // the kernel's n, m; the bytes of a discrepancy and the words of a codeword
    int n, m, nb, words;
    __device__ HShapeNM(int n_, int m_) : n(n_), m(m_), nb((n_ + 7) >> 3), words((n_ + 63) >> 6) {}
};

// what every block scan reads: the two LLR inputs, the front end's results, the TEP table in blocks, the labels (or nullptr)
struct HScanIn {
    const float *__restrict__ xo, *__restrict__ xm;
    long long F;
    const unsigned char *__restrict__ lri, *__restrict__ uidx;
    const u64 *__restrict__ Mrows;
    const uchar4 *__restrict__ teps;
    const int *__restrict__ block_off;
    int nblk;
    const u64 *__restrict__ label;
};
// ... and the per-frame results that both scans write (each may be nullptr)
struct HBestOut {
    float *__restrict__ truth;
    u64 *__restrict__ cw;
    float *__restrict__ metric;
    int *__restrict__ best;
};

struct SlideFcnArg {                     // Predict_outlier_light, by value: dense1 [win+1][win+1], dense2 [win+1][2]
    float w1[(kSlideMaxWin + 1) * (kSlideMaxWin + 1)];
    float w2[(kSlideMaxWin + 1) * 2];
};

struct SlideLds {
    int boff[kHosdMaxBlocks + 1];        // block_off, once per workgroup
    float x[kSlideMaxWin + 1];           // classifier input: the sorted window, then the window index
    float h[kSlideMaxWin + 1];           // dense1 output
    int done, deep;
};

// A block's key: (metric bits << 32) | TEP index, ~0 for a block without a candidate.  Metrics are sums of magnitudes, so
// their bit patterns order like the floats and the smallest key is the FIRST minimum.
__device__ __forceinline__ u64 hosd_key(float metric, int t) { return ((u64)(unsigned)__float_as_int(metric) << 32) | (unsigned)t; }
__device__ __forceinline__ float key_metric(u64 k) { return k == ~0ull ? INFINITY : __int_as_float((int)(k >> 32)); }

// the block that holds TEP t among blocks lo..hi-1: the last b with boff[b] <= t (blocks may be empty)
__device__ __forceinline__ int hosd_block_of(const int *boff, int lo, int hi, int t)
{
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (boff[mid] <= t) lo = mid; else hi = mid; }
    return lo;
}

// Wave 0 of a frame's workgroup, after the keys of the candidate blocks have been folded into L.best: the first minimum's
// metric and TEP index and its codeword in the original bit order (d_metric / d_best / d_cw), `words` words per frame.
template <class LDS>
__device__ __forceinline__ void hosd_frame_best(LDS &L, const uchar4 *__restrict__ teps, long long f, u64 DL0, u64 DM0,
                                                const HBestOut &out, int words)
{
    const int lane = threadIdx.x & 63;
    const u64 k = L.best;
    const bool none = k == ~0ull;
    if (lane == 0) {
        if (out.metric) out.metric[f] = none ? INFINITY : __int_as_float((int)(k >> 32));
        if (out.best) out.best[f] = none ? -1 : (int)(unsigned)k;
    }
    if (out.cw) {
        u64 DL = DL0, DM = DM0;
        if (!none) hosd_apply(L, teps[(unsigned)k], DL, DM);
        const u64 bitsL = DL ^ L.hgL, bitsM = DM ^ L.hgM;
        const int o1 = L.o[lane], o2 = L.o[64 + lane];
        if ((bitsL >> lane) & 1) atomicOr(&L.cw[o1 >> 6], 1ull << (o1 & 63));
        if ((bitsM >> lane) & 1) atomicOr(&L.cw[o2 >> 6], 1ull << (o2 & 63));
        wave_fence();
        if (lane < words) out.cw[f * words + lane] = L.cw[lane];
    }
}

// ---- the search: which form works, and the per-thread-run form's table in LDS ------------------------------------------
// Both instantiations of a search kernel are launched and decide alike from device data which of them works (the other
// returns at once): the per-thread-run form takes a table of ntep <= kHosdLdsTeps TEPs of weight <= 2 in <= kHosdRunBlocks
// blocks.  Returns whether that form works (uniform).
template <class LDS>
__device__ __forceinline__ bool hosd_runs_form(LDS &L, const uchar4 *__restrict__ teps, int ntep, int nblk)
{
    const int tid = threadIdx.x;
    bool runs = ntep <= kHosdLdsTeps && nblk <= kHosdRunBlocks;
    if (runs) {         // (uniform) any TEP of weight 3?
        if (tid == 0) L.heavy = 0;
        __syncthreads();
        bool h = false;
        for (int t = tid; t < ntep; t += 256) h |= teps[t].w > 2;
        if (h) L.heavy = 1;
        __syncthreads();
        runs = L.heavy == 0;
    }
    return runs;
}

// The per-thread-run form, once per workgroup: the block offsets and the table go to LDS (a TEP as x | y << kPosBits |
// weight << 2 kPosBits), and this thread gets its run [run0, run1) of ceil(ntep / 256) consecutive TEPs, made odd (a lane's
// run starts on its own LDS bank), and the block b0 that holds TEP run0.
template <class FAM, class LDS>
__device__ __forceinline__ void hosd_stage_table(LDS &L, const uchar4 *__restrict__ teps, const int *__restrict__ block_off, int nblk, int ntep,
                                                 int &run0, int &run1, int &b0)
{
    constexpr int PB = FAM::kPosBits;
    const int tid = threadIdx.x;
    for (int b = tid; b <= nblk; b += 256) L.boff[b] = block_off[b];
    for (int t = tid; t < ntep; t += 256) { const uchar4 s = teps[t]; L.tl[t] = (unsigned short)(FAM::pos(s.x) | (FAM::pos(s.y) << PB) | (s.w << (2 * PB))); }
    __syncthreads();
    const int per = ((ntep + 255) / 256) | 1;
    run0 = tid * per < ntep ? tid * per : ntep; run1 = run0 + per < ntep ? run0 + per : ntep;
    b0 = hosd_block_of(L.boff, 0, nblk, run0);
}

// the TEP t of the table that hosd_stage_table put into LDS
template <class FAM, class LDS>
__device__ __forceinline__ uchar4 hosd_lds_tep(const LDS &L, int t)
{
    constexpr unsigned PB = FAM::kPosBits, mask = (1u << PB) - 1u;
    const unsigned tv = L.tl[t];
    // hosd_runs_form admits no TEP of weight 3 and every family's pos() keeps a position inside its field, so the weight
    // field holds 0..2 whatever the caller passed: the third flip of hosd_apply is dead in the run form
    __builtin_assume((tv >> (2 * PB)) <= 2u);
    return make_uchar4((unsigned char)(tv & mask), (unsigned char)((tv >> PB) & mask), 0, (unsigned char)(tv >> (2 * PB)));
}

// ---- the per-thread-run scan: this thread's run [run0, run1) of consecutive TEPs, which starts in block b ----------------
// The thread keeps a running first minimum that it flushes -- a 64-bit LDS atomicMin on the block's key -- when its run
// crosses into the next block and at its end: ~1.2 atomics per thread and frame, no per-block wave reductions.
// boff: the block offsets (LDS); tep(t): TEP t, from the LDS table (the searches) or from global memory (the sliding scans).
template <class FAM, class LDS, class SH, class TEP>
__device__ __forceinline__ void hosd_run_scan(LDS &L, const SH &sh, const int *boff, TEP tep, int run0, int run1, int b, u64 DL0, u64 DM0)
{
    float best = INFINITY;
    int bestt = 0;
    for (int t = run0; t < run1; ++t) {
        while (t >= boff[b + 1]) {      // the run leaves block b (the next ones may be empty)
            if (best < INFINITY) atomicMin(&L.keys[b], hosd_key(best, bestt));
            best = INFINITY;
            ++b;
        }
        u64 DL = DL0, DM = DM0;
        hosd_apply(L, tep(t), DL, DM);
        const float c = FAM::cost(L, DL, DM, sh);
        if (c < best) { best = c; bestt = t; }                     // ascending t: first minimum
    }
    if (best < INFINITY) atomicMin(&L.keys[b], hosd_key(best, bestt));
}

// ---- the work-item scan (a table too large or too heavy for the run form): items of kHosdChunk TEPs, numbered block by
// block, slice by slice, pulled by each wavefront from the frame's LDS ticket; a wave arg-min and an atomic per item
template <class FAM, class LDS, class SH>
__device__ __forceinline__ void hosd_ticket_scan(LDS &L, const SH &sh, const uchar4 *__restrict__ teps, const int *__restrict__ block_off,
                                                 int nblk, u64 DL0, u64 DM0)
{
    const int lane = threadIdx.x & 63;
    int item = 0, b = 0, s = nblk > 0 ? block_off[0] : 0, t1 = nblk > 0 ? block_off[1] : 0;
    for (;;) {
        int want = 0;
        if (lane == 0) want = atomicAdd(&L.ticket, 1);
        want = __builtin_amdgcn_readfirstlane(want);
        // advance (b, s) to item `want`; empty blocks own no item
        while (b < nblk) {
            if (s >= t1) { ++b; if (b < nblk) { s = block_off[b]; t1 = block_off[b + 1]; } continue; }
            if (item == want) break;
            ++item; s += kHosdChunk;
        }
        if (b >= nblk) break;
        const int e = s + kHosdChunk < t1 ? s + kHosdChunk : t1;
        float best = INFINITY;
        int bestt = 0x7FFFFFFF;
        for (int t = s + lane; t < e; t += 64) {
            u64 DL = DL0, DM = DM0;
            hosd_apply(L, teps[t], DL, DM);
            const float c = FAM::cost(L, DL, DM, sh);
            if (c < best) { best = c; bestt = t; }                 // ascending t per lane: first minimum
        }
        const int wl = wave_argmin_lane(best, bestt);
        if (lane == wl) atomicMin(&L.keys[b], hosd_key(best, bestt));
        ++item; s += kHosdChunk;
    }
}

// ---- the search's results: per block the first minimum and its TEP index, and the fold of all blocks into L.best ----------
template <class LDS>
__device__ __forceinline__ void hosd_search_results(LDS &L, long long f, int nblk, float *__restrict__ block_min, int *__restrict__ block_arg)
{
    u64 mine = ~0ull;
    for (int b = threadIdx.x; b < nblk; b += 256) {
        const u64 k = L.keys[b];
        const bool empty = k == ~0ull;
        block_min[f * nblk + b] = empty ? INFINITY : __int_as_float((int)(k >> 32));
        if (block_arg) block_arg[f * nblk + b] = empty ? -1 : (int)(unsigned)k;
        mine = k < mine ? k : mine;
    }
    if (mine != ~0ull) atomicMin(&L.best, mine);
}

// The body of a search kernel.  One frame per 256-thread workgroup: the four wavefronts share the frame's LUTs.
template <class FAM, bool RUNS, class LDS, class SH>
__device__ __forceinline__ void hosd_search_body(LDS &L, const SH sh, const HScanIn in, float *__restrict__ block_min,
                                                 int *__restrict__ block_arg, const HBestOut out)
{
    int run0 = 0, run1 = 0, b0 = 0;
    const int ntep = in.nblk > 0 ? in.block_off[in.nblk] : 0;
    if (hosd_runs_form(L, in.teps, ntep, in.nblk) != RUNS) return;
    if constexpr (RUNS) hosd_stage_table<FAM>(L, in.teps, in.block_off, in.nblk, ntep, run0, run1, b0);
    for (long long f = blockIdx.x; f < in.F; f += gridDim.x) {
        u64 DL0, DM0;
        FAM::setup(L, sh, in, f, out.truth, DL0, DM0);
        if constexpr (RUNS) hosd_run_scan<FAM>(L, sh, L.boff, [&L](int t) { return hosd_lds_tep<FAM>(L, t); }, run0, run1, b0, DL0, DM0);
        else hosd_ticket_scan<FAM>(L, sh, in.teps, in.block_off, in.nblk, DL0, DM0);
        __syncthreads();
        hosd_search_results(L, f, in.nblk, block_min, block_arg);
        __syncthreads();
        if ((threadIdx.x >> 6) == 0) hosd_frame_best(L, in.teps, f, DL0, DM0, out, sh.words);
        __syncthreads();
    }
}

// ---- the block scan with the reference's sliding-window early stop (sliding_osd :187-218, sliding_window_ops :140-151) ----
// One frame per 256-thread workgroup.  The blocks are scanned in GROUPS of consecutive blocks, all threads on one group
// (per-thread runs of consecutive TEPs as above, TEPs read from the table in global memory); then lane 0 replays every
// window decision the group's block minima make possible and the workgroup stops scanning the frame as soon as the
// classifier fires.  Blocks of a group past the stopping block are speculative work: they count in d_teps_evaluated but
// in no result, so the results do not depend on the group size.

// p1 of the classifier on S.x[0..win]: h = x . W1, z = h . W2, each output a sequential f32 sum over the input index
// (starting from the first product), then softmax with the maximum subtracted: p1 = e1 / (e0 + e1), e_c = expf(z_c - max).
__device__ __forceinline__ float slide_p1(SlideLds &S, int win, const SlideFcnArg &w)
{
    const int d = win + 1;
    for (int j = 0; j < d; ++j) {
        float acc = S.x[0] * w.w1[j];
        for (int i = 1; i < d; ++i) acc = acc + S.x[i] * w.w1[i * d + j];
        S.h[j] = acc;
    }
    float z0 = S.h[0] * w.w2[0], z1 = S.h[0] * w.w2[1];
    for (int j = 1; j < d; ++j) {
        z0 = z0 + S.h[j] * w.w2[2 * j];
        z1 = z1 + S.h[j] * w.w2[2 * j + 1];
    }
    const float m = z1 > z0 ? z1 : z0;
    const float e0 = expf(z0 - m), e1 = expf(z1 - m);
    return e1 / (e0 + e1);
}

// ---- the sliding kernel of a family, as text: NAME, the family's traits, the shape parameters of the kernel (with their
// trailing comma) and the declaration of sh.  A macro and not a function template: called through a function, this very text
// compiles to other code than the kernels it replaced.
#define HOSD_NO_SHAPE_PARAMS
#define HOSD_NM_SHAPE_PARAMS int n, int m,
#define HOSD_SLIDING_KERNEL(NAME, FAM, SHAPE_PARAMS, SHAPE) \
template <class... COUNT>   /* (the counted form: ldpc_wave.h) */                                                                     \
__global__ __launch_bounds__(256) void NAME(const float *__restrict__ xo, const float *__restrict__ xm, long long F,                   \
                                                            SHAPE_PARAMS const unsigned char *__restrict__ lri,                        \
                                                            const unsigned char *__restrict__ uidx, const u64 *__restrict__ Mrows,     \
                                                            const uchar4 *__restrict__ teps, const int *__restrict__ block_off,        \
                                                            int nblk, int win, double margin, SlideFcnArg fcn, int group,              \
                                                            const u64 *__restrict__ label, int *__restrict__ deep_out,                 \
                                                            float *__restrict__ gmin_out, float *__restrict__ truth,                   \
                                                            unsigned char *__restrict__ success, u64 *__restrict__ cw_out,             \
                                                            float *__restrict__ metric_out, int *__restrict__ best_out,                \
                                                            int *__restrict__ nteps_out, COUNT... count)                               \
{                                                                                                                                      \
    if constexpr (kCounted<COUNT...>) {                                                                                                \
        F = counted_frames(F, count...);                                                                                               \
        if (blockIdx.x >= F) return;   /* (the grid is sized by the capacity, not by the count) */                                     \
    }                                                                                                                                  \
    __shared__ FAM::Lds<false> L;                                                                                                      \
    __shared__ SlideLds S;                                                                                                             \
    const int tid = threadIdx.x, wave = tid >> 6;                                                                                      \
    const SHAPE;                                                                                                                       \
    for (int b = tid; b <= nblk; b += 256) S.boff[b] = block_off[b];                                                                   \
    __syncthreads();                                                                                                                   \
                                                                                                                                       \
    for (long long f = blockIdx.x; f < F; f += gridDim.x) {                                                                            \
        u64 DL0, DM0;                                                                                                                  \
        FAM::setup(L, sh, {xo, xm, F, lri, uidx, Mrows, teps, block_off, nblk, label}, f, truth, DL0, DM0);                            \
        int k = 0, deep = win;   /* (lane 0) the next window decision, blocks evaluated so far in the reference's sense */             \
        float gmin = INFINITY;   /* (lane 0) global_min */                                                                             \
        int g0 = 0, g1 = 0;                                                                                                            \
        for (;;) {                                                                                                                     \
            /* ---- the group [g0, g1): `group` blocks, or blocks until kSlideGroupTeps TEPs and the first window */                   \
            if (group > 0) {                                                                                                           \
                g1 = g0 + group < nblk ? g0 + group : nblk;                                                                            \
            } else {                                                                                                                   \
                g1 = g0 + 1;                                                                                                           \
                while (g1 < nblk && (g1 < win || S.boff[g1] - S.boff[g0] < kSlideGroupTeps)) ++g1;                                     \
            }                                                                                                                          \
            const int t0 = S.boff[g0], nt = S.boff[g1] - t0, per = (nt + 255) / 256;                                                   \
            const int run0 = t0 + (tid * per < nt ? tid * per : nt), run1 = t0 + (tid * per + per < nt ? tid * per + per : nt);        \
            if (run0 < run1)                                                                                                           \
                hosd_run_scan<FAM>(L, sh, S.boff, [teps](int t) { return teps[t]; }, run0, run1, hosd_block_of(S.boff, g0, g1, run0),  \
                                   DL0, DM0);                                                                                          \
            __syncthreads();                                                                                                           \
            /* ---- lane 0: every decision whose window lies in the blocks scanned so far (:193-209) */                                \
            if (tid == 0) {                                                                                                            \
                bool stop = false;                                                                                                     \
                for (; !stop && k <= nblk - win && k + win <= g1; ++k) {                                                               \
                    deep = k + win;                                                                                                    \
                    if (k != 0 && key_metric(L.keys[k + win - 1]) > gmin) continue;   /* :203-204 */                                   \
                    for (int i = 0; i < win; ++i) {   /* the window, ascending */                                                      \
                        const float v = key_metric(L.keys[k + i]);                                                                     \
                        int j = i;                                                                                                     \
                        while (j > 0 && S.x[j - 1] > v) { S.x[j] = S.x[j - 1]; --j; }                                                  \
                        S.x[j] = v;                                                                                                    \
                    }                                                                                                                  \
                    S.x[win] = (float)k;                                                                                               \
                    const float p1 = slide_p1(S, win, fcn);                                                                            \
                    gmin = S.x[0] < gmin ? S.x[0] : gmin;   /* min(global_min, window.min()) */                                        \
                    stop = (double)p1 > margin;                                                                                        \
                }                                                                                                                      \
                S.done = stop || g1 >= nblk;                                                                                           \
                S.deep = deep;                                                                                                         \
            }                                                                                                                          \
            __syncthreads();                                                                                                           \
            if (S.done) break;                                                                                                         \
            g0 = g1;                                                                                                                   \
        }                                                                                                                              \
        /* ---- per-frame results; the best candidate among the blocks the reference evaluates (0 .. deep_limit-1) */                  \
        const int dl = S.deep;                                                                                                         \
        if (tid == 0) {                                                                                                                \
            if (deep_out) deep_out[f] = dl;                                                                                            \
            if (gmin_out) gmin_out[f] = gmin;                                                                                          \
            if (success) success[f] = gmin == L.truth;   /* :213 */                                                                    \
            if (nteps_out) nteps_out[f] = S.boff[g1] - S.boff[0];                                                                      \
        }                                                                                                                              \
        u64 mine = ~0ull;                                                                                                              \
        for (int b = tid; b < dl; b += 256) mine = L.keys[b] < mine ? L.keys[b] : mine;                                                \
        if (mine != ~0ull) atomicMin(&L.best, mine);                                                                                   \
        __syncthreads();                                                                                                               \
        if (wave == 0) hosd_frame_best(L, teps, f, DL0, DM0, {truth, cw_out, metric_out, best_out}, sh.words);                         \
        __syncthreads();                                                                                                               \
    }                                                                                                                                  \
}

// ---- mag_input_gen (:25-28) for n <= 128 positions, one frame per wavefront: rank in ascending |x|, ties -> lower index ----
// Writes L.lri (sorted position -> slot; lane owns slots lane and 64 + lane) through L.rank.  Ascending order of (|x| bits,
// index) = descending order of the complemented key, buckets mirrored.  A slot at or beyond n takes the magnitude word
// 0xFFFFFFFF, above every real one (<= 0x7FFFFFFF), and the lowest mirrored bucket: its complemented key (0, ~slot) lies
// below every real key whatever the frame holds, so the real positions take ranks 0..n-1 in the order their own keys define.
// The bucket scale comes from the real magnitudes alone.  The caller fences before it reads L.lri.
template <class LDS>
__device__ __forceinline__ void hosd_sort_ascending(LDS &L, const float *__restrict__ x, long long f, int n, int lane)
{
    const bool in1 = lane < n, in2 = 64 + lane < n;
    const unsigned a1 = in1 ? (__float_as_uint(x[f * n + lane]) & 0x7FFFFFFFu) : 0u;
    const unsigned a2 = in2 ? (__float_as_uint(x[f * n + 64 + lane]) & 0x7FFFFFFFu) : 0u;
    const float bs = bucket_scale(a1, a2);
    const u64 k1 = in1 ? ~(((u64)a1 << 32) | (unsigned)lane) : (u64)(unsigned)~(unsigned)lane;
    const u64 k2 = in2 ? ~(((u64)a2 << 32) | (unsigned)(lane + 64)) : (u64)(unsigned)~(unsigned)(lane + 64);
    int r1, r2;
    bucket_ranks(L.rank, k1, k2, in1 ? 63 - bucket_of(a1, bs) : 0, in2 ? 63 - bucket_of(a2, bs) : 0, lane, r1, r2);
    L.lri[r1] = (unsigned char)lane;
    L.lri[r2] = (unsigned char)(lane + 64);
}

}  // namespace ldpc
