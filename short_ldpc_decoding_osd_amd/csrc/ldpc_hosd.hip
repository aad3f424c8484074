// H-form ordered-statistics primitives for the DL-OSD stage on gfx950 (MI355X): the (128,64) kernels here, the any-shape
// kernels (ldpc_hosdx_*) in ldpc_hosdx.h, the ones for high-rate codes and an H with redundant rows (ldpc_hosdw_*) in
// ldpc_hosdw.h.
//
// Reference (paths relative to LDPC_128/DL_OSD_Testing_serial/ of the reference):
//   mag_input_gen / check_matrix_reorder   ordered_statistics_decoding.py:25-41
//   identify_mrb / full_gf2elim            ordered_statistics_decoding.py:43-80, 222-257
//   acquire_min / sliding_osd              ordered_statistics_decoding.py:153-186
//
// The dual of ldpc_osd.hip: positions are sorted by ASCENDING reliability, the elimination runs
// on the permuted H (-> [I | M], the identity part on the least reliable independent positions),
// a candidate is [M . mrb, mrb], and the scan is organised in caller-defined TEP blocks whose
// minima feed the reference's sliding-window network on the host.  Two separate LLR inputs: one
// orders the positions and supplies the starting MRB hard decisions (the CNN-refined values in
// the reference), the other (trajectory row 0) supplies the metric.  One frame per wavefront.
#include "ldpc_internal.h"
#include "ldpc_wave.h"

namespace ldpc {

struct __attribute__((aligned(16))) HFrontLds {
    RankLds rank;              // reliability sort (bucket_ranks, ldpc_wave.h)
    u64 colbuf[64];            // M columns in updated MRB order, bit = physical row
    unsigned mask[4];          // which sorted positions ended up in the MRB
    unsigned char lri[128];    // sorted position -> original bit
};

__global__ __launch_bounds__(256) void hosd_front_kernel(const float *__restrict__ x, long long F,
                                                         const u64 *__restrict__ Hcols,
                                                         unsigned char *__restrict__ lri_out,
                                                         unsigned char *__restrict__ uidx_out, u64 *__restrict__ M_out,
                                                         int *__restrict__ nswaps)
{
    __shared__ HFrontLds lds[4];
    const int lane = threadIdx.x & 63;
    HFrontLds &L = lds[threadIdx.x >> 6];
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);

    for (long long f = wave; f < F; f += (long long)gridDim.x * 4) {
        // ---- mag_input_gen (:25-28): rank in ascending |x|, ties -> lower index ------------
        // ascending order of (|x| bits, index) = descending order of the complemented key, buckets mirrored
        const unsigned a1 = __float_as_uint(x[f * 128 + lane]) & 0x7FFFFFFFu, a2 = __float_as_uint(x[f * 128 + 64 + lane]) & 0x7FFFFFFFu;
        const float bs = bucket_scale(a1, a2);
        int r1, r2;
        bucket_ranks(L.rank, ~(((u64)a1 << 32) | (unsigned)lane), ~(((u64)a2 << 32) | (unsigned)(lane + 64)), 63 - bucket_of(a1, bs),
                     63 - bucket_of(a2, bs), lane, r1, r2);
        L.lri[r1] = (unsigned char)lane;
        L.lri[r2] = (unsigned char)(lane + 64);
        if (lane < 4) L.mask[lane] = 0;
        wave_fence();
        // ---- H with columns in sorted order (:38-40), column-major, then full_gf2elim (:222-257)
        const int s1 = L.lri[lane], s2 = L.lri[lane + 64];
        u64 C1 = Hcols[s1];
        u64 C2 = Hcols[s2];
        int rho = lane, idx1 = lane, idx2 = lane + 64;
        const int ns = ge_columns(C1, C2, rho, idx1, idx2, lane, nullptr);
        // ---- identify_mrb (:58-69): LRB = index_order[:64] as left by the elimination, MRB sorted
        atomicOr(&L.mask[idx2 >> 5], 1u << (idx2 & 31));
        wave_fence();
        const unsigned m[4] = {L.mask[0], L.mask[1], L.mask[2], L.mask[3]};
        const int rankM = below_mask(m, idx2);          // updated MRB position of column 64 + lane
        L.colbuf[rankM] = C2;
        wave_fence();
        // rows of updated_M: transpose to (lane = physical row, bit = MRB position), then logical row
        // r = the row whose pivot sits in column r = physical row rho[r]
        const u64 R = transpose64(L.colbuf[lane], lane);
        M_out[f * 64 + lane] = shfl64(R, rho);
        lri_out[f * 128 + lane] = (unsigned char)s1;
        lri_out[f * 128 + 64 + lane] = (unsigned char)s2;
        uidx_out[f * 128 + lane] = (unsigned char)idx1;
        uidx_out[f * 128 + 64 + rankM] = (unsigned char)idx2;
        if (nswaps && lane == 0) nswaps[f] = ns;
        wave_fence();
    }
}

constexpr int kHosdMaxBlocks = 1024;   // keys kept in LDS (8 KiB); the reference's paths have 30 blocks
constexpr int kHosdLdsTeps = 2304;     // a TEP table up to this size (256 threads x 9) of weight <= 2 in <= kHosdRunBlocks blocks is kept in LDS,
constexpr int kHosdRunBlocks = 128;    // two bytes per TEP, and scanned in per-thread runs (the reference's order-2 paths: 2081 TEPs, 28 blocks)
constexpr int kHosdChunk = 256;        // larger tables: TEPs per work item (a block larger than this is split)

// RUNS: the per-thread-run form (a small table: 23 KiB of LDS, 6 workgroups per CU -- the kernel answers to occupancy: 0.34 ms at
// 4 workgroups per CU with 4-byte TEPs and 1024 block keys, 0.31 at 5); otherwise rounds 1-2's work items (25.7 KiB).
template <bool RUNS>
struct __attribute__((aligned(16))) HSearchLds {
    float lut[16][256];   // lut[b][v]: partial metric of discrepancy byte b (updated positions 8b..8b+7)
    u64 Mcol[64];         // column j of updated_M (bit r = M[r][j])
    float w[128];         // |metric_llr| in updated order
    u64 keys[RUNS ? kHosdRunBlocks : kHosdMaxBlocks];   // per block: (metric bits << 32) | TEP index, minimum = first minimum
    u64 hgL, hgM, mrb0, DL0, best, cw[2];
    int ticket, heavy;
    float truth;          // the label's metric (hosd_frame_setup with labels)
    unsigned char o[128]; // original bit index of updated position p
    int boff[RUNS ? kHosdRunBlocks + 1 : 1];            // block_off, once per workgroup
    unsigned short tl[RUNS ? kHosdLdsTeps : 2];         // the TEP table, once per workgroup: x | y << 6 | weight << 12
};

template <class LDS>
__device__ __forceinline__ float hosd_cost(const LDS &L, u64 DL, u64 DM)
{
    float acc = lut_byte<0>(L.lut, DL);
    acc = acc + lut_byte<1>(L.lut, DL); acc = acc + lut_byte<2>(L.lut, DL); acc = acc + lut_byte<3>(L.lut, DL);
    acc = acc + lut_byte<4>(L.lut, DL); acc = acc + lut_byte<5>(L.lut, DL); acc = acc + lut_byte<6>(L.lut, DL);
    acc = acc + lut_byte<7>(L.lut, DL);
    acc = acc + lut_byte<0>(&L.lut[8], DM); acc = acc + lut_byte<1>(&L.lut[8], DM); acc = acc + lut_byte<2>(&L.lut[8], DM);
    acc = acc + lut_byte<3>(&L.lut[8], DM); acc = acc + lut_byte<4>(&L.lut[8], DM); acc = acc + lut_byte<5>(&L.lut[8], DM);
    acc = acc + lut_byte<6>(&L.lut[8], DM); acc = acc + lut_byte<7>(&L.lut[8], DM);
    return acc;
}

template <class LDS>
__device__ __forceinline__ void hosd_apply(const LDS &L, uchar4 s, u64 &DL, u64 &DM)
{
    if (s.w > 0) { DL ^= L.Mcol[s.x]; DM ^= 1ull << s.x; }
    if (s.w > 1) { DL ^= L.Mcol[s.y]; DM ^= 1ull << s.y; }
    if (s.w > 2) { DL ^= L.Mcol[s.z]; DM ^= 1ull << s.z; }
}

// Per-frame set-up shared by the block scans (hosd_search_kernel, hosd_sliding_kernel): values in updated order, hard
// decisions, M columns, block keys reset, byte LUTs, the order-0 discrepancies DL0 / DM0 and (with labels) the label's metric
// (L.truth, and truth[f] where truth is given).
// On return every thread sees the LUTs, the M columns and the keys of blocks 0..nblk-1 reset to ~0.
template <class LDS>
__device__ __forceinline__ void hosd_frame_setup(LDS &L, const float *__restrict__ xo, const float *__restrict__ xm, long long f,
                                                 const unsigned char *__restrict__ lri, const unsigned char *__restrict__ uidx,
                                                 const u64 *__restrict__ Mrows, int nblk, const u64 *__restrict__ label,
                                                 float *__restrict__ truth, u64 &DL0, u64 &DM0)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- phase 0: values in updated order (:172-176), hard decisions, M columns, key reset --------
    if (tid < 128) {
        const int o = lri[f * 128 + uidx[f * 128 + tid]];
        const float m = xm[f * 128 + o];
        L.o[tid] = (unsigned char)o;
        L.w[tid] = __builtin_fabsf(m);
        const u64 hg = __ballot(!(m > 0.0f));                       // order_hard_original (:180)
        if (wave == 0) { if (lane == 0) L.hgL = hg; }
        else {
            const u64 h0 = __ballot(!(xo[f * 128 + o] > 0.0f));      // initial_mrb (:186-187)
            if (lane == 0) { L.hgM = hg; L.mrb0 = h0; }
        }
    } else if (wave == 2) {
        L.Mcol[lane] = transpose64(Mrows[f * 64 + lane], lane);
    } else {
        if (lane == 0) { L.ticket = 0; L.best = ~0ull; L.cw[0] = 0; L.cw[1] = 0; }
    }
    for (int b = tid; b < nblk; b += 256) L.keys[b] = ~0ull;
    __syncthreads();
    // ---- phase 1: byte LUTs (four per wavefront), order-0 discrepancy of the LRB part (:155,:159) --
    build_byte_luts<4>(&L.lut[4 * wave], &L.w[32 * wave], lane);
    if (wave == 0) {
        const u64 d = wave_xor64(((L.mrb0 >> lane) & 1) ? L.Mcol[lane] : 0ull) ^ L.hgL;
        if (lane == 0) L.DL0 = d;
    }
    __syncthreads();
    DL0 = L.DL0; DM0 = L.mrb0 ^ L.hgM;
    if (label && wave == 1) {
        const u64 l0 = label[f * 2], l1 = label[f * 2 + 1];
        const int o1 = L.o[lane], o2 = L.o[64 + lane];
        const u64 labL = __ballot(((o1 < 64 ? l0 : l1) >> (o1 & 63)) & 1);
        const u64 labM = __ballot(((o2 < 64 ? l0 : l1) >> (o2 & 63)) & 1);
        const float t = hosd_cost(L, labL ^ L.hgL, labM ^ L.hgM);     // (:181-183)
        if (lane == 0) { if (truth) truth[f] = t; L.truth = t; }
    }
}

// Wave 0 of a frame's workgroup, after the keys of the candidate blocks have been folded into L.best: the first minimum's
// metric and TEP index and its codeword in the original bit order (ldpc_hosd_search's d_metric / d_best / d_cw), `words` words
// per frame (the any-shape kernels of ldpc_hosdx.h pass ceil(n / 64); their hosd_apply is the overload on two-word columns).
template <class LDS>
__device__ __forceinline__ void hosd_frame_best(LDS &L, const uchar4 *__restrict__ teps, long long f, u64 DL0, u64 DM0,
                                                u64 *__restrict__ cw_out, float *__restrict__ metric_out, int *__restrict__ best_out,
                                                int words = 2)
{
    const int lane = threadIdx.x & 63;
    const u64 k = L.best;
    const bool none = k == ~0ull;
    if (lane == 0) {
        if (metric_out) metric_out[f] = none ? INFINITY : __int_as_float((int)(k >> 32));
        if (best_out) best_out[f] = none ? -1 : (int)(unsigned)k;
    }
    if (cw_out) {
        u64 DL = DL0, DM = DM0;
        if (!none) hosd_apply(L, teps[(unsigned)k], DL, DM);
        const u64 bitsL = DL ^ L.hgL, bitsM = DM ^ L.hgM;
        const int o1 = L.o[lane], o2 = L.o[64 + lane];
        if ((bitsL >> lane) & 1) atomicOr(&L.cw[o1 >> 6], 1ull << (o1 & 63));
        if ((bitsM >> lane) & 1) atomicOr(&L.cw[o2 >> 6], 1ull << (o2 & 63));
        wave_fence();
        if (lane < words) cw_out[f * words + lane] = L.cw[lane];
    }
}

// One frame per 256-thread workgroup: the four wavefronts share the frame's LUTs.  Every thread scans ITS OWN run of
// consecutive TEPs (ceil(N / 256), made odd: LDS banks) and keeps a running first minimum that it flushes -- a 64-bit LDS
// atomicMin on the block's (metric bits, TEP index) key -- when its run crosses into the next block and at its end: ~1.2
// atomics per thread and frame, no per-block wave reductions (round 1-2: work items pulled from an LDS ticket, a wave
// arg-min and an atomic per item -- 40 % of the kernel's instructions for the reference's 28 blocks of ~75 TEPs).
// Metrics are sums of magnitudes, so their bit patterns order like the floats and the smallest key is the FIRST minimum.
template <bool RUNS>
__global__ __launch_bounds__(256) void hosd_search_kernel(const float *__restrict__ xo, const float *__restrict__ xm,
                                                          long long F, const unsigned char *__restrict__ lri,
                                                          const unsigned char *__restrict__ uidx,
                                                          const u64 *__restrict__ Mrows, const uchar4 *__restrict__ teps,
                                                          const int *__restrict__ block_off, int nblk,
                                                          const u64 *__restrict__ label, float *__restrict__ block_min,
                                                          int *__restrict__ block_arg, float *__restrict__ truth,
                                                          u64 *__restrict__ cw_out, float *__restrict__ metric_out,
                                                          int *__restrict__ best_out)
{
    __shared__ HSearchLds<RUNS> L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // Both instantiations are launched and decide alike from device data which of them works (the other returns here): the
    // per-thread-run form takes a table of <= kHosdLdsTeps TEPs of weight <= 2 in <= kHosdRunBlocks blocks.
    int run0 = 0, run1 = 0, b0 = 0;
    const int ntep = nblk > 0 ? block_off[nblk] : 0;
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
    if (runs != RUNS) return;
    if constexpr (RUNS) {
        // once per workgroup: the block offsets and the table in LDS, this thread's run and its first block
        for (int b = tid; b <= nblk; b += 256) L.boff[b] = block_off[b];
        for (int t = tid; t < ntep; t += 256) { const uchar4 s = teps[t]; L.tl[t] = (unsigned short)(s.x | (s.y << 6) | (s.w << 12)); }
        __syncthreads();
        const int per = ((ntep + 255) / 256) | 1;      // (odd: a lane's run starts on its own LDS bank)
        run0 = tid * per < ntep ? tid * per : ntep; run1 = run0 + per < ntep ? run0 + per : ntep;
        int lo = 0, hi = nblk;       // the block that holds TEP run0: the last b with boff[b] <= run0 (blocks may be empty)
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (L.boff[mid] <= run0) lo = mid; else hi = mid; }
        b0 = lo;
    }

    for (long long f = blockIdx.x; f < F; f += gridDim.x) {
        u64 DL0, DM0;
        hosd_frame_setup(L, xo, xm, f, lri, uidx, Mrows, nblk, label, truth, DL0, DM0);
        if constexpr (RUNS) {
            // ---- phase 2: the scan: this thread's run, a flush per block boundary -----------------------------
            int b = b0;
            float best = INFINITY;
            int bestt = 0;
            for (int t = run0; t < run1; ++t) {
                while (t >= L.boff[b + 1]) {      // the run leaves block b (the next ones may be empty)
                    if (best < INFINITY) atomicMin(&L.keys[b], ((u64)(unsigned)__float_as_int(best) << 32) | (unsigned)bestt);
                    best = INFINITY;
                    ++b;
                }
                u64 DL = DL0, DM = DM0;
                const unsigned tv = L.tl[t];
                hosd_apply(L, make_uchar4((unsigned char)(tv & 63u), (unsigned char)((tv >> 6) & 63u), 0, (unsigned char)(tv >> 12)), DL, DM);
                const float c = hosd_cost(L, DL, DM);
                if (c < best) { best = c; bestt = t; }                     // ascending t: first minimum
            }
            if (best < INFINITY) atomicMin(&L.keys[b], ((u64)(unsigned)__float_as_int(best) << 32) | (unsigned)bestt);
        } else {
            // ---- phase 2: the scan; items are numbered block by block, slice by slice -----------------------
            {
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
                        const float c = hosd_cost(L, DL, DM);
                        if (c < best) { best = c; bestt = t; }                 // ascending t per lane: first minimum
                    }
                    const int wl = wave_argmin_lane(best, bestt);
                    if (lane == wl)
                        atomicMin(&L.keys[b], ((u64)(unsigned)__float_as_int(best) << 32) | (unsigned)bestt);
                    ++item; s += kHosdChunk;
                }
            }
        }
        __syncthreads();
        // ---- phase 3: per-block results, the overall first minimum, its codeword -------------------------
        u64 mine = ~0ull;
        for (int b = tid; b < nblk; b += 256) {
            const u64 k = L.keys[b];
            const bool empty = k == ~0ull;
            block_min[f * nblk + b] = empty ? INFINITY : __int_as_float((int)(k >> 32));
            if (block_arg) block_arg[f * nblk + b] = empty ? -1 : (int)(unsigned)k;
            mine = k < mine ? k : mine;
        }
        if (mine != ~0ull) atomicMin(&L.best, mine);
        __syncthreads();
        if (wave == 0) hosd_frame_best(L, teps, f, DL0, DM0, cw_out, metric_out, best_out);
        __syncthreads();
    }
}

// ---- the block scan with the reference's sliding-window early stop (sliding_osd :187-218, sliding_window_ops :140-151) ----
// One frame per 256-thread workgroup.  The blocks are scanned in GROUPS of consecutive blocks, all threads on one group
// (per-thread runs of consecutive TEPs as above, TEPs read from the table in global memory); then lane 0 replays every
// window decision the group's block minima make possible and the workgroup stops scanning the frame as soon as the
// classifier fires.  Blocks of a group past the stopping block are speculative work: they count in d_teps_evaluated but
// in no result, so the results do not depend on the group size.
constexpr int kSlideMaxWin = 15;         // window + the block index: at most 16 classifier inputs
constexpr int kSlideGroupTeps = 256;     // default group: consecutive blocks until the group holds one TEP per thread

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

__device__ __forceinline__ float key_metric(u64 k) { return k == ~0ull ? INFINITY : __int_as_float((int)(k >> 32)); }

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

__global__ __launch_bounds__(256) void hosd_sliding_kernel(const float *__restrict__ xo, const float *__restrict__ xm, long long F,
                                                           const unsigned char *__restrict__ lri,
                                                           const unsigned char *__restrict__ uidx, const u64 *__restrict__ Mrows,
                                                           const uchar4 *__restrict__ teps, const int *__restrict__ block_off,
                                                           int nblk, int win, double margin, SlideFcnArg fcn, int group,
                                                           const u64 *__restrict__ label, int *__restrict__ deep_out,
                                                           float *__restrict__ gmin_out, float *__restrict__ truth,
                                                           unsigned char *__restrict__ success, u64 *__restrict__ cw_out,
                                                           float *__restrict__ metric_out, int *__restrict__ best_out,
                                                           int *__restrict__ nteps_out)
{
    __shared__ HSearchLds<false> L;
    __shared__ SlideLds S;
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int b = tid; b <= nblk; b += 256) S.boff[b] = block_off[b];
    __syncthreads();

    for (long long f = blockIdx.x; f < F; f += gridDim.x) {
        u64 DL0, DM0;
        hosd_frame_setup(L, xo, xm, f, lri, uidx, Mrows, nblk, label, truth, DL0, DM0);
        int k = 0, deep = win;           // (lane 0) the next window decision, blocks evaluated so far in the reference's sense
        float gmin = INFINITY;           // (lane 0) global_min
        int g0 = 0, g1 = 0;
        for (;;) {
            // ---- the group [g0, g1): `group` blocks, or blocks until kSlideGroupTeps TEPs and the first window
            if (group > 0) {
                g1 = g0 + group < nblk ? g0 + group : nblk;
            } else {
                g1 = g0 + 1;
                while (g1 < nblk && (g1 < win || S.boff[g1] - S.boff[g0] < kSlideGroupTeps)) ++g1;
            }
            const int t0 = S.boff[g0], nt = S.boff[g1] - t0, per = (nt + 255) / 256;
            const int run0 = t0 + (tid * per < nt ? tid * per : nt), run1 = t0 + (tid * per + per < nt ? tid * per + per : nt);
            if (run0 < run1) {
                int lo = g0, hi = g1;    // the block that holds TEP run0: the last b with boff[b] <= run0 (blocks may be empty)
                while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (S.boff[mid] <= run0) lo = mid; else hi = mid; }
                int b = lo;
                float best = INFINITY;
                int bestt = 0;
                for (int t = run0; t < run1; ++t) {
                    while (t >= S.boff[b + 1]) {
                        if (best < INFINITY) atomicMin(&L.keys[b], ((u64)(unsigned)__float_as_int(best) << 32) | (unsigned)bestt);
                        best = INFINITY;
                        ++b;
                    }
                    u64 DL = DL0, DM = DM0;
                    hosd_apply(L, teps[t], DL, DM);
                    const float c = hosd_cost(L, DL, DM);
                    if (c < best) { best = c; bestt = t; }                     // ascending t: first minimum
                }
                if (best < INFINITY) atomicMin(&L.keys[b], ((u64)(unsigned)__float_as_int(best) << 32) | (unsigned)bestt);
            }
            __syncthreads();
            // ---- lane 0: every decision whose window lies in the blocks scanned so far (:193-209)
            if (tid == 0) {
                bool stop = false;
                for (; !stop && k <= nblk - win && k + win <= g1; ++k) {
                    deep = k + win;
                    if (k != 0 && key_metric(L.keys[k + win - 1]) > gmin) continue;       // :203-204
                    for (int i = 0; i < win; ++i) {                                     // the window, ascending
                        const float v = key_metric(L.keys[k + i]);
                        int j = i;
                        while (j > 0 && S.x[j - 1] > v) { S.x[j] = S.x[j - 1]; --j; }
                        S.x[j] = v;
                    }
                    S.x[win] = (float)k;
                    const float p1 = slide_p1(S, win, fcn);
                    gmin = S.x[0] < gmin ? S.x[0] : gmin;                               // min(global_min, window.min())
                    stop = (double)p1 > margin;
                }
                S.done = stop || g1 >= nblk;
                S.deep = deep;
            }
            __syncthreads();
            if (S.done) break;
            g0 = g1;
        }
        // ---- per-frame results; the best candidate among the blocks the reference evaluates (0 .. deep_limit-1)
        const int dl = S.deep;
        if (tid == 0) {
            if (deep_out) deep_out[f] = dl;
            if (gmin_out) gmin_out[f] = gmin;
            if (success) success[f] = gmin == L.truth;                                 // :213
            if (nteps_out) nteps_out[f] = S.boff[g1] - S.boff[0];
        }
        u64 mine = ~0ull;
        for (int b = tid; b < dl; b += 256) mine = L.keys[b] < mine ? L.keys[b] : mine;
        if (mine != ~0ull) atomicMin(&L.best, mine);
        __syncthreads();
        if (wave == 0) hosd_frame_best(L, teps, f, DL0, DM0, cw_out, metric_out, best_out);
        __syncthreads();
    }
}

}  // namespace ldpc

#include "ldpc_hosdx.h"   // the same three kernels for any shape with k, n - k <= 64
#include "ldpc_hosdw.h"   // ... and for k up to 127 and an H of up to 127 rows of rank <= 64
#include "ldpc_fcn.h"     // training of the sliding-window classifier: window builder, loss and gradient

namespace ldpc {

// The H columns for every shape the H-form kernels serve.  ldpc_hosdw_* take n <= 128, an H of 1 <= R <= 127 rows as given
// and rank 1 <= n - k <= 64 (two-word R-bit columns); of these ldpc_hosdx_* take 1 <= k <= 64 and an H of exactly n - k
// rows (m-bit words), and ldpc_hosd_* (128,64) alone.
int hosd_ctx_init(ldpc_ctx *ctx)
{
    const ldpc_code &c = ctx->code;
    ctx->hosd_ok = ctx->hosdx_ok = ctx->hosdw_ok = false;
    const int rank = c.n - c.k;
    if (c.n > 128 || c.m < 1 || c.m > 127 || rank < 1 || rank > 64 || rank > c.m || c.k < 1 || c.k > 127)
        return LDPC_OK;                                                                     // entry points will report UNSUPPORTED
    std::vector<u64> wide(256, 0);
    for (int r = 0; r < c.m; ++r)
        for (int v = 0; v < c.n; ++v)
            if (c.H[(size_t)r * c.n + v]) wide[2 * v + (r >> 6)] |= 1ull << (r & 63);
    LDPC_HIP(hipMalloc((void **)&ctx->d_HcolsW, sizeof(u64) * 256));
    LDPC_HIP(hipMemcpy(ctx->d_HcolsW, wide.data(), sizeof(u64) * 256, hipMemcpyHostToDevice));
    ctx->hosdw_ok = true;
    if (c.k > 64 || c.m != rank) return LDPC_OK;
    std::vector<u64> cols(128, 0);
    for (int v = 0; v < c.n; ++v) cols[v] = wide[2 * v];
    LDPC_HIP(hipMalloc((void **)&ctx->d_Hcols, sizeof(u64) * 128));
    LDPC_HIP(hipMemcpy(ctx->d_Hcols, cols.data(), sizeof(u64) * 128, hipMemcpyHostToDevice));
    ctx->hosdx_ok = true;
    ctx->hosd_ok = c.n == 128 && c.m == 64 && c.k == 64;
    return LDPC_OK;
}

void hosd_ctx_release(ldpc_ctx *ctx)
{
    (void)hipFree(ctx->d_Hcols);
    (void)hipFree(ctx->d_HcolsW);
    ctx->d_Hcols = ctx->d_HcolsW = nullptr;
}

static unsigned grid_for(int64_t F, int waves_per_block)
{
    const int64_t want = (F + waves_per_block - 1) / waves_per_block;
    return (unsigned)(want < 1 ? 1 : (want < 8192 ? want : 8192));
}

// The refusal of every ldpc_hosdx_* entry point for a code outside the family, LDPC_OK inside it.
static int hosdx_check(const ldpc_ctx *ctx, const char *who)
{
    if (ctx->hosdx_ok) return LDPC_OK;
    const ldpc_code &c = ctx->code;
    return fail(LDPC_E_UNSUPPORTED, "%s: H-form OSD kernels need 1 <= k <= 64 and an H of exactly n-k <= 64 rows; this H has %d rows, "
                "n-k = %d, code (%d,%d)", who, c.m, c.n - c.k, c.n, c.k);
}

// The refusal of every ldpc_hosdw_* entry point for a code outside the family, LDPC_OK inside it.
static int hosdw_check(const ldpc_ctx *ctx, const char *who)
{
    if (ctx->hosdw_ok) return LDPC_OK;
    const ldpc_code &c = ctx->code;
    return fail(LDPC_E_UNSUPPORTED, "%s: wide H-form OSD kernels need n <= 128, an H of 1 <= R <= 127 rows and 1 <= n-k <= 64; this H has "
                "%d rows, n-k = %d, code (%d,%d)", who, c.m, c.n - c.k, c.n, c.k);
}

}  // namespace ldpc

using namespace ldpc;

extern "C" {

int ldpc_hosd_front(ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint8_t *d_lri, uint8_t *d_uidx,
                    uint64_t *d_M, int32_t *d_nswaps, void *stream)
{
    if (!ctx || F < 0 || (F > 0 && (!d_order_llr || !d_lri || !d_uidx || !d_M)))
        return fail(LDPC_E_ARG, "ldpc_hosd_front: bad arguments");
    if (!ctx->hosd_ok)
        return fail(LDPC_E_UNSUPPORTED, "H-form OSD kernels need n=128, m=k=64; this code is n=%d m=%d k=%d", ctx->code.n,
                    ctx->code.m, ctx->code.k);
    if (F == 0) return LDPC_OK;
    hipLaunchKernelGGL(hosd_front_kernel, dim3(grid_for(F, 4)), dim3(256), 0, (hipStream_t)stream, d_order_llr, (long long)F,
                       reinterpret_cast<const u64 *>(ctx->d_Hcols), d_lri, d_uidx, reinterpret_cast<u64 *>(d_M), d_nswaps);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_hosd_search(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F,
                     const uint8_t *d_lri, const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps,
                     const int32_t *d_block_off, int32_t nblk, const uint64_t *d_label_bits, float *d_block_min,
                     int32_t *d_block_arg, float *d_truth, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                     void *stream)
{
    if (!ctx || F < 0 || nblk < 0 ||
        (F > 0 && (!d_order_llr || !d_metric_llr || !d_lri || !d_uidx || !d_M || !d_block_off ||
                   (nblk > 0 && (!d_block_min || !d_teps)))))     // (the kernels read d_teps[0 .. d_block_off[nblk]), device data)
        return fail(LDPC_E_ARG, "ldpc_hosd_search: bad arguments");
    if (d_truth && !d_label_bits) return fail(LDPC_E_ARG, "ldpc_hosd_search: d_truth needs d_label_bits");
    if (!ctx->hosd_ok)
        return fail(LDPC_E_UNSUPPORTED, "H-form OSD kernels need n=128, m=k=64; this code is n=%d m=%d k=%d", ctx->code.n,
                    ctx->code.m, ctx->code.k);
    if (nblk > kHosdMaxBlocks) return fail(LDPC_E_UNSUPPORTED, "ldpc_hosd_search: %d TEP blocks, at most %d", nblk, kHosdMaxBlocks);
    if (F == 0) return LDPC_OK;
    // (the TEP table's size is device data: both forms are launched and one of them returns at once)
    hipLaunchKernelGGL(hosd_search_kernel<true>, dim3(grid_for(F, 1)), dim3(256), 0, (hipStream_t)stream, d_order_llr, d_metric_llr,
                       (long long)F, d_lri, d_uidx, reinterpret_cast<const u64 *>(d_M),
                       reinterpret_cast<const uchar4 *>(d_teps), d_block_off, (int)nblk,
                       reinterpret_cast<const u64 *>(d_label_bits), d_block_min, d_block_arg, d_truth,
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_best);
    hipLaunchKernelGGL(hosd_search_kernel<false>, dim3(grid_for(F, 1)), dim3(256), 0, (hipStream_t)stream, d_order_llr, d_metric_llr,
                       (long long)F, d_lri, d_uidx, reinterpret_cast<const u64 *>(d_M),
                       reinterpret_cast<const uchar4 *>(d_teps), d_block_off, (int)nblk,
                       reinterpret_cast<const u64 *>(d_label_bits), d_block_min, d_block_arg, d_truth,
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_best);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_hosd_sliding(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                      const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                      int32_t nblk, int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights,
                      int32_t group, const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min,
                      float *d_truth, uint8_t *d_success, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                      int32_t *d_teps_evaluated, void *stream)
{
    if (!ctx || F < 0 || win < 1 || win > kSlideMaxWin || nblk < win || group < 0 || !fcn_weights ||
        (F > 0 && (!d_order_llr || !d_metric_llr || !d_lri || !d_uidx || !d_M || !d_teps || !d_block_off)))
        return fail(LDPC_E_ARG, "ldpc_hosd_sliding: bad arguments (win %d, nblk %d, group %d)", (int)win, (int)nblk, (int)group);
    const int d = win + 1;
    if (n_weights != d * d + 2 * d)
        return fail(LDPC_E_ARG, "ldpc_hosd_sliding: %d classifier weights, a window of %d takes %d", (int)n_weights, (int)win,
                    d * d + 2 * d);
    if ((d_truth || d_success) && !d_label_bits) return fail(LDPC_E_ARG, "ldpc_hosd_sliding: d_truth / d_success need d_label_bits");
    if (!ctx->hosd_ok)
        return fail(LDPC_E_UNSUPPORTED, "H-form OSD kernels need n=128, m=k=64; this code is n=%d m=%d k=%d", ctx->code.n,
                    ctx->code.m, ctx->code.k);
    if (nblk > kHosdMaxBlocks) return fail(LDPC_E_UNSUPPORTED, "ldpc_hosd_sliding: %d TEP blocks, at most %d", nblk, kHosdMaxBlocks);
    if (F == 0) return LDPC_OK;
    SlideFcnArg w = {};
    for (int i = 0; i < d * d; ++i) w.w1[i] = fcn_weights[i];
    for (int i = 0; i < 2 * d; ++i) w.w2[i] = fcn_weights[d * d + i];
    hipLaunchKernelGGL(hosd_sliding_kernel, dim3(grid_for(F, 1)), dim3(256), 0, (hipStream_t)stream, d_order_llr, d_metric_llr,
                       (long long)F, d_lri, d_uidx, reinterpret_cast<const u64 *>(d_M), reinterpret_cast<const uchar4 *>(d_teps),
                       d_block_off, (int)nblk, (int)win, soft_margin, w, (int)group, reinterpret_cast<const u64 *>(d_label_bits),
                       d_deep_limit, d_global_min, d_truth, d_success, reinterpret_cast<u64 *>(d_cw), d_metric, d_best,
                       d_teps_evaluated);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_hosdx_supported(const ldpc_ctx *ctx) { return ctx && ctx->hosdx_ok ? 1 : 0; }

int ldpc_hosdx_front(ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint8_t *d_lri, uint8_t *d_uidx, uint64_t *d_M,
                     int32_t *d_nswaps, void *stream)
{
    const char *who = "ldpc_hosdx_front";
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "%s: bad arguments (ctx %p, F %lld)", who, (void *)ctx, (long long)F);
    if (F > 0)
        if (int rc = first_null(who, {{"d_order_llr", d_order_llr}, {"d_lri", d_lri}, {"d_uidx", d_uidx}, {"d_M", d_M}})) return rc;
    if (int rc = hosdx_check(ctx, who)) return rc;
    if (F == 0) return LDPC_OK;
    hipLaunchKernelGGL(hosdx_front_kernel, dim3(grid_for(F, 4)), dim3(256), 0, (hipStream_t)stream, d_order_llr, (long long)F,
                       ctx->code.n, ctx->code.m, reinterpret_cast<const u64 *>(ctx->d_Hcols), d_lri, d_uidx,
                       reinterpret_cast<u64 *>(d_M), d_nswaps);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_hosdx_search(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                      const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                      int32_t nblk, const uint64_t *d_label_bits, float *d_block_min, int32_t *d_block_arg, float *d_truth,
                      uint64_t *d_cw, float *d_metric, int32_t *d_best, void *stream)
{
    const char *who = "ldpc_hosdx_search";
    if (!ctx || F < 0 || nblk < 0)
        return fail(LDPC_E_ARG, "%s: bad arguments (ctx %p, F %lld, nblk %d)", who, (void *)ctx, (long long)F, (int)nblk);
    if (F > 0) {
        if (int rc = first_null(who, {{"d_order_llr", d_order_llr}, {"d_metric_llr", d_metric_llr}, {"d_lri", d_lri},
                                      {"d_uidx", d_uidx}, {"d_M", d_M}, {"d_block_off", d_block_off}})) return rc;
        if (nblk > 0)     // (the kernels read d_teps[0 .. d_block_off[nblk]), device data)
            if (int rc = first_null(who, {{"d_teps", d_teps}, {"d_block_min", d_block_min}})) return rc;
    }
    if (d_truth && !d_label_bits) return fail(LDPC_E_ARG, "%s: d_truth needs d_label_bits", who);
    if (int rc = hosdx_check(ctx, who)) return rc;
    if (nblk > kHosdMaxBlocks) return fail(LDPC_E_UNSUPPORTED, "%s: %d TEP blocks, at most %d", who, nblk, kHosdMaxBlocks);
    if (F == 0) return LDPC_OK;
    // (the TEP table's size is device data: both forms are launched and one of them returns at once)
    hipLaunchKernelGGL(hosdx_search_kernel<true>, dim3(grid_for(F, 1)), dim3(256), 0, (hipStream_t)stream, d_order_llr, d_metric_llr,
                       (long long)F, ctx->code.n, ctx->code.m, d_lri, d_uidx, reinterpret_cast<const u64 *>(d_M),
                       reinterpret_cast<const uchar4 *>(d_teps), d_block_off, (int)nblk,
                       reinterpret_cast<const u64 *>(d_label_bits), d_block_min, d_block_arg, d_truth,
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_best);
    hipLaunchKernelGGL(hosdx_search_kernel<false>, dim3(grid_for(F, 1)), dim3(256), 0, (hipStream_t)stream, d_order_llr, d_metric_llr,
                       (long long)F, ctx->code.n, ctx->code.m, d_lri, d_uidx, reinterpret_cast<const u64 *>(d_M),
                       reinterpret_cast<const uchar4 *>(d_teps), d_block_off, (int)nblk,
                       reinterpret_cast<const u64 *>(d_label_bits), d_block_min, d_block_arg, d_truth,
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_best);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_hosdx_sliding(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                       const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                       int32_t nblk, int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights,
                       int32_t group, const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min,
                       float *d_truth, uint8_t *d_success, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                       int32_t *d_teps_evaluated, void *stream)
{
    const char *who = "ldpc_hosdx_sliding";
    if (!ctx || F < 0 || win < 1 || win > kSlideMaxWin || nblk < win || group < 0)
        return fail(LDPC_E_ARG, "%s: bad arguments (ctx %p, F %lld, win %d, nblk %d, group %d)", who, (void *)ctx, (long long)F,
                    (int)win, (int)nblk, (int)group);
    if (int rc = first_null(who, {{"fcn_weights", fcn_weights}})) return rc;
    if (F > 0)
        if (int rc = first_null(who, {{"d_order_llr", d_order_llr}, {"d_metric_llr", d_metric_llr}, {"d_lri", d_lri},
                                      {"d_uidx", d_uidx}, {"d_M", d_M}, {"d_teps", d_teps}, {"d_block_off", d_block_off}})) return rc;
    const int d = win + 1;
    if (n_weights != d * d + 2 * d)
        return fail(LDPC_E_ARG, "%s: %d classifier weights, a window of %d takes %d", who, (int)n_weights, (int)win, d * d + 2 * d);
    if ((d_truth || d_success) && !d_label_bits) return fail(LDPC_E_ARG, "%s: d_truth / d_success need d_label_bits", who);
    if (int rc = hosdx_check(ctx, who)) return rc;
    if (nblk > kHosdMaxBlocks) return fail(LDPC_E_UNSUPPORTED, "%s: %d TEP blocks, at most %d", who, nblk, kHosdMaxBlocks);
    if (F == 0) return LDPC_OK;
    SlideFcnArg w = {};
    for (int i = 0; i < d * d; ++i) w.w1[i] = fcn_weights[i];
    for (int i = 0; i < 2 * d; ++i) w.w2[i] = fcn_weights[d * d + i];
    hipLaunchKernelGGL(hosdx_sliding_kernel, dim3(grid_for(F, 1)), dim3(256), 0, (hipStream_t)stream, d_order_llr, d_metric_llr,
                       (long long)F, ctx->code.n, ctx->code.m, d_lri, d_uidx, reinterpret_cast<const u64 *>(d_M),
                       reinterpret_cast<const uchar4 *>(d_teps), d_block_off, (int)nblk, (int)win, soft_margin, w, (int)group,
                       reinterpret_cast<const u64 *>(d_label_bits), d_deep_limit, d_global_min, d_truth, d_success,
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_best, d_teps_evaluated);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_hosdw_supported(const ldpc_ctx *ctx) { return ctx && ctx->hosdw_ok ? 1 : 0; }

int ldpc_hosdw_front(ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint8_t *d_lri, uint8_t *d_uidx, uint64_t *d_M,
                     int32_t *d_nswaps, void *stream)
{
    const char *who = "ldpc_hosdw_front";
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "%s: bad arguments (ctx %p, F %lld)", who, (void *)ctx, (long long)F);
    if (F > 0)
        if (int rc = first_null(who, {{"d_order_llr", d_order_llr}, {"d_lri", d_lri}, {"d_uidx", d_uidx}, {"d_M", d_M}})) return rc;
    if (int rc = hosdw_check(ctx, who)) return rc;
    if (F == 0) return LDPC_OK;
    hipLaunchKernelGGL(hosdw_front_kernel, dim3(grid_for(F, 4)), dim3(256), 0, (hipStream_t)stream, d_order_llr, (long long)F,
                       ctx->code.n, ctx->code.m, ctx->code.n - ctx->code.k, reinterpret_cast<const u64 *>(ctx->d_HcolsW), d_lri, d_uidx,
                       reinterpret_cast<u64 *>(d_M), d_nswaps);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_hosdw_search(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                      const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                      int32_t nblk, const uint64_t *d_label_bits, float *d_block_min, int32_t *d_block_arg, float *d_truth,
                      uint64_t *d_cw, float *d_metric, int32_t *d_best, void *stream)
{
    const char *who = "ldpc_hosdw_search";
    if (!ctx || F < 0 || nblk < 0)
        return fail(LDPC_E_ARG, "%s: bad arguments (ctx %p, F %lld, nblk %d)", who, (void *)ctx, (long long)F, (int)nblk);
    if (F > 0) {
        if (int rc = first_null(who, {{"d_order_llr", d_order_llr}, {"d_metric_llr", d_metric_llr}, {"d_lri", d_lri},
                                      {"d_uidx", d_uidx}, {"d_M", d_M}, {"d_block_off", d_block_off}})) return rc;
        if (nblk > 0)     // (the kernels read d_teps[0 .. d_block_off[nblk]), device data)
            if (int rc = first_null(who, {{"d_teps", d_teps}, {"d_block_min", d_block_min}})) return rc;
    }
    if (d_truth && !d_label_bits) return fail(LDPC_E_ARG, "%s: d_truth needs d_label_bits", who);
    if (int rc = hosdw_check(ctx, who)) return rc;
    if (nblk > kHosdMaxBlocks) return fail(LDPC_E_UNSUPPORTED, "%s: %d TEP blocks, at most %d", who, nblk, kHosdMaxBlocks);
    if (F == 0) return LDPC_OK;
    // (the TEP table's size is device data: both forms are launched and one of them returns at once)
    hipLaunchKernelGGL(hosdw_search_kernel<true>, dim3(grid_for(F, 1)), dim3(256), 0, (hipStream_t)stream, d_order_llr, d_metric_llr,
                       (long long)F, ctx->code.n, ctx->code.n - ctx->code.k, d_lri, d_uidx, reinterpret_cast<const u64 *>(d_M),
                       reinterpret_cast<const uchar4 *>(d_teps), d_block_off, (int)nblk,
                       reinterpret_cast<const u64 *>(d_label_bits), d_block_min, d_block_arg, d_truth,
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_best);
    hipLaunchKernelGGL(hosdw_search_kernel<false>, dim3(grid_for(F, 1)), dim3(256), 0, (hipStream_t)stream, d_order_llr, d_metric_llr,
                       (long long)F, ctx->code.n, ctx->code.n - ctx->code.k, d_lri, d_uidx, reinterpret_cast<const u64 *>(d_M),
                       reinterpret_cast<const uchar4 *>(d_teps), d_block_off, (int)nblk,
                       reinterpret_cast<const u64 *>(d_label_bits), d_block_min, d_block_arg, d_truth,
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_best);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_hosdw_sliding(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                       const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                       int32_t nblk, int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights,
                       int32_t group, const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min,
                       float *d_truth, uint8_t *d_success, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                       int32_t *d_teps_evaluated, void *stream)
{
    const char *who = "ldpc_hosdw_sliding";
    if (!ctx || F < 0 || win < 1 || win > kSlideMaxWin || nblk < win || group < 0)
        return fail(LDPC_E_ARG, "%s: bad arguments (ctx %p, F %lld, win %d, nblk %d, group %d)", who, (void *)ctx, (long long)F,
                    (int)win, (int)nblk, (int)group);
    if (int rc = first_null(who, {{"fcn_weights", fcn_weights}})) return rc;
    if (F > 0)
        if (int rc = first_null(who, {{"d_order_llr", d_order_llr}, {"d_metric_llr", d_metric_llr}, {"d_lri", d_lri},
                                      {"d_uidx", d_uidx}, {"d_M", d_M}, {"d_teps", d_teps}, {"d_block_off", d_block_off}})) return rc;
    const int d = win + 1;
    if (n_weights != d * d + 2 * d)
        return fail(LDPC_E_ARG, "%s: %d classifier weights, a window of %d takes %d", who, (int)n_weights, (int)win, d * d + 2 * d);
    if ((d_truth || d_success) && !d_label_bits) return fail(LDPC_E_ARG, "%s: d_truth / d_success need d_label_bits", who);
    if (int rc = hosdw_check(ctx, who)) return rc;
    if (nblk > kHosdMaxBlocks) return fail(LDPC_E_UNSUPPORTED, "%s: %d TEP blocks, at most %d", who, nblk, kHosdMaxBlocks);
    if (F == 0) return LDPC_OK;
    SlideFcnArg w = {};
    for (int i = 0; i < d * d; ++i) w.w1[i] = fcn_weights[i];
    for (int i = 0; i < 2 * d; ++i) w.w2[i] = fcn_weights[d * d + i];
    hipLaunchKernelGGL(hosdw_sliding_kernel, dim3(grid_for(F, 1)), dim3(256), 0, (hipStream_t)stream, d_order_llr, d_metric_llr,
                       (long long)F, ctx->code.n, ctx->code.n - ctx->code.k, d_lri, d_uidx, reinterpret_cast<const u64 *>(d_M),
                       reinterpret_cast<const uchar4 *>(d_teps), d_block_off, (int)nblk, (int)win, soft_margin, w, (int)group,
                       reinterpret_cast<const u64 *>(d_label_bits), d_deep_limit, d_global_min, d_truth, d_success,
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_best, d_teps_evaluated);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_fcn_windows(ldpc_ctx *ctx, const float *d_block_min, const uint8_t *d_success, const int32_t *d_index, int64_t R,
                     int32_t nblk, int32_t win, float *d_inputs, uint8_t *d_labels, int64_t *d_class_count, void *stream)
{
    static const char who[] = "ldpc_fcn_windows";
    if (!ctx) return fail(LDPC_E_ARG, "%s: ctx is NULL", who);
    if (R < 0) return fail(LDPC_E_ARG, "%s: R = %lld is negative", who, (long long)R);
    if (win < 1 || win > kSlideMaxWin) return fail(LDPC_E_ARG, "%s: win = %d outside 1..%d", who, (int)win, kSlideMaxWin);
    if (nblk < win || nblk > kHosdMaxBlocks)
        return fail(LDPC_E_ARG, "%s: nblk = %d outside win = %d .. %d", who, (int)nblk, (int)win, kHosdMaxBlocks);
    if (R == 0) return LDPC_OK;
    if (int rc = first_null(who, {{"d_block_min", d_block_min}, {"d_success", d_success}, {"d_inputs", d_inputs},
                                  {"d_labels", d_labels}})) return rc;
    return fcn_windows_run(d_block_min, d_success, d_index, R, nblk, win, d_inputs, d_labels, d_class_count, (hipStream_t)stream);
}

int ldpc_fcn_grad(ldpc_ctx *ctx, const float *d_inputs, const uint8_t *d_labels, const float *d_weight, const int32_t *d_index,
                  int64_t B, int32_t win, const float *fcn_weights, int32_t n_weights, float penalty, float *d_p,
                  double *d_loss_sum, double *d_grad_sum, double *d_acc, int64_t *d_counts, void *stream)
{
    static const char who[] = "ldpc_fcn_grad";
    if (!ctx) return fail(LDPC_E_ARG, "%s: ctx is NULL", who);
    if (B < 0) return fail(LDPC_E_ARG, "%s: B = %lld is negative", who, (long long)B);
    if (win < 1 || win > kSlideMaxWin) return fail(LDPC_E_ARG, "%s: win = %d outside 1..%d", who, (int)win, kSlideMaxWin);
    const int d = win + 1, want = d * d + 2 * d;
    if (n_weights != want) return fail(LDPC_E_ARG, "%s: n_weights = %d, win = %d takes %d", who, (int)n_weights, (int)win, want);
    if (int rc = first_null(who, {{"fcn_weights", fcn_weights}})) return rc;
    if (B == 0) return LDPC_OK;
    if (int rc = first_null(who, {{"d_inputs", d_inputs}})) return rc;
    const bool sums = d_loss_sum || d_grad_sum || d_acc || d_counts;
    if (sums)
        if (int rc = first_null(who, {{"d_labels", d_labels}})) return rc;
    if (!sums && !d_p) return LDPC_OK;
    SlideFcnArg w = {};
    for (int i = 0; i < d * d; ++i) w.w1[i] = fcn_weights[i];
    for (int i = 0; i < 2 * d; ++i) w.w2[i] = fcn_weights[d * d + i];
    return fcn_grad_run(d_inputs, d_labels, d_weight, d_index, B, win, w, penalty, d_p, d_loss_sum, d_grad_sum, d_acc, d_counts,
                        (hipStream_t)stream);
}

}  // extern "C"
