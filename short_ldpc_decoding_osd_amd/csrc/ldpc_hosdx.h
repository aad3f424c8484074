// H-form ordered-statistics primitives for short codes of any shape (1 <= k <= 64, 1 <= m = n - k <= 64, H of m rows): the
// kernels of ldpc_hosd.hip with the code's n and m as kernel arguments.  Included from ldpc_hosd.hip, after the (128,64)
// kernels whose helpers it shares: hosd_frame_best, SlideLds / slide_p1 / key_metric, the kHosd* limits.
//   mag_input_gen / check_matrix_reorder   ordered_statistics_decoding.py:25-41
//   identify_mrb / full_gf2elim            ordered_statistics_decoding.py:43-80, 222-257
//   acquire_min / sliding_osd              ordered_statistics_decoding.py:153-218
// Front end: lane l owns sorted column l (live for l < m: the columns the identity is built on) and sorted column m + l (live
// for l < k); idle slots carry zero columns.  The elimination is gex_columns (ldpc_wave.h) on m rows: the H form is the G form
// with m rows, n columns and the sort reversed.
// Scans: the n updated positions are ONE sequence, LRB (0..m-1) first, and a frame's discrepancy is one 128-bit value in that
// order, D = DL | DM << m, kept as two words (positions 0..63, 64..127).  MRB position j owns the two-word column
// Mcol[j] | 1 << (m + j), so a TEP is at most three two-word XORs, and the metric reads the ceil(n / 8) bytes of D through the
// byte LUTs.  On (128,64) the two words are DL and DM of ldpc_hosd.hip and every result is the same bit for bit.
#pragma once

#include "ldpc_wave.h"

namespace ldpc {

struct __attribute__((aligned(16))) HFrontXLds {
    RankLds rank;              // reliability sort (bucket_ranks, ldpc_wave.h)
    u64 colbuf[64];            // M columns in updated MRB order, bit = physical row (zero beyond k)
    unsigned mask[4];          // which sorted positions ended up in the MRB
    unsigned char lri[128];    // sorted position -> original bit
    unsigned char uidx[128];   // updated position -> sorted position (zero beyond n)
};

// One frame per wavefront.  lri_out / uidx_out [F][128]: entries >= n are written as 0; M_out [F][64]: rows >= m and bits >= k
// are written as 0.
__global__ __launch_bounds__(256) void hosdx_front_kernel(const float *__restrict__ x, long long F, int n, int m,
                                                          const u64 *__restrict__ Hcols, unsigned char *__restrict__ lri_out,
                                                          unsigned char *__restrict__ uidx_out, u64 *__restrict__ M_out,
                                                          int *__restrict__ nswaps)
{
    __shared__ HFrontXLds lds[4];
    const int lane = threadIdx.x & 63;
    HFrontXLds &L = lds[threadIdx.x >> 6];
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int k = n - m;
    const bool in1 = lane < n, in2 = 64 + lane < n;      // slots lane / 64 + lane hold an original bit
    const bool live1 = lane < m, live2 = lane < k;       // lanes that own a column of the LRB / MRB side

    for (long long f = wave; f < F; f += (long long)gridDim.x * 4) {
        // ---- mag_input_gen (:25-28): rank in ascending |x|, ties -> lower index ------------
        // ascending order of (|x| bits, index) = descending order of the complemented key, buckets mirrored.  A slot at or
        // beyond n takes the magnitude word 0xFFFFFFFF, above every real one (<= 0x7FFFFFFF), and the lowest mirrored bucket:
        // its complemented key (0, ~slot) lies below every real key whatever the frame holds, so the real positions take
        // ranks 0..n-1 in the order their own keys define.  The bucket scale comes from the real magnitudes alone.
        const unsigned a1 = in1 ? (__float_as_uint(x[f * n + lane]) & 0x7FFFFFFFu) : 0u;
        const unsigned a2 = in2 ? (__float_as_uint(x[f * n + 64 + lane]) & 0x7FFFFFFFu) : 0u;
        const float bs = bucket_scale(a1, a2);
        const u64 k1 = in1 ? ~(((u64)a1 << 32) | (unsigned)lane) : (u64)(unsigned)~(unsigned)lane;
        const u64 k2 = in2 ? ~(((u64)a2 << 32) | (unsigned)(lane + 64)) : (u64)(unsigned)~(unsigned)(lane + 64);
        int r1, r2;
        bucket_ranks(L.rank, k1, k2, in1 ? 63 - bucket_of(a1, bs) : 0, in2 ? 63 - bucket_of(a2, bs) : 0, lane, r1, r2);
        L.lri[r1] = (unsigned char)lane;
        L.lri[r2] = (unsigned char)(lane + 64);
        if (lane < 4) L.mask[lane] = 0;
        L.colbuf[lane] = 0ull;
        L.uidx[lane] = 0; L.uidx[lane + 64] = 0;
        wave_fence();
        // ---- H with columns in sorted order (:38-40), column-major, then full_gf2elim (:222-257) on m rows
        const int s1 = L.lri[lane], s2 = L.lri[lane + 64];
        u64 C1 = live1 ? Hcols[s1] : 0ull;
        u64 C2 = live2 ? Hcols[L.lri[m + lane]] : 0ull;      // (m + lane < n <= 128)
        int rho = lane, idx1 = lane, idx2 = m + lane;
        const int ns = gex_columns(C1, C2, rho, idx1, idx2, m, lane);
        // ---- identify_mrb (:58-69): LRB = index_order[:m] as left by the elimination, MRB sorted
        if (live2) atomicOr(&L.mask[idx2 >> 5], 1u << (idx2 & 31));
        wave_fence();
        const unsigned mk[4] = {L.mask[0], L.mask[1], L.mask[2], L.mask[3]};
        const int rankM = live2 ? below_mask(mk, idx2) : 0;   // updated MRB position of column m + lane
        if (live1) L.uidx[lane] = (unsigned char)idx1;
        if (live2) {
            L.uidx[m + rankM] = (unsigned char)idx2;
            L.colbuf[rankM] = C2;
        }
        wave_fence();
        // rows of updated_M: transpose to (lane = physical row, bit = MRB position), then logical row
        // r = the row whose pivot sits in column r = physical row rho[r]  (idle lanes kept rho = lane)
        const u64 R = transpose64(L.colbuf[lane], lane);
        const u64 Mrow = shfl64(R, rho);
        M_out[f * 64 + lane] = live1 ? Mrow : 0ull;
        lri_out[f * 128 + lane] = in1 ? (unsigned char)s1 : (unsigned char)0;
        lri_out[f * 128 + 64 + lane] = in2 ? (unsigned char)s2 : (unsigned char)0;
        uidx_out[f * 128 + lane] = L.uidx[lane];
        uidx_out[f * 128 + 64 + lane] = L.uidx[64 + lane];
        if (nswaps && lane == 0) nswaps[f] = ns;
        wave_fence();
    }
}

// The LDS plan of HSearchLds with the two-word columns: 0.5 KiB more (RUNS: 23.9 KiB, still 6 workgroups per CU).
template <bool RUNS>
struct __attribute__((aligned(16))) HSearchXLds {
    float lut[16][256];   // lut[b][v]: partial metric of discrepancy byte b (updated positions 8b..8b+7); built for b < 4 ceil(nb / 4)
    ulonglong2 Mcol[64];  // MRB position j < k: column j of updated_M (bit r < m) | 1 << (m + j), as two words; zero for j >= k
    float w[128];         // |metric_llr| in updated order, zero beyond n
    u64 keys[RUNS ? kHosdRunBlocks : kHosdMaxBlocks];   // per block: (metric bits << 32) | TEP index, minimum = first minimum
    u64 hgL, hgM;         // hard decisions of the metric input at updated positions 0..63 / 64..127
    u64 h0L, h0H;         // hard decisions of the ordering input at the MRB's updated positions m..n-1, same two words
    u64 DL0, best, cw[2];
    int ticket, heavy;
    float truth;          // the label's metric (hosdx_frame_setup with labels)
    unsigned char o[128]; // original bit index of updated position p (zero beyond n)
    int boff[RUNS ? kHosdRunBlocks + 1 : 1];            // block_off, once per workgroup
    unsigned short tl[RUNS ? kHosdLdsTeps : 2];         // the TEP table, once per workgroup: x | y << 6 | weight << 12
};

// The metric over the nb = ceil(n / 8) bytes of the discrepancy, summed ascending from byte 0.  The bytes are read in fours
// (one wave-uniform branch each): a LUT of the last four that lies at or beyond nb is all zeros, as is the part of a
// partial last byte's LUT beyond n (w = 0 there), and adding 0.0f changes no bit of a sum >= 0.
template <class LDS>
__device__ __forceinline__ float hosdx_cost(const LDS &L, u64 lo, u64 hi, int nb)
{
    float acc = lut_byte<0>(L.lut, lo);
    acc = acc + lut_byte<1>(L.lut, lo); acc = acc + lut_byte<2>(L.lut, lo); acc = acc + lut_byte<3>(L.lut, lo);
    if (nb > 4) {
        acc = acc + lut_byte<4>(L.lut, lo); acc = acc + lut_byte<5>(L.lut, lo); acc = acc + lut_byte<6>(L.lut, lo);
        acc = acc + lut_byte<7>(L.lut, lo);
    }
    if (nb > 8) {
        acc = acc + lut_byte<0>(&L.lut[8], hi); acc = acc + lut_byte<1>(&L.lut[8], hi); acc = acc + lut_byte<2>(&L.lut[8], hi);
        acc = acc + lut_byte<3>(&L.lut[8], hi);
    }
    if (nb > 12) {
        acc = acc + lut_byte<4>(&L.lut[8], hi); acc = acc + lut_byte<5>(&L.lut[8], hi); acc = acc + lut_byte<6>(&L.lut[8], hi);
        acc = acc + lut_byte<7>(&L.lut[8], hi);
    }
    return acc;
}

// hosd_apply on the two-word columns (the overload hosd_frame_best picks for this LDS type).  A TEP position is taken
// modulo 64: one at or beyond k is the caller's error and meets a zero column.
template <bool RUNS>
__device__ __forceinline__ void hosd_apply(const HSearchXLds<RUNS> &L, uchar4 s, u64 &lo, u64 &hi)
{
    if (s.w > 0) { const ulonglong2 c = L.Mcol[s.x & 63]; lo ^= c.x; hi ^= c.y; }
    if (s.w > 1) { const ulonglong2 c = L.Mcol[s.y & 63]; lo ^= c.x; hi ^= c.y; }
    if (s.w > 2) { const ulonglong2 c = L.Mcol[s.z & 63]; lo ^= c.x; hi ^= c.y; }
}

// hosd_frame_setup for any shape: values in updated order, hard decisions, the two-word columns, block keys reset, the byte
// LUTs, the order-0 discrepancy (D0lo, D0hi) and (with labels) the label's metric (L.truth, and truth[f] where truth is given).
// Rows >= m and bits >= k of Mrows, and lri / uidx entries >= n, are not looked at.
// On return every thread sees the LUTs, the columns and the keys of blocks 0..nblk-1 reset to ~0.
template <class LDS>
__device__ __forceinline__ void hosdx_frame_setup(LDS &L, const float *__restrict__ xo, const float *__restrict__ xm, long long f,
                                                  int n, int m, const unsigned char *__restrict__ lri,
                                                  const unsigned char *__restrict__ uidx, const u64 *__restrict__ Mrows, int nblk,
                                                  const u64 *__restrict__ label, float *__restrict__ truth, u64 &D0lo, u64 &D0hi)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = n - m, nb = (n + 7) >> 3, words = (n + 63) >> 6;
    // ---- phase 0: values in updated order (:172-176), hard decisions, columns, key reset --------
    if (tid < 128) {
        const bool live = tid < n;
        int o = 0;
        float mv = 0.0f;
        bool h0 = false;
        if (live) {
            o = lri[f * 128 + (uidx[f * 128 + tid] & 127)];
            o = o < n ? o : 0;                                            // (front-end results hold original bits < n)
            mv = xm[f * n + o];
            h0 = tid >= m && !(xo[f * n + o] > 0.0f);                     // initial_mrb (:186-187)
        }
        L.o[tid] = (unsigned char)o;
        L.w[tid] = __builtin_fabsf(mv);
        const u64 hg = __ballot(live && !(mv > 0.0f));                    // order_hard_original (:180)
        const u64 hb = __ballot(h0);
        if (lane == 0) {
            if (wave == 0) { L.hgL = hg; L.h0L = hb; }
            else { L.hgM = hg; L.h0H = hb; }
        }
    } else if (wave == 2) {
        const u64 kmask = k >= 64 ? ~0ull : ((1ull << k) - 1ull);
        const u64 col = transpose64(lane < m ? (Mrows[f * 64 + lane] & kmask) : 0ull, lane);   // lane j: bit r = M[r][j]
        const int p = m + lane;                                           // the updated position of MRB position `lane`
        const u64 unit = 1ull << (p & 63);
        ulonglong2 c;
        c.x = lane < k ? (col | (p < 64 ? unit : 0ull)) : 0ull;
        c.y = (lane < k && p >= 64) ? unit : 0ull;
        L.Mcol[lane] = c;
    } else {
        if (lane == 0) { L.ticket = 0; L.best = ~0ull; L.cw[0] = 0; L.cw[1] = 0; }
    }
    for (int b = tid; b < nblk; b += 256) L.keys[b] = ~0ull;
    __syncthreads();
    // ---- phase 1: byte LUTs (four per wavefront, the fours that hold a byte of the metric), order-0 discrepancy (:155,:159)
    if (4 * wave < nb) build_byte_luts<4>(&L.lut[4 * wave], &L.w[32 * wave], lane);
    if (wave == 0) {
        const u64 mrb0 = m >= 64 ? L.h0H : ((L.h0L >> m) | (L.h0H << (64 - m)));     // initial_mrb by MRB position
        const u64 rows = m >= 64 ? ~0ull : ((1ull << m) - 1ull);
        const u64 d = wave_xor64(((mrb0 >> lane) & 1) ? (L.Mcol[lane].x & rows) : 0ull);
        if (lane == 0) L.DL0 = d ^ L.hgL ^ L.h0L;
    }
    __syncthreads();
    D0lo = L.DL0; D0hi = L.hgM ^ L.h0H;
    if (label && wave == 1) {
        const u64 l0 = label[f * words], l1 = words > 1 ? label[f * words + 1] : 0ull;
        const int o1 = L.o[lane], o2 = L.o[64 + lane];
        const u64 labL = __ballot(lane < n && (((o1 < 64 ? l0 : l1) >> (o1 & 63)) & 1));
        const u64 labM = __ballot(64 + lane < n && (((o2 < 64 ? l0 : l1) >> (o2 & 63)) & 1));
        const float t = hosdx_cost(L, labL ^ L.hgL, labM ^ L.hgM, nb);    // (:181-183)
        if (lane == 0) { if (truth) truth[f] = t; L.truth = t; }
    }
}

// hosd_search_kernel for any shape: one frame per 256-thread workgroup, the per-thread-run form for a small table (RUNS) and
// the work-item form otherwise, decided alike from device data by both instantiations.
template <bool RUNS>
__global__ __launch_bounds__(256) void hosdx_search_kernel(const float *__restrict__ xo, const float *__restrict__ xm,
                                                           long long F, int n, int m, const unsigned char *__restrict__ lri,
                                                           const unsigned char *__restrict__ uidx,
                                                           const u64 *__restrict__ Mrows, const uchar4 *__restrict__ teps,
                                                           const int *__restrict__ block_off, int nblk,
                                                           const u64 *__restrict__ label, float *__restrict__ block_min,
                                                           int *__restrict__ block_arg, float *__restrict__ truth,
                                                           u64 *__restrict__ cw_out, float *__restrict__ metric_out,
                                                           int *__restrict__ best_out)
{
    __shared__ HSearchXLds<RUNS> L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = (n + 7) >> 3, words = (n + 63) >> 6;
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
        for (int t = tid; t < ntep; t += 256) { const uchar4 s = teps[t]; L.tl[t] = (unsigned short)((s.x & 63) | ((s.y & 63) << 6) | (s.w << 12)); }
        __syncthreads();
        const int per = ((ntep + 255) / 256) | 1;      // (odd: a lane's run starts on its own LDS bank)
        run0 = tid * per < ntep ? tid * per : ntep; run1 = run0 + per < ntep ? run0 + per : ntep;
        int lo = 0, hi = nblk;       // the block that holds TEP run0: the last b with boff[b] <= run0 (blocks may be empty)
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (L.boff[mid] <= run0) lo = mid; else hi = mid; }
        b0 = lo;
    }

    for (long long f = blockIdx.x; f < F; f += gridDim.x) {
        u64 DL0, DM0;
        hosdx_frame_setup(L, xo, xm, f, n, m, lri, uidx, Mrows, nblk, label, truth, DL0, DM0);
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
                const float c = hosdx_cost(L, DL, DM, nb);
                if (c < best) { best = c; bestt = t; }                     // ascending t: first minimum
            }
            if (best < INFINITY) atomicMin(&L.keys[b], ((u64)(unsigned)__float_as_int(best) << 32) | (unsigned)bestt);
        } else {
            // ---- phase 2: the scan; items are numbered block by block, slice by slice -----------------------
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
                    const float c = hosdx_cost(L, DL, DM, nb);
                    if (c < best) { best = c; bestt = t; }                 // ascending t per lane: first minimum
                }
                const int wl = wave_argmin_lane(best, bestt);
                if (lane == wl)
                    atomicMin(&L.keys[b], ((u64)(unsigned)__float_as_int(best) << 32) | (unsigned)bestt);
                ++item; s += kHosdChunk;
            }
        }
        __syncthreads();
        // ---- phase 3: per-block results, the overall first minimum, its codeword -------------------------
        u64 mine = ~0ull;
        for (int b = tid; b < nblk; b += 256) {
            const u64 key = L.keys[b];
            const bool empty = key == ~0ull;
            block_min[f * nblk + b] = empty ? INFINITY : __int_as_float((int)(key >> 32));
            if (block_arg) block_arg[f * nblk + b] = empty ? -1 : (int)(unsigned)key;
            mine = key < mine ? key : mine;
        }
        if (mine != ~0ull) atomicMin(&L.best, mine);
        __syncthreads();
        if (wave == 0) hosd_frame_best(L, teps, f, DL0, DM0, cw_out, metric_out, best_out, words);
        __syncthreads();
    }
}

// hosd_sliding_kernel for any shape: the block scan in groups with the reference's sliding-window early stop.
__global__ __launch_bounds__(256) void hosdx_sliding_kernel(const float *__restrict__ xo, const float *__restrict__ xm, long long F,
                                                            int n, int m, const unsigned char *__restrict__ lri,
                                                            const unsigned char *__restrict__ uidx, const u64 *__restrict__ Mrows,
                                                            const uchar4 *__restrict__ teps, const int *__restrict__ block_off,
                                                            int nblk, int win, double margin, SlideFcnArg fcn, int group,
                                                            const u64 *__restrict__ label, int *__restrict__ deep_out,
                                                            float *__restrict__ gmin_out, float *__restrict__ truth,
                                                            unsigned char *__restrict__ success, u64 *__restrict__ cw_out,
                                                            float *__restrict__ metric_out, int *__restrict__ best_out,
                                                            int *__restrict__ nteps_out)
{
    __shared__ HSearchXLds<false> L;
    __shared__ SlideLds S;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int nb = (n + 7) >> 3, words = (n + 63) >> 6;
    for (int b = tid; b <= nblk; b += 256) S.boff[b] = block_off[b];
    __syncthreads();

    for (long long f = blockIdx.x; f < F; f += gridDim.x) {
        u64 DL0, DM0;
        hosdx_frame_setup(L, xo, xm, f, n, m, lri, uidx, Mrows, nblk, label, truth, DL0, DM0);
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
                    const float c = hosdx_cost(L, DL, DM, nb);
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
        if (wave == 0) hosd_frame_best(L, teps, f, DL0, DM0, cw_out, metric_out, best_out, words);
        __syncthreads();
    }
}

}  // namespace ldpc
