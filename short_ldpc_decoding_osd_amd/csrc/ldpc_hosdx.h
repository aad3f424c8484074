// H-form ordered-statistics primitives for short codes of any shape (1 <= k <= 64, 1 <= m = n - k <= 64, H of m rows), the
// code's n and m as kernel arguments: what this family owns -- its front end, its LDS plan with two-word columns, its metric
// over ceil(n / 8) bytes and its per-frame set-up -- and its traits (HosdX) for the scans of ldpc_hosd_scan.h, which its
// search and sliding kernels call.  Included from ldpc_hosd.hip after ldpc_hosd_scan.h.
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
template <class... COUNT>   // (the counted form: ldpc_wave.h)
__global__ __launch_bounds__(256) void hosdx_front_kernel(const float *__restrict__ x, long long F, int n, int m,
                                                          const u64 *__restrict__ Hcols, unsigned char *__restrict__ lri_out,
                                                          unsigned char *__restrict__ uidx_out, u64 *__restrict__ M_out,
                                                          int *__restrict__ nswaps, COUNT... count)
{
    if constexpr (kCounted<COUNT...>) {
        F = counted_frames(F, count...);
        if ((long long)blockIdx.x * 4 >= F) return;   // (the grid is sized by the capacity, not by the count)
    }
    __shared__ HFrontXLds lds[4];
    const int lane = threadIdx.x & 63;
    HFrontXLds &L = lds[threadIdx.x >> 6];
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int k = n - m;
    const bool in1 = lane < n, in2 = 64 + lane < n;      // slots lane / 64 + lane hold an original bit
    const bool live1 = lane < m, live2 = lane < k;       // lanes that own a column of the LRB / MRB side

    for (long long f = wave; f < F; f += (long long)gridDim.x * 4) {
        hosd_sort_ascending(L, x, f, n, lane);               // mag_input_gen (:25-28), padded slots last
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

// ---- the two parts of the per-frame set-up that this family and the wide one (ldpc_hosdw.h) share ----------------------
// Threads 0..127 (tid = updated position): values in updated order (:172-176) into L.o / L.w, and the two ballots per
// wavefront: hard decisions of the metric input (order_hard_original :180) into L.hgL / L.hgM, those of the ordering input at
// the MRB's positions m..n-1 (initial_mrb :186-187) into L.h0L / L.h0H.  lri / uidx entries >= n are not looked at.
template <class LDS>
__device__ __forceinline__ void hosdx_updated_values(LDS &L, const HShapeNM &sh, const HScanIn &in, long long f)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = sh.n;
    const bool live = tid < n;
    int o = 0;
    float mv = 0.0f;
    bool h0 = false;
    if (live) {
        o = in.lri[f * 128 + (in.uidx[f * 128 + tid] & 127)];
        o = o < n ? o : 0;                                            // (front-end results hold original bits < n)
        mv = in.xm[f * n + o];
        h0 = tid >= sh.m && !(in.xo[f * n + o] > 0.0f);
    }
    L.o[tid] = (unsigned char)o;
    L.w[tid] = __builtin_fabsf(mv);
    const u64 hg = __ballot(live && !(mv > 0.0f));
    const u64 hb = __ballot(h0);
    if (lane == 0) {
        if (wave == 0) { L.hgL = hg; L.h0L = hb; }
        else { L.hgM = hg; L.h0H = hb; }
    }
}

// Wavefront 1, with labels, after the LUTs are built: the label's metric (:181-183) into L.truth, and truth[f] where given.
template <class LDS>
__device__ __forceinline__ void hosdx_label_metric(LDS &L, const HShapeNM &sh, const u64 *__restrict__ label, long long f,
                                                   float *__restrict__ truth)
{
    const int lane = threadIdx.x & 63, n = sh.n, words = sh.words;
    const u64 l0 = label[f * words], l1 = words > 1 ? label[f * words + 1] : 0ull;
    const int o1 = L.o[lane], o2 = L.o[64 + lane];
    const u64 labL = __ballot(lane < n && (((o1 < 64 ? l0 : l1) >> (o1 & 63)) & 1));
    const u64 labM = __ballot(64 + lane < n && (((o2 < 64 ? l0 : l1) >> (o2 & 63)) & 1));
    const float t = hosdx_cost(L, labL ^ L.hgL, labM ^ L.hgM, sh.nb);
    if (lane == 0) { if (truth) truth[f] = t; L.truth = t; }
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

// The per-frame set-up for any shape: values in updated order, hard decisions, the two-word columns, block keys reset, the byte
// LUTs, the order-0 discrepancy (D0lo, D0hi) and (with labels) the label's metric (L.truth, and truth[f] where truth is given).
// Rows >= m and bits >= k of Mrows, and lri / uidx entries >= n, are not looked at.
// On return every thread sees the LUTs, the columns and the keys of blocks 0..nblk-1 reset to ~0.
template <class LDS>
__device__ __forceinline__ void hosdx_frame_setup(LDS &L, const HShapeNM &sh, const HScanIn &in, long long f, float *__restrict__ truth,
                                                  u64 &D0lo, u64 &D0hi)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = sh.n, m = sh.m, k = n - m, nb = sh.nb, nblk = in.nblk;
    // ---- phase 0: values in updated order, hard decisions, columns, key reset --------
    if (tid < 128) {
        hosdx_updated_values(L, sh, in, f);
    } else if (wave == 2) {
        const u64 kmask = k >= 64 ? ~0ull : ((1ull << k) - 1ull);
        const u64 col = transpose64(lane < m ? (in.Mrows[f * 64 + lane] & kmask) : 0ull, lane);   // lane j: bit r = M[r][j]
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
    if (in.label && wave == 1) hosdx_label_metric(L, sh, in.label, f, truth);
}

// The any-shape family for the scans of ldpc_hosd_scan.h: 64 two-word columns, the kernel's n and m, TEP positions of 6 bits
// taken modulo 64.
struct HosdX {
    template <bool RUNS> using Lds = HSearchXLds<RUNS>;
    static constexpr int kPosBits = 6;
    static __device__ __forceinline__ unsigned pos(unsigned char v) { return v & 63; }
    template <class LDS> static __device__ __forceinline__ float cost(const LDS &L, u64 lo, u64 hi, const HShapeNM &sh) { return hosdx_cost(L, lo, hi, sh.nb); }
    template <class LDS>
    static __device__ __forceinline__ void setup(LDS &L, const HShapeNM &sh, const HScanIn &in, long long f, float *__restrict__ truth, u64 &D0lo,
                                                 u64 &D0hi)
    {
        hosdx_frame_setup(L, sh, in, f, truth, D0lo, D0hi);
    }
};

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
    __shared__ HosdX::Lds<RUNS> L;
    hosd_search_body<HosdX, RUNS>(L, HShapeNM(n, m), {xo, xm, F, lri, uidx, Mrows, teps, block_off, nblk, label}, block_min, block_arg,
                                  {truth, cw_out, metric_out, best_out});
}

HOSD_SLIDING_KERNEL(hosdx_sliding_kernel, HosdX, HOSD_NM_SHAPE_PARAMS, HShapeNM sh(n, m))

}  // namespace ldpc
