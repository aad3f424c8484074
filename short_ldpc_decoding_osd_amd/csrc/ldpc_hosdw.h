// H-form ordered-statistics primitives for high-rate codes and for an H with redundant rows (n <= 128, H of R <= 127 rows and
// rank m <= 64 as given, k = n - m up to 127): what this family owns -- a front end with two-word columns on the row side,
// an LDS plan with 128 MRB columns and its per-frame set-up -- and its traits (HosdW) for the scans of ldpc_hosd_scan.h, which
// its search and sliding kernels call.  Included from ldpc_hosd.hip after ldpc_hosdx.h, whose metric (hosdx_cost) and shared
// set-up parts (hosdx_updated_values, hosdx_label_metric) it uses unchanged.
//   mag_input_gen / check_matrix_reorder   ordered_statistics_decoding.py:25-41
//   identify_mrb / full_gf2elim            ordered_statistics_decoding.py:43-80, 222-257
//   acquire_min / sliding_osd              ordered_statistics_decoding.py:153-218
// Front end: lane l owns sorted columns l and 64 + l (a slot at or beyond n carries a zero column), each column two words of
// PHYSICAL rows 0..63 / 64..127, and two entries of the logical-to-physical row map.  full_gf2elim deletes a row that it finds
// all-zero when column i has no pivot (:247-250), so which column exchange comes next depends on where the redundant rows
// sit: the elimination here works on all R rows as given and deletes logical rows as the reference does.  It stops after m
// pivot steps -- the rows still left are zero by rank and deleting them records nothing -- so a pivot column and the map
// entry of its row always lie in the lower slot; only the row side of a step needs both halves.
// Scans: as ldpc_hosdx.h, one 128-bit discrepancy D = DL | DM << m; MRB position j < k <= 127 owns the two-word column
// Mcol[j] | 1 << (m + j).  Wherever ldpc_hosdx_* serves the code every result is the same bit for bit.
#pragma once

#include "ldpc_wave.h"

namespace ldpc {

// bit p of the two-word column (w0, w1): p = 0..127, or (TALL = false: no row beyond 63 exists, w1 is zero) p = 0..63
template <bool TALL>
__device__ __forceinline__ bool hw_bit(u64 w0, u64 w1, int p)
{
    return (((TALL && (p & 64) ? w1 : w0) >> (p & 63)) & 1ull) != 0;
}

// One try at pivot step i < 64 with `nrows` logical rows left (full_gf2elim :229-257), columns in registers:
//   A0 A1 / B0 B1 : sorted columns lane / 64 + lane, bit = PHYSICAL row (rows >= R do not exist: those bits are zero)
//   rhoA / rhoB   : logical rows lane / 64 + lane -> physical row (entries at or beyond nrows are not looked at)
//   idxA / idxB   : the sorted position travelling with each column (:58-62)
// TALL: H has more than 64 rows.  Without it the upper words and the upper half of the row map are never looked at
// (R <= 64: A1 = B1 = 0 and nrows <= 64 throughout), which saves a ballot and half of the selects per step.
// Returns true when the step deleted logical row i instead of pivoting (the caller lowers nrows and tries step i again).
// gew_step<false> (ldpc_osdw.h) with the deletion in place of its rank-deficiency flag: every lane-varying choice on the
// common path is a select and nothing is indexed; the deletion is rare and wave-uniform and is branched on.
template <bool TALL>
__device__ __forceinline__ bool hgew_step(u64 &A0, u64 &A1, u64 &B0, u64 &B1, int &rhoA, int &rhoB, int &idxA, int &idxB, int i,
                                          int nrows, int lane, int &nsw)
{
    const u64 from = ~0ull << i;
    const u64 rowsA = nrows >= 64 ? ~0ull : ((1ull << nrows) - 1ull);
    const u64 rowsB = TALL && nrows > 64 ? ((1ull << (nrows - 64)) - 1ull) : 0ull;       // (nrows <= 127)
    u64 cj0 = readlane64(A0, i), cj1 = TALL ? readlane64(A1, i) : 0ull;
    u64 balA = __ballot(hw_bit<TALL>(cj0, cj1, rhoA)) & rowsA & from;    // logical rows >= i with a 1 in column i
    u64 balB = TALL ? (__ballot(hw_bit<TALL>(cj0, cj1, rhoB)) & rowsB) : 0ull;
    if ((balA | balB) == 0) {
        const int pri = __builtin_amdgcn_readlane(rhoA, i);
        const u64 b1 = __ballot(hw_bit<TALL>(A0, A1, pri)) & from;  // (columns < i are cleared in row i; idle slots are zero)
        const u64 b2 = __ballot(hw_bit<TALL>(B0, B1, pri));
        if ((b1 | b2) == 0) {
            // logical row i is zero in every column: it is removed and every later row moves down by one (:247-250)
            const int upA = __shfl(rhoA, (lane + 1) & 63, 64), upB = __shfl(rhoB, (lane + 1) & 63, 64);
            const int b0 = __builtin_amdgcn_readlane(rhoB, 0);     // the move from the upper half into lane 63 of the lower
            rhoA = lane < i ? rhoA : (lane == 63 ? b0 : upA);
            rhoB = lane == 63 ? rhoB : upB;
            return true;
        }
        // exchange column i with the first later column, in sorted order, that has a 1 in logical row i (:251-256)
        const bool lo = b1 != 0;
        const unsigned cl = lo ? __builtin_ctzll(b1) : __builtin_ctzll(b2);
        const u64 ca0 = readlane64(A0, cl), cb0 = readlane64(B0, cl);
        const u64 ca1 = TALL ? readlane64(A1, cl) : 0ull, cb1 = TALL ? readlane64(B1, cl) : 0ull;
        const int ia = __builtin_amdgcn_readlane(idxA, cl), ib = __builtin_amdgcn_readlane(idxB, cl);
        const u64 cc0 = lo ? ca0 : cb0, cc1 = lo ? ca1 : cb1;
        const int ic = lo ? ia : ib;
        const int ii = __builtin_amdgcn_readlane(idxA, i);
        const bool hit = (unsigned)lane == cl;
        A0 = (hit && lo) ? cj0 : A0;
        idxA = (hit && lo) ? ii : idxA;
        B0 = (hit && !lo) ? cj0 : B0;
        idxB = (hit && !lo) ? ii : idxB;
        A0 = (lane == i) ? cc0 : A0;
        idxA = (lane == i) ? ic : idxA;
        if constexpr (TALL) {
            A1 = (hit && lo) ? cj1 : A1;
            B1 = (hit && !lo) ? cj1 : B1;
            A1 = (lane == i) ? cc1 : A1;
        }
        ++nsw;
        cj0 = cc0; cj1 = cc1;                                      // the exchanged-in column has its 1 in logical row i
        balA = 1ull << i;
        balB = 0ull;
    }
    // the first logical row wins; exchange logical rows i and r (r == i: no change)
    const bool rlo = balA != 0;
    const int rl = rlo ? __builtin_ctzll(balA) : __builtin_ctzll(balB);
    const int pra = __builtin_amdgcn_readlane(rhoA, rl), prb = TALL ? __builtin_amdgcn_readlane(rhoB, rl) : 0;
    const int pr = rlo ? pra : prb;
    const int pi = __builtin_amdgcn_readlane(rhoA, i);
    rhoA = (rlo && lane == rl) ? pi : rhoA;
    if constexpr (TALL) rhoB = (!rlo && lane == rl) ? pi : rhoB;
    rhoA = (lane == i) ? pr : rhoA;
    // clear column i in every other row: the pivot column without its pivot
    const u64 pbit = 1ull << (pr & 63);
    const u64 e0 = cj0 & ~((TALL && (pr & 64)) ? 0ull : pbit);
    const bool ha = hw_bit<TALL>(A0, A1, pr), hb = hw_bit<TALL>(B0, B1, pr);
    A0 ^= ha ? e0 : 0ull;
    B0 ^= hb ? e0 : 0ull;
    if constexpr (TALL) {
        const u64 e1 = cj1 & ~((pr & 64) ? pbit : 0ull);
        A1 ^= ha ? e1 : 0ull;
        B1 ^= hb ? e1 : 0ull;
    }
    return false;
}

struct __attribute__((aligned(16))) HFrontWLds {
    RankLds rank;              // reliability sort (bucket_ranks, ldpc_wave.h); after it rank.bk holds the rows of M by physical row
    u64 col[2][128];           // M columns in updated MRB order, physical rows 0..63 / 64..127 (zero beyond k)
    unsigned mask[4];          // which sorted positions ended up in the MRB
    unsigned char lri[128];    // sorted position -> original bit
    unsigned char uidx[128];   // updated position -> sorted position (zero beyond n)
};

// One frame per wavefront.  R rows of H as given, of rank m; Hcols [128][2]: column v of H, rows 0..63 / 64..127.
// lri_out / uidx_out [F][128]: entries >= n are written as 0; M_out [F][128]: entry r < m bits j = 0..63 of row r of updated_M,
// entry 64 + r bits j = 64..k-1; rows >= m and bits >= k are written as 0.
template <class... COUNT>   // (the counted form: ldpc_wave.h)
__global__ __launch_bounds__(256) void hosdw_front_kernel(const float *__restrict__ x, long long F, int n, int R, int m,
                                                          const u64 *__restrict__ Hcols, unsigned char *__restrict__ lri_out,
                                                          unsigned char *__restrict__ uidx_out, u64 *__restrict__ M_out,
                                                          int *__restrict__ nswaps, COUNT... count)
{
    if constexpr (kCounted<COUNT...>) {
        F = counted_frames(F, count...);
        if ((long long)blockIdx.x * 4 >= F) return;   // (the grid is sized by the capacity, not by the count)
    }
    __shared__ HFrontWLds lds[4];
    const int lane = threadIdx.x & 63;
    HFrontWLds &L = lds[threadIdx.x >> 6];
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int k = n - m;
    const bool in1 = lane < n, in2 = 64 + lane < n;      // slots lane / 64 + lane hold an original bit
    const bool mrbA = lane >= m && in1, mrbB = in2;      // ... and a column of the MRB side (m <= 64)

    for (long long f = wave; f < F; f += (long long)gridDim.x * 4) {
        hosd_sort_ascending(L, x, f, n, lane);               // mag_input_gen (:25-28), padded slots last
        if (lane < 4) L.mask[lane] = 0;
        L.col[0][lane] = 0ull; L.col[0][64 + lane] = 0ull; L.col[1][lane] = 0ull; L.col[1][64 + lane] = 0ull;
        L.uidx[lane] = 0; L.uidx[lane + 64] = 0;
        wave_fence();
        // ---- H with columns in sorted order (:38-40), column-major, two words per column; full_gf2elim (:222-257)
        const int s1 = L.lri[lane], s2 = L.lri[lane + 64];
        u64 A0 = in1 ? Hcols[2 * s1] : 0ull, A1 = in1 ? Hcols[2 * s1 + 1] : 0ull;
        u64 B0 = in2 ? Hcols[2 * s2] : 0ull, B1 = in2 ? Hcols[2 * s2 + 1] : 0ull;
        int rhoA = lane, rhoB = 64 + lane, idxA = lane, idxB = 64 + lane;
        int ns = 0, nrows = R, i = 0;
        // (i < nrows holds by rank: it bounds the loops whatever the input)
        if (R > 64) {
#pragma unroll 1
            while (i < m && i < nrows) {
                if (hgew_step<true>(A0, A1, B0, B1, rhoA, rhoB, idxA, idxB, i, nrows, lane, ns)) --nrows;
                else ++i;
            }
        } else {
#pragma unroll 1
            while (i < m && i < nrows) {
                if (hgew_step<false>(A0, A1, B0, B1, rhoA, rhoB, idxA, idxB, i, nrows, lane, ns)) --nrows;
                else ++i;
            }
        }
        // ---- identify_mrb (:58-69): LRB = index_order[:m] as left by the elimination, MRB = index_order[-k:] sorted
        if (mrbA) atomicOr(&L.mask[idxA >> 5], 1u << (idxA & 31));
        if (mrbB) atomicOr(&L.mask[idxB >> 5], 1u << (idxB & 31));
        wave_fence();
        const unsigned mk[4] = {L.mask[0], L.mask[1], L.mask[2], L.mask[3]};
        const int rankA = mrbA ? below_mask(mk, idxA) : 0, rankB = mrbB ? below_mask(mk, idxB) : 0;   // updated MRB positions < k
        if (lane < m) L.uidx[lane] = (unsigned char)idxA;
        if (mrbA) { L.uidx[m + rankA] = (unsigned char)idxA; L.col[0][rankA] = A0; L.col[1][rankA] = A1; }
        if (mrbB) { L.uidx[m + rankB] = (unsigned char)idxB; L.col[0][rankB] = B0; L.col[1][rankB] = B1; }
        wave_fence();
        // rows of updated_M: transpose to (lane = physical row, bit = MRB position) per half of the rows and of the MRB,
        // then logical row r = the row whose pivot sits in column r = physical row rhoA[r]
        // (the sort's key array is free by now: rows[p] = MRB bits 0..63 of physical row p, rows[128 + p] = bits 64..127)
        u64 *rows = L.rank.bk;
        rows[lane] = transpose64(L.col[0][lane], lane);
        rows[128 + lane] = k > 64 ? transpose64(L.col[0][64 + lane], lane) : 0ull;
        if (R > 64) {
            rows[64 + lane] = transpose64(L.col[1][lane], lane);
            rows[192 + lane] = k > 64 ? transpose64(L.col[1][64 + lane], lane) : 0ull;
        }
        wave_fence();
        const int pr = rhoA & (R > 64 ? 127 : 63);
        M_out[f * 128 + lane] = lane < m ? rows[pr] : 0ull;
        M_out[f * 128 + 64 + lane] = lane < m ? rows[128 + pr] : 0ull;
        lri_out[f * 128 + lane] = in1 ? (unsigned char)s1 : (unsigned char)0;
        lri_out[f * 128 + 64 + lane] = in2 ? (unsigned char)s2 : (unsigned char)0;
        uidx_out[f * 128 + lane] = L.uidx[lane];
        uidx_out[f * 128 + 64 + lane] = L.uidx[64 + lane];
        if (nswaps && lane == 0) nswaps[f] = ns;
        wave_fence();
    }
}

// The LDS plan of HSearchXLds with 128 columns: 1 KiB more.
template <bool RUNS>
struct __attribute__((aligned(16))) HSearchWLds {
    float lut[16][256];   // lut[b][v]: partial metric of discrepancy byte b (updated positions 8b..8b+7); built for b < 4 ceil(nb / 4)
    ulonglong2 Mcol[128]; // MRB position j < k: column j of updated_M (bit r < m) | 1 << (m + j), as two words; zero for j >= k
    float w[128];         // |metric_llr| in updated order, zero beyond n
    u64 keys[RUNS ? kHosdRunBlocks : kHosdMaxBlocks];   // per block: (metric bits << 32) | TEP index, minimum = first minimum
    u64 hgL, hgM;         // hard decisions of the metric input at updated positions 0..63 / 64..127
    u64 h0L, h0H;         // hard decisions of the ordering input at the MRB's updated positions m..n-1, same two words
    u64 DL0, best, cw[2];
    int ticket, heavy;
    float truth;          // the label's metric (hosdw_frame_setup with labels)
    unsigned char o[128]; // original bit index of updated position p (zero beyond n)
    int boff[RUNS ? kHosdRunBlocks + 1 : 1];            // block_off, once per workgroup
    unsigned short tl[RUNS ? kHosdLdsTeps : 2];         // the TEP table, once per workgroup: x | y << 7 | weight << 14
};

// hosd_apply on 128 two-word columns (the overload hosd_frame_best picks for this LDS type).  A TEP position is taken
// modulo 128: one at or beyond k is the caller's error and meets a zero column.
template <bool RUNS>
__device__ __forceinline__ void hosd_apply(const HSearchWLds<RUNS> &L, uchar4 s, u64 &lo, u64 &hi)
{
    if (s.w > 0) { const ulonglong2 c = L.Mcol[s.x & 127]; lo ^= c.x; hi ^= c.y; }
    if (s.w > 1) { const ulonglong2 c = L.Mcol[s.y & 127]; lo ^= c.x; hi ^= c.y; }
    if (s.w > 2) { const ulonglong2 c = L.Mcol[s.z & 127]; lo ^= c.x; hi ^= c.y; }
}

// The per-frame set-up with Mrows [F][128] (two word-planes of 64 rows) and up to 127 MRB positions.  Rows >= m and bits >= k
// of Mrows, and lri / uidx entries >= n, are not looked at.
// On return every thread sees the LUTs, the columns and the keys of blocks 0..nblk-1 reset to ~0.
template <class LDS>
__device__ __forceinline__ void hosdw_frame_setup(LDS &L, const HShapeNM &sh, const HScanIn &in, long long f, float *__restrict__ truth,
                                                  u64 &D0lo, u64 &D0hi)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = sh.n, m = sh.m, k = n - m, nb = sh.nb, nblk = in.nblk;
    // ---- phase 0: values in updated order, hard decisions, columns, key reset --------
    if (tid < 128) {
        hosdx_updated_values(L, sh, in, f);
    } else {
        // wavefront 2 / 3: the word-plane of MRB positions 0..63 / 64..127
        const int j = 64 * (wave - 2) + lane, kw = k - 64 * (wave - 2);   // this lane's MRB position; MRB positions in the plane
        const u64 kmask = kw >= 64 ? ~0ull : (kw > 0 ? ((1ull << kw) - 1ull) : 0ull);
        const u64 col = transpose64(lane < m ? (in.Mrows[f * 128 + 64 * (wave - 2) + lane] & kmask) : 0ull, lane);   // bit r = M[r][j]
        const int p = m + j;                                              // the updated position of MRB position j
        const u64 unit = 1ull << (p & 63);
        ulonglong2 c;
        c.x = j < k ? (col | (p < 64 ? unit : 0ull)) : 0ull;
        c.y = (j < k && p >= 64) ? unit : 0ull;
        L.Mcol[j] = c;
        if (tid == 128) { L.ticket = 0; L.best = ~0ull; L.cw[0] = 0; L.cw[1] = 0; }
    }
    for (int b = tid; b < nblk; b += 256) L.keys[b] = ~0ull;
    __syncthreads();
    // ---- phase 1: byte LUTs (four per wavefront, the fours that hold a byte of the metric), order-0 discrepancy (:155,:159)
    if (4 * wave < nb) build_byte_luts<4>(&L.lut[4 * wave], &L.w[32 * wave], lane);
    if (wave == 0) {
        // initial_mrb by MRB position: the 128-bit value (h0L, h0H) shifted right by m (1 <= m <= 64)
        const u64 mrbL = m >= 64 ? L.h0H : ((L.h0L >> m) | (L.h0H << (64 - m)));
        const u64 mrbH = m >= 64 ? 0ull : (L.h0H >> m);
        const u64 rows = m >= 64 ? ~0ull : ((1ull << m) - 1ull);
        const u64 c = (((mrbL >> lane) & 1) ? L.Mcol[lane].x : 0ull) ^ (((mrbH >> lane) & 1) ? L.Mcol[64 + lane].x : 0ull);
        const u64 d = wave_xor64(c & rows);
        if (lane == 0) L.DL0 = d ^ L.hgL ^ L.h0L;
    }
    __syncthreads();
    D0lo = L.DL0; D0hi = L.hgM ^ L.h0H;
    if (in.label && wave == 1) hosdx_label_metric(L, sh, in.label, f, truth);
}

// The wide family for the scans of ldpc_hosd_scan.h: 128 two-word columns, the kernel's n and m, TEP positions of 7 bits taken
// modulo 128; the metric is the any-shape family's.
struct HosdW {
    template <bool RUNS> using Lds = HSearchWLds<RUNS>;
    static constexpr int kPosBits = 7;
    static __device__ __forceinline__ unsigned pos(unsigned char v) { return v & 127; }
    template <class LDS> static __device__ __forceinline__ float cost(const LDS &L, u64 lo, u64 hi, const HShapeNM &sh) { return hosdx_cost(L, lo, hi, sh.nb); }
    template <class LDS>
    static __device__ __forceinline__ void setup(LDS &L, const HShapeNM &sh, const HScanIn &in, long long f, float *__restrict__ truth, u64 &D0lo,
                                                 u64 &D0hi)
    {
        hosdw_frame_setup(L, sh, in, f, truth, D0lo, D0hi);
    }
};

template <bool RUNS>
__global__ __launch_bounds__(256) void hosdw_search_kernel(const float *__restrict__ xo, const float *__restrict__ xm,
                                                           long long F, int n, int m, const unsigned char *__restrict__ lri,
                                                           const unsigned char *__restrict__ uidx,
                                                           const u64 *__restrict__ Mrows, const uchar4 *__restrict__ teps,
                                                           const int *__restrict__ block_off, int nblk,
                                                           const u64 *__restrict__ label, float *__restrict__ block_min,
                                                           int *__restrict__ block_arg, float *__restrict__ truth,
                                                           u64 *__restrict__ cw_out, float *__restrict__ metric_out,
                                                           int *__restrict__ best_out)
{
    __shared__ HosdW::Lds<RUNS> L;
    hosd_search_body<HosdW, RUNS>(L, HShapeNM(n, m), {xo, xm, F, lri, uidx, Mrows, teps, block_off, nblk, label}, block_min, block_arg,
                                  {truth, cw_out, metric_out, best_out});
}

HOSD_SLIDING_KERNEL(hosdw_sliding_kernel, HosdW, HOSD_NM_SHAPE_PARAMS, HShapeNM sh(n, m))

}  // namespace ldpc
