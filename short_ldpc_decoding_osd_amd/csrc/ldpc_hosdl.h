// H-form ordered-statistics primitives for longer and low-rate codes (n <= 384, an H of R <= 192 rows as given and rank
// m = n - k <= 192, 1 <= k <= 192): the kernels of the ldpc_hosdl_* entry points (ldpc_hosdl.hip).
//   mag_input_gen / check_matrix_reorder   ordered_statistics_decoding.py:25-41
//   identify_mrb / full_gf2elim            ordered_statistics_decoding.py:43-80, 222-257
//   acquire_min / sliding_osd              ordered_statistics_decoding.py:153-218
// The kernels of ldpc_hosdw.h one size up, as ldpc_osdl.h stands to ldpc_osdw.h.  With Sn = ceil(n / 64), Wm = ceil(m / 64)
// and Wk = ceil(k / 64):
//   front end: one frame per wavefront, a template on (S slots, W = ceil(R / 64) row words); lane l owns the sorted columns
//     64 s + l, each W words of PHYSICAL rows, and the entries 64 w + l of the logical-to-physical row map.  The pivot step is
//     gel_step's shape (ldpc_osdl.h) with hgew_step's row deletion (ldpc_hosdw.h) in place of the rank-deficiency flag.
//   scans: one frame per 256-thread workgroup, templates on (NW = Sn words of discrepancy, MW = Wm words of an M column).
//     The n updated positions are one sequence, LRB first; MRB position j < k owns the MW-word column of updated_M and the
//     unit bit at position m + j, which is applied by selects over the unrolled words (nothing in registers is indexed).
// What does not depend on the width of the discrepancy or on the index type is used from ldpc_hosd_scan.h as it is: the block
// keys, hosd_block_of, hosd_runs_form, hosd_search_results, the classifier (slide_p1, SlideLds, SlideFcnArg) and the constants.
// The run scan, the ticket scan, the best-candidate epilogue, the sliding kernel's body and the per-frame set-up are written
// here over NW-word discrepancies and 16-bit indices.  Wherever ldpc_hosdw_* serves the code every result is the same bit for
// bit once the layouts are converted.
// LDS per workgroup and occupancy of every instantiation: DESIGN.md and profiles/hosdl/README.md.
#pragma once

#include "ldpc_wave.h"
#include "ldpc_hosd_scan.h"

namespace ldpc {

constexpr int kHosdlN = 384, kHosdlK = 192, kHosdlM = 192;   // the limits of the family: n, k, rows of H (and so n - k)
constexpr int kHosdlFrontGrid = 32768;                       // workgroups of the front end (one wavefront, one frame each per trip)
constexpr int kHosdlScanGrid = 8192;                         // workgroups of the scans (one frame each per trip)

// bit p (0..64 W - 1) of the W-word column c (bitw of ldpc_osdl.h: each word against zero, so that no array is indexed)
template <int W>
__device__ __forceinline__ bool hl_bit(const u64 (&c)[W], int p)
{
    u64 w = c[0];
    if constexpr (W > 1) {
        w = (p >> 6) == 0 ? w : 0ull;
#pragma unroll
        for (int v = 1; v < W; ++v) w |= (p >> 6) == v ? c[v] : 0ull;
    }
    return ((w >> (p & 63)) & 1ull) != 0;
}

// One try at pivot step i with `nrows` logical rows left (full_gf2elim :229-257), columns in registers:
//   C[s][w] : sorted column 64 s + lane, word w: bit = PHYSICAL row 64 w + bit (rows >= R do not exist: those bits are zero)
//   rho[w]  : logical row 64 w + lane -> physical row (entries at or beyond nrows are not looked at)
//   idx[s]  : the sorted position travelling with the column of slot s (:58-62)
// HW = i / 64: the slot of pivot column i and the row word of logical row i, a compile-time fact in each third of the loop.
// Returns true when the step deleted logical row i instead of pivoting (the caller lowers nrows and tries step i again).
// Every lane-varying choice on the common path is a select; the deletion is rare and wave-uniform and is branched on.
template <int S, int W, int HW>
__device__ __forceinline__ bool hgel_step(u64 (&C)[S][W], int (&rho)[W], int (&idx)[S], int i, int nrows, int lane, int &nsw)
{
    const int il = i & 63;                                        // the lane of column i and of logical row i
    const u64 from = ~0ull << il;
    u64 rows[W], cj[W], bal[W];
    u64 any = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) rows[w] = nrows >= 64 * (w + 1) ? ~0ull : (nrows > 64 * w ? ((1ull << (nrows - 64 * w)) - 1ull) : 0ull);
#pragma unroll
    for (int w = 0; w < W; ++w) cj[w] = readlane64(C[HW][w], il);
#pragma unroll
    for (int w = 0; w < W; ++w) {                                 // logical rows >= i with a 1 in column i
        bal[w] = w < HW ? 0ull : (__ballot(hl_bit<W>(cj, rho[w])) & (w == HW ? (rows[w] & from) : rows[w]));
        any |= bal[w];
    }
    if (any == 0) {
        const int pri = __builtin_amdgcn_readlane(rho[HW], il);
        int sc = HW;                                              // the partner's slot and its ballot; the first slot wins
        u64 bsel = 0;
#pragma unroll
        for (int s = S - 1; s >= HW; --s) {                       // (columns < i are cleared in row i; idle slots are zero)
            const u64 b = __ballot(hl_bit<W>(C[s], pri)) & (s == HW ? from : ~0ull);
            if (b != 0) { sc = s; bsel = b; }
        }
        if (bsel == 0) {
            // logical row i is zero in every column: it is removed and every later row moves down by one (:247-250)
#pragma unroll
            for (int w = HW; w < W; ++w) {
                const int up = __shfl(rho[w], (lane + 1) & 63, 64);
                int last = rho[w];                                // (the last entry of the map keeps its value: not looked at)
                if constexpr (W > 1) { if (w + 1 < W) last = __builtin_amdgcn_readlane(rho[w + 1 < W ? w + 1 : w], 0); }
                const int moved = lane == 63 ? last : up;
                rho[w] = (w == HW && lane < il) ? rho[w] : moved;
            }
            return true;
        }
        // exchange column i with the first later column, in sorted order, that has a 1 in logical row i (:251-256)
        const unsigned cl = __builtin_ctzll(bsel);
        u64 cc[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            u64 v = C[HW][w];
#pragma unroll
            for (int s = HW + 1; s < S; ++s) v = (sc == s) ? C[s][w] : v;
            cc[w] = readlane64(v, cl);
        }
        int vi = idx[HW];
#pragma unroll
        for (int s = HW + 1; s < S; ++s) vi = (sc == s) ? idx[s] : vi;
        const int ic = __builtin_amdgcn_readlane(vi, cl);
        const int ii = __builtin_amdgcn_readlane(idx[HW], il);
#pragma unroll
        for (int s = HW; s < S; ++s) {
            const bool hit = (unsigned)lane == cl && sc == s;
#pragma unroll
            for (int w = 0; w < W; ++w) C[s][w] = hit ? cj[w] : C[s][w];
            idx[s] = hit ? ii : idx[s];
        }
#pragma unroll
        for (int w = 0; w < W; ++w) C[HW][w] = (lane == il) ? cc[w] : C[HW][w];
        idx[HW] = (lane == il) ? ic : idx[HW];
        ++nsw;
#pragma unroll
        for (int w = 0; w < W; ++w) {                             // the exchanged-in column has its 1 in logical row i
            cj[w] = cc[w];
            bal[w] = w == HW ? (1ull << il) : 0ull;
        }
    }
    // the first logical row wins; exchange logical rows i and r (r == i: no change)
    int rw = W - 1;
    u64 rsel = bal[W - 1];
#pragma unroll
    for (int w = W - 2; w >= HW; --w)
        if (bal[w] != 0) { rw = w; rsel = bal[w]; }
    const int rl = rsel ? __builtin_ctzll(rsel) : 0;
    int vr = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) vr |= (rw == w) ? rho[w] : 0;
    const int pr = __builtin_amdgcn_readlane(vr, rl);
    const int pi = __builtin_amdgcn_readlane(rho[HW], il);
#pragma unroll
    for (int w = HW; w < W; ++w) rho[w] = (rw == w && lane == rl) ? pi : rho[w];
    rho[HW] = (lane == il) ? pr : rho[HW];
    // clear column i in every other row: the pivot column without its pivot
    u64 e[W];
#pragma unroll
    for (int w = 0; w < W; ++w) e[w] = cj[w] & ~((pr >> 6) == w ? (1ull << (pr & 63)) : 0ull);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const bool h = hl_bit<W>(C[s], pr);
#pragma unroll
        for (int w = 0; w < W; ++w) C[s][w] ^= h ? e[w] : 0ull;
    }
    return false;
}

struct __attribute__((aligned(16))) HFrontLLds {
    u64 key[kHosdlN];                 // sort keys of the frame's positions: (|x| bits, position)
    u64 col[3][kHosdlK];              // M columns in updated MRB order, one array per row word (zero beyond k)
    u64 rows[kHosdlM][3];             // physical row -> its k MRB bits, Wk words
    unsigned mask[kHosdlN / 32];      // which sorted positions ended up in the MRB
    unsigned pre[kHosdlN / 32];       // set bits of the mask in the words below each word
    unsigned short lri[kHosdlN];      // sorted position -> original bit
    unsigned short uidx[kHosdlN];     // updated position -> sorted position (zero beyond n)
};

// One frame per wavefront, one wavefront per workgroup.  S >= Sn slots, W = ceil(R / 64) row words; R rows of H as given, of
// rank m.  Hcols [384][3]: column v of H, rows 0..63 / 64..127 / 128..191.
//   lri_out / uidx_out [F][64 Sn] u16 : entries >= n are written as 0
//   M_out [F][64 Wm][Wk] u64          : entry [r][q] bits j = 64 q .. 64 q + 63 of row r of updated_M; rows >= m, bits >= k zero
// The sort ranks every key against all n keys of the frame through LDS (every lane reads the same entry: a broadcast); the
// keys are distinct, ascending |x| with ties to the lower index, and a padded slot has no key: it never sorts in front.
template <int S, int W, class... COUNT>   // (the counted form: ldpc_wave.h)
__global__ __launch_bounds__(64) void hosdl_front_kernel(const float *__restrict__ x, long long F, int n, int R, int m,
                                                         const u64 *__restrict__ Hcols, unsigned short *__restrict__ lri_out,
                                                         unsigned short *__restrict__ uidx_out, u64 *__restrict__ M_out,
                                                         int *__restrict__ nswaps, COUNT... count)
{
    if constexpr (kCounted<COUNT...>) {
        F = counted_frames(F, count...);
        if (blockIdx.x >= F) return;   // (the grid is sized by the capacity, not by the count)
    }
    __shared__ HFrontLLds L;
    const int lane = threadIdx.x;
    const int k = n - m, Sn = (n + 63) >> 6, Wm = (m + 63) >> 6, Wk = (k + 63) >> 6;

    for (long long f = blockIdx.x; f < F; f += gridDim.x) {
        // ---- mag_input_gen (:25-28): rank in ascending |x|, ties -> lower index ------------------------
        u64 key[S];
        int rank[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int p = 64 * s + lane;
            const unsigned a = p < n ? (__float_as_uint(x[f * n + p]) & 0x7FFFFFFFu) : 0u;
            key[s] = ((u64)a << 32) | (unsigned)p;
            rank[s] = 0;
            if (p < n) L.key[p] = key[s];
            L.uidx[p] = 0;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) { L.col[w][lane] = 0ull; L.col[w][64 + lane] = 0ull; L.col[w][128 + lane] = 0ull; }
        if (lane < kHosdlN / 32) L.mask[lane] = 0;
        wave_fence();
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const u64 kj = L.key[j];
#pragma unroll
            for (int s = 0; s < S; ++s) rank[s] += kj < key[s];
        }
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (64 * s + lane < n) L.lri[rank[s]] = (unsigned short)(64 * s + lane);
        wave_fence();
        // ---- H with columns in sorted order (:38-40), column-major, W words per column; full_gf2elim (:222-257)
        u64 C[S][W];
        int idx[S], rho[W];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int p = 64 * s + lane;
            const int o = p < n ? L.lri[p] : 0;
#pragma unroll
            for (int w = 0; w < W; ++w) C[s][w] = p < n ? Hcols[o * 3 + w] : 0ull;
            idx[s] = p;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) rho[w] = 64 * w + lane;
        int ns = 0, nrows = R, i = 0;
        // (i < nrows holds by rank: it bounds the loops whatever the input)
        {
            const int e = m < 64 ? m : 64;
#pragma unroll 1
            while (i < e && i < nrows) {
                if (hgel_step<S, W, 0>(C, rho, idx, i, nrows, lane, ns)) --nrows;
                else ++i;
            }
        }
        if constexpr (W > 1) {
            const int e = m < 128 ? m : 128;
#pragma unroll 1
            while (i < e && i < nrows) {
                if (hgel_step<S, W, 1>(C, rho, idx, i, nrows, lane, ns)) --nrows;
                else ++i;
            }
        }
        if constexpr (W > 2 && S > 2) {
#pragma unroll 1
            while (i < m && i < nrows) {
                if (hgel_step<S, W, 2>(C, rho, idx, i, nrows, lane, ns)) --nrows;
                else ++i;
            }
        }
        // ---- identify_mrb (:58-69): LRB = index_order[:m] as left by the elimination, MRB = index_order[-k:] sorted
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int p = 64 * s + lane;
            if (p >= m && p < n) atomicOr(&L.mask[idx[s] >> 5], 1u << (idx[s] & 31));
        }
        wave_fence();
        if (lane == 0) {
            unsigned a = 0;
            for (int j = 0; j < kHosdlN / 32; ++j) { L.pre[j] = a; a += __popc(L.mask[j]); }
        }
        wave_fence();
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int p = 64 * s + lane, v = idx[s];
            if (p < m) {
                L.uidx[p] = (unsigned short)v;
            } else if (p < n) {
                const int cnt = (int)(L.pre[v >> 5] + __popc(L.mask[v >> 5] & ((1u << (v & 31)) - 1u)));   // updated MRB position < k
                L.uidx[m + cnt] = (unsigned short)v;
#pragma unroll
                for (int w = 0; w < W; ++w) L.col[w][cnt] = C[s][w];
            }
        }
        wave_fence();
        // rows of updated_M: transpose to (lane = physical row, bit = MRB position) per row word and word of the MRB, then
        // logical row r = the row whose pivot sits in column r = physical row rho[r]
#pragma unroll
        for (int w = 0; w < W; ++w)
            for (int q = 0; q < Wk; ++q) L.rows[64 * w + lane][q] = transpose64(L.col[w][64 * q + lane], lane);
        wave_fence();
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (s < Sn) {
                const int p = 64 * s + lane;
                lri_out[(f * Sn + s) * 64 + lane] = p < n ? L.lri[p] : (unsigned short)0;
                uidx_out[(f * Sn + s) * 64 + lane] = L.uidx[p];
            }
#pragma unroll
        for (int w = 0; w < W; ++w)
            if (w < Wm) {
                const bool live = 64 * w + lane < m;
                const int pr = live ? rho[w] : 0;
                for (int q = 0; q < Wk; ++q) M_out[((f * Wm + w) * 64 + lane) * Wk + q] = live ? L.rows[pr][q] : 0ull;
            }
        if (nswaps && lane == 0) nswaps[f] = ns;
        wave_fence();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the block scans
// ---------------------------------------------------------------------------------------------------------------------
// what every block scan of this family reads (HScanIn with 16-bit indices)
struct HLScanIn {
    const float *__restrict__ xo, *__restrict__ xm;
    long long F;
    const unsigned short *__restrict__ lri, *__restrict__ uidx;
    const u64 *__restrict__ Mrows;
    const uchar4 *__restrict__ teps;
    const int *__restrict__ block_off;
    int nblk;
    const u64 *__restrict__ label;
};

// The LDS plan: byte LUTs for the 8 NW bytes of a discrepancy (built for the fours that hold a byte of the code), 192 columns of
// MW words.  The run form keeps the table as 16 bits per TEP: x | y << 8 with the weight in the pair itself -- two different
// positions: weight 2; the same position twice: weight 1; 0xFFFF: weight 0 (a position is < 192, so 0xFF is free).
template <int NW, int MW, bool RUNS>
struct __attribute__((aligned(16))) HSearchLLds {
    float lut[8 * NW][256];      // lut[b][v]: partial metric of discrepancy byte b (updated positions 8b..8b+7)
    u64 Mcol[kHosdlK][MW];       // MRB position j < k: column j of updated_M (bit r < m); zero for j >= k
    float w[64 * NW];            // |metric_llr| in updated order, zero beyond n
    u64 keys[RUNS ? kHosdRunBlocks : kHosdMaxBlocks];   // per block: (metric bits << 32) | TEP index, minimum = first minimum
    u64 hg[NW];                  // hard decisions of the metric input at the updated positions
    u64 h0[NW];                  // hard decisions of the ordering input at the MRB's updated positions m..n-1
    u64 D0[NW];                  // the order-0 discrepancy
    u64 best, cw[kHosdlN / 64];
    int ticket, heavy;
    float truth;                 // the label's metric (hosdl_frame_setup with labels)
    unsigned short o[64 * NW];   // original bit index of updated position p (zero beyond n)
    int boff[RUNS ? kHosdRunBlocks + 1 : 1];            // block_off, once per workgroup
    unsigned short tl[RUNS ? kHosdLdsTeps : 2];         // the TEP table, once per workgroup
};

// a TEP position as the scans take it: one at or beyond 192 (the caller's error) becomes 0, so that no column is read outside
// the table; one in k..191 meets a zero column
__device__ __forceinline__ unsigned hosdl_pos(unsigned char v) { return v < kHosdlK ? v : 0u; }

// D ^= column of MRB position j: the MW words of updated_M's column and the unit bit at updated position m + j
template <int NW, int MW, class LDS>
__device__ __forceinline__ void hosdl_flip(const LDS &L, unsigned j, int m, u64 (&D)[NW])
{
#pragma unroll
    for (int w = 0; w < MW; ++w) D[w] ^= L.Mcol[j][w];
    const int p = m + (int)j;
    const u64 bit = 1ull << (p & 63);
#pragma unroll
    for (int w = MW - 1; w < NW; ++w) D[w] ^= (p >> 6) == w ? bit : 0ull;       // (m > 64 (MW - 1): no lower word holds it)
}

template <int NW, int MW, class LDS>
__device__ __forceinline__ void hosdl_apply(const LDS &L, uchar4 s, int m, u64 (&D)[NW])
{
    if (s.w > 0) hosdl_flip<NW, MW>(L, hosdl_pos(s.x), m, D);
    if (s.w > 1) hosdl_flip<NW, MW>(L, hosdl_pos(s.y), m, D);
    if (s.w > 2) hosdl_flip<NW, MW>(L, hosdl_pos(s.z), m, D);
}

// The metric over the nb = ceil(n / 8) bytes of the discrepancy, summed ascending from byte 0 (hosdx_cost over NW words): the
// bytes are read in fours (one wave-uniform branch each); a LUT inside the last four that lies at or beyond nb is all zeros.
template <int NW, class LDS>
__device__ __forceinline__ float hosdl_cost(const LDS &L, const u64 (&D)[NW], int nb)
{
    float acc = lut_byte<0>(L.lut, D[0]);
    acc = acc + lut_byte<1>(L.lut, D[0]); acc = acc + lut_byte<2>(L.lut, D[0]); acc = acc + lut_byte<3>(L.lut, D[0]);
    if (nb > 4) {
        acc = acc + lut_byte<4>(L.lut, D[0]); acc = acc + lut_byte<5>(L.lut, D[0]); acc = acc + lut_byte<6>(L.lut, D[0]);
        acc = acc + lut_byte<7>(L.lut, D[0]);
    }
#pragma unroll
    for (int q = 1; q < NW; ++q) {
        const float(*lut)[256] = &L.lut[8 * q];
        if (nb > 8 * q) {
            acc = acc + lut_byte<0>(lut, D[q]); acc = acc + lut_byte<1>(lut, D[q]); acc = acc + lut_byte<2>(lut, D[q]);
            acc = acc + lut_byte<3>(lut, D[q]);
        }
        if (nb > 8 * q + 4) {
            acc = acc + lut_byte<4>(lut, D[q]); acc = acc + lut_byte<5>(lut, D[q]); acc = acc + lut_byte<6>(lut, D[q]);
            acc = acc + lut_byte<7>(lut, D[q]);
        }
    }
    return acc;
}

// The per-frame set-up: values in updated order (:172-176), hard decisions, the columns, block keys reset, the byte LUTs, the
// order-0 discrepancy D0 and (with labels) the label's metric (L.truth, and truth[f] where truth is given).
// Rows >= m and bits >= k of Mrows, and lri / uidx entries >= n, are not looked at.
// On return every thread sees the LUTs, the columns and the keys of blocks 0..nblk-1 reset to ~0.
template <int NW, int MW, class LDS>
__device__ __forceinline__ void hosdl_frame_setup(LDS &L, const HShapeNM &sh, const HLScanIn &in, long long f, float *__restrict__ truth,
                                                  u64 (&D0)[NW])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = sh.n, m = sh.m, k = n - m, nb = sh.nb, nblk = in.nblk;
    const int Wk = (k + 63) >> 6;
    // ---- phase 0: values in updated order, hard decisions, columns, key reset --------
    for (int w = wave; w < NW; w += 4) {                   // updated positions 64 w + lane
        const int p = 64 * w + lane;
        const bool live = p < n;
        int o = 0;
        float mv = 0.0f;
        bool h0 = false;
        if (live) {
            const int u = in.uidx[f * (64 * NW) + p];
            o = in.lri[f * (64 * NW) + (u < n ? u : 0)];
            o = o < n ? o : 0;                               // (front-end results hold original bits < n)
            mv = in.xm[f * n + o];
            h0 = p >= m && !(in.xo[f * n + o] > 0.0f);       // initial_mrb (:186-187)
        }
        L.o[p] = (unsigned short)o;
        L.w[p] = __builtin_fabsf(mv);
        const u64 hg = __ballot(live && !(mv > 0.0f));       // order_hard_original (:180)
        const u64 hb = __ballot(h0);
        if (lane == 0) { L.hg[w] = hg; L.h0[w] = hb; }
    }
    // the 64 x 64 blocks of Mrows: row word rw, MRB word q -> columns 64 q + lane, word rw (zero columns beyond k)
    for (int b = wave; b < MW * 3; b += 4) {
        const int rw = b / 3, q = b - 3 * rw;
        const int kw = k - 64 * q;                            // MRB positions in this word
        const u64 kmask = kw >= 64 ? ~0ull : (kw > 0 ? ((1ull << kw) - 1ull) : 0ull);
        const bool live = q < Wk && 64 * rw + lane < m;
        const u64 row = live ? (in.Mrows[((f * MW + rw) * 64 + lane) * Wk + q] & kmask) : 0ull;
        L.Mcol[64 * q + lane][rw] = transpose64(row, lane);   // lane j: bit r = M[64 rw + r][64 q + j]
    }
    if (tid == 0) {
        L.ticket = 0; L.best = ~0ull;
#pragma unroll
        for (int v = 0; v < kHosdlN / 64; ++v) L.cw[v] = 0;
    }
    for (int b = tid; b < nblk; b += 256) L.keys[b] = ~0ull;
    __syncthreads();
    // ---- phase 1: byte LUTs (the fours that hold a byte of the metric), order-0 discrepancy (:155,:159)
    for (int g = wave; g < 2 * NW; g += 4)
        if (4 * g < nb) build_byte_luts<4>(&L.lut[4 * g], &L.w[32 * g], lane);
    if (wave == 3) {
        u64 c[MW];
#pragma unroll
        for (int w = 0; w < MW; ++w) c[w] = 0ull;
#pragma unroll
        for (int s = 0; s < 3; ++s) {                        // initial_mrb by MRB position j = 64 s + lane: updated position m + j
            const int p = m + 64 * s + lane, ps = p < n ? p : 0;
            const bool on = p < n && ((L.h0[ps >> 6] >> (ps & 63)) & 1ull);
#pragma unroll
            for (int w = 0; w < MW; ++w) c[w] ^= on ? L.Mcol[64 * s + lane][w] : 0ull;
        }
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const u64 d = w < MW ? wave_xor64(c[w < MW ? w : 0]) : 0ull;
            if (lane == 0) L.D0[w] = d ^ L.hg[w] ^ L.h0[w];
        }
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w) D0[w] = L.D0[w];
    if (in.label && wave == 1) {                             // the label's metric (:181-183)
        u64 d[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int p = 64 * w + lane, o = L.o[p];
            const u64 lw = in.label[f * sh.words + (o >> 6)];      // (o < n: inside the frame's words)
            d[w] = __ballot(p < n && ((lw >> (o & 63)) & 1ull)) ^ L.hg[w];
        }
        const float t = hosdl_cost<NW>(L, d, nb);
        if (lane == 0) { if (truth) truth[f] = t; L.truth = t; }
    }
}

// Wave 0 of a frame's workgroup, after the keys of the candidate blocks have been folded into L.best: the first minimum's
// metric and TEP index and its codeword in the original bit order (hosd_frame_best over NW words).
template <int NW, int MW, class LDS>
__device__ __forceinline__ void hosdl_frame_best(LDS &L, const HShapeNM &sh, const uchar4 *__restrict__ teps, long long f, const u64 (&D0)[NW],
                                                 const HBestOut &out)
{
    const int lane = threadIdx.x & 63;
    const u64 k = L.best;
    const bool none = k == ~0ull;
    if (lane == 0) {
        if (out.metric) out.metric[f] = none ? INFINITY : __int_as_float((int)(k >> 32));
        if (out.best) out.best[f] = none ? -1 : (int)(unsigned)k;
    }
    if (out.cw) {
        u64 D[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) D[w] = D0[w];
        if (!none) hosdl_apply<NW, MW>(L, teps[(unsigned)k], sh.m, D);
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const u64 bits = D[w] ^ L.hg[w];
            const int o = L.o[64 * w + lane];
            if ((bits >> lane) & 1) atomicOr(&L.cw[o >> 6], 1ull << (o & 63));
        }
        wave_fence();
        if (lane < sh.words) out.cw[f * sh.words + lane] = L.cw[lane];
    }
}

// the run form's table in LDS (hosd_stage_table with the 16-bit entry of HSearchLLds) and this thread's run
template <class LDS>
__device__ __forceinline__ void hosdl_stage_table(LDS &L, const uchar4 *__restrict__ teps, const int *__restrict__ block_off, int nblk, int ntep,
                                                  int &run0, int &run1, int &b0)
{
    const int tid = threadIdx.x;
    for (int b = tid; b <= nblk; b += 256) L.boff[b] = block_off[b];
    for (int t = tid; t < ntep; t += 256) {
        const uchar4 s = teps[t];                            // (hosd_runs_form admitted no TEP of weight 3)
        const unsigned x = hosdl_pos(s.x), y = s.w > 1 ? hosdl_pos(s.y) : x;
        L.tl[t] = (unsigned short)(s.w == 0 ? 0xFFFFu : (x | (y << 8)));
    }
    __syncthreads();
    const int per = ((ntep + 255) / 256) | 1;
    run0 = tid * per < ntep ? tid * per : ntep; run1 = run0 + per < ntep ? run0 + per : ntep;
    b0 = hosd_block_of(L.boff, 0, nblk, run0);
}

template <class LDS>
__device__ __forceinline__ uchar4 hosdl_lds_tep(const LDS &L, int t)
{
    const unsigned tv = L.tl[t], x = tv & 255u, y = tv >> 8;
    // (a pair given with the same position twice, the caller's error, is taken as a single)
    return tv == 0xFFFFu ? make_uchar4(0, 0, 0, 0) : make_uchar4((unsigned char)x, (unsigned char)y, 0, (unsigned char)(x == y ? 1 : 2));
}

// hosd_run_scan over NW words: this thread's run [run0, run1) of consecutive TEPs, which starts in block b
template <int NW, int MW, class LDS, class TEP>
__device__ __forceinline__ void hosdl_run_scan(LDS &L, const HShapeNM &sh, const int *boff, TEP tep, int run0, int run1, int b, const u64 (&D0)[NW])
{
    float best = INFINITY;
    int bestt = 0;
    for (int t = run0; t < run1; ++t) {
        while (t >= boff[b + 1]) {      // the run leaves block b (the next ones may be empty)
            if (best < INFINITY) atomicMin(&L.keys[b], hosd_key(best, bestt));
            best = INFINITY;
            ++b;
        }
        u64 D[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) D[w] = D0[w];
        hosdl_apply<NW, MW>(L, tep(t), sh.m, D);
        const float c = hosdl_cost<NW>(L, D, sh.nb);
        if (c < best) { best = c; bestt = t; }                     // ascending t: first minimum
    }
    if (best < INFINITY) atomicMin(&L.keys[b], hosd_key(best, bestt));
}

// hosd_ticket_scan over NW words: items of kHosdChunk TEPs pulled by each wavefront from the frame's LDS ticket
template <int NW, int MW, class LDS>
__device__ __forceinline__ void hosdl_ticket_scan(LDS &L, const HShapeNM &sh, const uchar4 *__restrict__ teps, const int *__restrict__ block_off,
                                                  int nblk, const u64 (&D0)[NW])
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
            u64 D[NW];
#pragma unroll
            for (int w = 0; w < NW; ++w) D[w] = D0[w];
            hosdl_apply<NW, MW>(L, teps[t], sh.m, D);
            const float c = hosdl_cost<NW>(L, D, sh.nb);
            if (c < best) { best = c; bestt = t; }                 // ascending t per lane: first minimum
        }
        const int wl = wave_argmin_lane(best, bestt);
        if (lane == wl) atomicMin(&L.keys[b], hosd_key(best, bestt));
        ++item; s += kHosdChunk;
    }
}

// The search: one frame per 256-thread workgroup.  Both instantiations are launched and decide alike from device data which of
// them works (hosd_runs_form); the other returns at once.
template <int NW, int MW, bool RUNS>
__global__ __launch_bounds__(256) void hosdl_search_kernel(const float *__restrict__ xo, const float *__restrict__ xm, long long F, int n, int m,
                                                           const unsigned short *__restrict__ lri, const unsigned short *__restrict__ uidx,
                                                           const u64 *__restrict__ Mrows, const uchar4 *__restrict__ teps,
                                                           const int *__restrict__ block_off, int nblk, const u64 *__restrict__ label,
                                                           float *__restrict__ block_min, int *__restrict__ block_arg,
                                                           float *__restrict__ truth, u64 *__restrict__ cw_out,
                                                           float *__restrict__ metric_out, int *__restrict__ best_out)
{
    __shared__ HSearchLLds<NW, MW, RUNS> L;
    const HShapeNM sh(n, m);
    const HLScanIn in = {xo, xm, F, lri, uidx, Mrows, teps, block_off, nblk, label};
    const HBestOut out = {truth, cw_out, metric_out, best_out};
    int run0 = 0, run1 = 0, b0 = 0;
    const int ntep = nblk > 0 ? block_off[nblk] : 0;
    if (hosd_runs_form(L, teps, ntep, nblk) != RUNS) return;
    if constexpr (RUNS) hosdl_stage_table(L, teps, block_off, nblk, ntep, run0, run1, b0);
    for (long long f = blockIdx.x; f < F; f += gridDim.x) {
        u64 D0[NW];
        hosdl_frame_setup<NW, MW>(L, sh, in, f, truth, D0);
        if constexpr (RUNS) hosdl_run_scan<NW, MW>(L, sh, L.boff, [](int t) { return hosdl_lds_tep(L, t); }, run0, run1, b0, D0);
        else hosdl_ticket_scan<NW, MW>(L, sh, teps, block_off, nblk, D0);
        __syncthreads();
        hosd_search_results(L, f, nblk, block_min, block_arg);
        __syncthreads();
        if ((threadIdx.x >> 6) == 0) hosdl_frame_best<NW, MW>(L, sh, teps, f, D0, out);
        __syncthreads();
    }
}

// The block scan with the reference's sliding-window early stop (sliding_osd :187-218): the text of HOSD_SLIDING_KERNEL
// (ldpc_hosd_scan.h) on this family's set-up, run scan and epilogue.  Group rule, decision replay and results as there.
template <int NW, int MW, class... COUNT>   // (the counted form: ldpc_wave.h)
__global__ __launch_bounds__(256) void hosdl_sliding_kernel(const float *__restrict__ xo, const float *__restrict__ xm, long long F, int n, int m,
                                                            const unsigned short *__restrict__ lri, const unsigned short *__restrict__ uidx,
                                                            const u64 *__restrict__ Mrows, const uchar4 *__restrict__ teps,
                                                            const int *__restrict__ block_off, int nblk, int win, double margin,
                                                            SlideFcnArg fcn, int group, const u64 *__restrict__ label,
                                                            int *__restrict__ deep_out, float *__restrict__ gmin_out,
                                                            float *__restrict__ truth, unsigned char *__restrict__ success,
                                                            u64 *__restrict__ cw_out, float *__restrict__ metric_out,
                                                            int *__restrict__ best_out, int *__restrict__ nteps_out, COUNT... count)
{
    if constexpr (kCounted<COUNT...>) {
        F = counted_frames(F, count...);
        if (blockIdx.x >= F) return;   // (the grid is sized by the capacity, not by the count)
    }
    __shared__ HSearchLLds<NW, MW, false> L;
    __shared__ SlideLds S;
    const int tid = threadIdx.x, wave = tid >> 6;
    const HShapeNM sh(n, m);
    const HLScanIn in = {xo, xm, F, lri, uidx, Mrows, teps, block_off, nblk, label};
    for (int b = tid; b <= nblk; b += 256) S.boff[b] = block_off[b];
    __syncthreads();

    for (long long f = blockIdx.x; f < F; f += gridDim.x) {
        u64 D0[NW];
        hosdl_frame_setup<NW, MW>(L, sh, in, f, truth, D0);
        int k = 0, deep = win;   // (lane 0) the next window decision, blocks evaluated so far in the reference's sense
        float gmin = INFINITY;   // (lane 0) global_min
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
            if (run0 < run1)
                hosdl_run_scan<NW, MW>(L, sh, S.boff, [teps](int t) { return teps[t]; }, run0, run1, hosd_block_of(S.boff, g0, g1, run0), D0);
            __syncthreads();
            // ---- lane 0: every decision whose window lies in the blocks scanned so far (:193-209)
            if (tid == 0) {
                bool stop = false;
                for (; !stop && k <= nblk - win && k + win <= g1; ++k) {
                    deep = k + win;
                    if (k != 0 && key_metric(L.keys[k + win - 1]) > gmin) continue;   // :203-204
                    for (int i = 0; i < win; ++i) {   // the window, ascending
                        const float v = key_metric(L.keys[k + i]);
                        int j = i;
                        while (j > 0 && S.x[j - 1] > v) { S.x[j] = S.x[j - 1]; --j; }
                        S.x[j] = v;
                    }
                    S.x[win] = (float)k;
                    const float p1 = slide_p1(S, win, fcn);
                    gmin = S.x[0] < gmin ? S.x[0] : gmin;   // min(global_min, window.min())
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
            if (success) success[f] = gmin == L.truth;   // :213
            if (nteps_out) nteps_out[f] = S.boff[g1] - S.boff[0];
        }
        u64 mine = ~0ull;
        for (int b = tid; b < dl; b += 256) mine = L.keys[b] < mine ? L.keys[b] : mine;
        if (mine != ~0ull) atomicMin(&L.best, mine);
        __syncthreads();
        if (wave == 0) hosdl_frame_best<NW, MW>(L, sh, teps, f, D0, {truth, cw_out, metric_out, best_out});
        __syncthreads();
    }
}

}  // namespace ldpc
