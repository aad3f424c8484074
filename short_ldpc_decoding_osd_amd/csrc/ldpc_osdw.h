// OSD for high-rate short codes (n <= 128, 1 <= n - k <= 64, hence k up to 127): the front end and the conventional order-p
// table scan with the code's n and k as kernel arguments, one frame per wavefront.
//   swapped_info / identify_mrb / full_gf2elim   PB_OSD/pb_testing.py:231-320
//   convention_osd_main                           FS_OSD/convention_osd.py:49-76
// A column of G has up to 127 rows, so it is TWO 64-bit words (physical rows 0..63 and 64..127), and the row map has two entries
// per lane.  Layout of a frame on the wavefront: lane l owns sorted columns l and 64 + l (the slots of the reliability sort), a
// slot at or beyond n carries a zero column.  The n - k <= 64 parity columns keep a row of P' and the discrepancy D in one word,
// so the scan is the one of ldpc_osdx.h with 128 rows of P' and two words of MRB hard decisions.
// The helpers of ldpc_wave.h and the metric of ldpc_search.h (tep_cost, tep_cost_bounded: templates on the LDS type, they read
// only its byte LUTs) are used unchanged.  tep_apply and wave_argmin carry a one-word flip mask, which 127 MRB positions do not
// fit: their counterparts without the mask are here (tepw_apply, five lines of arg-min in the scan) and in ldpc_search.h
// (tep_flips).
#pragma once

#include "ldpc_search.h"

namespace ldpc {

struct __attribute__((aligned(16))) FrontWLds {
    RankLds rank;             // reliability sort (bucket_ranks, ldpc_wave.h)
    u64 col0[64], col1[64];   // parity columns in primed order, physical rows 0..63 / 64..127 (zero beyond n - k)
    u64 rows[128];            // physical row -> its n - k parity bits
    unsigned mask[4];         // 128-bit membership mask of the MRB's sorted positions
    unsigned char pi1[128];   // sorted position -> original bit
    unsigned char rowsrc[128];// primed MRB position -> physical row of its pivot
    unsigned char perm[128];  // primed position -> original bit (zero beyond n)
};

// bit p (0..127) of the two-word column (w0, w1)
__device__ __forceinline__ bool bit128(u64 w0, u64 w1, int p) { return ((((p & 64) ? w1 : w0) >> (p & 63)) & 1ull) != 0; }

// One pivot step i of the Gauss-Jordan elimination over k <= 127 rows (full_gf2elim :231-266), columns in registers:
//   A0 A1 / B0 B1 : sorted columns lane / 64 + lane, bit = PHYSICAL row (rows >= k do not exist: those bits are zero)
//   rhoA / rhoB   : logical rows lane / 64 + lane -> physical row (row exchanges permute this map only)
//   idxA / idxB   : the sorted position travelling with each column (:276-281)
//   rowsA / rowsB : the logical rows that exist, per half
// HI = (i >= 64): the slot of pivot column i and of logical row i is a compile-time fact in each half of the loop.
// Every lane-varying choice is a select and nothing is indexed: the columns stay in registers (no scratch).  Idle slots hold
// zero columns, so they are never a pivot row nor an exchange partner.
template <bool HI>
__device__ __forceinline__ void gew_step(u64 &A0, u64 &A1, u64 &B0, u64 &B1, int &rhoA, int &rhoB, int &idxA, int &idxB, int i,
                                         u64 rowsA, u64 rowsB, int lane, int &nsw, bool &deficient)
{
    const int il = i & 63;                                        // the lane of column i and of logical row i
    const u64 from = ~0ull << il;
    const u64 geA = HI ? 0ull : (rowsA & from);                   // logical rows >= i, lower / upper half
    const u64 geB = HI ? (rowsB & from) : rowsB;
    u64 cj0 = readlane64(HI ? B0 : A0, il), cj1 = readlane64(HI ? B1 : A1, il);
    u64 balA = __ballot(bit128(cj0, cj1, rhoA)) & geA;            // logical rows >= i with a 1 in column i
    u64 balB = __ballot(bit128(cj0, cj1, rhoB)) & geB;
    if ((balA | balB) == 0) {
        // no pivot in column i: exchange it with the first later column, in sorted order, that has a 1 in logical row i
        const int pri = __builtin_amdgcn_readlane(HI ? rhoB : rhoA, il);
        const u64 b1 = __ballot(bit128(A0, A1, pri)) & (HI ? 0ull : from);
        const u64 b2 = __ballot(bit128(B0, B1, pri)) & (HI ? from : ~0ull);
        deficient |= (b1 | b2) == 0;                              // all-zero row: carry on with garbage, report at the end
        const bool lo = b1 != 0;
        const unsigned cl = lo ? __builtin_ctzll(b1) : (b2 ? __builtin_ctzll(b2) : 0);
        const u64 ca0 = readlane64(A0, cl), ca1 = readlane64(A1, cl), cb0 = readlane64(B0, cl), cb1 = readlane64(B1, cl);
        const int ia = __builtin_amdgcn_readlane(idxA, cl), ib = __builtin_amdgcn_readlane(idxB, cl);
        const u64 cc0 = lo ? ca0 : cb0, cc1 = lo ? ca1 : cb1;
        const int ic = lo ? ia : ib;
        const int ii = __builtin_amdgcn_readlane(HI ? idxB : idxA, il);
        const bool hit = (unsigned)lane == cl;
        A0 = (hit && lo) ? cj0 : A0; A1 = (hit && lo) ? cj1 : A1;
        idxA = (hit && lo) ? ii : idxA;
        B0 = (hit && !lo) ? cj0 : B0; B1 = (hit && !lo) ? cj1 : B1;
        idxB = (hit && !lo) ? ii : idxB;
        if constexpr (HI) {
            B0 = (lane == il) ? cc0 : B0; B1 = (lane == il) ? cc1 : B1;
            idxB = (lane == il) ? ic : idxB;
        } else {
            A0 = (lane == il) ? cc0 : A0; A1 = (lane == il) ? cc1 : A1;
            idxA = (lane == il) ? ic : idxA;
        }
        ++nsw;
        cj0 = cc0; cj1 = cc1;                                     // the exchanged-in column has its 1 in logical row i
        balA = HI ? 0ull : (1ull << il);
        balB = HI ? (1ull << il) : 0ull;
    }
    // the first logical row wins; exchange logical rows i and r (r == i: no change)
    const bool rlo = balA != 0;
    const int rl = rlo ? __builtin_ctzll(balA) : __builtin_ctzll(balB);
    const int pra = __builtin_amdgcn_readlane(rhoA, rl), prb = __builtin_amdgcn_readlane(rhoB, rl);
    const int pr = rlo ? pra : prb;
    const int pi = __builtin_amdgcn_readlane(HI ? rhoB : rhoA, il);
    rhoA = (rlo && lane == rl) ? pi : rhoA;
    rhoB = (!rlo && lane == rl) ? pi : rhoB;
    if constexpr (HI) rhoB = (lane == il) ? pr : rhoB;
    else rhoA = (lane == il) ? pr : rhoA;
    // clear column i in every other row: the pivot column without its pivot
    const u64 pbit = 1ull << (pr & 63);
    const u64 e0 = cj0 & ~((pr & 64) ? 0ull : pbit), e1 = cj1 & ~((pr & 64) ? pbit : 0ull);
    const bool ha = bit128(A0, A1, pr), hb = bit128(B0, B1, pr);
    A0 ^= ha ? e0 : 0ull; A1 ^= ha ? e1 : 0ull;
    B0 ^= hb ? e0 : 0ull; B1 ^= hb ? e1 : 0ull;
}

// k pivot steps with a run-time trip count, split at step 64.  Returns the number of column exchanges, or -1 for a
// rank-deficient matrix (as gex_columns, ldpc_osdx.h).
__device__ __forceinline__ int gew_columns(u64 &A0, u64 &A1, u64 &B0, u64 &B1, int &rhoA, int &rhoB, int &idxA, int &idxB, int k, int lane)
{
    int nsw = 0;
    bool deficient = false;
    const u64 rowsA = k >= 64 ? ~0ull : ((1ull << k) - 1ull);
    const u64 rowsB = k > 64 ? ((1ull << (k - 64)) - 1ull) : 0ull;   // (k <= 127)
    const int k1 = k < 64 ? k : 64;
#pragma unroll 1
    for (int i = 0; i < k1; ++i) gew_step<false>(A0, A1, B0, B1, rhoA, rhoB, idxA, idxB, i, rowsA, rowsB, lane, nsw, deficient);
#pragma unroll 1
    for (int i = 64; i < k; ++i) gew_step<true>(A0, A1, B0, B1, rhoA, rhoB, idxA, idxB, i, rowsA, rowsB, lane, nsw, deficient);
    return deficient ? -1 : nsw;
}

// ---------------------------------------------------------------------------------------
// front end: reliability sort, column gather, elimination, MRB / LRB bookkeeping
//   Gcols      [n][2] u64   : column v of G, rows 0..63 / 64..127
//   perm_out   [F][128] u8  : original bit at primed position p (MRB 0..k-1, parity k..n-1), 0 for p >= n
//   parity_out [F][128] u64 : row r < k, bit c < n - k = P'[r][c]; 0 elsewhere
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void osdw_front_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const u64 *__restrict__ Gcols, unsigned char *__restrict__ perm_out, u64 *__restrict__ parity_out,
        int *__restrict__ nswaps)
{
    __shared__ FrontWLds L;   // one wavefront per workgroup
    const int lane = threadIdx.x;
    const long long nframes = frame_count(count, F);

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        // ---- reliability sort: as osdx_front_kernel (ldpc_osdx.h), padded slots included ------
        const unsigned a1 = lane < n ? (__float_as_uint(y[src * n + lane]) & 0x7FFFFFFFu) : 0u;
        const unsigned a2 = 64 + lane < n ? (__float_as_uint(y[src * n + 64 + lane]) & 0x7FFFFFFFu) : 0u;
        const float bs = bucket_scale(a1, a2);
        int r1, r2;
        bucket_ranks(L.rank, ((u64)a1 << 32) | (unsigned)(127 - lane), ((u64)a2 << 32) | (unsigned)(63 - lane), bucket_of(a1, bs),
                     bucket_of(a2, bs), lane, r1, r2);
        L.pi1[r1] = (unsigned char)lane;
        L.pi1[r2] = (unsigned char)(lane + 64);
        if (lane < 4) L.mask[lane] = 0;
        L.col0[lane] = 0ull; L.col1[lane] = 0ull;
        L.perm[lane] = 0; L.perm[lane + 64] = 0;
        wave_fence();
        // ---- G with columns in sorted order, column-major, two words per column ----------------
        const int pA = lane, pB = 64 + lane;                    // the sorted positions of this lane's slots
        const bool liveA = pA < n, liveB = pB < n;
        const int oA = L.pi1[pA], oB = L.pi1[pB];
        u64 A0 = liveA ? Gcols[2 * oA] : 0ull, A1 = liveA ? Gcols[2 * oA + 1] : 0ull;
        u64 B0 = liveB ? Gcols[2 * oB] : 0ull, B1 = liveB ? Gcols[2 * oB + 1] : 0ull;
        int rhoA = pA, rhoB = pB, idxA = pA, idxB = pB;
        const int ns = gew_columns(A0, A1, B0, B1, rhoA, rhoB, idxA, idxB, k, lane);
        // ---- identify_mrb bookkeeping (:276-304): both index sets ascending ------------------
        const bool mrbA = pA < k, mrbB = pB < k;
        if (mrbA) atomicOr(&L.mask[idxA >> 5], 1u << (idxA & 31));
        if (mrbB) atomicOr(&L.mask[idxB >> 5], 1u << (idxB & 31));
        wave_fence();
        const unsigned mk[4] = {L.mask[0], L.mask[1], L.mask[2], L.mask[3]};
        const int cntA = below_mask(mk, idxA), cntB = below_mask(mk, idxB);   // MRB members below this slot's index
        if (mrbA) {
            L.perm[cntA] = L.pi1[idxA];                         // new MRB position of slot A
            L.rowsrc[cntA] = (unsigned char)rhoA;               // its pivot is physical row rhoA
        } else if (liveA) {
            const int c = idxA - cntA;                          // new parity column of slot A (< n - k unless the matrix is deficient)
            if (c < n - k) { L.perm[k + c] = L.pi1[idxA]; L.col0[c] = A0; L.col1[c] = A1; }
        }
        if (mrbB) {
            L.perm[cntB] = L.pi1[idxB];
            L.rowsrc[cntB] = (unsigned char)rhoB;
        } else if (liveB) {
            const int c = idxB - cntB;
            if (c < n - k) { L.perm[k + c] = L.pi1[idxB]; L.col0[c] = B0; L.col1[c] = B1; }
        }
        wave_fence();
        L.rows[lane] = transpose64(L.col0[lane], lane);         // lane = physical row, bit = parity column
        L.rows[64 + lane] = transpose64(L.col1[lane], lane);
        wave_fence();
        perm_out[f * 128 + lane] = L.perm[lane];
        perm_out[f * 128 + 64 + lane] = L.perm[64 + lane];
        parity_out[f * 128 + lane] = mrbA ? L.rows[L.rowsrc[lane] & 127] : 0ull;
        parity_out[f * 128 + 64 + lane] = mrbB ? L.rows[L.rowsrc[64 + lane] & 127] : 0ull;
        if (nswaps && lane == 0) nswaps[f] = ns;
        wave_fence();
    }
}

// ---------------------------------------------------------------------------------------
// conventional order-p search over the reference's TEP table for THIS k (the scan of osdx_search_kernel with up to 127 MRB
// positions)
//   SearchWLds: w[0..k-1] = |y'| of the MRB, w[128..128+n-k-1] = |y'| of the parity part, zero elsewhere; the eight byte LUTs
//   hold the sums of np_oracle._weighted_distance_k (bytes of eight positions from primed position k, each ascending from
//   0.0f: a padded position adds 0.0f, which changes no bit of a sum >= 0).
//   cw_out [F][words] u64, words = ceil(n / 64); label [*][words] addressed through `index`.
//   counts[3] += {frames, frames_wrong, teps_total} (with label; teps_total only with ntep_out): one atomic per counter and
//   wavefront, after its last frame.
// ---------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) SearchWLds {
    float lut[8][256];   // lut[b][v] = sum of |y'[k+8b+t]| over the set bits t of v, ascending t
    u64 P[128];          // rows of P'
    float w[192];        // |y'|: MRB at 0..127, parity part at 128..191
    u64 cw[2];           // codeword being assembled in original bit order
};

// one TEP (ascending support s.x < s.y < s.z, weight s.w) -> parity discrepancy, MRB weight sum (tep_apply without the mask)
__device__ __forceinline__ void tepw_apply(const SearchWLds &L, uchar4 s, u64 d0, u64 &D, float &mrb)
{
    D = d0; mrb = 0.0f;
    if (s.w > 0) { D ^= L.P[s.x]; mrb = L.w[s.x]; }
    if (s.w > 1) { D ^= L.P[s.y]; mrb = mrb + L.w[s.y]; }
    if (s.w > 2) { D ^= L.P[s.z]; mrb = mrb + L.w[s.z]; }
}

__global__ __launch_bounds__(64) void osdw_search_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const unsigned char *__restrict__ perm_in, const u64 *__restrict__ parity_in,
        const uchar4 *__restrict__ teps, int ntep, u64 *__restrict__ cw_out, float *__restrict__ metric_out, int *__restrict__ best_out,
        int *__restrict__ ntep_out, const u64 *__restrict__ label, u64 *__restrict__ counts)
{
    __shared__ SearchWLds L;   // one wavefront per workgroup: compile-time LDS base for the LUT reads
    const int lane = threadIdx.x;
    const int m = n - k;
    const int words = (n + 63) >> 6;
    const u64 colmask = m >= 64 ? ~0ull : ((1ull << m) - 1ull);
    const bool liveA = lane < k, liveB = 64 + lane < k, liveP = lane < m;   // primed positions lane, 64 + lane, k + lane
    const long long nframes = frame_count(count, F);
    unsigned long long seen = 0, wrong = 0, nteps = 0;

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        // ---- primed-order values, rows of P', hard decisions, byte LUTs, the order-0 discrepancy ----
        const int oA = liveA ? perm_in[f * 128 + lane] : 0, oB = liveB ? perm_in[f * 128 + 64 + lane] : 0;
        const int oP = liveP ? perm_in[f * 128 + k + lane] : 0;
        const float yA = liveA ? y[src * n + oA] : 0.0f, yB = liveB ? y[src * n + oB] : 0.0f, yP = liveP ? y[src * n + oP] : 0.0f;
        L.w[lane] = __builtin_fabsf(yA);
        L.w[64 + lane] = __builtin_fabsf(yB);
        L.w[128 + lane] = __builtin_fabsf(yP);
        const u64 rowA = liveA ? (parity_in[f * 128 + lane] & colmask) : 0ull;
        const u64 rowB = liveB ? (parity_in[f * 128 + 64 + lane] & colmask) : 0ull;
        L.P[lane] = rowA;
        L.P[64 + lane] = rowB;
        if (lane < 2) L.cw[lane] = 0;
        const u64 hmA = __ballot(liveA && !(yA > 0.0f)), hmB = __ballot(liveB && !(yB > 0.0f));   // idle lanes stay out: y = 0 is a hard 1
        const u64 hp = __ballot(liveP && !(yP > 0.0f));
        wave_fence();
        build_byte_luts<8>(L.lut, &L.w[128], lane);
        // d0 = (u0 . P') ^ h_parity : XOR-reduce the rows selected by the MRB hard decisions, two rows per lane
        const u64 d0 = wave_xor64((((hmA >> lane) & 1) ? rowA : 0ull) ^ (((hmB >> lane) & 1) ? rowB : 0ull)) ^ hp;
        wave_fence();
        // ---- scan the TEP table, one TEP per lane per round; strict '<' keeps the first minimum ----
        float best = __builtin_inff();
        int bestt = 0x7FFFFFFF;
        u64 bestD = 0;
        float bound = __builtin_inff();   // exact early exit on the metric prefix (tep_cost_bounded): the wave's best so far
        int trip = 0;
        for (int t0 = 0; t0 < ntep; t0 += 64, ++trip) {
            const int t = t0 + lane;
            if (t < ntep) {
                u64 D;
                float mrb, c;
                tepw_apply(L, teps[t], d0, D, mrb);
                if (tep_cost_bounded(L, mrb, D, bound, c) && c < best) { best = c; bestt = t; bestD = D; }
            }
            if ((trip & 7) == 0) bound = wave_min_f32(best);
        }
        {   // wave_argmin (ldpc_search.h) without the flip mask: the winner's flipped positions are its table entry
            const int wl = wave_argmin_lane(best, bestt);
            best = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(best), wl));
            bestt = __builtin_amdgcn_readlane(bestt, wl);
            bestD = readlane64(bestD, wl);
        }
        uchar4 win;   // (no lane found a candidate -- every cost a NaN or +inf --: bestt is no index, nothing is flipped)
        win.x = win.y = win.z = win.w = 0;
        if (bestt < ntep) win = teps[bestt];
        // ---- candidate -> codeword in ORIGINAL bit order, ceil(n / 64) words ---------------------
        const u64 par_bits = bestD ^ hp;
        if (liveA && ((((hmA >> lane) & 1) != 0) != tep_flips(win, lane))) atomicOr(&L.cw[oA >> 6], 1ull << (oA & 63));
        if (liveB && ((((hmB >> lane) & 1) != 0) != tep_flips(win, 64 + lane))) atomicOr(&L.cw[oB >> 6], 1ull << (oB & 63));
        if (liveP && ((par_bits >> lane) & 1)) atomicOr(&L.cw[oP >> 6], 1ull << (oP & 63));
        wave_fence();
        if (lane < words) cw_out[f * words + lane] = L.cw[lane];
        store_results(f, lane, best, bestt, ntep, metric_out, best_out, ntep_out);
        if (label) {
            bool bad = false;
            for (int w = 0; w < words; ++w) bad |= L.cw[w] != label[src * words + w];
            seen += 1; wrong += bad; nteps += ntep_out ? (unsigned long long)ntep : 0ull;
        }
        wave_fence();
    }
    if (label && lane == 0 && seen) {
        atomicAdd(&counts[0], seen);
        atomicAdd(&counts[1], wrong);
        if (nteps) atomicAdd(&counts[2], nteps);
    }
}

}  // namespace ldpc
