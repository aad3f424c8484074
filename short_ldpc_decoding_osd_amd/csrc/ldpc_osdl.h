// OSD for longer and low-rate codes (n <= 384, 1 <= k <= 192, 1 <= n - k <= 192): the front end and the conventional order-p
// table scan with the code's n and k as kernel arguments, one frame per wavefront.
//   swapped_info / identify_mrb / full_gf2elim   PB_OSD/pb_testing.py:231-320
//   convention_osd_main                           FS_OSD/convention_osd.py:49-76
// The kernels of ldpc_osdw.h one size up.  With S = ceil(n / 64), W = ceil(k / 64) and Wp = ceil((n - k) / 64):
//   a column of G is W words (physical rows 64 w .. 64 w + 63), lane l owns the sorted columns 64 s + l of the S slots and the
//   logical rows 64 w + l of the W row words; a row of P' and the discrepancy D of a TEP are Wp words.
// The front end is a template on (S, W) and the scan on Wp: every slot and word loop is unrolled and nothing in registers is
// indexed at run time, so the columns stay in registers (no scratch; profiles/osdl/README.md).  The host routes a code to S
// rounded up to 2, 4 or 6 (an idle slot carries zero columns) and to its own W and Wp.
// The metric (tep_cost_bounded, lut_byte) and the wave helpers of ldpc_search.h / ldpc_wave.h are used unchanged.
// osdl_prepare / osdl_finish are the per-frame prologue and epilogue every search on such front-end results shares.
#pragma once

#include "ldpc_search.h"

namespace ldpc {

constexpr int kOsdlN = 384, kOsdlK = 192, kOsdlM = 192;   // the limits of the family: n, k, n - k

struct __attribute__((aligned(16))) FrontLLds {
    u64 key[kOsdlN];                  // sort keys of the frame's positions: (|y| bits, 0xFFFF - position)
    u64 col[3][kOsdlM];               // parity columns in primed order, one array per row word (zero beyond n - k)
    u64 rows[kOsdlK][3];              // physical row -> its n - k parity bits, Wp words
    unsigned mask[kOsdlN / 32];       // membership mask of the MRB's sorted positions
    unsigned pre[kOsdlN / 32];        // set bits of the mask in the words below each word
    unsigned short pi1[kOsdlN];       // sorted position -> original bit
    unsigned short perm[kOsdlN];      // primed position -> original bit (zero beyond n)
    unsigned char rowsrc[kOsdlK];     // primed MRB position -> physical row of its pivot
};

// bit p (0..64 W - 1) of the W-word column c
template <int W>
__device__ __forceinline__ bool bitw(const u64 (&c)[W], int p)
{
    // (each word against zero, never one word against another: a select between two elements of an array becomes an indexed
    //  read of it, and an array that is indexed at run time lives in scratch)
    u64 w = c[0];
    if constexpr (W > 1) {
        w = (p >> 6) == 0 ? w : 0ull;
#pragma unroll
        for (int v = 1; v < W; ++v) w |= (p >> 6) == v ? c[v] : 0ull;
    }
    return ((w >> (p & 63)) & 1ull) != 0;
}

// One pivot step i of the Gauss-Jordan elimination over k <= 192 rows (full_gf2elim :231-266), columns in registers: gew_step
// (ldpc_osdw.h) with S slots and W row words.
//   C[s][w] : sorted column 64 s + lane, word w: bit = PHYSICAL row 64 w + bit (rows >= k do not exist: those bits are zero)
//   rho[w]  : logical row 64 w + lane -> physical row (row exchanges permute this map only)
//   idx[s]  : the sorted position travelling with the column of slot s (:276-281)
//   rows[w] : the logical rows that exist, per row word
// HW = i / 64: the slot of pivot column i and the row word of logical row i are compile-time facts in each third of the loop.
// The slot of an exchange partner and the word of the pivot row are wave-uniform run-time values: each is resolved by selects
// over the unrolled slots / words, never by an index.  Idle slots hold zero columns, so they are never a pivot row nor a partner.
template <int S, int W, int HW>
__device__ __forceinline__ void gel_step(u64 (&C)[S][W], int (&rho)[W], int (&idx)[S], int i, const u64 (&rows)[W], int lane, int &nsw,
                                         bool &deficient)
{
    const int il = i & 63;                                        // the lane of column i and of logical row i
    const u64 from = ~0ull << il;
    u64 cj[W], bal[W];
    u64 any = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) cj[w] = readlane64(C[HW][w], il);
#pragma unroll
    for (int w = 0; w < W; ++w) {                                 // logical rows >= i with a 1 in column i
        bal[w] = w < HW ? 0ull : (__ballot(bitw<W>(cj, rho[w])) & (w == HW ? (rows[w] & from) : rows[w]));
        any |= bal[w];
    }
    if (any == 0) {
        // no pivot in column i: exchange it with the first later column, in sorted order, that has a 1 in logical row i
        const int pri = __builtin_amdgcn_readlane(rho[HW], il);
        int sc = HW;                                              // the partner's slot and its ballot; the first slot wins
        u64 bsel = 0;
#pragma unroll
        for (int s = S - 1; s >= HW; --s) {
            const u64 b = __ballot(bitw<W>(C[s], pri)) & (s == HW ? from : ~0ull);
            if (b != 0) { sc = s; bsel = b; }
        }
        deficient |= bsel == 0;                                   // all-zero row: carry on with garbage, report at the end
        const unsigned cl = bsel ? __builtin_ctzll(bsel) : 0;
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
        const bool h = bitw<W>(C[s], pr);
#pragma unroll
        for (int w = 0; w < W; ++w) C[s][w] ^= h ? e[w] : 0ull;
    }
}

// k pivot steps with a run-time trip count, split at steps 64 and 128.  Returns the number of column exchanges, or -1 for a
// rank-deficient matrix (as gew_columns, ldpc_osdw.h).
template <int S, int W>
__device__ __forceinline__ int gel_columns(u64 (&C)[S][W], int (&rho)[W], int (&idx)[S], int k, int lane)
{
    int nsw = 0;
    bool deficient = false;
    u64 rows[W];
#pragma unroll
    for (int w = 0; w < W; ++w) rows[w] = k >= 64 * (w + 1) ? ~0ull : (k > 64 * w ? ((1ull << (k - 64 * w)) - 1ull) : 0ull);
    {
        const int e = k < 64 ? k : 64;
#pragma unroll 1
        for (int i = 0; i < e; ++i) gel_step<S, W, 0>(C, rho, idx, i, rows, lane, nsw, deficient);
    }
    if constexpr (W > 1) {
        const int e = k < 128 ? k : 128;
#pragma unroll 1
        for (int i = 64; i < e; ++i) gel_step<S, W, 1>(C, rho, idx, i, rows, lane, nsw, deficient);
    }
    if constexpr (W > 2) {
#pragma unroll 1
        for (int i = 128; i < k; ++i) gel_step<S, W, 2>(C, rho, idx, i, rows, lane, nsw, deficient);
    }
    return deficient ? -1 : nsw;
}

// ---------------------------------------------------------------------------------------
// front end: reliability sort, column gather, elimination, MRB / LRB bookkeeping
//   S >= ceil(n / 64) slots, W = ceil(k / 64) row words; Sn = ceil(n / 64), Wp = ceil((n - k) / 64)
//   Gcols      [n][W] u64        : column v of G, word w = rows 64 w .. 64 w + 63
//   perm_out   [F][64 Sn] u16    : original bit at primed position p (MRB 0..k-1, parity k..n-1), 0 for p >= n
//   parity_out [F][64 W][Wp] u64 : row r < k, bit c of word q = P'[r][64 q + c]; 0 in rows >= k and bits >= n - k
// The sort ranks every key against all n keys of the frame through LDS (every lane reads the same entry: a broadcast); the
// keys are distinct, descending |y| with ties to the lower index.
// ---------------------------------------------------------------------------------------
template <int S, int W>
__global__ __launch_bounds__(64) void osdl_front_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const u64 *__restrict__ Gcols, unsigned short *__restrict__ perm_out, u64 *__restrict__ parity_out,
        int *__restrict__ nswaps)
{
    __shared__ FrontLLds L;   // one wavefront per workgroup
    const int lane = threadIdx.x;
    const int m = n - k, Sn = (n + 63) >> 6, Wp = (m + 63) >> 6;
    const long long nframes = frame_count(count, F);

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        // ---- reliability sort --------------------------------------------------------------------
        u64 key[S];
        int rank[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int p = 64 * s + lane;
            const unsigned a = p < n ? (__float_as_uint(y[src * n + p]) & 0x7FFFFFFFu) : 0u;
            key[s] = ((u64)a << 32) | (unsigned)(0xFFFF - p);
            rank[s] = 0;
            if (p < n) L.key[p] = key[s];
            L.perm[p] = 0;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) { L.col[w][lane] = 0ull; L.col[w][64 + lane] = 0ull; L.col[w][128 + lane] = 0ull; }
        if (lane < kOsdlN / 32) L.mask[lane] = 0;
        wave_fence();
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const u64 kj = L.key[j];
#pragma unroll
            for (int s = 0; s < S; ++s) rank[s] += kj > key[s];
        }
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (64 * s + lane < n) L.pi1[rank[s]] = (unsigned short)(64 * s + lane);
        wave_fence();
        // ---- G with columns in sorted order, column-major, W words per column ----------------------
        u64 C[S][W];
        int idx[S], rho[W];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int p = 64 * s + lane;                        // the sorted position of this lane's slot s
            const int o = p < n ? L.pi1[p] : 0;
#pragma unroll
            for (int w = 0; w < W; ++w) C[s][w] = p < n ? Gcols[(long long)o * W + w] : 0ull;
            idx[s] = p;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) rho[w] = 64 * w + lane;
        const int ns = gel_columns<S, W>(C, rho, idx, k, lane);
        // ---- identify_mrb bookkeeping (:276-304): both index sets ascending ------------------
#pragma unroll
        for (int s = 0; s < W; ++s)
            if (64 * s + lane < k) atomicOr(&L.mask[idx[s] >> 5], 1u << (idx[s] & 31));
        wave_fence();
        if (lane == 0) {
            unsigned a = 0;
            for (int j = 0; j < kOsdlN / 32; ++j) { L.pre[j] = a; a += __popc(L.mask[j]); }
        }
        wave_fence();
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int p = 64 * s + lane, x = idx[s];
            const int cnt = (int)(L.pre[x >> 5] + __popc(L.mask[x >> 5] & ((1u << (x & 31)) - 1u)));   // MRB members below this slot's index
            const unsigned short orig = L.pi1[x];
            if (s < W && p < k) {                               // (s is a constant once the loop is unrolled)
                L.perm[cnt] = orig;                             // new MRB position of the slot
                L.rowsrc[cnt] = (unsigned char)rho[s < W ? s : 0];   // its pivot is physical row rho[s]
            } else if (p < n) {
                const int c = x - cnt;                          // new parity column of the slot (< n - k unless the matrix is deficient)
                if (c < m) {
                    L.perm[k + c] = orig;
#pragma unroll
                    for (int w = 0; w < W; ++w) L.col[w][c] = C[s][w];
                }
            }
        }
        wave_fence();
#pragma unroll
        for (int w = 0; w < W; ++w)
            for (int q = 0; q < Wp; ++q) L.rows[64 * w + lane][q] = transpose64(L.col[w][64 * q + lane], lane);   // lane = physical row, bit = parity column
        wave_fence();
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (s < Sn) perm_out[(f * Sn + s) * 64 + lane] = L.perm[64 * s + lane];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int p = 64 * w + lane;
            const int rs = p < k ? L.rowsrc[p] : 0;
            for (int q = 0; q < Wp; ++q) parity_out[((f * W + w) * 64 + lane) * Wp + q] = p < k ? L.rows[rs][q] : 0ull;
        }
        if (nswaps && lane == 0) nswaps[f] = ns;
        wave_fence();
    }
}

// ---------------------------------------------------------------------------------------
// LDS of the searches: up to 192 MRB positions and a discrepancy of WP = ceil((n - k) / 64) words
//   SearchLLds: w[0..k-1] = |y'| of the MRB, w[192..192+n-k-1] = |y'| of the parity part, zero elsewhere; the 8 WP byte LUTs
//   hold the sums of np_oracle._weighted_distance_k (bytes of eight positions from primed position k, each ascending from
//   0.0f: a padded position adds 0.0f, which changes no bit of a sum >= 0).
// ---------------------------------------------------------------------------------------
template <int WP>
struct __attribute__((aligned(16))) SearchLLds {
    float lut[8 * WP][256];       // lut[8 q + b][v] = sum of |y'[k + 64 q + 8 b + t]| over the set bits t of v, ascending t
    u64 P[kOsdlK][WP];            // rows of P'
    float w[kOsdlK + 64 * WP];    // |y'|: MRB at 0..191, parity part from 192
    u64 cw[kOsdlN / 64];          // codeword being assembled in original bit order
};

template <int WP>
struct __attribute__((aligned(16))) SearchLLdsLean {   // SearchLLds without the byte LUTs (at WP = 3: 7.6 KiB instead of 31.6)
    u64 P[kOsdlK][WP];
    float w[kOsdlK + 64 * WP];
    u64 cw[kOsdlN / 64];
};

// ---------------------------------------------------------------------------------------
// per-frame prologue and epilogue of every search on this family's front-end results (osdw_prepare / osdw_finish of ldpc_osdw.h
// with three MRB slots per lane and WP parity words).  Idle lanes stay out of the hard-decision ballots -- their y = 0 would
// count as a hard 1 --, rows of P' are masked to n - k columns, and w[] and P[] are zero beyond the live positions.
//   LDS: SearchLLds<WP> (LUTS = true: the 8 WP byte LUTs over w[192..] are built) or SearchLLdsLean<WP> (LUTS = false).
//   perm_in [F][64 ceil(n/64)] u16 and parity_in [F][64 ceil(k/64)][WP] u64 as osdl_front_kernel writes them; an entry of
//   perm_in at or beyond n is read as 0 (the caller's error: nothing is read or written outside the buffers).
// ---------------------------------------------------------------------------------------
template <int WP>
struct OsdlFrame {
    u64 hm[3], hp[WP], d0[WP];   // hard decisions (y' > 0 ? 0 : 1) of MRB positions 64 s + lane / the parity part, order-0 discrepancy
    int oM[3], oP[WP];           // original bit of primed positions 64 s + lane / k + 64 q + lane
};

template <int WP, bool LUTS, class LDS>
__device__ __forceinline__ OsdlFrame<WP> osdl_prepare(LDS &L, const float *__restrict__ y, long long src, const unsigned short *__restrict__ perm_in,
                                                     const u64 *__restrict__ parity_in, long long f, int n, int k, int lane)
{
    OsdlFrame<WP> S;
    const int m = n - k;
    const int words = (n + 63) >> 6, Wk = (k + 63) >> 6;
    const unsigned short *perm = perm_in + f * words * 64;
    u64 colmask[WP];
#pragma unroll
    for (int q = 0; q < WP; ++q) colmask[q] = m >= 64 * (q + 1) ? ~0ull : (m > 64 * q ? ((1ull << (m - 64 * q)) - 1ull) : 0ull);
#pragma unroll
    for (int q = 0; q < WP; ++q) S.d0[q] = 0ull;
#pragma unroll
    for (int s = 0; s < 3; ++s) {                           // primed MRB position 64 s + lane
        const int p = 64 * s + lane;
        const bool live = p < k;
        const int o = live ? perm[p] : 0;
        S.oM[s] = o < n ? o : 0;
        const float yv = live ? y[src * n + S.oM[s]] : 0.0f;
        L.w[p] = __builtin_fabsf(yv);
        S.hm[s] = __ballot(live && !(yv > 0.0f));           // idle lanes stay out: y = 0 is a hard 1
#pragma unroll
        for (int q = 0; q < WP; ++q) {
            const u64 row = live ? (parity_in[((f * Wk * 64) + p) * WP + q] & colmask[q]) : 0ull;
            L.P[p][q] = row;
            S.d0[q] ^= ((S.hm[s] >> lane) & 1) ? row : 0ull;
        }
    }
#pragma unroll
    for (int q = 0; q < WP; ++q) {                          // primed parity position k + 64 q + lane
        const int p = 64 * q + lane;
        const bool live = p < m;
        const int o = live ? perm[k + p] : 0;
        S.oP[q] = o < n ? o : 0;
        const float yv = live ? y[src * n + S.oP[q]] : 0.0f;
        L.w[kOsdlK + p] = __builtin_fabsf(yv);
        S.hp[q] = __ballot(live && !(yv > 0.0f));
    }
    if (lane < kOsdlN / 64) L.cw[lane] = 0;
    wave_fence();
#pragma unroll
    for (int q = 0; q < WP; ++q) {
        if constexpr (LUTS) build_byte_luts<8>(&L.lut[8 * q], &L.w[kOsdlK + 64 * q], lane);
        S.d0[q] = wave_xor64(S.d0[q]) ^ S.hp[q];            // d0 = (u0 . P') ^ h_parity
    }
    wave_fence();
    return S;
}

// candidate (flip[s]: whether it flips MRB position 64 s + lane, D = parity discrepancy) -> codeword in ORIGINAL bit order,
// ceil(n / 64) words; L.cw holds it afterwards (the callers compare it with the label before their closing wave_fence)
template <int WP, class LDS>
__device__ __forceinline__ void osdl_finish(LDS &L, const OsdlFrame<WP> &S, const bool (&flip)[3], const u64 (&D)[WP], long long f, int n, int k,
                                            int lane, u64 *__restrict__ cw_out)
{
    const int m = n - k, words = (n + 63) >> 6;
#pragma unroll
    for (int s = 0; s < 3; ++s)
        if (64 * s + lane < k && ((((S.hm[s] >> lane) & 1) != 0) != flip[s])) atomicOr(&L.cw[S.oM[s] >> 6], 1ull << (S.oM[s] & 63));
#pragma unroll
    for (int q = 0; q < WP; ++q) {
        const u64 par_bits = D[q] ^ S.hp[q];
        if (64 * q + lane < m && ((par_bits >> lane) & 1)) atomicOr(&L.cw[S.oP[q] >> 6], 1ull << (S.oP[q] & 63));
    }
    wave_fence();
    if (lane < words) cw_out[f * words + lane] = L.cw[lane];
}

// tep_cost_bounded (ldpc_search.h) over WP words of discrepancy: word 0 as there (exit after its two most reliable bytes), then
// a word at a time, with the same exact exit before each: every term is >= 0, so a prefix above the bound can neither win nor tie.
template <int WP>
__device__ __forceinline__ bool tepl_cost_bounded(const SearchLLds<WP> &L, float mrb, const u64 (&D)[WP], float bound, float &cost)
{
    float acc;
    if (!tep_cost_bounded(L, mrb, D[0], bound, acc)) return false;
#pragma unroll
    for (int q = 1; q < WP; ++q) {
        if (acc > bound) return false;
        const float(*lut)[256] = &L.lut[8 * q];
        acc = acc + lut_byte<0>(lut, D[q]); acc = acc + lut_byte<1>(lut, D[q]); acc = acc + lut_byte<2>(lut, D[q]);
        acc = acc + lut_byte<3>(lut, D[q]); acc = acc + lut_byte<4>(lut, D[q]); acc = acc + lut_byte<5>(lut, D[q]);
        acc = acc + lut_byte<6>(lut, D[q]); acc = acc + lut_byte<7>(lut, D[q]);
    }
    cost = acc;
    return true;
}

// one TEP (ascending support s.x < s.y < s.z, weight s.w) -> parity discrepancy, MRB weight sum (tepw_apply with WP words)
template <int WP>
__device__ __forceinline__ void tepl_apply(const SearchLLds<WP> &L, uchar4 s, const u64 (&d0)[WP], u64 (&D)[WP], float &mrb)
{
    mrb = 0.0f;
#pragma unroll
    for (int q = 0; q < WP; ++q) D[q] = d0[q];
    if (s.w > 0) { mrb = L.w[s.x];
#pragma unroll
        for (int q = 0; q < WP; ++q) D[q] ^= L.P[s.x][q]; }
    if (s.w > 1) { mrb = mrb + L.w[s.y];
#pragma unroll
        for (int q = 0; q < WP; ++q) D[q] ^= L.P[s.y][q]; }
    if (s.w > 2) { mrb = mrb + L.w[s.z];
#pragma unroll
        for (int q = 0; q < WP; ++q) D[q] ^= L.P[s.z][q]; }
}

// ---------------------------------------------------------------------------------------
// conventional order-p search over the reference's TEP table for THIS k (the scan of osdw_search_kernel with up to 192 MRB
// positions and a discrepancy of WP words), on osdl_prepare / osdl_finish
//   cw_out [F][words] u64, words = ceil(n / 64); label [*][words] addressed through `index`.
//   counts[3] += {frames, frames_wrong, teps_total} (with label; teps_total only with ntep_out): one atomic per counter and
//   wavefront, after its last frame.
// The first minimum wins, +inf included: when every cost is +inf the winner is the first TEP of the table, as np.argmin has it
// (the two older families return "no candidate" there: best = 0x7FFFFFFF, nothing flipped).
// ---------------------------------------------------------------------------------------
template <int WP>
__global__ __launch_bounds__(64) void osdl_search_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const unsigned short *__restrict__ perm_in, const u64 *__restrict__ parity_in,
        const uchar4 *__restrict__ teps, int ntep, u64 *__restrict__ cw_out, float *__restrict__ metric_out, int *__restrict__ best_out,
        int *__restrict__ ntep_out, const u64 *__restrict__ label, u64 *__restrict__ counts)
{
    __shared__ SearchLLds<WP> L;   // one wavefront per workgroup: compile-time LDS base for the LUT reads
    const int lane = threadIdx.x;
    const int words = (n + 63) >> 6;
    const long long nframes = frame_count(count, F);
    unsigned long long seen = 0, wrong = 0, nteps = 0;

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        const OsdlFrame<WP> S = osdl_prepare<WP, true>(L, y, src, perm_in, parity_in, f, n, k, lane);
        // ---- scan the TEP table, one TEP per lane per round; the first minimum wins ------------------
        float best = __builtin_inff();
        int bestt = 0x7FFFFFFF;
        u64 bestD[WP];
#pragma unroll
        for (int q = 0; q < WP; ++q) bestD[q] = 0ull;
        float bound = __builtin_inff();   // exact early exit on the metric prefix (tepl_cost_bounded): the wave's best so far
        int trip = 0;
        for (int t0 = 0; t0 < ntep; t0 += 64, ++trip) {
            const int t = t0 + lane;
            if (t < ntep) {
                u64 D[WP];
                float mrb, c;
                tepl_apply<WP>(L, teps[t], S.d0, D, mrb);
                // (c == best: only while the lane holds no candidate yet -- t ascends in a lane -- i.e. for a first cost of +inf)
                if (tepl_cost_bounded<WP>(L, mrb, D, bound, c) && (c < best || (c == best && t < bestt))) {
                    best = c; bestt = t;
#pragma unroll
                    for (int q = 0; q < WP; ++q) bestD[q] = D[q];
                }
            }
            if ((trip & 7) == 0) bound = wave_min_f32(best);
        }
        {   // wave arg-min on (cost, index); the winner's flipped positions are its table entry
            const int wl = wave_argmin_lane(best, bestt);
            best = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(best), wl));
            bestt = __builtin_amdgcn_readlane(bestt, wl);
#pragma unroll
            for (int q = 0; q < WP; ++q) bestD[q] = readlane64(bestD[q], wl);
        }
        uchar4 win;   // (no lane found a candidate -- every cost a NaN --: bestt is no index, nothing is flipped)
        win.x = win.y = win.z = win.w = 0;
        if (bestt < ntep) win = teps[bestt];
        const bool flip[3] = {tep_flips(win, lane), tep_flips(win, 64 + lane), tep_flips(win, 128 + lane)};
        osdl_finish<WP>(L, S, flip, bestD, f, n, k, lane, cw_out);
        store_results(f, lane, best, bestt, ntep, metric_out, best_out, ntep_out);
        if (label) { seen += 1; wrong += cw_wrong(L, label, src, words); nteps += ntep_out ? (unsigned long long)ntep : 0ull; }
        wave_fence();
    }
    if (label && lane == 0 && seen) {
        atomicAdd(&counts[0], seen);
        atomicAdd(&counts[1], wrong);
        if (nteps) atomicAdd(&counts[2], nteps);
    }
}

}  // namespace ldpc
