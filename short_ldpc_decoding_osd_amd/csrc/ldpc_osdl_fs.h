// OSD for longer and low-rate codes: osdl_fs_kernel and osdl_tep_eval_kernel.
// FS-OSD (fs_osd, FS_OSD/fs_testing.py:129-161) with the control flow of osdw_fs_kernel (ldpc_osdw_fs.h) -- 64 TEPs per round, a
// ballot for the first tau_e hit, an arg-min over the lanes before it, only those lanes counted in num_teps, both quirk modes
// -- on the data of osdl_search_kernel (ldpc_osdl.h): SearchLLds<WP> with 192 rows of P' of WP = ceil((n - k) / 64) words each,
// 192 MRB weights and 8 WP byte LUTs; the lower bound of weight w summed over w[k-w .. k-1], HD = w + popcount over the WP words
// of D, the visit-order table of this k <= 192 (classes 1..min(3, k)).
// As in osdw_fs_kernel no flip mask is carried through the scan (it would be three words per lane): the winner and the
// stopping candidate are remembered as table positions and their flipped positions read from their entries after the scan.
// The metric is tepl_cost_bounded (ldpc_osdl.h): the float order of osdl_search_kernel and of np_oracle._weighted_distance_k.
// Every slot and word loop is unrolled and nothing in registers is indexed at run time (no scratch; profiles/osdl_fs/README.md).
#pragma once

#include "ldpc_osdl.h"

namespace ldpc {

template <int WP>
struct __attribute__((aligned(16))) SearchLLdsLean {   // SearchLLds without the byte LUTs (at WP = 3: 7.6 KiB instead of 31.6)
    u64 P[kOsdlK][WP];
    float w[kOsdlK + 64 * WP];
    u64 cw[kOsdlN / 64];
};

// ---------------------------------------------------------------------------------------
// per-frame prologue and epilogue of the FS scan and the one-TEP kernel (osdw_prepare / osdw_finish of ldpc_osdw_fs.h with three
// MRB slots per lane and WP parity words).  They are the prologue and epilogue of osdl_search_kernel (ldpc_osdl.h) word for
// word, as a COPY, for the reason ldpc_osdw_fs.h records: that kernel's register counts are the ones its measurements were
// taken with (profiles/osdl/README.md), so it keeps its own text.  Idle lanes stay out of the hard-decision ballots -- their
// y = 0 would count as a hard 1 --, rows of P' are masked to n - k columns, and w[] and P[] are zero beyond the live positions.
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

// the whole metric: tepl_cost_bounded under a bound nothing exceeds
template <int WP>
__device__ __forceinline__ float tepl_cost(const SearchLLds<WP> &L, float mrb, const u64 (&D)[WP])
{
    float c = 0.0f;
    (void)tepl_cost_bounded<WP>(L, mrb, D, __builtin_inff(), c);
    return c;
}

template <int WP>
__device__ __forceinline__ int popc_words(const u64 (&D)[WP])
{
    int h = 0;
#pragma unroll
    for (int q = 0; q < WP; ++q) h += __popcll(D[q]);
    return h;
}

//   counts[3] += {frames, frames_wrong, teps_total} (with label; teps_total sums the frame's own ntep, only with ntep_out): one
//   atomic per counter and wavefront, after its last frame.
template <int WP>
__global__ __launch_bounds__(64) void osdl_fs_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const unsigned short *__restrict__ perm_in, const u64 *__restrict__ parity_in,
        const uchar4 *__restrict__ teps_fs, FsParams P, u64 *__restrict__ cw_out, float *__restrict__ metric_out,
        int *__restrict__ best_out, int *__restrict__ ntep_out, const u64 *__restrict__ label, u64 *__restrict__ counts)
{
    __shared__ SearchLLds<WP> L;   // one wavefront per workgroup: compile-time LDS base for the LUT reads
    const int lane = threadIdx.x;
    const int words = (n + 63) >> 6;
    const long long nframes = frame_count(count, F);
    unsigned long long seen = 0, wrong = 0, nteps = 0;

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        const OsdlFrame<WP> S = osdl_prepare<WP, true>(L, y, src, perm_in, parity_in, f, n, k, lane);
        float best = tepl_cost<WP>(L, 0.0f, S.d0);      // all-zero TEP (:131)
        u64 bestD[WP], hitD[WP];
#pragma unroll
        for (int q = 0; q < WP; ++q) { bestD[q] = S.d0[q]; hitD[q] = 0ull; }
        float hitc = 0.0f;
        int bestidx = 0, ntep = 1, visited = 1, hitidx = 0;
        int bestpos = -1, hitpos = -1;                  // position inside teps_fs; -1: the all-zero TEP
        bool hit = false;
        if (!((float)popc_words<WP>(S.d0) < P.tau_e)) {
            for (int w = 1; w <= P.order && !hit; ++w) {   // (the host keeps order <= min(3, k))
                float bsum = 0.0f;                      // w least reliable MRB values, ascending position (in whichever words)
                for (int t = k - w; t < k; ++t) bsum = bsum + L.w[t];
                if (!(bsum + P.beta_term < best)) break;
                const int cnt = P.cls_cnt[w], off = P.cls_off[w];
                const uchar4 *tab = teps_fs + off;
                for (int t0 = 0; t0 < cnt && !hit; t0 += 64) {
                    const int t = t0 + lane;
                    const bool valid = t < cnt;
                    u64 D[WP];
#pragma unroll
                    for (int q = 0; q < WP; ++q) D[q] = 0ull;
                    float mrb = 0.0f;
                    if (valid) tepl_apply<WP>(L, tab[t], S.d0, D, mrb);
                    const float hd = (float)(w + popc_words<WP>(D));
                    const u64 stop = __ballot(valid && hd < P.tau_e);
                    const int lim = stop ? __builtin_ctzll(stop) : 64;
                    const int nvalid = (cnt - t0) < 64 ? (cnt - t0) : 64;
                    ntep += stop ? lim + 1 : nvalid;
                    // best among the TEPs visited before the stop that pass the tau_psc rule: the metric is only
                    // needed for those, and only if it can beat `best` (exact prefix early exit, tepl_cost_bounded)
                    float cc = __builtin_inff();
                    if (valid && lane < lim && hd < P.tau_psc) {
                        float c;
                        if (tepl_cost_bounded<WP>(L, mrb, D, best, c)) cc = c;
                    }
                    if (__ballot(cc < best)) {
                        const int wl = wave_argmin_lane(cc, lane);
                        best = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cc), wl));
#pragma unroll
                        for (int q = 0; q < WP; ++q) bestD[q] = readlane64(D[q], wl);
                        bestidx = visited + t0 + wl; bestpos = off + t0 + wl;
                    }
                    if (stop) {
                        hit = true;
#pragma unroll
                        for (int q = 0; q < WP; ++q) hitD[q] = readlane64(D[q], lim);
                        hitc = tepl_cost<WP>(L, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mrb), lim)), hitD);   // the stopping candidate's own metric
                        hitidx = visited + t0 + lim; hitpos = off + t0 + lim;
                    }
                }
                visited += cnt;
            }
        }
        const bool use_hit = hit && !P.quirk;
        const int pos = use_hit ? hitpos : bestpos;
        uchar4 win;   // rank 0 -- the all-zero TEP, also of a frame where nothing was found -- flips nothing
        win.x = win.y = win.z = win.w = 0;
        if (pos >= 0) win = teps_fs[pos];
        bool flip[3];
        u64 winD[WP];
#pragma unroll
        for (int s = 0; s < 3; ++s) flip[s] = tepl_flips(win, 64 * s + lane);
#pragma unroll
        for (int q = 0; q < WP; ++q) winD[q] = use_hit ? hitD[q] : bestD[q];
        osdl_finish<WP>(L, S, flip, winD, f, n, k, lane, cw_out);
        store_results(f, lane, use_hit ? hitc : best, use_hit ? hitidx : bestidx, ntep, metric_out, best_out, ntep_out);
        if (label) { seen += 1; wrong += cw_wrong(L, label, src, words); nteps += ntep_out ? (unsigned long long)ntep : 0ull; }
        wave_fence();
    }
    if (label && lane == 0 && seen) {
        atomicAdd(&counts[0], seen);
        atomicAdd(&counts[1], wrong);
        if (nteps) atomicAdd(&counts[2], nteps);
    }
}

// One given TEP per frame (one_tep_compare, FS_OSD/fs_testing.py:51-64) on the front-end results of this family:
// osdw_tep_eval_kernel with W = ceil(k / 64) mask words and WP words of discrepancy.  mask [F][W]: bit p of word w flips MRB
// position 64 w + p; bits at or beyond k are ignored.  A frame evaluates one candidate, so there are no byte LUTs
// (SearchLLdsLean) and the metric is tep_cost_direct over the parity weights word by word, the same additions in the same order.
template <int WP>
__global__ __launch_bounds__(64) void osdl_tep_eval_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const unsigned short *__restrict__ perm_in, const u64 *__restrict__ parity_in,
        const u64 *__restrict__ mask, u64 *__restrict__ cw_out, float *__restrict__ metric_out, int *__restrict__ hd_out)
{
    __shared__ SearchLLdsLean<WP> L;
    const int lane = threadIdx.x;
    const int Wk = (k + 63) >> 6;
    u64 rows[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) rows[s] = k >= 64 * (s + 1) ? ~0ull : (k > 64 * s ? ((1ull << (k - 64 * s)) - 1ull) : 0ull);
    const long long nframes = frame_count(count, F);

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        const OsdlFrame<WP> S = osdl_prepare<WP, false>(L, y, src, perm_in, parity_in, f, n, k, lane);
        u64 E[3], D[WP];
        bool flip[3];
#pragma unroll
        for (int q = 0; q < WP; ++q) D[q] = 0ull;
#pragma unroll
        for (int s = 0; s < 3; ++s) {                       // (a mask row has Wk words: a word beyond them is not read)
            E[s] = s < Wk ? (mask[f * Wk + s] & rows[s]) : 0ull;
            flip[s] = ((E[s] >> lane) & 1) != 0;
#pragma unroll
            for (int q = 0; q < WP; ++q) D[q] ^= flip[s] ? L.P[64 * s + lane][q] : 0ull;
        }
#pragma unroll
        for (int q = 0; q < WP; ++q) D[q] = S.d0[q] ^ wave_xor64(D[q]);
        float cost = 0.0f;                                  // flipped MRB weights, ascending position, sequential
#pragma unroll
        for (int s = 0; s < 3; ++s)
            for (u64 e = E[s]; e; e &= e - 1) cost = cost + L.w[64 * s + __builtin_ctzll(e)];
#pragma unroll
        for (int q = 0; q < WP; ++q) cost = tep_cost_direct(&L.w[kOsdlK + 64 * q - 64], cost, D[q]);   // (it reads w[64 ..]: the parity weights of word q)
        osdl_finish<WP>(L, S, flip, D, f, n, k, lane, cw_out);
        if (lane == 0) {
            if (metric_out) metric_out[f] = cost;
            if (hd_out) hd_out[f] = __popcll(E[0]) + __popcll(E[1]) + __popcll(E[2]) + popc_words<WP>(D);
        }
        wave_fence();
    }
}

}  // namespace ldpc
