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

// ---------------------------------------------------------------------------------------
// The per-frame prologue and epilogue are osdl_prepare / osdl_finish (ldpc_osdl.h), shared with osdl_search_kernel and the PB
// kernel.  The FS scan itself stays a text per family: written as one body over traits for the three families, with the same
// round loop, the launch of this kernel measured 1.8 % and 2.0 % above this text in two
// alternating sessions at WP = 2 (a (200,100) code, 159 TEPs per frame; 1.9 % at WP = 3 in one), about ten times the spread of
// this text's own runs, and the cause was not found (profiles/osd_scan_shared/README.md): the three FS kernels stay three texts.
// ---------------------------------------------------------------------------------------
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
        for (int s = 0; s < 3; ++s) flip[s] = tep_flips(win, 64 * s + lane);
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
