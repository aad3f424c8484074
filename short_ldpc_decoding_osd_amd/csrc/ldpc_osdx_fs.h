// OSD for short codes of any shape: osdx_fs_kernel and osdx_tep_eval_kernel.
// FS-OSD (fs_osd, FS_OSD/fs_testing.py:129-161) as osd_fs_kernel (ldpc_osd_fs.h) evaluates it -- 64 TEPs per round, a ballot
// for the first tau_e hit, an arg-min over the lanes before it, only those lanes counted in num_teps, both quirk modes -- with
// the code's n and k as kernel arguments.  What changes with the shape:
//   the lower bound of weight w sums w[k-w .. k-1] (acquire_pnc_boundary :22-30), beta_term = beta (n - k) comes from the host,
//   HD = w + popcount(D) with D confined to n - k bits, and the visit-order table is the one of this k (classes 1..min(3, k)).
// The per-frame prologue and epilogue are osdx_prepare / osdx_finish (ldpc_osdx.h); the metric is tep_apply / tep_cost /
// tep_cost_bounded unchanged (the float order of np_oracle._weighted_distance_k).
#pragma once

#include "ldpc_osdx.h"

namespace ldpc {

//   counts[3] += {frames, frames_wrong, teps_total} (with label; teps_total sums the frame's own ntep, only with ntep_out): one
//   atomic per counter and wavefront, after its last frame.
__global__ __launch_bounds__(64) void osdx_fs_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const unsigned char *__restrict__ perm_in, const u64 *__restrict__ parity_in,
        const uchar4 *__restrict__ teps_fs, FsParams P, u64 *__restrict__ cw_out, float *__restrict__ metric_out,
        int *__restrict__ best_out, int *__restrict__ ntep_out, const u64 *__restrict__ label, u64 *__restrict__ counts)
{
    __shared__ SearchLds L;   // one wavefront per workgroup: compile-time LDS base for the LUT reads
    const int lane = threadIdx.x;
    const int words = (n + 63) >> 6;
    const long long nframes = frame_count(count, F);
    unsigned long long seen = 0, wrong = 0, nteps = 0;

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        const OsdxFrame S = osdx_prepare(L, y, src, perm_in, parity_in, f, n, k, lane);
        float best = tep_cost(L, 0.0f, S.d0);      // all-zero TEP (:131)
        u64 bestD = S.d0, bestE = 0, hitD = 0, hitE = 0;
        float hitc = 0.0f;
        int bestidx = 0, ntep = 1, visited = 1, hitidx = 0;
        bool hit = false;
        if (!((float)__popcll(S.d0) < P.tau_e)) {
            for (int w = 1; w <= P.order && !hit; ++w) {   // (the host keeps order <= min(3, k))
                float bsum = 0.0f;                  // w least reliable MRB values, ascending position
                for (int t = k - w; t < k; ++t) bsum = bsum + L.w[t];
                if (!(bsum + P.beta_term < best)) break;
                const int cnt = P.cls_cnt[w];
                const uchar4 *tab = teps_fs + P.cls_off[w];
                for (int t0 = 0; t0 < cnt && !hit; t0 += 64) {
                    const int t = t0 + lane;
                    const bool valid = t < cnt;
                    u64 D = 0, E = 0;
                    float mrb = 0.0f;
                    if (valid) tep_apply(L, tab[t], S.d0, D, E, mrb);
                    const float hd = (float)(w + __popcll(D));
                    const u64 stop = __ballot(valid && hd < P.tau_e);
                    const int lim = stop ? __builtin_ctzll(stop) : 64;
                    const int nvalid = (cnt - t0) < 64 ? (cnt - t0) : 64;
                    ntep += stop ? lim + 1 : nvalid;
                    // best among the TEPs visited before the stop that pass the tau_psc rule: the metric is only
                    // needed for those, and only if it can beat `best` (exact prefix early exit, tep_cost_bounded)
                    float cc = __builtin_inff();
                    if (valid && lane < lim && hd < P.tau_psc) {
                        float c;
                        if (tep_cost_bounded(L, mrb, D, best, c)) cc = c;
                    }
                    if (__ballot(cc < best)) {
                        int ci = lane;
                        u64 cD = D, cE = E;
                        wave_argmin(cc, ci, cD, cE, lane);
                        best = cc; bestD = cD; bestE = cE; bestidx = visited + t0 + ci;
                    }
                    if (stop) {
                        hit = true;
                        hitD = readlane64(D, lim); hitE = readlane64(E, lim);
                        hitc = tep_cost(L, __shfl(mrb, lim, 64), hitD);   // the stopping candidate's own metric
                        hitidx = visited + t0 + lim;
                    }
                }
                visited += cnt;
            }
        }
        const bool use_hit = hit && !P.quirk;
        osdx_finish(L, S, use_hit ? hitE : bestE, use_hit ? hitD : bestD, f, words, lane, cw_out);
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

// One given TEP per frame (one_tep_compare, FS_OSD/fs_testing.py:51-64) on front-end results of any shape: ldpc_osd_tep_eval
// with the split at k.  A frame evaluates one candidate, so there are no byte LUTs (SearchLdsLean) and the metric is
// tep_cost_direct, the same additions in the same order; bits of `mask` at or beyond k are ignored.
__global__ __launch_bounds__(64) void osdx_tep_eval_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const unsigned char *__restrict__ perm_in, const u64 *__restrict__ parity_in,
        const u64 *__restrict__ mask, u64 *__restrict__ cw_out, float *__restrict__ metric_out, int *__restrict__ hd_out)
{
    __shared__ SearchLdsLean L;
    const int lane = threadIdx.x;
    const int words = (n + 63) >> 6;
    const u64 rows = k >= 64 ? ~0ull : ((1ull << k) - 1ull);
    const long long nframes = frame_count(count, F);

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        const OsdxFrame S = osdx_prepare<false>(L, y, src, perm_in, parity_in, f, n, k, lane);
        const u64 E = mask[f] & rows;
        const u64 D = S.d0 ^ wave_xor64(((E >> lane) & 1) ? L.P[lane] : 0ull);
        float mrb = 0.0f;                                  // flipped MRB weights, ascending position, sequential
        for (u64 e = E; e; e &= e - 1) mrb = mrb + L.w[__builtin_ctzll(e)];
        const float cost = tep_cost_direct(L.w, mrb, D);
        osdx_finish(L, S, E, D, f, words, lane, cw_out);
        if (lane == 0) {
            if (metric_out) metric_out[f] = cost;
            if (hd_out) hd_out[f] = __popcll(E) + __popcll(D);
        }
        wave_fence();
    }
}

}  // namespace ldpc
