// OSD kernels: osd_fs_kernel.
// FS-OSD (fs_osd, FS_OSD/fs_testing.py:129-161): order-by-order scan in the order of
// generate_sequential_teps (:32-49) with two Hamming-distance rules (one_tep_compare :51-64):
//   HD < tau_e            -> stop everything (the candidate is appended to optimal_list, :143-146)
//   HD < tau_psc and a smaller weighted distance -> new best (:147-152)
// and a lower bound per order: scan weight w only if (sum of the w least reliable MRB |y'|) +
// beta (n-k) < best so far (:137-139, acquire_pnc_boundary :22-30).  64 TEPs are evaluated per
// round; the sequential semantics are recovered with a ballot (first tau_e hit) and an arg-min
// over the lanes before it.  quirk = 1 returns what the reference keeps in `optimal_codeword`
// (the best BEFORE a tau_e hit), quirk = 0 the tau_e candidate itself.
#pragma once

#include "ldpc_search.h"

namespace ldpc {

// (one wavefront per workgroup, as the order-2 scan: compile-time LDS base for the LUT reads, and the
//  dispatcher balances the very uneven per-frame TEP counts)
__global__ __launch_bounds__(64) void osd_fs_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, const unsigned char *__restrict__ perm_in, const u64 *__restrict__ parity_in, const uchar4 *__restrict__ teps_fs, FsParams P,
        u64 *__restrict__ cw_out, float *__restrict__ metric_out, int *__restrict__ best_out, int *__restrict__ ntep_out)
{
    __shared__ SearchLds L;
    const int lane = threadIdx.x;
    long long nframes = F;      // (frame_count() and store_results() written out: through the helpers this kernel is scheduled differently)
    if (count) { const long long c = *count; nframes = c < F ? c : F; }

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        const SearchFrame S = search_prepare(L, y, src, perm_in, parity_in, f, lane);
        float best = tep_cost(L, 0.0f, S.d0);      // all-zero TEP (:131)
        u64 bestD = S.d0, bestE = 0, hitD = 0, hitE = 0;
        float hitc = 0.0f;
        int bestidx = 0, ntep = 1, visited = 1, hitidx = 0;
        bool hit = false;
        if (!((float)__popcll(S.d0) < P.tau_e)) {
            for (int w = 1; w <= P.order && !hit; ++w) {
                float bsum = 0.0f;                  // w least reliable MRB values, ascending position
                for (int t = 64 - w; t < 64; ++t) bsum = bsum + L.w[t];
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
        search_finish(L, S, use_hit ? hitE : bestE, use_hit ? hitD : bestD, f, lane, cw_out);
        if (lane == 0) {
            if (metric_out) metric_out[f] = use_hit ? hitc : best;
            if (best_out) best_out[f] = use_hit ? hitidx : bestidx;
            if (ntep_out) ntep_out[f] = ntep;
        }
    }
}

}  // namespace ldpc
