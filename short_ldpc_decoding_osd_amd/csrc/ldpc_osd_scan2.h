// OSD kernels: osd_search2_kernel (the round-1 form of the order-2 scan: fallback and cross-check route of the rotation scan,
// ldpc_osd_scan2r.h) and the pieces both order-2 scans share.
// Order-2 conventional search, register-resident: same result as osd_search_kernel with the
// 2081-entry table, without per-TEP reads of P' / |y'| / the table.  Lane l keeps P'[l], P'[63-l],
// |y'_l|, |y'_{63-l}|; order 1 = one TEP per lane; order 2 = 32 rounds over a triangular pairing
//   lanes l > r : pair (r, l)          lanes l <= r : pair (62 - r, 63 - l)      (r = 0..31)
// (63 - r) + (r + 1) = 64 pairs per round, 2016 in all; the pivot rows of a round arrive by
// v_readlane.  "First minimum in table order" is kept by ranking the TEPs with the closed form of
// the reference's ordering (weight class, then descending index sum, then ascending first index;
// convention_osd.py:19-24): rank({}) = 0, rank({p}) = 64 - p, rank({i<j}) = 65 + base[i+j] +
// i - max(0, i+j-63), base[s] = number of pairs with a larger sum (uploaded table).
#pragma once

#include "ldpc_search.h"

namespace ldpc {

__device__ __forceinline__ int tep2_rank(int bi, int bj, const int *__restrict__ base2)
{
    if (bj < 0) return 0;
    if (bi < 0) return 64 - bj;
    const int s = bi + bj;
    return 65 + base2[s] + bi - (s > 63 ? s - 63 : 0);
}

// ---- shared by both order-2 scans (this one and the rotation-paired one, ldpc_osd_scan2r.h)
// order 0 (rank 0, identical in every lane), then order 1: lane l owns TEP {l}; cost(mrb, D) = the scan's full metric
template <class Cost>
__device__ __forceinline__ void search2_start(Cost cost, u64 d0, u64 Pl, float wl, int lane, float &best, int &bi, int &bj, u64 &bestD)
{
    best = cost(0.0f, d0);
    bi = -1; bj = -1; bestD = d0;
    const u64 D = d0 ^ Pl;
    const float c = cost(wl, D);
    if (c < best) { best = c; bj = lane; bestD = D; }      // a tie keeps the lower rank (order 0)
}

// a finished pair (ci < cj, acc <= best) against the lane's best: equal metrics are ordered by table rank (practically never taken)
__device__ __forceinline__ void search2_take(float acc, int ci, int cj, u64 D, const int *__restrict__ base2, float &best, int &bi, int &bj, u64 &bestD)
{
    if (acc < best || tep2_rank(ci, cj, base2) < tep2_rank(bi, bj, base2)) { best = acc; bi = ci; bj = cj; bestD = D; }
}

// The order-0/1/2 scan of one frame per wavefront (one wavefront per workgroup: the LDS base is then a
// compile-time constant and every LUT read is "SDWA shift + ds_read with an immediate offset").
//
// Order 2 runs in two stages.  Stage 1 (every round, all lanes): candidate D, MRB weight and the first two
// parity bytes; a candidate whose prefix already exceeds `bound` (the smallest complete metric seen by any
// lane) can neither win nor tie -- every further term is >= 0 -- and is dropped: ~70-95 % of the TEPs.
// The survivors are appended to a 128-entry LDS ring (ballot + mbcnt compaction) and stage 2 finishes them
// 64 at a time, so the six remaining LUT reads and the arg-min bookkeeping run on full wavefronts only.
// The order of evaluation changes, the result does not: the arg-min is on (metric, table rank).
// (Measured alternatives: four wavefronts per frame sharing one LUT set -- 139 us against 123 us, the
//  barriers and the single-wave prologue cost more than the occupancy gains; pivot rows through the scalar
//  cache instead of v_readlane -- no difference.)
struct __attribute__((aligned(16))) Search2Lds {
    SearchLds s;
    uint4 q[128];   // survivors: D.lo, D.hi, prefix metric bits, r * 64 + lane
};

__device__ __forceinline__ void search2_finish_batch(const SearchLds &L, uint4 e, bool valid, const int *__restrict__ base2,
                                                     float &best, int &bi, int &bj, u64 &bestD)
{
    if (!valid) return;
    const u64 D = ((u64)e.y << 32) | e.x;
    float acc = __uint_as_float(e.z);
    acc = acc + lut_term<2>(L, D); acc = acc + lut_term<3>(L, D); acc = acc + lut_term<4>(L, D);
    acc = acc + lut_term<5>(L, D); acc = acc + lut_term<6>(L, D); acc = acc + lut_term<7>(L, D);
    if (!(acc <= best)) return;
    const int r = (int)(e.w >> 6), l = (int)(e.w & 63);
    const bool up = l > r;
    search2_take(acc, up ? r : 62 - r, up ? l : 63 - l, D, base2, best, bi, bj, bestD);
}

__device__ __forceinline__ void search2_device(Search2Lds &LL, const SearchFrame &S, const int *__restrict__ base2, int lane,
                                               float &best_out, int &rank_out, u64 &D_out, u64 &E_out)
{
    SearchLds &L = LL.s;
    const u64 Pl = L.P[lane], Pm = L.P[63 - lane];
    const float wl = L.w[lane], wm = L.w[63 - lane];
    float best;
    int bi, bj;
    u64 bestD;
    search2_start([&](float mrb, u64 D) { return tep_cost(L, mrb, D); }, S.d0, Pl, wl, lane, best, bi, bj, bestD);
    float bound = wave_min_f32(best);
    int qhead = 0, qn = 0;   // ring state (wave-uniform)
    for (int r = 0; r < 32; ++r) {
        const u64 Pr = readlane64(Pl, r), Pq = readlane64(Pl, 62 - r);
        const float wr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wl), r));
        const float wq = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wl), 62 - r));
        const bool up = lane > r;
        const bool active = up || r < 31;        // at r = 31 the lower half would repeat i = 31
        const float M = up ? (wr + wl) : (wq + wm);            // |y'_i| + |y'_j|, i < j
        const u64 D = S.d0 ^ (up ? (Pr ^ Pl) : (Pq ^ Pm));
        float acc = M + lut_term<0>(L, D);
        acc = acc + lut_term<1>(L, D);
        const bool keep = active && !(acc > bound);
        const u64 km = __ballot(keep);
        if (km) {
            if (keep) {
                const int slot = (qhead + qn + wave_lane_rank(km)) & 127;
                LL.q[slot] = make_uint4((unsigned)D, (unsigned)(D >> 32), __float_as_uint(acc), (unsigned)(r * 64 + lane));
            }
            qn += __popcll(km);
            if (qn >= 64) {
                wave_fence();
                search2_finish_batch(L, LL.q[(qhead + lane) & 127], true, base2, best, bi, bj, bestD);
                qhead = (qhead + 64) & 127;
                qn -= 64;
                bound = wave_min_f32(best);
                wave_fence();
            }
        }
    }
    wave_fence();
    search2_finish_batch(L, LL.q[(qhead + lane) & 127], lane < qn, base2, best, bi, bj, bestD);
    wave_fence();
    int bestt = tep2_rank(bi, bj, base2);
    u64 bestE = (bi >= 0 ? 1ull << bi : 0ull) | (bj >= 0 ? 1ull << bj : 0ull);
    wave_argmin(best, bestt, bestD, bestE, lane);
    best_out = best; rank_out = bestt; D_out = bestD; E_out = bestE;
}

__global__ __launch_bounds__(64) void osd_search2_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, const unsigned char *__restrict__ perm_in, const u64 *__restrict__ parity_in, const int *__restrict__ base2,
        u64 *__restrict__ cw_out, float *__restrict__ metric_out, int *__restrict__ best_out, int *__restrict__ ntep_out)
{
    __shared__ Search2Lds LL;
    SearchLds &L = LL.s;
    const int lane = threadIdx.x;
    const long long nframes = frame_count(count, F);

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        const SearchFrame S = search_prepare(L, y, src, perm_in, parity_in, f, lane);
        float best; int bestt; u64 bestD, bestE;
        search2_device(LL, S, base2, lane, best, bestt, bestD, bestE);
        search_finish(L, S, bestE, bestD, f, lane, cw_out);
        store_results(f, lane, best, bestt, 2081, metric_out, best_out, ntep_out);
    }
}

}  // namespace ldpc
