// OSD for short codes of any shape: osdx_pb_kernel.
// PB-OSD (pb_osd, PB_OSD/pb_testing.py:100-149) as pb_seq_kernel (ldpc_pb_seq.h) replays it -- pop the first minimum of the
// frontier by (sum, insertion order), append at most two children, the promising rule, the cost, the success rule -- with the
// code's n and k as kernel arguments, one frame per wavefront, the float conventions of oracle/ldpc_oracle.c orc_pb_osd with 64
// replaced by k (MRB) and m = n - k (parity part).  The per-frame prologue and epilogue are osdx_prepare / osdx_finish.
//
// The frontier needs no list that grows and no workspace.  Every TEP has one parent (ldpc_pb_common.h, fact 1), and an adjacent
// child replaces its parent, so the live entries form RUNS: the weight-1 run, one weight-2 run per smaller index a, one weight-3
// run per pair (a, b) with b < k - 1 -- 1 + (k - 1) + C(k - 1, 2) <= 2017 runs, one live entry each at most.  A run owns a fixed
// slot of LDS; the slot number is the run's prefix, the slot holds the sum, the insertion sequence number and the cursor (the
// largest index):
//   slot 0                        {c}
//   slot 1 + a                    {a, c}        a = 0 .. k-2
//   slot k + b (b - 1) / 2 + a    {a, b, c}     a < b <= k-2
// A pop rewrites its own slot with the adjacent child (or empties it) and fills one other slot with the extended child.
// Orders <= 2 use k <= 64 slots, one per lane: a pop is one wave arg-min.  Order 3 keeps the minimum of every chunk of 64 slots
// in the registers of lane `chunk` (<= 32 chunks): a pop is an arg-min over those, a re-reduction of the popped slot's chunk and
// a compare for the extended child's chunk.
#pragma once

#include "ldpc_osdx.h"
#include "ldpc_pb_expf.h"

namespace ldpc {

struct PbxParams {
    int order, nmax;         // nmax = sum_{w <= order} C(k, w)
    float c4;                // (float)(-4 / 10^(snr_db / 10))
};

// the context's PB table (OsdTables::d_pb, float64): cdfH[65] = P[Bin(m, 1/2) <= b] (zero beyond m), then the ratios of consecutive
// binomial coefficients (m - i) / (i + 1) and (k - i) / (i + 1), 64 entries each (zero beyond m - 1 / k - 1)
constexpr int kPbxCdfH = 0, kPbxCoefM = 65, kPbxCoefK = 129, kPbxTabSize = 193;

constexpr int kPbxEmpty = 0x7FFFFFFF;   // meta of an empty slot (its sum is +inf); a live one holds seq << 8 | cursor, seq <= 43744

template <int SLOTS>
struct __attribute__((aligned(16))) PbxLds {
    double cdfA[65];         // P[Bin(m, p1) <= b]
    double cdfH[65];         // P[Bin(m, 1/2) <= b]
    float q[128];            // q[l] = sigmoid(c4 |y'_l|) (MRB), q[64 + l] = the same of parity position k + l
    float fsum[SLOTS];       // the runs' live entries: reliability sum (+inf: none)
    int fmeta[SLOTS];        //                         seq << 8 | cursor
};

__device__ __forceinline__ double readlane_f64(double v, int lane)
{
    return __longlong_as_double((long long)readlane64((u64)__double_as_longlong(v), lane));
}

// per-frame PB quantities (wave-uniform): pb_frame_setup of ldpc_pb_common.h with the split at k.  w = |y'| in the layout of
// osdx_prepare; coef_m / coef_k: lane i holds (m - i) / (i + 1) and (k - i) / (i + 1).
struct PbxFrame {
    float spl, lrb_mean;
    double p_t_suc, p_t_pro;
};
__device__ __forceinline__ PbxFrame pbx_frame_setup(const float *w, float *q, double *cdfA, const PbxParams &P, int k, int m, double coef_m,
                                                    double coef_k, float best0, int lane)
{
    q[lane] = 1.0f / (1.0f + det_expf(-(P.c4 * w[lane])));
    q[lane + 64] = 1.0f / (1.0f + det_expf(-(P.c4 * w[lane + 64])));
    wave_fence();
    // four sequential chains, ascending position, one per lane 0..3 with one fused multiply-add per step (acc * 1 + x is the sum,
    // acc * x + 0 the product, both rounded once like the plain operations); a chain ends at its own length
    const int ch = lane & 3;
    const float *src = ch == 0 ? q + 64 : (ch == 1 ? w + 64 : q);
    const int len = ch < 2 ? m : k;
    const bool prod = ch == 3;
    float acc = prod ? 1.0f : 0.0f;
#pragma unroll 8
    for (int p = 0; p < 64; ++p) {
        const float x = src[p];
        const float nx = __builtin_fmaf(acc, prod ? 1.0f - x : 1.0f, prod ? 0.0f : x);
        acc = p < len ? nx : acc;
    }
    const float a1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 0));
    const float aw = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 1));
    const float at = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 2));
    const float spl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 3));
    const float p1 = a1 / (float)m, lrb_mean = aw / (float)m, pt = at / (float)k;
    // entries of cdfA above floor(best0 / lrb_mean) are never read (beta <= floor((best - sum) / lrb_mean), best <= best0, sum >= 0)
    const float bq = __builtin_floorf(best0 / lrb_mean);
    const int ncdf = bq > 0.0f ? (bq < (float)m ? (int)bq : m) : 0;
    // q^N by square-and-multiply over the bits of N below its top bit, then the pmf recurrence (float64)
    const auto qpow = [](double qq, int N) {
        double t = qq;
        for (int b = 30 - __builtin_clz(N); b >= 0; --b) {
            t = t * t;
            if ((N >> b) & 1) t = t * qq;
        }
        return t;
    };
    double niu;
    {
        double qq = 1.0 - (double)p1, t = qpow(qq, m);
        const double ratio = (double)p1 / qq;
        double a = t;
        if (lane == 0) cdfA[0] = a;
        for (int i = 0; i < ncdf; ++i) {
            t = t * readlane_f64(coef_m, i) * ratio;
            a = a + t;
            if (lane == 0) cdfA[i + 1] = a;
        }
        qq = 1.0 - (double)pt; t = qpow(qq, k);
        const double ratio2 = (double)pt / qq;
        a = t;
        for (int i = 0; i < P.order; ++i) { t = t * readlane_f64(coef_k, i) * ratio2; a = a + t; }
        niu = a;
    }
    PbxFrame F;
    F.spl = spl; F.lrb_mean = lrb_mean;
    F.p_t_suc = 0.99 * niu;
    F.p_t_pro = 0.002 * __builtin_sqrt((1.0 - niu) / (double)P.nmax);
    wave_fence();
    return F;
}

// wave arg-min on (sum, meta): the lane of the first minimum, sum and meta of it in every lane
__device__ __forceinline__ int pbx_argmin(float &s, int &meta)
{
    const int wl = wave_argmin_lane(s, meta);
    s = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), wl));
    meta = __builtin_amdgcn_readlane(meta, wl);
    return wl;
}

//   aux_out [F][4] i32 (nullable): {frontier comparisons, suc1, suc2, stop reason}
//   counts[3] += {frames, frames_wrong, teps_total} (with label; teps_total sums the frame's own ntep, only with ntep_out): one
//   atomic per counter and wavefront, after its last frame.
template <bool O3>
__global__ __launch_bounds__(64) void osdx_pb_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const unsigned char *__restrict__ perm_in, const u64 *__restrict__ parity_in,
        const double *__restrict__ pbtab, PbxParams P, u64 *__restrict__ cw_out, float *__restrict__ metric_out,
        int *__restrict__ best_out, int *__restrict__ ntep_out, int *__restrict__ aux_out, const u64 *__restrict__ label,
        u64 *__restrict__ counts)
{
    constexpr int SLOTS = O3 ? 2048 : 64;
    __shared__ SearchLds L;   // one wavefront per workgroup: compile-time LDS base for the LUT reads
    __shared__ PbxLds<SLOTS> B;
    const int lane = threadIdx.x;
    const int m = n - k;
    const int words = (n + 63) >> 6;
    const int nchunks = O3 ? (k + (k - 1) * (k - 2) / 2 + 63) >> 6 : 1;
    const long long nframes = frame_count(count, F);
    unsigned long long seen = 0, wrong = 0, nteps = 0;
    const double coef_m = pbtab[kPbxCoefM + lane], coef_k = pbtab[kPbxCoefK + lane];
    B.cdfH[lane] = pbtab[kPbxCdfH + lane];
    if (lane == 0) B.cdfH[64] = pbtab[kPbxCdfH + 64];
    wave_fence();

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        const OsdxFrame S = osdx_prepare(L, y, src, perm_in, parity_in, f, n, k, lane);
        float best = tep_cost(L, 0.0f, S.d0);      // all-zero TEP (:101-106)
        u64 bestD = S.d0, bestE = 0;
        int bestidx = 0, ntep = P.nmax, stop = 0, cmp = 0, suc1 = 0, suc2 = 0;
        if (P.nmax > 1) {
            const PbxFrame Fr = pbx_frame_setup(L.w, B.q, B.cdfA, P, k, m, coef_m, coef_k, best, lane);
            const float wk = L.w[k - 1];
            // the frontier: every run empty, then the starting point {k-1} (:109-110) in the weight-1 run
            for (int c = 0; c < nchunks; ++c) { B.fsum[c * 64 + lane] = __builtin_inff(); B.fmeta[c * 64 + lane] = kPbxEmpty; }
            wave_fence();
            if (lane == 0) { B.fsum[0] = wk; B.fmeta[0] = k - 1; }
            wave_fence();
            // order 3: lane c holds the minimum of chunk c as (sum, meta, slot)
            float csum = lane == 0 ? wk : __builtin_inff();
            int cmeta = lane == 0 ? k - 1 : kPbxEmpty, cslot = lane * 64;
            int seq = 1, nlive = 1;
            for (int j = 0; j < P.nmax - 1; ++j) {
                // ---- pop the first minimum by (sum, seq)
                float s;
                int meta, slot;
                if constexpr (O3) {
                    s = csum; meta = cmeta;
                    const int wl = pbx_argmin(s, meta);
                    slot = __builtin_amdgcn_readlane(cslot, wl);
                } else {
                    s = B.fsum[lane]; meta = B.fmeta[lane];
                    slot = pbx_argmin(s, meta);
                }
                cmp += nlive == 1 ? 1 : 2;
                const int last = meta & 0xFF;
                int wt, p0, p1 = 0, p2 = 0;
                if (slot == 0) { wt = 1; p0 = last; }
                else if (slot < k) { wt = 2; p0 = slot - 1; p1 = last; }
                else {
                    const int t = slot - k;                // = b (b - 1) / 2 + a with a < b: lane b finds itself
                    const int b = __builtin_ctzll(__ballot(lane >= 1 && lane * (lane - 1) / 2 <= t && t < lane * (lane + 1) / 2));
                    wt = 3; p0 = t - b * (b - 1) / 2; p1 = b; p2 = last;
                }
                const int prev = wt == 2 ? p0 : p1;        // second largest index (wt > 1)
                // ---- children: extended e U {k-1} into the run with e as its prefix, adjacent into the popped run
                const bool has1 = last < k - 1 && wt < P.order;
                const bool has2 = wt > 1 ? (last - prev > 1) : (last - 1 >= 0);
                const int eslot = wt == 1 ? 1 + p0 : k + last * (last - 1) / 2 + p0;
                float esum = __builtin_inff(), asum = __builtin_inff();
                int emeta = kPbxEmpty, ameta = kPbxEmpty;
                if (has1) { esum = s + wk; emeta = (seq++ << 8) | (k - 1); }
                if (has2) {
                    asum = wt == 1 ? L.w[last - 1] : (wt == 2 ? L.w[p0] + L.w[last - 1] : (L.w[p0] + L.w[p1]) + L.w[last - 1]);
                    ameta = (seq++ << 8) | (last - 1);
                }
                if (lane == 0) {
                    B.fsum[slot] = asum; B.fmeta[slot] = ameta;
                    if (has1) { B.fsum[eslot] = esum; B.fmeta[eslot] = emeta; }
                }
                nlive += (has1 ? 1 : 0) + (has2 ? 1 : 0) - 1;
                wave_fence();
                if constexpr (O3) {
                    const int c0 = slot >> 6, ce = eslot >> 6;
                    float ms = B.fsum[c0 * 64 + lane];
                    int mm = B.fmeta[c0 * 64 + lane];
                    const int wl = pbx_argmin(ms, mm);
                    if (lane == c0) { csum = ms; cmeta = mm; cslot = c0 * 64 + wl; }
                    if (has1 && ce != c0 && lane == ce && (esum < csum || (esum == csum && emeta < cmeta))) {
                        csum = esum; cmeta = emeta; cslot = eslot;
                    }
                }
                // ---- promising-probability rule (acquire_prob_promising :448-461)
                const float rs = s;
                const float w1 = det_expf(P.c4 * rs) * Fr.spl, w2 = 1.0f - w1;
                const float bt = __builtin_floorf((best - rs) / Fr.lrb_mean);
                const int beta = bt > 0.0f ? (bt < (float)m ? (int)bt : m) : 0;
                float bs = 0.0f;
                bs = bs + w1 * (float)B.cdfA[beta];
                bs = bs + w2 * (float)B.cdfH[beta];
                if ((double)bs < Fr.p_t_pro) { stop = 1; ntep = j + 1; break; }
                u64 D = S.d0 ^ L.P[p0], E = 1ull << p0;
                if (wt > 1) { D ^= L.P[p1]; E |= 1ull << p1; }
                if (wt > 2) { D ^= L.P[p2]; E |= 1ull << p2; }
                const float cost = tep_cost(L, rs, D);
                ++suc1;
                if (cost < best) {
                    best = cost; bestD = D; bestE = E; bestidx = j + 1;
                    // success rule (acquire_p_e_suc :423-436)
                    const float ratio = (1.0f - w1) / w1;
                    float prod = 1.0f;
#pragma unroll 4
                    for (int p = 0; p < m; ++p) {
                        const float qp = B.q[64 + p];
                        prod = prod * (((D >> p) & 1) ? 2.0f * qp : 2.0f * (1.0f - qp));
                    }
                    const float p_suc = 1.0f / (1.0f + ratio / prod);
                    ++suc2;
                    if (p_suc > (float)Fr.p_t_suc) { stop = 2; ntep = j + 1; break; }
                }
            }
        }
        osdx_finish(L, S, bestE, bestD, f, words, lane, cw_out);
        store_results(f, lane, best, bestidx, ntep, metric_out, best_out, ntep_out);
        if (aux_out && lane == 0) { aux_out[f * 4] = cmp; aux_out[f * 4 + 1] = suc1; aux_out[f * 4 + 2] = suc2; aux_out[f * 4 + 3] = stop; }
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
