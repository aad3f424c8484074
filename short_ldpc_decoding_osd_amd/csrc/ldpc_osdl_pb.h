// OSD for longer and low-rate codes: osdl_pb_kernel.
// PB-OSD (pb_osd, PB_OSD/pb_testing.py:100-149) as osdw_pb_kernel (ldpc_osdw_pb.h) replays it -- pop the first minimum of the
// frontier by (sum, insertion order), append the extended and then the adjacent child, the promising rule, the cost, the success
// rule, the same bookkeeping of cmp, suc1, suc2, stop and ntep -- for k up to 192 and m = n - k up to 192: on SearchLLdsLean<WP>
// (192 rows of P' of WP = ceil(m / 64) words, 192 + 64 WP weights, no byte LUTs), with osdl_prepare / osdl_finish
// (ldpc_osdl.h) as prologue and epilogue, one frame per wavefront.  The float conventions are those of
// oracle/ldpc_oracle.c orc_pb_osd with 64 replaced by k (MRB) and m (parity part).
//
// The frontier is the one of osdw_pb_kernel: a run owns a fixed slot of LDS, the slot number is the run's prefix and the slot
// holds the sum, the insertion sequence number and the cursor (meta = seq << 8 | cursor; cursor <= 191 and
// seq < 2 N_max = 2 359 618 < 2^23 at k = 192):
//   slot 0                        {c}
//   slot 1 + a                    {a, c}        a = 0 .. k-2
//   slot k + b (b - 1) / 2 + a    {a, b, c}     a < b <= k-2
// What k <= 192 and m <= 192 change:
//   - the per-frame chains (p1, lrb_mean over the parity part, pt and spl over the MRB) run over up to 192 positions, q[] holds
//     192 + 192 entries, cdfA / cdfH up to 193; lane i holds the coefficients (m - i) / (i + 1) of i, 64 + i and 128 + i, and
//     the CDF recurrence walks them a register at a time; beta is clamped to m;
//   - orders <= 2 have up to 191 weight-2 runs: a lane reads the slots lane, 64 + lane and 128 + lane and a pop is one wave
//     arg-min over the smallest of the three;
//   - order 3 has up to k + (k - 1)(k - 2) / 2 = 18 337 runs, 287 chunks of 64 slots: lane c holds the minima of the chunks
//     c + 64 i (CPL <= 5 chunks per lane);
//   - the b of a weight-3 slot is found by three ballots (candidates lane, 64 + lane, 128 + lane);
//   - the metric has no LUTs.  The discrepancy D of the popped TEP is the same in every lane, so lane b < 8 WP sums the set
//     positions of byte b of D ascending from 0.0f (selects over eight weights it holds in registers for the frame) and the
//     wave adds the 8 WP byte sums to the reliability sum in byte order by lane reads: the additions of tepl_cost
//     (ldpc_osdl_fs.h) in the same order, without the 24 x 256 table entries a frame would have to build first -- most channel
//     frames stop within a few TEPs;
//   - the success product runs ascending over the m parity positions of the WP words: lane l holds the factors of positions
//     64 q + l, the product walks them by lane reads;
//   - only the chunks the previous frame of this wavefront wrote are emptied before a frame (a high-water mark), so a frame
//     that stops at its first TEP does not pay for 287 chunks.
// LDS, by the slot count SLOTS (a template parameter, chosen by the host from the order and k); beside the slots there are
// SearchLLdsLean<WP> (2.6 / 4.4 / 6.2 KB) and 4.6 KB of q and the two CDFs.  Tiers by occupancy (160 KiB per CU), at WP = 3:
//   orders <= 2      192 slots     12 352 B
//   order 3          2048 slots    27 200 B   k <= 64     (6 workgroups per CU)
//                    4096 slots    43 584 B   k <= 91     (3)
//                    8064 slots    75 328 B   k <= 127    (2)
//                    18 368 slots  157 760 B  k <= 192    (1)
// No tier lies between the last two: a workgroup of more than 80 KiB is alone on its CU whatever its size, and 80 KiB hold at
// most 8 700 slots beside the rest, so any tier above 8064 slots has the occupancy of the largest.  The slots a k does not
// need are never touched (the emptying and the chunk minima go by the chunk count of k, not by SLOTS).
// Every word, slot and chunk loop is unrolled and nothing in registers is indexed at run time: no scratch in any of the 15
// instantiations (profiles/osdl_pb/README.md).  No workspace and no per-stream state: the call is graph-capturable as it is.
#pragma once

#include "ldpc_osd_tables.h"
#include "ldpc_osdl.h"
#include "ldpc_pb_expf.h"
#include "ldpc_pbx.h"

namespace ldpc {

static_assert(kPblCoefM == kOsdlM + 1 && kPblCoefK == kPblCoefM + kOsdlM && kPblTabSize == kPblCoefK + 64, "the kPbl* layout (ldpc_osd_tables.h)");

template <int SLOTS>
struct __attribute__((aligned(16))) PblLds {
    double cdfA[kOsdlM + 1];      // P[Bin(m, p1) <= b]
    double cdfH[kOsdlM + 1];      // P[Bin(m, 1/2) <= b]
    float q[kOsdlK + kOsdlM];     // q[l] = sigmoid(c4 |y'_l|) (MRB, l < 192), q[192 + l] = the same of parity position k + l
    float fsum[SLOTS];            // the runs' live entries: reliability sum (+inf: none)
    int fmeta[SLOTS];             //                         seq << 8 | cursor
};

// the slots an order-3 frontier of k needs (orders <= 2 need k <= 192 of them)
constexpr int pbl_slots3(int k) { return k + (k - 1) * (k - 2) / 2; }

// per-frame PB quantities (wave-uniform): pbw_frame_setup of ldpc_osdw_pb.h on the layout of osdl_prepare (w[0..191] the MRB,
// w[192..] the parity part).  coef_m[s]: lane i holds (m - 64 s - i) / (64 s + i + 1); coef_k: lane i holds (k - i) / (i + 1).
struct PblFrame {
    float spl, lrb_mean;
    double p_t_suc, p_t_pro;
};
template <int WP>
__device__ __forceinline__ PblFrame pbl_frame_setup(const float *w, float *q, double *cdfA, const PbxParams &P, int k, int m,
                                                    const double (&coef_m)[3], double coef_k, float best0, int lane)
{
#pragma unroll
    for (int s = 0; s < 3; ++s) q[64 * s + lane] = 1.0f / (1.0f + det_expf(-(P.c4 * w[64 * s + lane])));
#pragma unroll
    for (int s = 0; s < WP; ++s) q[kOsdlK + 64 * s + lane] = 1.0f / (1.0f + det_expf(-(P.c4 * w[kOsdlK + 64 * s + lane])));
    wave_fence();
    // four sequential chains, ascending position, one per lane 0..3 with one fused multiply-add per step (acc * 1 + x is the sum,
    // acc * x + 0 the product, both rounded once like the plain operations); a chain ends at its own length (beyond it the
    // step reads position 0 and is discarded)
    const int ch = lane & 3;
    const float *src = ch == 0 ? q + kOsdlK : (ch == 1 ? w + kOsdlK : q);
    const int len = ch < 2 ? m : k;
    const int longest = m > k ? m : k;
    const bool prod = ch == 3;
    float acc = prod ? 1.0f : 0.0f;
#pragma unroll 8
    for (int p = 0; p < longest; ++p) {
        const float x = src[p < len ? p : 0];
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
#pragma unroll
        for (int s = 0; s < 3; ++s) {                       // the coefficients of 64 s .. 64 s + 63 are one register
            const int end = ncdf - 64 * s < 64 ? ncdf - 64 * s : 64;
            for (int i = 0; i < end; ++i) {
                t = t * readlane_f64(coef_m[s], i) * ratio;
                a = a + t;
                if (lane == 0) cdfA[64 * s + i + 1] = a;
            }
        }
        qq = 1.0 - (double)pt; t = qpow(qq, k);
        const double ratio2 = (double)pt / qq;
        a = t;
        for (int i = 0; i < P.order; ++i) { t = t * readlane_f64(coef_k, i) * ratio2; a = a + t; }
        niu = a;
    }
    PblFrame F;
    F.spl = spl; F.lrb_mean = lrb_mean;
    F.p_t_suc = 0.99 * niu;
    F.p_t_pro = 0.002 * __builtin_sqrt((1.0 - niu) / (double)P.nmax);
    wave_fence();
    return F;
}

// The metric of a candidate that is the same in every lane, without LUTs: lane b < 8 WP sums the set positions of byte b of D
// (pw[t] = |y'| of parity position 8 b + t, held for the frame) ascending from 0.0f by selects, the byte sums are added to
// mrb in byte order -- the additions of tepl_cost (and of tep_cost in the older families) in the same order.
template <int WP>
__device__ __forceinline__ float pbl_cost(const float (&pw)[8], float mrb, const u64 (&D)[WP], int lane)
{
    const int sh = 8 * (lane & 7);
    unsigned v = 0u;                                        // byte lane & 7 of word lane >> 3 (a select over the bytes, not the words)
#pragma unroll
    for (int q = 0; q < WP; ++q) v = (lane >> 3) == q ? (unsigned)(D[q] >> sh) & 255u : v;
    float bs = 0.0f;
#pragma unroll
    for (int t = 0; t < 8; ++t) bs = ((v >> t) & 1u) ? bs + pw[t] : bs;
    float acc = mrb;
#pragma unroll
    for (int b = 0; b < 8 * WP; ++b) acc = acc + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bs), b));
    return acc;
}

//   WP: words of parity discrepancy; O3: the frontier holds weight-3 runs (order 3); SLOTS >= 64 * ceil(slots of this order
//   and k / 64), 192 for orders <= 2
//   aux_out [F][4] i32 (nullable): {frontier comparisons, suc1, suc2, stop reason}
//   counts[3] += {frames, frames_wrong, teps_total} (with label; teps_total sums the frame's own ntep, only with ntep_out): one
//   atomic per counter and wavefront, after its last frame.
template <int WP, bool O3, int SLOTS>
__global__ __launch_bounds__(64) void osdl_pb_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const unsigned short *__restrict__ perm_in, const u64 *__restrict__ parity_in,
        const double *__restrict__ pbtab, PbxParams P, u64 *__restrict__ cw_out, float *__restrict__ metric_out,
        int *__restrict__ best_out, int *__restrict__ ntep_out, int *__restrict__ aux_out, const u64 *__restrict__ label,
        u64 *__restrict__ counts)
{
    static_assert(O3 ? SLOTS % 64 == 0 && SLOTS <= 320 * 64 : SLOTS == 192, "at most five chunks, or three slots, per lane");
    constexpr int CPL = O3 ? (SLOTS / 64 + 63) / 64 : 3;   // per lane: chunk minima held (order 3), slots read (orders <= 2)
    __shared__ SearchLLdsLean<WP> L;
    __shared__ PblLds<SLOTS> B;
    const int lane = threadIdx.x;
    const int m = n - k;
    const int words = (n + 63) >> 6;
    const int nchunks = O3 ? (pbl_slots3(k) + 63) >> 6 : 3;   // (the host keeps 64 * nchunks <= SLOTS)
    const long long nframes = frame_count(count, F);
    unsigned long long seen = 0, wrong = 0, nteps = 0;
    double coef_m[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) coef_m[s] = pbtab[kPblCoefM + 64 * s + lane];
    const double coef_k = pbtab[kPblCoefK + lane];
#pragma unroll
    for (int s = 0; s < 3; ++s) B.cdfH[64 * s + lane] = pbtab[kPblCdfH + 64 * s + lane];
    if (lane == 0) B.cdfH[kOsdlM] = pbtab[kPblCdfH + kOsdlM];
    int dirty = nchunks - 1;                                // the highest chunk that may hold anything but empty slots
    wave_fence();

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        const OsdlFrame<WP> S = osdl_prepare<WP, false>(L, y, src, perm_in, parity_in, f, n, k, lane);
        float pw[8];                                        // the parity weights of byte min(lane, 8 WP - 1)
        {
            const int b = lane < 8 * WP ? lane : 8 * WP - 1;
#pragma unroll
            for (int t = 0; t < 8; ++t) pw[t] = L.w[kOsdlK + 8 * b + t];
        }
        float best = pbl_cost<WP>(pw, 0.0f, S.d0, lane);    // all-zero TEP (:101-106)
        u64 bestD[WP];
#pragma unroll
        for (int q = 0; q < WP; ++q) bestD[q] = S.d0[q];
        int bw = 0, b0 = 0, b1 = 0, b2 = 0;                 // the winner's support: weight and positions (ascending)
        int bestidx = 0, ntep = P.nmax, stop = 0, cmp = 0, suc1 = 0, suc2 = 0;
        if (P.nmax > 1) {
            const PblFrame Fr = pbl_frame_setup<WP>(L.w, B.q, B.cdfA, P, k, m, coef_m, coef_k, best, lane);
            const float wk = L.w[k - 1];
            // the frontier: every run empty (the chunks above `dirty` are), then the starting point {k-1} (:109-110) in the weight-1 run
            for (int c = 0; c <= dirty; ++c) { B.fsum[c * 64 + lane] = __builtin_inff(); B.fmeta[c * 64 + lane] = kPbxEmpty; }
            dirty = 0;
            wave_fence();
            if (lane == 0) { B.fsum[0] = wk; B.fmeta[0] = k - 1; }
            wave_fence();
            // order 3: lane c holds the minima of the chunks c + 64 i as (sum, meta, slot)
            float csum[CPL];
            int cmeta[CPL], cslot[CPL];
#pragma unroll
            for (int i = 0; i < CPL; ++i) { csum[i] = __builtin_inff(); cmeta[i] = kPbxEmpty; cslot[i] = (i * 64 + lane) * 64; }
            if (lane == 0) { csum[0] = wk; cmeta[0] = k - 1; }
            int seq = 1, nlive = 1;
            for (int j = 0; j < P.nmax - 1; ++j) {
                // ---- pop the first minimum by (sum, seq): the smallest of the lane's own candidates, then the wave's
                float s = 0.0f;
                int meta = 0, slot;
                {
                    int ls = 0;
#pragma unroll
                    for (int i = 0; i < CPL; ++i) {
                        const float s2 = O3 ? csum[i] : B.fsum[i * 64 + lane];
                        const int m2 = O3 ? cmeta[i] : B.fmeta[i * 64 + lane], sl2 = O3 ? cslot[i] : i * 64 + lane;
                        const bool lt = i == 0 || s2 < s || (s2 == s && m2 < meta);
                        s = lt ? s2 : s; meta = lt ? m2 : meta; ls = lt ? sl2 : ls;
                    }
                    const int wl = pbx_argmin(s, meta);
                    slot = __builtin_amdgcn_readlane(ls, wl);
                }
                cmp += nlive == 1 ? 1 : 2;
                const int last = meta & 0xFF;
                int wt, p0, p1 = 0, p2 = 0;
                if (slot == 0) { wt = 1; p0 = last; }
                else if (!O3 || slot < k) { wt = 2; p0 = slot - 1; p1 = last; }
                else {
                    const int t = slot - k;                // = b (b - 1) / 2 + a with a < b <= 190: candidate b finds itself
                    const int bA = lane, bB = 64 + lane, bC = 128 + lane;
                    const u64 hA = __ballot(bA >= 1 && bA * (bA - 1) / 2 <= t && t < bA * (bA + 1) / 2);
                    const u64 hB = __ballot(bB * (bB - 1) / 2 <= t && t < bB * (bB + 1) / 2);
                    const u64 hC = __ballot(bC * (bC - 1) / 2 <= t && t < bC * (bC + 1) / 2);
                    const int b = hA ? __builtin_ctzll(hA) : (hB ? 64 + __builtin_ctzll(hB) : 128 + __builtin_ctzll(hC));
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
                {
                    const int hi = has1 && eslot > slot ? eslot : slot;
                    dirty = (hi >> 6) > dirty ? (hi >> 6) : dirty;
                }
                wave_fence();
                if constexpr (O3) {
                    const int c0 = slot >> 6, ce = eslot >> 6;
                    float ms = B.fsum[c0 * 64 + lane];
                    int mm = B.fmeta[c0 * 64 + lane];
                    const int wl = pbx_argmin(ms, mm);
#pragma unroll
                    for (int i = 0; i < CPL; ++i) {
                        if ((c0 >> 6) == i && lane == (c0 & 63)) { csum[i] = ms; cmeta[i] = mm; cslot[i] = c0 * 64 + wl; }
                        if (has1 && ce != c0 && (ce >> 6) == i && lane == (ce & 63) &&
                            (esum < csum[i] || (esum == csum[i] && emeta < cmeta[i]))) {
                            csum[i] = esum; cmeta[i] = emeta; cslot[i] = eslot;
                        }
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
                u64 D[WP];
#pragma unroll
                for (int q = 0; q < WP; ++q) {
                    D[q] = S.d0[q] ^ L.P[p0][q];
                    if (wt > 1) D[q] ^= L.P[p1][q];
                    if (wt > 2) D[q] ^= L.P[p2][q];
                }
                const float cost = pbl_cost<WP>(pw, rs, D, lane);
                ++suc1;
                if (cost < best) {
                    best = cost; bw = wt; b0 = p0; b1 = p1; b2 = p2; bestidx = j + 1;
#pragma unroll
                    for (int q = 0; q < WP; ++q) bestD[q] = D[q];
                    // success rule (acquire_p_e_suc :423-436): the factors of positions 64 q + lane, multiplied ascending
                    const float ratio = (1.0f - w1) / w1;
                    float prod = 1.0f;
#pragma unroll
                    for (int q = 0; q < WP; ++q) {
                        const float qp = B.q[kOsdlK + 64 * q + lane];
                        const float fq = ((D[q] >> lane) & 1) ? 2.0f * qp : 2.0f * (1.0f - qp);
                        const int end = m - 64 * q < 64 ? m - 64 * q : 64;
                        for (int p = 0; p < end; ++p) prod = prod * __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fq), p));
                    }
                    const float p_suc = 1.0f / (1.0f + ratio / prod);
                    ++suc2;
                    if (p_suc > (float)Fr.p_t_suc) { stop = 2; ntep = j + 1; break; }
                }
            }
        }
        bool flip[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int p = 64 * s + lane;
            flip[s] = (bw > 0 && p == b0) || (bw > 1 && p == b1) || (bw > 2 && p == b2);
        }
        osdl_finish<WP>(L, S, flip, bestD, f, n, k, lane, cw_out);
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
