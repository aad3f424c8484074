// PB-OSD: the algorithm, and what its four kernels share (ldpc_osd_pb.hip is their translation unit).
//
// Reference (paths relative to LDPC_128/): pb_osd, PB_OSD/pb_testing.py:100-149 -- best-first TEP generation
// from a growing frontier list (optimal_tep_sequence :366-397: "first minimum of the reliability sums in list
// order", pop, append <= 2 children) with two probabilistic stopping rules (acquire_prob_promising :448-461,
// acquire_p_e_suc :423-436, thresholds :485-500).  All probabilities follow the float conventions of
// oracle/ldpc_oracle.c orc_pb_osd: float32 with det_expf (IEEE + - * / only, host and device agree bit for
// bit), float64 binomial-CDF recurrences; the promising rule compares in float64 (both sides are float64 tensors in the
// reference, :129), the success rule in float32 (:145: a float32 tensor against a NumPy double, which TensorFlow casts down).
//
// The list is NOT replayed TEP by TEP (the round-1 kernel did that: one wavefront, ~1.2 us per TEP, 51 ms for
// the rare frame on which no rule fires).  Three facts make the search batch-parallel and still exact
// (tests/pb_chunk_model.py states the algorithm in NumPy and checks it against the literal oracle):
//   1. every TEP has exactly one parent (extended child: e U {63}; adjacent child: largest index - 1), so the
//      list never holds duplicates and the pop sequence visits each TEP of weight 1..order exactly once;
//   2. a child's float32 sum is >= its parent's (monotone rounding), hence the pop sequence is the TEPs sorted
//      by (sum, list slot), and slot(t) < slot(u) <=> parent(t) is popped before parent(u), or they share the
//      parent and t is the extended child -- a comparator that only recurses when sums tie exactly;
//   3. the stopping rules see the visit order only through "best so far", a prefix minimum.
// So: a CHUNK of the visit order = all TEPs with sum in (lo, hi], sorted; its costs are evaluated in parallel and
// the sequential rules are recovered with prefix scans and a "first stop" reduction.
#pragma once

#include "ldpc_internal.h"
#include "ldpc_wave.h"
#include "ldpc_search.h"
#include "ldpc_front.h"
#include "ldpc_osd_state.h"
#include "ldpc_pb_expf.h"

namespace ldpc {

// Frontier = the reference's growing TEP list (optimal_tep_sequence :366-397) kept in INSERTION order:
// a popped entry is tombstoned in place (sum = +inf), children are appended, so "first minimum in list
// order" is the arg-min on (sum, slot).  A search that never stops visits all N_max TEPs with a list of
// tens of thousands of entries, so the arg-min is kept hierarchical: cmin[c] = best (sum, slot) of the 64
// slots of chunk c, smin[s] = best of the 64 chunks of super-chunk s.  A pop reads the <= 32 super-minima,
// then re-reduces one chunk and one super-chunk: ~3 wave reductions per TEP whatever the list length.
// Slots < kPbLdsSlots and chunk minima < kPbLdsChunks live in LDS, the rest in a per-wave global area.
struct PbEntry {
    float sum;          // reliability sum of the flipped MRB positions (ascending, sequential); +inf = removed
    unsigned pos;       // slots: pos0 | pos1 << 8 | pos2 << 16 | weight << 24;  minima: slot index
};
constexpr int kPbLdsSlots = 512, kPbLdsChunks = 64, kPbSuper = 32;   // 32 super-chunks x 4096 slots >= 2 N_max (order 3)

struct __attribute__((aligned(16))) PbLds {
    double cdfA[65];             // P[Bin(64, p1) <= b]
    double cdfH[65];             // P[Bin(64, 1/2) <= b] (copied once per wavefront: a global read per TEP sat on the critical path)
    float q[128];                // sigmoid(c4 |y'_p|)
    PbEntry fr[kPbLdsSlots];     // head of the list
    PbEntry cmin[kPbLdsChunks];  // chunk minima of the first 4096 slots
    PbEntry smin[kPbSuper];      // super-chunk minima
};

struct PbParams {
    int order, nmax;
    int t1, t2;                  // chunk targets: first chunk / later chunks
    int t3, budget;              // chunk target of the workgroup kernel; TEPs after which a frame may be handed to it
    int budget_s, budget_m;      // ... when its sub-list is short (< 128 frames) / of medium length (< 448)
    int budget_l, budget_xl;     // ... long (1400 .. 3000) / very long
    int late_min, late_maxlen, late_pct, late_div;   // once late_pct % of a sub-list's frames have STARTED (lists of more than late_min frames in all, sub-lists shorter than late_maxlen) a search leaves after budget / late_div
    int handoff_maxlen;          // ... if its sub-list of list A holds fewer frames than this (many searches: throughput counts, none leaves)
    float c4;
    long long cmin_off;          // offset of the spilled chunk minima inside a wave's global area
};

struct PbList {
    PbLds *B;
    PbEntry *spill;              // slots >= kPbLdsSlots, then chunk minima >= kPbLdsChunks at cmin_off
    long long cmin_off;
    __device__ __forceinline__ PbEntry slot(int i) const { return i < kPbLdsSlots ? B->fr[i] : spill[i - kPbLdsSlots]; }
    __device__ __forceinline__ void set_slot(int i, PbEntry e) const { if (i < kPbLdsSlots) B->fr[i] = e; else spill[i - kPbLdsSlots] = e; }
    __device__ __forceinline__ PbEntry cmin(int c) const { return c < kPbLdsChunks ? B->cmin[c] : spill[cmin_off + c - kPbLdsChunks]; }
    __device__ __forceinline__ void set_cmin(int c, PbEntry e) const { if (c < kPbLdsChunks) B->cmin[c] = e; else spill[cmin_off + c - kPbLdsChunks] = e; }
};

// wave arg-min on (sum, index): lower index wins ties; result in every lane
// (the minimum is handed on as a value, hence the float form of the reduction: see wave_min_f32, ldpc_wave.h)
__device__ __forceinline__ void argmin_si(float &s, int &idx, int lane)
{
    const float m = wave_min_f32_value(s);
    idx = wave_min_i32(s == m ? idx : 0x7FFFFFFF);
    s = m;
}

// (64 - i) / (i + 1): the ratio of consecutive binomial coefficients C(64, i+1) / C(64, i), correctly rounded
// float64 -- the same values the host computes for the oracle's recurrence
struct PbCoef {
    double v[64];
    constexpr PbCoef() : v() { for (int i = 0; i < 64; ++i) v[i] = (double)(64 - i) / (double)(i + 1); }
};
__constant__ PbCoef kPbCoef;

// per-frame PB quantities (wave-uniform), float conventions of the oracle
struct PbFrame {
    float spl, lrb_mean;       // prod (1 - q_p) over the MRB (com_mrb_prob :35-41), mean |y'| over the LRB (:401)
    double p_t_suc, p_t_pro;   // calculate_two_thresholds :485-500
};

// One wavefront: q[p] = sigmoid(c4 |y'_p|), the binomial CDF table of the mean LRB error probability and
// the two thresholds.  w = |y'| (LDS) must be in place; q / cdfA are per-frame LDS arrays.
// `pairs` (optional, [4][64] float2 of LDS): the four chains' (multiplier, addend) per step, written side by side here so that a
// step of the chains is ONE instruction (see below); without it the operands are formed per step.
__device__ __forceinline__ PbFrame pb_frame_setup(const float *w, float *q, double *cdfA, float c4, int order, int nmax, int lane,
                                                  float best0 = __builtin_inff(), float2 *pairs = nullptr)
{
    {
        const float q0 = 1.0f / (1.0f + det_expf(-(c4 * w[lane]))), q1 = 1.0f / (1.0f + det_expf(-(c4 * w[lane + 64])));
        q[lane] = q0;
        q[lane + 64] = q1;
        if (pairs) {
            pairs[lane] = make_float2(1.0f, q1);                  // chain 0: sum of q over the parity part
            pairs[64 + lane] = make_float2(1.0f, w[lane + 64]);    // chain 1: sum of |y'| over the parity part
            pairs[128 + lane] = make_float2(1.0f, q0);            // chain 2: sum of q over the MRB
            pairs[192 + lane] = make_float2(1.0f - q0, 0.0f);     // chain 3: product of 1 - q over the MRB
        }
    }
    wave_fence();
    // sequential (ascending position) means / product, as the oracle defines them: four dependent chains of 64 steps.  Lanes 0..3
    // run one chain each with ONE fused multiply-add per step -- acc * 1 + x is the sum, acc * x + 0 the product, both rounded
    // once like the plain operations (-ffp-contract=off does not touch an explicit fma) -- instead of every lane running all four.
    float a1, aw, at, spl;
    if (pairs) {
        const float2 *const src = pairs + 64 * (lane & 3);
        float acc = (lane & 3) == 3 ? 1.0f : 0.0f;
#pragma unroll 8
        for (int p = 0; p < 64; ++p) {
            const float2 t = src[p];
            acc = __builtin_fmaf(acc, t.x, t.y);
        }
        a1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 0));
        aw = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 1));
        at = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 2));
        spl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 3));
    } else {
        const int ch = lane & 3;
        const float *src = ch == 0 ? q + 64 : (ch == 1 ? w + 64 : q);
        const bool prod = ch == 3;
        float acc = prod ? 1.0f : 0.0f;
#pragma unroll 8
        for (int p = 0; p < 64; ++p) {
            const float x = src[p];
            const float b = prod ? 1.0f - x : 1.0f, c = prod ? 0.0f : x;
            acc = __builtin_fmaf(acc, b, c);
        }
        a1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 0));
        aw = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 1));
        at = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 2));
        spl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 3));
    }
    const float p1 = a1 / 64.0f, lrb_mean = aw / 64.0f, pt = at / 64.0f;
    // The rules read cdfA[beta] with beta = clamp(floor((best - sum) / lrb_mean)), best <= best0 (the order-0 metric) and
    // sum >= 0, so entries above floor(best0 / lrb_mean) are never read (division and floor are monotone): the table's
    // dependent float64 recurrence stops there -- typically after ~10 of its 64 steps.
    const float bq = __builtin_floorf(best0 / lrb_mean);
    const int ncdf = bq > 0.0f ? (bq < 64.0f ? (int)bq : 64) : 0;
    // binomial CDF tables by the pmf recurrence (float64): full table for p1, up to `order` for pt.  Lane i holds the
    // i-th coefficient; the dependent chain takes it by v_readlane (a scalar load per step sat on the critical path).
    double niu;
    const double coef_l = kPbCoef.v[lane];
    const auto coef = [coef_l](int i) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(coef_l);
        const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)b, i), hi = __builtin_amdgcn_readlane((int)(unsigned)(b >> 32), i);
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    };
    {
        double qq = 1.0 - (double)p1, t = qq;
        for (int s = 0; s < 6; ++s) t = t * t;
        const double ratio = (double)p1 / qq;
        double acc = t;
        if (lane == 0) cdfA[0] = acc;
#pragma unroll 2
        for (int i = 0; i < ncdf; ++i) {
            t = t * coef(i) * ratio;
            acc = acc + t;
            if (lane == 0) cdfA[i + 1] = acc;
        }
        qq = 1.0 - (double)pt; t = qq;
        for (int s = 0; s < 6; ++s) t = t * t;
        const double ratio2 = (double)pt / qq;
        acc = t;
        for (int i = 0; i < order; ++i) { t = t * coef(i) * ratio2; acc = acc + t; }
        niu = acc;
    }
    PbFrame F;
    F.spl = spl; F.lrb_mean = lrb_mean;
    F.p_t_suc = 0.99 * niu;
    F.p_t_pro = 0.002 * __builtin_sqrt((1.0 - niu) / (double)nmax);
    wave_fence();
    return F;
}

// promising-probability rule (acquire_prob_promising :448-461): true = stop
// (cdfA / cdfH: float64 tables, or the same tables already rounded to float32 -- they are only read through the cast)
template <typename TA>
__device__ __forceinline__ float pb_promising_bs(float rs, float best, const PbFrame &F, float c4, const TA *cdfA, const TA *cdfH, float &w1_out)
{
    const float w1 = det_expf(c4 * rs) * F.spl, w2 = 1.0f - w1;
    const float bt = __builtin_floorf((best - rs) / F.lrb_mean);
    const int beta = bt > 0.0f ? (bt < 64.0f ? (int)bt : 64) : 0;
    float bs = 0.0f;
    bs = bs + w1 * (float)cdfA[beta];
    bs = bs + w2 * (float)cdfH[beta];
    w1_out = w1;
    return bs;
}
template <typename TA>
__device__ __forceinline__ bool pb_not_promising(float rs, float best, const PbFrame &F, float c4, const TA *cdfA,
                                                 const TA *cdfH, float &w1_out)
{
    return (double)pb_promising_bs(rs, best, F, c4, cdfA, cdfH, w1_out) < F.p_t_pro;
}

// success rule (acquire_p_e_suc :423-436) for a candidate that became the best: true = stop.
// tq[p] = {2 (1 - q_p), 2 q_p} of parity position p (pb_success_terms): the factor of the sequential product is picked
// by the discrepancy bit -- a broadcast LDS read and a select per position instead of recomputing both terms.
__device__ __forceinline__ void pb_success_terms(const float *q, float2 *tq, int lane)
{
    const float qp = q[64 + lane];
    tq[lane] = make_float2(2.0f * (1.0f - qp), 2.0f * qp);
}

// the same from the table of q_p alone (the chunk kernels: half the LDS; the factor is formed per position, as pb_seq_kernel does)
__device__ __forceinline__ bool pb_success_q(u64 D, float w1, const float *qpar, const PbFrame &F)
{
    const float ratio = (1.0f - w1) / w1;
    float prod = 1.0f;
#pragma unroll 8
    for (int p = 0; p < 64; ++p) {
        const float qp = qpar[p];
        prod = prod * (((D >> p) & 1) ? 2.0f * qp : 2.0f * (1.0f - qp));
    }
    const float p_suc = 1.0f / (1.0f + ratio / prod);
    return p_suc > (float)F.p_t_suc;      // (pb_testing.py:145: TensorFlow compares the float32 tensor with the double cast TO float32)
}

// (D differs from lane to lane here: the factor is picked bitwise -- bit -> 0 / -1 by a signed field extract of the word's
//  half, then (y & m) | (x & ~m): three 32-bit instructions a position where (D >> p) & 1 compiled to a 64-bit shift, a 64-bit
//  compare and a select, five)
__device__ __forceinline__ bool pb_success(u64 D, float w1, const float2 *tq, const PbFrame &F)
{
    const float ratio = (1.0f - w1) / w1;
    float prod = 1.0f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int dw = (int)(unsigned)(h ? D >> 32 : D);
#pragma unroll 8
        for (int u = 0; u < 32; ++u) {
            const float2 t = tq[32 * h + u];
            const int m = __builtin_amdgcn_sbfe(dw, u, 1);
            prod = prod * __int_as_float((__float_as_int(t.y) & m) | (__float_as_int(t.x) & ~m));
        }
    }
    const float p_suc = 1.0f / (1.0f + ratio / prod);
    return p_suc > (float)F.p_t_suc;      // (pb_testing.py:145: TensorFlow compares the float32 tensor with the double cast TO float32)
}

// number of TEPs of weight 1, 1..2, 1..3 over 64 positions
constexpr int kPbPairs0 = 64, kPbTriples0 = 64 + 2016, kPbTabSize = 64 + 2016 + 41664;

struct PbTep {
    int p0, p1, p2, wt;
};
__device__ __forceinline__ float pb_sum(const float *w, const PbTep &t)
{
    float s = w[t.p0];
    if (t.wt > 1) s = s + w[t.p1];
    if (t.wt > 2) s = s + w[t.p2];
    return s;
}
__device__ __forceinline__ int pb_last(const PbTep &t) { return t.wt == 1 ? t.p0 : (t.wt == 2 ? t.p1 : t.p2); }
// children pushed by a pop minus the popped entry itself (optimal_tep_sequence :381-396)
__device__ __forceinline__ int pb_delta(const PbTep &t, int order)
{
    const int last = pb_last(t), prev = t.wt == 2 ? t.p0 : t.p1;
    const int has1 = last < 63 && t.wt < order;
    const int has2 = t.wt > 1 ? (last - prev > 1) : (last - 1 > -1);
    return has1 + has2 - 1;
}
// t := parent(t); returns 0 = t was the extended child, 1 = the adjacent child, -1 = t is the root {63}
__device__ __forceinline__ int pb_to_parent(PbTep &t)
{
    const int last = pb_last(t);
    if (last == 63) {
        if (t.wt == 1) return -1;
        --t.wt;
        return 0;
    }
    if (t.wt == 1) t.p0 = last + 1; else if (t.wt == 2) t.p1 = last + 1; else t.p2 = last + 1;
    return 1;
}
__device__ __forceinline__ bool pb_same(const PbTep &a, const PbTep &b)
{
    return a.wt == b.wt && a.p0 == b.p0 && (a.wt < 2 || a.p1 == b.p1) && (a.wt < 3 || a.p2 == b.p2);
}
// t is popped before u (t != u): (sum, list slot) order, the slot order through the parents
__device__ bool pb_visit_less(const float *w, PbTep t, PbTep u)
{
    for (;;) {
        const float st = pb_sum(w, t), su = pb_sum(w, u);
        if (st != su) return st < su;
        const int kt = pb_to_parent(t), ku = pb_to_parent(u);
        if (kt < 0) return true;
        if (ku < 0) return false;
        if (pb_same(t, u)) return kt < ku;
    }
}
struct PbOut {
    u64 *cw; float *metric; int *best, *ntep, *aux;
};

// What pb_singles_kernel hands to the chunk kernel: ONE contiguous record per frame (1536 B) with everything the search
// needs, so that the receiving wavefront starts after a single wide load instead of the chain frame number -> source
// index -> permutation -> y (round 4; the record replaces the separate 1096-byte per-frame table of rounds 2-3):
//   words [0, 128)     w[128]     |y'|                                       } the head of PbWaveLds (behind its four pad
//   words [128, 256)   P[64]      rows of P'                                 } words): the chunk kernel copies these 360 words
//   words [256, 258)   0          the "row" an unused position of a key reads } into LDS as they are
//   words [258, 326)   cdfA[68]   P[Bin(64, p1) <= b] rounded to float32     }
//   words [326, 358)   perm[128]  original bit index of primed position p, one byte each (+ 2 pad words)
//   words [360, ...)   PbHead     the frame's scalars and the search state after the weight-1 head
// Derived on arrival (a few dozen instructions): the cost-bound table (sorted parity weights) and the success-rule factors.
struct PbHead {
    PbFrame fr;
    u64 d0, hm, hp;            // order-0 parity discrepancy, hard decisions of the MRB / parity part
    u64 hbestD, hbestE;        // the search state after the weight-1 head of the pop sequence (no rule fired on it)
    float hbest;
    int nhead, hsuc2, hbestidx;
};
constexpr int kPbR1Zero = 256, kPbR1Cdf = 258, kPbR1Perm = 326, kPbR1Head = 360, kPbR1Words = 384;     // (words [0, kPbR1Head) are copied into LDS)
static_assert(kPbR1Head * 4 % 8 == 0 && kPbR1Head * 4 + sizeof(PbHead) <= kPbR1Words * 4, "record layout");

template <class LDS>
__device__ __forceinline__ void pb_write(LDS &L, const SearchFrame &S, const PbOut &O, long long f, int lane, u64 bestE,
                                         u64 bestD, float best, int bestidx, int ntep, int cmp, int suc1, int suc2, int stop)
{
    search_finish(L, S, bestE, bestD, f, lane, O.cw);
    if (lane == 0) {
        if (O.metric) O.metric[f] = best;
        if (O.best) O.best[f] = bestidx;
        if (O.ntep) O.ntep[f] = ntep;
        if (O.aux) { O.aux[f * 4] = cmp; O.aux[f * 4 + 1] = suc1; O.aux[f * 4 + 2] = suc2; O.aux[f * 4 + 3] = stop; }
    }
    wave_fence();
}

}  // namespace ldpc
