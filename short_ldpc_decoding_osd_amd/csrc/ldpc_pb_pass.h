// PB-OSD stage 2, judging a chunk with one wavefront: the cost of a candidate (pbw_cost_floor / _exact), the sort-free pass over
// 8-byte keys in registers (pbw_scan_chunk) and over 4-byte keys in LDS (pbw_scan4) -- their loops here, what follows the loop in
// ldpc_pb_rules.h -- and the sorted path for what the pass cannot settle (pbw_process_chunk).
#pragma once
#include "ldpc_pb_rules.h"

namespace ldpc {

// The weighted distance of a candidate, two ways.  The chunk kernel keeps no byte LUT (8 KiB of LDS per frame: with it two
// wavefronts fit a SIMD, without it three to four, and the kernel spends half its time waiting):
//   pbw_cost_floor  a LOWER bound from the NUMBER of parity discrepancies in each quarter of the parity part: the candidate
//                   differs from the hard decisions in popcount(D_g) positions of quarter g, which weigh at least as much as
//                   that quarter's popcount(D_g) lightest positions.  The rules need a cost only to know whether it beats
//                   the best so far; past the first chunk the bound settles that for all but ~1 key in 10^3..10^4 (measured
//                   on NMS failures: 0.01 % at 1.0 dB, 0.06 % at 2.5 dB; one popcount over all 64 positions lets 13-17 %
//                   through: a random D has ~32 ones, and the 32 lightest weights are light).  Rounded down twice (table
//                   entries, then the sum) so that it stays below the float32 value of the canonical summation, whose
//                   rounding errors are < 1e-6 relative.
//   pbw_cost_exact  the canonical order of the byte LUT (each byte ascending from 0, bytes added in order; tep_cost),
//                   64 conditional adds: bit-identical to the LUT form.  For the survivors of the bound.
template <int CAP>
__device__ __forceinline__ float pbw_cost_floor(const PbWaveLds<CAP> &L, float mrb, u64 D)
{
    const unsigned lo = (unsigned)D, hi = (unsigned)(D >> 32);
    const float t0 = L.tail[0][__popc(lo & 0xFFFFu)], t1 = L.tail[1][__popc(lo >> 16)];
    const float t2 = L.tail[2][__popc(hi & 0xFFFFu)], t3 = L.tail[3][__popc(hi >> 16)];
    return (((mrb + t0) + t1) + (t2 + t3)) * 0.99999f;
}
template <int CAP>
__device__ __forceinline__ float pbw_cost_exact(const PbWaveLds<CAP> &L, float mrb, u64 D)
{
    float acc = mrb;
#pragma unroll 1
    for (int b = 0; b < 8; ++b) {
        const unsigned v = (unsigned)(D >> (8 * b)) & 255u;
        float bs = 0.0f;
#pragma unroll
        for (int t = 0; t < 8; ++t) bs = ((v >> t) & 1u) ? bs + L.w[64 + 8 * b + t] : bs;
        acc = acc + bs;
    }
    return acc;
}
// cost if it can be below `bound`, +inf otherwise (exact for every use: the rules only compare costs with bests <= bound)
template <int CAP>
__device__ __forceinline__ float pbw_cost(const PbWaveLds<CAP> &L, float mrb, u64 D, float bound)
{
    float c = __builtin_inff();
    if (pbw_cost_floor<CAP>(L, mrb, D) < bound) c = pbw_cost_exact<CAP>(L, mrb, D);
    return c;
}

// Sort-free pass over a chunk (the n keys as the walk left them, in no particular order).  The visit order matters to the
// rules only through (i) "best so far", which changes only at a key whose cost beats the best the chunk STARTED with -- a
// candidate; deep in a search a chunk holds none, or one or two -- and (ii) the frontier size, which matters only when it
// can be 1.  So: every key's cost, frontier growth and rule 1 against the chunk-start best, in parallel and in any order;
//   no candidate:  rule 1 depends on the sum alone, so the search stops at the SMALLEST firing sum, and the number of TEPs
//                  visited is the number of smaller sums: one count, no sort;
//   <= 16 candidates: they are put in visit order among themselves (a handful of comparisons), the records and their
//                  success rule follow sequentially, rule 1 is re-evaluated for the keys behind the first record with the
//                  best they see, and the stop / winner positions are counts again;
//   otherwise -1 and nothing changed: the caller sorts the chunk (pbw_process_chunk).  That is: many candidates (the first
//                  chunk or two), a frontier that may shrink to one entry (the first chunk, the tail of a complete scan),
//                  or a key whose sum EQUALS that of a key a position is counted against (list order would decide; the
//                  pass compares sums only, which keeps it small: it is compared against a handful of keys per chunk).
// Returns 0 = no rule fired (state advanced), 1 = stopped (stop / ntep set), -1 = not handled.
template <int CAP>
__device__ __forceinline__ int pbw_scan_chunk(PbWaveLds<CAP> &L, const PbParams &P, const PbFrame &Fr, u64 d0, int n, float mn, float mx, int lane,
                                              PbwState &S, int &stop, int &ntep)
{
    constexpr int PER = CAP / 64, STEP = PER % 4 == 0 ? 4 : 3;
    static_assert(CAP % 64 == 0 && PER % STEP == 0, "the pass reads its keys STEP slices at a time");
    if (S.nlive <= 1) return -1;      // (the first chunk: one entry in the frontier, its pops are counted one by one)
    const float best0 = S.best;
    const float r_safe = pb_rule1_safe_sum(mn, mx, best0, Fr, P.c4, L.cdfA, L.cdfH, lane);      // rule 1 by probes
    const auto parity = [&](const PbTep &t) { return pb_tep_parity(L.P, d0, t); };
    u64 kq[PER];
    unsigned npneed = 0, npmask = 0, survmask = 0;
    int sumf = 0, neg = 0, nsurv = 0;
    unsigned short *const slist = reinterpret_cast<unsigned short *>(L.list);     // keys the cost bound could not rule out
    // Branch-free, STEP keys of the lane side by side: the keys, then their three P' rows each (an unused position reads the
    // zero row: no select), then the bound's four table entries each -- three LDS round trips per STEP keys.  An empty slot
    // holds a key whose sum is a NaN (every comparison false), whose positions read in-range garbage and whose growth field
    // says 0: no validity mask anywhere.  (Round 3's form compiled to a branch and a wait behind every single LDS read.)
    constexpr u64 kEmpty = 0xFFFFFFFFF7FFFFFFull;
    const char *const Pb = reinterpret_cast<const char *>(L.P);
    const char *const tb = reinterpret_cast<const char *>(L.tail);
    const unsigned d0l = (unsigned)d0, d0h = (unsigned)(d0 >> 32);
#pragma unroll
    for (int k0 = 0; k0 < PER; k0 += STEP) {
#pragma unroll
        for (int u = 0; u < STEP; ++u) { const int i = lane + 64 * (k0 + u); kq[k0 + u] = i < n ? L.keys[i] : kEmpty; }
        uint2 r0[STEP], r1[STEP], r2[STEP];
#pragma unroll
        for (int u = 0; u < STEP; ++u) {
            const unsigned code = (unsigned)kq[k0 + u];
            r0[u] = *reinterpret_cast<const uint2 *>(Pb + ((code & 255u) << 3));
            r1[u] = *reinterpret_cast<const uint2 *>(Pb + (((code >> 8) & 255u) << 3));
            r2[u] = *reinterpret_cast<const uint2 *>(Pb + (((code >> 16) & 255u) << 3));
        }
        float t0[STEP], t1[STEP], t2[STEP], t3[STEP];
#pragma unroll
        for (int u = 0; u < STEP; ++u) {
            const unsigned lo = __builtin_amdgcn_bitop3_b32(r0[u].x, r1[u].x, r2[u].x, 0x96) ^ d0l;
            const unsigned hi = __builtin_amdgcn_bitop3_b32(r0[u].y, r1[u].y, r2[u].y, 0x96) ^ d0h;
            t0[u] = *reinterpret_cast<const float *>(tb + (__popc(lo & 0xFFFFu) << 2));
            t1[u] = *reinterpret_cast<const float *>(tb + 68 + (__popc(lo >> 16) << 2));
            t2[u] = *reinterpret_cast<const float *>(tb + 136 + (__popc(hi & 0xFFFFu) << 2));
            t3[u] = *reinterpret_cast<const float *>(tb + 204 + (__popc(hi >> 16) << 2));
        }
#pragma unroll
        for (int u = 0; u < STEP; ++u) {
            const int k = k0 + u;
            const unsigned code = (unsigned)kq[k];
            const float rs = __uint_as_float((unsigned)(kq[k] >> 32));
            const bool surv = (((rs + t0[u]) + t1[u]) + (t2[u] + t3[u])) * 0.99999f < best0;      // (pbw_cost_floor)
            survmask |= surv ? 1u << k : 0u;
            npneed |= rs > r_safe ? 1u << k : 0u;
            const int fld = (int)((code >> 26) & 3u);     // growth + 1
            sumf += fld; neg += fld == 0;
        }
        asm volatile("" : "+v"(survmask), "+v"(npneed), "+v"(sumf), "+v"(neg) : : "memory");
    }
    const int sumdel = sumf - PER;       // (every slot, empty or not, carried a + 1)
    if (__ballot(survmask != 0)) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const bool surv = (survmask >> k) & 1u;
            const u64 sm = __ballot(surv);
            if (sm) {
                if (surv) slist[nsurv + wave_lane_rank(sm)] = (unsigned short)(lane + 64 * k);
                nsurv += __popcll(sm);
            }
        }
    }
    const int negtot = wave_add_i32(neg), deltot = wave_add_i32(sumdel);
    if (S.nlive - negtot <= 1) return -1;
    // the survivors' costs, 64 at a time (the canonical summation, no LUT: ~200 instructions, but per BATCH); those that beat the
    // chunk-start best are the candidates
    int ncand = 0;
    if (nsurv) {
        wave_fence();
        for (int b0 = 0; b0 < nsurv && ncand <= 16; b0 += 64) {
            const bool has = b0 + lane < nsurv;
            const u64 key = has ? L.keys[slist[b0 + lane]] : 0ull;
            const float c = has ? pbw_cost_exact<CAP>(L, __uint_as_float((unsigned)(key >> 32)), parity(pbw_tep((unsigned)key))) : __builtin_inff();
            const bool cand = c < best0;
            const u64 cm = __ballot(cand);
            if (cm) {
                const int idx = ncand + wave_lane_rank(cm);
                if (cand && idx < 16) { L.ck[idx] = key; L.cc[idx] = c; }
                ncand += __popcll(cm);
            }
        }
        if (ncand > 16) return -1;
    }
    // rule 1 for the keys above the last safe probe (the last chunk of a search; nothing elsewhere)
    if (__ballot(npneed != 0)) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const bool need = (npneed >> k) & 1u;
            if (__ballot(need)) {
                float w1;
                if (need && pb_not_promising(__uint_as_float((unsigned)(kq[k] >> 32)), best0, Fr, P.c4, L.cdfA, L.cdfH, w1)) npmask |= 1u << k;
            }
        }
    }
    // (sums are >= +0: their bit patterns order like the floats; an invalid slot holds all ones)
    const auto sumbits = [](u64 key) { return (unsigned)(key >> 32); };
    bool tie = false;
    // number of my keys with a smaller sum than `ref`; a different key with the same sum is a tie
    const auto count_before = [&](u64 ref) {
        int c = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            c += sumbits(kq[k]) < sumbits(ref);
            tie |= sumbits(kq[k]) == sumbits(ref) && kq[k] != ref;
        }
        return wave_add_i32(c);
    };
    int nrec = 0, stop2 = 0;     // records among the candidates; stop2: the success rule fired on the last of them
    if (ncand > 0) {
        // ---- the candidates, in visit order
        wave_fence();
        {
            const u64 my = L.ck[lane & 15];
            const float myc = L.cc[lane & 15];
            int r = 0;
            for (int d = 0; d < ncand; ++d) { const u64 o = L.ck[d]; r += sumbits(o) < sumbits(my); tie |= lane < ncand && sumbits(o) == sumbits(my) && o != my; }
            wave_fence();
            if (lane < ncand) { L.ck[r] = my; L.cc[r] = myc; }
            wave_fence();
        }
        if (__ballot(tie)) return -1;
        // ---- records and the success rule, sequentially (every lane runs the same arithmetic on the same values)
        float before = best0;
        for (int t = 0; t < ncand && !stop2; ++t) {
            const u64 key = L.ck[t];
            const float c = L.cc[t];
            if (c < before) {
                if (lane == 0) { L.rk[nrec] = key; L.rc[nrec] = c; }
                ++nrec;
                const float w1 = det_expf(P.c4 * __uint_as_float((unsigned)(key >> 32))) * Fr.spl;
                if (pb_success_q(parity(pbw_tep((unsigned)key)), w1, L.qpar, Fr)) stop2 = 1;
                before = c;
            }
        }
        wave_fence();
        // ---- rule 1 again for the keys behind the first record, with the best they see
        if (nrec > 0) {
            const unsigned s0 = sumbits(L.rk[0]);
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                if (lane + 64 * k < n && sumbits(kq[k]) >= s0 && kq[k] != L.rk[0]) {
                    int t = 0;
                    for (int u = 0; u < nrec; ++u) { const u64 r = L.rk[u]; t += sumbits(r) < sumbits(kq[k]); tie |= sumbits(r) == sumbits(kq[k]) && r != kq[k]; }
                    if (t > 0) {
                        float w1;
                        const bool np = pb_not_promising(__uint_as_float(sumbits(kq[k])), L.rc[t - 1], Fr, P.c4, L.cdfA, L.cdfH, w1);
                        npmask = (npmask & ~(1u << k)) | (np ? 1u << k : 0u);
                    }
                }
            }
        }
    }
    // ---- the smallest sum on which rule 1 fires: every key of that sum sees the same best, so the first of them stops
    unsigned fs = 0x7FFFFFFFu;
#pragma unroll
    for (int k = 0; k < PER; ++k)
        if (((npmask >> k) & 1u) && sumbits(kq[k]) < fs) fs = sumbits(kq[k]);
    const unsigned sF = (unsigned)wave_min_i32((int)fs);
    // ---- the stop: the earlier of rule 1's first key and the record on which rule 2 fired
    int reason = 0;
    unsigned sstop = 0;
    if (sF != 0x7FFFFFFFu) { reason = 1; sstop = sF; }
    if (stop2) {
        const unsigned sR = sumbits(L.rk[nrec - 1]);
        if (reason == 1 && sR == sF) tie = true;
        if (reason == 0 || sR < sF) { reason = 2; sstop = sR; }
    }
    int nbefore = nrec;           // records that really happened: those before the stop (and the stop itself for rule 2)
    if (reason) {
        nbefore = 0;
        for (int u = 0; u < nrec; ++u) nbefore += sumbits(L.rk[u]) < sstop;
        nbefore += reason == 2;
    }
    int rank_best = 0, rank_stop = 0;
    if (nbefore > 0) rank_best = count_before(L.rk[nbefore - 1]);
    if (reason == 2) rank_stop = rank_best;
    if (reason == 1) {   // (the keys of the stopping sum all fire: the first of them in list order is at this position, whichever it is)
        int c = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) c += sumbits(kq[k]) < sstop;
        rank_stop = wave_add_i32(c);
    }
    if (__ballot(tie)) return -1;
    // ---- commit
    if (nbefore > 0) {
        const u64 bk = L.rk[nbefore - 1];
        const PbTep t = pbw_tep((unsigned)bk);
        const u64 E = pb_tep_mask(t);
        S.best = L.rc[nbefore - 1]; S.bestD = parity(t); S.bestE = E;
        S.bestidx = S.j + rank_best + 1;
    }
    return pbw_commit_counts(S, nbefore, reason, rank_stop, n, deltot, stop, ntep);
}

// pbw_scan_chunk for a chunk of 4-BYTE keys (pbw_walk<K4>: up to 2 CAP + 64 of them): the same sort-free pass, with a key's
// sum recomputed from its positions wherever it is needed -- (w[p0] + w[p1]) + w[p2], the order the walk formed it in, three LDS
// reads and two adds -- and NO key kept in registers: the ordinary chunk reads each key once; the rare paths (a rule fires,
// improvement candidates) read them again.  Same results as pbw_scan_chunk on the same keys; -1 leaves the state untouched and
// the caller redoes the chunk's sum range with 8-byte keys (pbw_redo_range).
template <int CAP>
__device__ __forceinline__ int pbw_scan4(PbWaveLds<CAP> &L, const PbParams &P, const PbFrame &Fr, u64 d0, int n, float mn, float mx, int lane,
                                         PbwState &S, int &stop, int &ntep)
{
    constexpr int STEP = 2;
    if (S.nlive <= 1) return -1;      // (the first chunk of a frame without its head: one entry in the frontier)
    const float best0 = S.best;
    const float r_safe = pb_rule1_safe_sum(mn, mx, best0, Fr, P.c4, L.cdfA, L.cdfH, lane);      // rule 1 by probes
    const unsigned *const codes = reinterpret_cast<const unsigned *>(L.keys);
    const char *const Pb = reinterpret_cast<const char *>(L.P);
    const char *const wb = reinterpret_cast<const char *>(L.w);
    const char *const tb = reinterpret_cast<const char *>(L.tail);
    const unsigned d0l = (unsigned)d0, d0h = (unsigned)(d0 >> 32);
    constexpr unsigned kEmpty = 0xF7FFFFFFu;       // an empty slot: growth field 0 + 1, positions that read in range; its sum is forced to NaN
    // sum bits of a key (all ones for an empty slot: a NaN, larger than every sum as an integer)
    const auto sum_of = [&](unsigned code, bool valid) {
        const float w0 = *reinterpret_cast<const float *>(wb + ((code & 255u) << 2));
        const float w1 = *reinterpret_cast<const float *>(wb + (((code >> 8) & 255u) << 2));
        const float w2 = *reinterpret_cast<const float *>(wb + (((code >> 16) & 255u) << 2));
        const unsigned wt = (code >> 24) & 3u;
        float rs = wt > 1u ? w0 + w1 : w0;
        rs = wt > 2u ? rs + w2 : rs;
        return valid ? __float_as_uint(rs) : 0xFFFFFFFFu;
    };
    const auto key_at = [&](int k, unsigned &code, unsigned &sb) {
        const int i = k * 64 + lane;
        code = i < n ? codes[i] : kEmpty;
        sb = sum_of(code, i < n);
    };
    const auto parity = [&](const PbTep &t) { return pb_tep_parity(L.P, d0, t); };
    int sumf = 0, neg = 0, nsurv = 0;
    unsigned fs = 0x7FFFFFFFu;     // the smallest sum on which rule 1 fires (against the chunk-start best)
    unsigned short *const slist = reinterpret_cast<unsigned short *>(L.list);     // keys the cost bound could not rule out
    const int nsl = (n + 63) >> 6;
#pragma unroll 1
    for (int k0 = 0; k0 < nsl; k0 += STEP) {       // (a rolled loop: unrolled over the 14 slices it is 12 KiB of code and the kernel spills)
        unsigned code[STEP], sb[STEP];
        uint2 r0[STEP], r1[STEP], r2[STEP];
#pragma unroll
        for (int u = 0; u < STEP; ++u) {
            key_at(k0 + u, code[u], sb[u]);
            r0[u] = *reinterpret_cast<const uint2 *>(Pb + ((code[u] & 255u) << 3));
            r1[u] = *reinterpret_cast<const uint2 *>(Pb + (((code[u] >> 8) & 255u) << 3));
            r2[u] = *reinterpret_cast<const uint2 *>(Pb + (((code[u] >> 16) & 255u) << 3));
        }
        float t0[STEP], t1[STEP], t2[STEP], t3[STEP];
#pragma unroll
        for (int u = 0; u < STEP; ++u) {
            const unsigned lo = __builtin_amdgcn_bitop3_b32(r0[u].x, r1[u].x, r2[u].x, 0x96) ^ d0l;
            const unsigned hi = __builtin_amdgcn_bitop3_b32(r0[u].y, r1[u].y, r2[u].y, 0x96) ^ d0h;
            t0[u] = *reinterpret_cast<const float *>(tb + (__popc(lo & 0xFFFFu) << 2));
            t1[u] = *reinterpret_cast<const float *>(tb + 68 + (__popc(lo >> 16) << 2));
            t2[u] = *reinterpret_cast<const float *>(tb + 136 + (__popc(hi & 0xFFFFu) << 2));
            t3[u] = *reinterpret_cast<const float *>(tb + 204 + (__popc(hi >> 16) << 2));
        }
#pragma unroll
        for (int u = 0; u < STEP; ++u) {
            const float rs = __uint_as_float(sb[u]);
            const bool surv = (((rs + t0[u]) + t1[u]) + (t2[u] + t3[u])) * 0.99999f < best0;      // (pbw_cost_floor)
            const u64 sm = __ballot(surv);
            if (sm) {
                if (surv) slist[nsurv + wave_lane_rank(sm)] = (unsigned short)((k0 + u) * 64 + lane);
                nsurv += __popcll(sm);
            }
            const int fld = (int)((code[u] >> 26) & 3u);     // growth + 1
            sumf += fld; neg += fld == 0;
            const bool need = rs > r_safe;      // above the last safe probe (the last chunk of a search): the rule itself
            if (__ballot(need)) {
                float w1;
                if (need && pb_not_promising(rs, best0, Fr, P.c4, L.cdfA, L.cdfH, w1) && sb[u] < fs) fs = sb[u];
            }
        }
    }
    const int negtot = wave_add_i32(neg), deltot = wave_add_i32(sumf) - 64 * STEP * ((nsl + STEP - 1) / STEP);     // (every slot looked at carried a + 1)
    if (S.nlive - negtot <= 1) return -1;
    // the survivors' exact costs, 64 at a time; those that beat the chunk-start best are the candidates (as 8-byte keys)
    int ncand = 0;
    if (nsurv) {
        wave_fence();
        for (int b0 = 0; b0 < nsurv && ncand <= 16; b0 += 64) {
            const bool has = b0 + lane < nsurv;
            const unsigned code = has ? codes[slist[b0 + lane]] : kEmpty;
            const unsigned sbits = sum_of(code, has);
            const float c = has ? pbw_cost_exact<CAP>(L, __uint_as_float(sbits), parity(pbw_tep(code))) : __builtin_inff();
            const bool cand = c < best0;
            const u64 cm = __ballot(cand);
            if (cm) {
                const int idx = ncand + wave_lane_rank(cm);
                if (cand && idx < 16) { L.ck[idx] = ((u64)sbits << 32) | code; L.cc[idx] = c; }
                ncand += __popcll(cm);
            }
        }
        if (ncand > 16) return -1;
    }
    const auto sumbits = [](u64 key) { return (unsigned)(key >> 32); };
    unsigned sF = (unsigned)wave_min_i32((int)fs);
    if (ncand == 0) {
        // no candidate, no key fires: the whole chunk is visited and nothing else happens
        if (sF == 0x7FFFFFFFu) return pbw_commit_counts(S, 0, 0, 0, n, deltot, stop, ntep);
        // no candidate, rule 1 fires: the search stops at the first key of the smallest firing sum (every key of that sum fires)
        int cs = 0;
        for (int k = 0; k < nsl; ++k) { unsigned code, sb; key_at(k, code, sb); cs += sb < sF; }
        const int rank_stop = wave_add_i32(cs);      // (pbw_commit_counts(S, 0, 1, rank_stop, ...), written out: the call changes nine lines of pb_wave_kernel)
        S.cmp += 2 * (rank_stop + 1);
        S.suc1 += rank_stop;
        stop = 1; ntep = S.j + rank_stop + 1;
        return 1;
    }
    // ---- the candidates, in visit order; records and the success rule, sequentially (every lane the same arithmetic)
    bool tie = false;
    int nrec = 0, stop2 = 0;
    wave_fence();
    {
        const u64 my = L.ck[lane & 15];
        const float myc = L.cc[lane & 15];
        int r = 0;
        for (int d = 0; d < ncand; ++d) { const u64 o = L.ck[d]; r += sumbits(o) < sumbits(my); tie |= lane < ncand && sumbits(o) == sumbits(my) && o != my; }
        wave_fence();
        if (lane < ncand) { L.ck[r] = my; L.cc[r] = myc; }
        wave_fence();
    }
    if (__ballot(tie)) return -1;
    {
        float before = best0;
        for (int t = 0; t < ncand && !stop2; ++t) {
            const u64 key = L.ck[t];
            const float c = L.cc[t];
            if (c < before) {
                if (lane == 0) { L.rk[nrec] = key; L.rc[nrec] = c; }
                ++nrec;
                const float w1 = det_expf(P.c4 * __uint_as_float((unsigned)(key >> 32))) * Fr.spl;
                if (pb_success_q(parity(pbw_tep((unsigned)key)), w1, L.qpar, Fr)) stop2 = 1;
                before = c;
            }
        }
    }
    wave_fence();
    // Rule 1 again for the keys from the first record on, each with the best it really sees (the record before it).  A lower
    // best fires sooner, so a key that the LAST record's cost does not stop is stopped by none: probes with that cost leave
    // the keys beyond the last safe probe to evaluate -- usually none.  Keys before the first record keep what the
    // chunk-start best said (fs, if it lies before the first record).
    if (nrec > 0) {
        const unsigned s0 = sumbits(L.rk[0]);
        float r_safe2;     // (pb_rule1_safe_sum with the last record's cost, written out: the helper costs pb_wave_kernel an instruction)
        {
            const float rp = lane == 63 ? mx : mn + (mx - mn) * ((float)(lane + 1) * (1.0f / 64.0f));
            float w1;
            const float bs = pb_promising_bs(rp, L.rc[nrec - 1], Fr, P.c4, L.cdfA, L.cdfH, w1);
            const u64 unsafe = ~__ballot((double)bs > Fr.p_t_pro * 1.001);
            const int u = unsafe ? __builtin_ctzll(unsafe) : 64;
            r_safe2 = u == 0 ? -1.0f : __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rp), u - 1));
        }
        fs = fs < s0 ? fs : 0x7FFFFFFFu;
        for (int k = 0; k < nsl; ++k) {
            unsigned code, sb;
            key_at(k, code, sb);
            const u64 key = ((u64)sb << 32) | code;
            const bool behind = sb != 0xFFFFFFFFu && sb >= s0;
            int t = 0;
            if (behind)
                for (int u = 0; u < nrec; ++u) { const u64 r = L.rk[u]; t += sumbits(r) < sb; tie |= sumbits(r) == sb && r != key; }
            const bool need = behind && __uint_as_float(sb) > r_safe2;
            if (__ballot(need)) {
                float w1;      // (the first record itself is judged with the chunk-start best: t = 0)
                if (need && pb_not_promising(__uint_as_float(sb), t > 0 ? L.rc[t - 1] : best0, Fr, P.c4, L.cdfA, L.cdfH, w1) && sb < fs) fs = sb;
            }
        }
        sF = (unsigned)wave_min_i32((int)fs);
    }
    // ---- the stop: the earlier of rule 1's first key and the record on which rule 2 fired
    int reason = 0;
    unsigned sstop = 0;
    if (sF != 0x7FFFFFFFu) { reason = 1; sstop = sF; }
    if (stop2) {
        const unsigned sR = sumbits(L.rk[nrec - 1]);
        if (reason == 1 && sR == sF) tie = true;
        if (reason == 0 || sR < sF) { reason = 2; sstop = sR; }
    }
    int nbefore = nrec;           // records that really happened: those before the stop (and the stop itself for rule 2)
    if (reason) {
        nbefore = 0;
        for (int u = 0; u < nrec; ++u) nbefore += sumbits(L.rk[u]) < sstop;
        nbefore += reason == 2;
    }
    // positions: the keys below the last record that counts, the keys below the stopping sum; ties
    const u64 bk = nbefore > 0 ? L.rk[nbefore - 1] : 0ull;
    int cb = 0, cs = 0;
    for (int k = 0; k < nsl; ++k) {
        unsigned code, sb;
        key_at(k, code, sb);
        const u64 key = ((u64)sb << 32) | code;
        if (nbefore > 0) { cb += sb < sumbits(bk); tie |= sb == sumbits(bk) && key != bk; }
        if (reason == 1) cs += sb < sstop;
    }
    const int rank_best = wave_add_i32(cb), rank_stop = reason == 2 ? rank_best : wave_add_i32(cs);
    if (__ballot(tie)) return -1;
    // ---- commit
    if (nbefore > 0) {
        const PbTep t = pbw_tep((unsigned)bk);
        const u64 E = pb_tep_mask(t);
        S.best = L.rc[nbefore - 1]; S.bestD = parity(t); S.bestE = E;
        S.bestidx = S.j + rank_best + 1;
    }
    return pbw_commit_counts(S, nbefore, reason, rank_stop, n, deltot, stop, ntep);
}

// The n keys of one chunk (all TEPs of a sum range (mn, mx]): sort into visit order, evaluate in parallel, apply the
// sequential rules.  Returns 0 = no rule fired (state advanced), 1 = stopped (stop / ntep set), 2 = a run of more than
// kPbMaxTie equal sums (frame goes to the list replay).
template <int CAP>
__device__ __forceinline__ int pbw_process_chunk(PbWaveLds<CAP> &L, const PbParams &P, const PbFrame &Fr, u64 d0, int n, float mn, float mx,
                                                 int lane, PbwState &S, int &stop, int &ntep)
{
    constexpr int PER = CAP / 64;
    // ---- bucket sort: CAP buckets over (mn, mx], counts -> offsets -> scatter (grouped by bucket) -> every key counts the
    // keys of its own bucket that sort before it.  Entries past a bucket's end belong to higher buckets (larger keys), past
    // the chunk's end to the all-ones pad: the count needs no mask and runs to the wave's fullest bucket.
    {
        static_assert(PER % 2 == 0, "a lane's bucket counters are read and written as pairs");
        int2 *h2 = reinterpret_cast<int2 *>(&L.hist[lane * PER]);
#pragma unroll
        for (int k = 0; k < PER / 2; ++k) h2[k] = make_int2(0, 0);
    }
    const float scale = mx > mn ? (float)CAP / (mx - mn) : 0.0f;
    const bool flat = !(scale < 3.0e38f);           // denormally close sums: one bucket
    const auto bucket = [&](u64 key) {
        const float sv = __uint_as_float((unsigned)(key >> 32));
        return flat ? 0 : (int)__builtin_fminf((sv - mn) * scale, (float)(CAP - 1));
    };
    u64 kreg[PER];
    int breg[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = lane + 64 * k;
        kreg[k] = i < n ? L.keys[i] : ~0ull;
        breg[k] = bucket(kreg[k]);
    }
    wave_fence();
#pragma unroll
    for (int k = 0; k < PER; ++k)
        if (lane + 64 * k < n) atomicAdd(&L.hist[breg[k]], 1);
    wave_fence();
    int maxsize;
    {
        int c[PER], local = 0, cmax = 0;
        const int2 *h2 = reinterpret_cast<const int2 *>(&L.hist[lane * PER]);
#pragma unroll
        for (int k = 0; k < PER / 2; ++k) { const int2 v = h2[k]; c[2 * k] = v.x; c[2 * k + 1] = v.y; }
#pragma unroll
        for (int k = 0; k < PER; ++k) { local += c[k]; cmax = c[k] > cmax ? c[k] : cmax; }
        int run = wave_incl_add_dpp(local) - local;
        maxsize = wave_max_i32(cmax);
#pragma unroll
        for (int k = 0; k < PER; ++k) { const int t = c[k]; c[k] = run; run += t; }
        int2 *o2 = reinterpret_cast<int2 *>(&L.hist[lane * PER]);
#pragma unroll
        for (int k = 0; k < PER / 2; ++k) o2[k] = make_int2(c[2 * k], c[2 * k + 1]);
    }
    wave_fence();
#pragma unroll
    for (int k = 0; k < PER; ++k)
        if (lane + 64 * k < n) L.keys[atomicAdd(&L.hist[breg[k]], 1)] = kreg[k];     // every lane holds its keys: in place
    L.keys[n + lane] = ~0ull;
    wave_fence();   // hist[b] is now the END of bucket b
    const int per = (n + 63) >> 6;
    const int i0 = lane * per;
    u64 kq[PER];
    {
        int st[PER], rk[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const bool valid = k < per && i0 + k < n;
            kq[k] = valid ? L.keys[i0 + k] : ~0ull;
            const int b = bucket(kq[k]);
            st[k] = valid ? (b > 0 ? L.hist[b > 0 ? b - 1 : 0] : 0) : n;
            rk[k] = 0;
        }
        if (maxsize <= 64) {
            for (int t = 0; t < maxsize; ++t) {
#pragma unroll
                for (int k = 0; k < PER; ++k) rk[k] += L.keys[st[k] + t] < kq[k];
            }
        } else {      // a crowded bucket (clustered sums): same count with the reads clamped to the pad
            for (int t = 0; t < maxsize; ++t) {
#pragma unroll
                for (int k = 0; k < PER; ++k) { const int x = st[k] + t; rk[k] += L.keys[x < n ? x : n] < kq[k]; }
            }
        }
        wave_fence();
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (k < per && i0 + k < n) L.keys[st[k] + rk[k]] = kq[k];
        wave_fence();
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) kq[k] = (k < per && i0 + k < n) ? L.keys[i0 + k] : 0ull;
    // ---- equal sums: list order (pb_visit_less).  A lane looks at its own entries (registers) and at the two entries next
    // to them; the lane that owns the first entry of a run of equal sums puts the run in order.  (Not rare: a deep chunk
    // spans ~2 % of a binade, 377 sums among ~170 k floats collide in one chunk out of three.)
    {
        const unsigned sprev = i0 > 0 && i0 < n ? (unsigned)(L.keys[i0 - 1] >> 32) : 0xFFFFFFFFu;
        const unsigned snext = i0 + per < n ? (unsigned)(L.keys[i0 + per] >> 32) : 0xFFFFFFFFu;
        unsigned starts = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = i0 + k;
            if (k < per && i + 1 < n) {
                const unsigned sk = (unsigned)(kq[k] >> 32);
                const unsigned sn = (k + 1 < per) ? (unsigned)(kq[k + 1 < PER ? k + 1 : k] >> 32) : snext;
                const unsigned sp = k > 0 ? (unsigned)(kq[k > 0 ? k - 1 : 0] >> 32) : sprev;
                if (sn == sk && (i == 0 || sp != sk)) starts |= 1u << k;
            }
        }
        if (__ballot(starts != 0)) {
            bool degenerate = false;
            for (unsigned m = starts; m; m &= m - 1) {
                const int i = i0 + __builtin_ctz(m);
                const unsigned si = (unsigned)(L.keys[i] >> 32);
                int g = 2;
                while (i + g < n && g <= kPbMaxTie && (unsigned)(L.keys[i + g] >> 32) == si) ++g;
                if (g > kPbMaxTie) { degenerate = true; continue; }
                for (int a = 1; a < g; ++a) {
                    const u64 ka = L.keys[i + a];
                    const PbTep ta = pbw_tep((unsigned)ka);
                    int b = a;
                    while (b > 0 && pb_visit_less(L.w, ta, pbw_tep((unsigned)L.keys[i + b - 1]))) { L.keys[i + b] = L.keys[i + b - 1]; --b; }
                    L.keys[i + b] = ka;
                }
            }
            if (__ballot(degenerate)) return 2;
            wave_fence();
#pragma unroll
            for (int k = 0; k < PER; ++k) kq[k] = (k < per && i0 + k < n) ? L.keys[i0 + k] : 0ull;
        }
    }
    // ---- evaluate: lane l owns the entries [l per, (l + 1) per) of the sorted chunk.  Rolled loops with the per-entry
    // values in LDS (the costs go where the bucket counters were): as register arrays, fully unrolled, they and the 64 LUT
    // reads the scheduler then hoists cost ~390 VGPRs -- one wavefront per SIMD.
    float *const costs = reinterpret_cast<float *>(L.hist);
    const auto parity = [&](const PbTep &t) { return pb_tep_parity(L.P, d0, t); };
    float tmin = __builtin_inff();
    int tdel = 0;
    // (rolled loops over the lane's entries, read back from LDS: this path only runs for the first chunk or two of a frame
    //  -- pbw_scan_chunk takes the others -- and unrolled it is 8 k instructions of a kernel that should fit the I-cache)
#pragma unroll 1
    for (int k = 0; k < per; ++k) {
        const int i = i0 + k;
        if (i < n) {
            const u64 key = L.keys[i];
            const PbTep t = pbw_tep((unsigned)key);
            const float c = pbw_cost<CAP>(L, __uint_as_float((unsigned)(key >> 32)), parity(t), S.best);   // (+inf if it cannot beat the best)
            costs[i] = c;
            tmin = __builtin_fminf(tmin, c);
            tdel += pb_delta(t, P.order);
        }
    }
    // exclusive scans over the lanes: min of the costs / sum of the frontier growth before my entries
    const float imin = wave_incl_min_dpp(tmin);
    const int iadd = wave_incl_add_dpp(tdel);
    float before = __shfl_up(imin, 1, 64);
    if (lane == 0) before = __builtin_inff();
    before = __builtin_fminf(before, S.best);
    int nlb = iadd - tdel + S.nlive;
    const int tot_del = __builtin_amdgcn_readlane(iadd, 63);
    // ---- the sequential rules on my entries, assuming no earlier stop (`before` is the running best)
    int ones = 0, nev = 0, nnb = 0, lnb = -1, lstop = 0x7FFFFFFF, lreason = 0;
    float lbest = 0.0f;
    u64 lD = 0;
    unsigned lcode = 0;
#pragma unroll 1
    for (int k = 0; k < per; ++k) {
        const int i = i0 + k;
        if (i < n && lstop == 0x7FFFFFFF) {
            const u64 key = L.keys[i];
            const float c = costs[i];
            const PbTep t = pbw_tep((unsigned)key);
            float w1;
            const bool np = pb_not_promising(__uint_as_float((unsigned)(key >> 32)), before, Fr, P.c4, L.cdfA, L.cdfH, w1);
            ones += nlb == 1;
            nlb += pb_delta(t, P.order);
            if (np) { lstop = i; lreason = 1; }
            else {
                ++nev;
                if (c < before) {
                    const u64 D = parity(t);
                    before = c; lnb = i; ++nnb; lbest = c; lD = D; lcode = (unsigned)key;
                    if (pb_success_q(D, w1, L.qpar, Fr)) { lstop = i; lreason = 2; }
                }
            }
        }
    }
    const int gstop = wave_min_i32(lstop);
    {   // my entries count if they lie before (or contain) the first stop
        const bool mine = i0 < n && i0 <= gstop;
        const int o = wave_add_i32(mine ? ones : 0), e = wave_add_i32(mine ? nev : 0), b = wave_add_i32(mine ? nnb : 0);
        const int l = wave_max_i32(mine ? lnb : -1);
        const int npop = gstop != 0x7FFFFFFF ? gstop + 1 : n;
        S.cmp += 2 * npop - o; S.suc1 += e; S.suc2 += b;
        if (l >= 0) {   // the last improvement before the stop
            const int src = __builtin_ctzll(__ballot(mine && lnb == l));
            const unsigned code = (unsigned)__builtin_amdgcn_readlane((int)lcode, src);
            const u64 E = pb_tep_mask(pbw_tep(code));
            S.best = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lbest), src));
            S.bestD = readlane64(lD, src);
            S.bestE = E;
            S.bestidx = S.j + l + 1;
        }
        if (gstop != 0x7FFFFFFF) {
            const int src = __builtin_ctzll(__ballot(lstop == gstop));
            stop = __builtin_amdgcn_readlane(lreason, src);
            ntep = S.j + gstop + 1;
            return 1;
        }
    }
    S.j += n; S.nlive += tot_del;
    return 0;
}

}  // namespace ldpc
