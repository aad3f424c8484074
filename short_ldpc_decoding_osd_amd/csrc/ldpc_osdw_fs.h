// OSD for high-rate short codes: osdw_fs_kernel and osdw_tep_eval_kernel.
// FS-OSD (fs_osd, FS_OSD/fs_testing.py:129-161) with the control flow of osdx_fs_kernel (ldpc_osdx_fs.h) -- 64 TEPs per round, a
// ballot for the first tau_e hit, an arg-min over the lanes before it, only those lanes counted in num_teps, both quirk modes
// -- on SearchWLds: 128 rows of P' and 128 MRB weights, the lower bound of weight w summed over w[k-w .. k-1] wherever that
// range lies, HD = w + popcount(D), the visit-order table of this k <= 127 (classes 1..min(3, k)).
// No flip mask is carried through the scan (it would be two words per lane): the winner and the stopping candidate are
// remembered as table positions and their flipped positions read from their entries after the scan, as osdw_search_kernel does
// with teps[best].  The per-frame prologue and epilogue are osdw_prepare / osdw_finish below; the metric is tepw_apply
// (ldpc_osdw.h) and tep_cost / tep_cost_bounded of ldpc_search.h (the float order of np_oracle._weighted_distance_k).
#pragma once

#include "ldpc_osdw.h"

namespace ldpc {

struct __attribute__((aligned(16))) SearchWLdsLean {   // the same without the byte LUTs (1.8 KiB instead of 9.8)
    u64 P[128];
    float w[192];
    u64 cw[2];
};

// ---------------------------------------------------------------------------------------
// per-frame prologue and epilogue of the FS scan and the one-TEP kernel (osdx_prepare / osdx_finish of ldpc_osdx.h with two MRB
// slots per lane).  They are the prologue and epilogue of osdw_search_kernel (ldpc_osdw.h) word for word, as a COPY: with that
// kernel built on these helpers the compiler allocated it 59 vector registers instead of the 61 its measurements were taken
// with and, the scan loop the same instructions, the launch measured 0.8 % and 0.5 % above this text on CCSDS (128,64) in two
// alternating sessions, above the spread of this text's own runs (profiles/osd_scan_shared/README.md): it keeps its own text.
// Idle lanes (lane >= k, 64 + lane >= k, lane >= n - k) stay out of the hard-decision ballots -- their y = 0 would count as a
// hard 1 --, rows of P' are masked to n - k columns, and w[] is zero beyond the live positions.
//   LDS: SearchWLds (LUTS = true: the eight byte LUTs over w[128..] are built) or SearchWLdsLean (LUTS = false).
// ---------------------------------------------------------------------------------------
struct OsdwFrame {
    u64 hmA, hmB, hp, d0;       // hard decisions (y' > 0 ? 0 : 1) of MRB positions 0..63 / 64..127 / the parity part, order-0 discrepancy
    int oA, oB, oP;             // original bit of primed positions lane / 64 + lane / k + lane
    bool liveA, liveB, liveP;   // lane < k, 64 + lane < k, lane < n - k
};

template <bool LUTS = true, class LDS = SearchWLds>
__device__ __forceinline__ OsdwFrame osdw_prepare(LDS &L, const float *__restrict__ y, long long src, const unsigned char *__restrict__ perm_in,
                                                  const u64 *__restrict__ parity_in, long long f, int n, int k, int lane)
{
    OsdwFrame S;
    const int m = n - k;
    const u64 colmask = m >= 64 ? ~0ull : ((1ull << m) - 1ull);
    S.liveA = lane < k; S.liveB = 64 + lane < k; S.liveP = lane < m;
    S.oA = S.liveA ? perm_in[f * 128 + lane] : 0; S.oB = S.liveB ? perm_in[f * 128 + 64 + lane] : 0;
    S.oP = S.liveP ? perm_in[f * 128 + k + lane] : 0;
    const float yA = S.liveA ? y[src * n + S.oA] : 0.0f, yB = S.liveB ? y[src * n + S.oB] : 0.0f, yP = S.liveP ? y[src * n + S.oP] : 0.0f;
    L.w[lane] = __builtin_fabsf(yA);
    L.w[64 + lane] = __builtin_fabsf(yB);
    L.w[128 + lane] = __builtin_fabsf(yP);
    const u64 rowA = S.liveA ? (parity_in[f * 128 + lane] & colmask) : 0ull;
    const u64 rowB = S.liveB ? (parity_in[f * 128 + 64 + lane] & colmask) : 0ull;
    L.P[lane] = rowA;
    L.P[64 + lane] = rowB;
    if (lane < 2) L.cw[lane] = 0;
    S.hmA = __ballot(S.liveA && !(yA > 0.0f)); S.hmB = __ballot(S.liveB && !(yB > 0.0f));   // idle lanes stay out: y = 0 is a hard 1
    S.hp = __ballot(S.liveP && !(yP > 0.0f));
    wave_fence();
    if constexpr (LUTS) build_byte_luts<8>(L.lut, &L.w[128], lane);
    // d0 = (u0 . P') ^ h_parity : XOR-reduce the rows selected by the MRB hard decisions, two rows per lane
    S.d0 = wave_xor64((((S.hmA >> lane) & 1) ? rowA : 0ull) ^ (((S.hmB >> lane) & 1) ? rowB : 0ull)) ^ S.hp;
    wave_fence();
    return S;
}

// candidate (flipA / flipB: whether it flips MRB positions lane / 64 + lane, D = parity discrepancy) -> codeword in ORIGINAL
// bit order, ceil(n / 64) words; L.cw holds it afterwards (the callers compare it with the label before their closing
// wave_fence)
template <class LDS>
__device__ __forceinline__ void osdw_finish(LDS &L, const OsdwFrame &S, bool flipA, bool flipB, u64 D, long long f, int words, int lane,
                                            u64 *__restrict__ cw_out)
{
    const u64 par_bits = D ^ S.hp;
    if (S.liveA && ((((S.hmA >> lane) & 1) != 0) != flipA)) atomicOr(&L.cw[S.oA >> 6], 1ull << (S.oA & 63));
    if (S.liveB && ((((S.hmB >> lane) & 1) != 0) != flipB)) atomicOr(&L.cw[S.oB >> 6], 1ull << (S.oB & 63));
    if (S.liveP && ((par_bits >> lane) & 1)) atomicOr(&L.cw[S.oP >> 6], 1ull << (S.oP & 63));
    wave_fence();
    if (lane < words) cw_out[f * words + lane] = L.cw[lane];
}

//   counts[3] += {frames, frames_wrong, teps_total} (with label; teps_total sums the frame's own ntep, only with ntep_out): one
//   atomic per counter and wavefront, after its last frame.
__global__ __launch_bounds__(64) void osdw_fs_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const unsigned char *__restrict__ perm_in, const u64 *__restrict__ parity_in,
        const uchar4 *__restrict__ teps_fs, FsParams P, u64 *__restrict__ cw_out, float *__restrict__ metric_out,
        int *__restrict__ best_out, int *__restrict__ ntep_out, const u64 *__restrict__ label, u64 *__restrict__ counts)
{
    __shared__ SearchWLds L;   // one wavefront per workgroup: compile-time LDS base for the LUT reads
    const int lane = threadIdx.x;
    const int words = (n + 63) >> 6;
    const long long nframes = frame_count(count, F);
    unsigned long long seen = 0, wrong = 0, nteps = 0;

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        const OsdwFrame S = osdw_prepare(L, y, src, perm_in, parity_in, f, n, k, lane);
        float best = tep_cost(L, 0.0f, S.d0);      // all-zero TEP (:131)
        u64 bestD = S.d0, hitD = 0;
        float hitc = 0.0f;
        int bestidx = 0, ntep = 1, visited = 1, hitidx = 0;
        int bestpos = -1, hitpos = -1;              // position inside teps_fs; -1: the all-zero TEP
        bool hit = false;
        if (!((float)__popcll(S.d0) < P.tau_e)) {
            for (int w = 1; w <= P.order && !hit; ++w) {   // (the host keeps order <= min(3, k))
                float bsum = 0.0f;                  // w least reliable MRB values, ascending position (on either side of 64)
                for (int t = k - w; t < k; ++t) bsum = bsum + L.w[t];
                if (!(bsum + P.beta_term < best)) break;
                const int cnt = P.cls_cnt[w], off = P.cls_off[w];
                const uchar4 *tab = teps_fs + off;
                for (int t0 = 0; t0 < cnt && !hit; t0 += 64) {
                    const int t = t0 + lane;
                    const bool valid = t < cnt;
                    u64 D = 0;
                    float mrb = 0.0f;
                    if (valid) tepw_apply(L, tab[t], S.d0, D, mrb);
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
                        const int wl = wave_argmin_lane(cc, lane);
                        best = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cc), wl));
                        bestD = readlane64(D, wl);
                        bestidx = visited + t0 + wl; bestpos = off + t0 + wl;
                    }
                    if (stop) {
                        hit = true;
                        hitD = readlane64(D, lim);
                        hitc = tep_cost(L, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mrb), lim)), hitD);   // the stopping candidate's own metric
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
        osdw_finish(L, S, tep_flips(win, lane), tep_flips(win, 64 + lane), use_hit ? hitD : bestD, f, words, lane, cw_out);
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
// osdx_tep_eval_kernel with a two-word E.  mask [F][2]: bit p of word 0 flips MRB position p, bit p of word 1 position 64 + p;
// bits at or beyond k are ignored.  A frame evaluates one candidate, so there are no byte LUTs (SearchWLdsLean) and the metric
// is tep_cost_direct over the parity weights, the same additions in the same order.
__global__ __launch_bounds__(64) void osdw_tep_eval_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const unsigned char *__restrict__ perm_in, const u64 *__restrict__ parity_in,
        const u64 *__restrict__ mask, u64 *__restrict__ cw_out, float *__restrict__ metric_out, int *__restrict__ hd_out)
{
    __shared__ SearchWLdsLean L;
    const int lane = threadIdx.x;
    const int words = (n + 63) >> 6;
    const u64 rowsA = k >= 64 ? ~0ull : ((1ull << k) - 1ull);
    const u64 rowsB = k > 64 ? ((1ull << (k - 64)) - 1ull) : 0ull;   // (k <= 127)
    const long long nframes = frame_count(count, F);

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        const OsdwFrame S = osdw_prepare<false>(L, y, src, perm_in, parity_in, f, n, k, lane);
        const u64 E0 = mask[2 * f] & rowsA, E1 = mask[2 * f + 1] & rowsB;
        const bool flipA = ((E0 >> lane) & 1) != 0, flipB = ((E1 >> lane) & 1) != 0;
        const u64 D = S.d0 ^ wave_xor64((flipA ? L.P[lane] : 0ull) ^ (flipB ? L.P[64 + lane] : 0ull));
        float mrb = 0.0f;                                  // flipped MRB weights, ascending position, sequential
        for (u64 e = E0; e; e &= e - 1) mrb = mrb + L.w[__builtin_ctzll(e)];
        for (u64 e = E1; e; e &= e - 1) mrb = mrb + L.w[64 + __builtin_ctzll(e)];
        const float cost = tep_cost_direct(&L.w[64], mrb, D);   // (its parity weights start 64 floats in: w[128..] here)
        osdw_finish(L, S, flipA, flipB, D, f, words, lane, cw_out);
        if (lane == 0) {
            if (metric_out) metric_out[f] = cost;
            if (hd_out) hd_out[f] = __popcll(E0) + __popcll(E1) + __popcll(D);
        }
        wave_fence();
    }
}

}  // namespace ldpc
