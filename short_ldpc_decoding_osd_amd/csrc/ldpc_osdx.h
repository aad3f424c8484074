// OSD for short codes of any shape (1 <= k <= 64, 1 <= n - k <= 64): the front end and the conventional order-p table scan
// with the code's n and k as kernel arguments, one frame per wavefront.
//   swapped_info / identify_mrb / full_gf2elim   PB_OSD/pb_testing.py:231-320
//   convention_osd_main                           FS_OSD/convention_osd.py:49-76
// Layout of a frame on the wavefront: lane l owns sorted column l (live for l < k) and sorted column k + l (live for
// l < n - k); idle slots carry zero columns, zero weights and zero rows, so every ballot, XOR reduction and LUT sum of the
// (128,64) kernels keeps its meaning with the split at k.  The helpers of ldpc_wave.h / ldpc_search.h are used unchanged.
// osdx_prepare / osdx_finish are the per-frame prologue and epilogue every search on such front-end results shares (the FS scan
// and the one-TEP kernel: ldpc_osdx_fs.h).
#pragma once

#include "ldpc_search.h"

namespace ldpc {

struct __attribute__((aligned(16))) FrontXLds {
    RankLds rank;            // reliability sort (bucket_ranks, ldpc_wave.h)
    u64 colbuf[64];          // parity columns in primed order (zero beyond n - k)
    unsigned mask[4];        // 128-bit membership mask of the MRB's sorted positions
    unsigned char pi1[128];  // sorted position -> original bit
    unsigned char rowsrc[64];
    unsigned char perm[128]; // primed position -> original bit (zero beyond n)
};

// (the elimination, gex_columns: ldpc_wave.h)

// ---------------------------------------------------------------------------------------
// front end: reliability sort, column gather, elimination, MRB / LRB bookkeeping
//   perm_out   [F][128] u8 : original bit at primed position p (MRB 0..k-1, parity k..n-1), 0 for p >= n
//   parity_out [F][64] u64 : row r < k, bit c < n - k = P'[r][c]; 0 elsewhere
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void osdx_front_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const u64 *__restrict__ Gcols, unsigned char *__restrict__ perm_out, u64 *__restrict__ parity_out,
        int *__restrict__ nswaps)
{
    __shared__ FrontXLds L;   // one wavefront per workgroup
    const int lane = threadIdx.x;
    const int m = n - k;
    const long long nframes = frame_count(count, F);

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        // ---- reliability sort: rank of each |y| in descending order, ties -> lower index ------
        // Slots lane and 64 + lane hold original bits lane and 64 + lane; a slot at or beyond n takes the magnitude 0.  Its key
        // (0, 127 - slot) is then distinct from and smaller than every real key -- a real zero has a lower index, hence a
        // larger low word -- whatever the frame holds, so the real bits take ranks 0..n-1 and the order among them is the
        // one the 128 distinct keys of bucket_ranks define.
        const unsigned a1 = lane < n ? (__float_as_uint(y[src * n + lane]) & 0x7FFFFFFFu) : 0u;
        const unsigned a2 = 64 + lane < n ? (__float_as_uint(y[src * n + 64 + lane]) & 0x7FFFFFFFu) : 0u;
        const float bs = bucket_scale(a1, a2);
        int r1, r2;
        bucket_ranks(L.rank, ((u64)a1 << 32) | (unsigned)(127 - lane), ((u64)a2 << 32) | (unsigned)(63 - lane), bucket_of(a1, bs),
                     bucket_of(a2, bs), lane, r1, r2);
        L.pi1[r1] = (unsigned char)lane;
        L.pi1[r2] = (unsigned char)(lane + 64);
        if (lane < 4) L.mask[lane] = 0;
        L.colbuf[lane] = 0ull;
        L.perm[lane] = 0; L.perm[lane + 64] = 0;
        wave_fence();
        // ---- G with columns in sorted order, column-major ------------------------------------
        const bool live1 = lane < k, live2 = lane < m;
        u64 C1 = live1 ? Gcols[L.pi1[lane]] : 0ull;
        u64 C2 = live2 ? Gcols[L.pi1[k + lane]] : 0ull;
        int rho = lane, idx1 = lane, idx2 = k + lane;
        const int ns = gex_columns(C1, C2, rho, idx1, idx2, k, lane);
        // ---- identify_mrb bookkeeping (:276-304): both index sets ascending ------------------
        if (live1) atomicOr(&L.mask[idx1 >> 5], 1u << (idx1 & 31));
        wave_fence();
        const unsigned mk[4] = {L.mask[0], L.mask[1], L.mask[2], L.mask[3]};
        const int rankM = below_mask(mk, idx1);         // new MRB position of slot `lane`
        const int rankL = idx2 - below_mask(mk, idx2);  // new parity column of slot `lane`
        if (live1) {
            L.perm[rankM] = L.pi1[idx1];
            L.rowsrc[rankM] = (unsigned char)rho;       // pivot of MRB slot `lane` is physical row rho
        }
        if (live2) {
            L.perm[k + rankL] = L.pi1[idx2];
            L.colbuf[rankL] = C2;
        }
        wave_fence();
        const u64 R = transpose64(L.colbuf[lane], lane);   // lane = physical row, bit = parity column
        const u64 Prow = shfl64(R, live1 ? L.rowsrc[lane] : lane);
        perm_out[f * 128 + lane] = L.perm[lane];
        perm_out[f * 128 + 64 + lane] = L.perm[64 + lane];
        parity_out[f * 64 + lane] = live1 ? Prow : 0ull;
        if (nswaps && lane == 0) nswaps[f] = ns;
        wave_fence();
    }
}

// ---------------------------------------------------------------------------------------
// per-frame prologue and epilogue of every search on front-end results of any shape (search_prepare / search_finish of
// ldpc_search.h with the split at k).  Idle lanes (lane >= k, lane >= n - k) stay out of the hard-decision ballots -- their
// y = 0 would count as a hard 1 --, rows of P' are masked to n - k columns, and w[] is zero beyond the live positions.
//   LDS: SearchLds (LUTS = true: the eight byte LUTs over w[64..] are built) or SearchLdsLean (LUTS = false).
// ---------------------------------------------------------------------------------------
struct OsdxFrame {
    u64 hm, hp, d0;       // hard decisions (y' > 0 ? 0 : 1) of the MRB / the parity part, order-0 discrepancy
    int o1, o2;           // original bit of primed positions lane / k + lane
    bool live1, live2;    // lane < k, lane < n - k
};

template <bool LUTS = true, class LDS = SearchLds>
__device__ __forceinline__ OsdxFrame osdx_prepare(LDS &L, const float *__restrict__ y, long long src, const unsigned char *__restrict__ perm_in,
                                                  const u64 *__restrict__ parity_in, long long f, int n, int k, int lane)
{
    OsdxFrame S;
    const int m = n - k;
    const u64 colmask = m >= 64 ? ~0ull : ((1ull << m) - 1ull);
    S.live1 = lane < k; S.live2 = lane < m;
    S.o1 = perm_in[f * 128 + lane]; S.o2 = perm_in[f * 128 + k + lane];   // (k + lane <= 127)
    const float y1 = S.live1 ? y[src * n + S.o1] : 0.0f, y2 = S.live2 ? y[src * n + S.o2] : 0.0f;
    L.w[lane] = __builtin_fabsf(y1);
    L.w[lane + 64] = __builtin_fabsf(y2);
    const u64 Prow = S.live1 ? (parity_in[f * 64 + lane] & colmask) : 0ull;
    L.P[lane] = Prow;
    if (lane < 2) L.cw[lane] = 0;
    S.hm = __ballot(S.live1 && !(y1 > 0.0f));
    S.hp = __ballot(S.live2 && !(y2 > 0.0f));
    wave_fence();
    if constexpr (LUTS) build_byte_luts<8>(L.lut, &L.w[64], lane);
    // d0 = (u0 . P') ^ h_parity : XOR-reduce the rows selected by the MRB hard decisions
    S.d0 = wave_xor64(((S.hm >> lane) & 1) ? Prow : 0ull) ^ S.hp;
    wave_fence();
    return S;
}

// candidate (E = flipped MRB positions, D = parity discrepancy) -> codeword in ORIGINAL bit order, ceil(n / 64) words; L.cw
// holds it afterwards (the callers compare it with the label before their closing wave_fence)
template <class LDS>
__device__ __forceinline__ void osdx_finish(LDS &L, const OsdxFrame &S, u64 E, u64 D, long long f, int words, int lane, u64 *__restrict__ cw_out)
{
    const u64 mrb_bits = S.hm ^ E, par_bits = D ^ S.hp;
    if (S.live1 && ((mrb_bits >> lane) & 1)) atomicOr(&L.cw[S.o1 >> 6], 1ull << (S.o1 & 63));
    if (S.live2 && ((par_bits >> lane) & 1)) atomicOr(&L.cw[S.o2 >> 6], 1ull << (S.o2 & 63));
    wave_fence();
    if (lane < words) cw_out[f * words + lane] = L.cw[lane];
}

// ---------------------------------------------------------------------------------------
// conventional order-p search over the reference's TEP table for THIS k (the scan of osd_search_kernel, split at k)
//   SearchLds: w[0..k-1] = |y'| of the MRB, w[64..64+n-k-1] = |y'| of the parity part, zero elsewhere; the eight byte LUTs
//   then hold the sums of np_oracle._weighted_distance_k (bytes of eight positions from primed position k, each ascending
//   from 0.0f: a padded position adds 0.0f, which changes no bit of a sum >= 0).
//   cw_out [F][words] u64, words = ceil(n / 64); label [*][words] addressed through `index`.
//   counts[3] += {frames, frames_wrong, teps_total} (with label; teps_total only with ntep_out): one atomic per counter and
//   wavefront, after its last frame.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void osdx_search_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, int n, int k, const unsigned char *__restrict__ perm_in, const u64 *__restrict__ parity_in,
        const uchar4 *__restrict__ teps, int ntep, u64 *__restrict__ cw_out, float *__restrict__ metric_out, int *__restrict__ best_out,
        int *__restrict__ ntep_out, const u64 *__restrict__ label, u64 *__restrict__ counts)
{
    __shared__ SearchLds L;   // one wavefront per workgroup: compile-time LDS base for the LUT reads
    const int lane = threadIdx.x;
    const int words = (n + 63) >> 6;
    const long long nframes = frame_count(count, F);
    unsigned long long seen = 0, wrong = 0, nteps = 0;

    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        const long long src = index ? index[f] : f;
        const OsdxFrame S = osdx_prepare(L, y, src, perm_in, parity_in, f, n, k, lane);
        const u64 d0 = S.d0;
        // scan the TEP table, one TEP per lane per round; strict '<' keeps the first minimum
        float best = __builtin_inff();
        int bestt = 0x7FFFFFFF;
        u64 bestD = 0, bestE = 0;
        float bound = __builtin_inff();   // exact early exit on the metric prefix (tep_cost_bounded): the wave's best so far
        int trip = 0;
        for (int t0 = 0; t0 < ntep; t0 += 64, ++trip) {
            const int t = t0 + lane;
            if (t < ntep) {
                u64 D, E;
                float mrb, c;
                tep_apply(L, teps[t], d0, D, E, mrb);
                if (tep_cost_bounded(L, mrb, D, bound, c) && c < best) { best = c; bestt = t; bestD = D; bestE = E; }
            }
            if ((trip & 7) == 0) bound = wave_min_f32(best);
        }
        wave_argmin(best, bestt, bestD, bestE, lane);
        osdx_finish(L, S, bestE, bestD, f, words, lane, cw_out);
        store_results(f, lane, best, bestt, ntep, metric_out, best_out, ntep_out);
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
