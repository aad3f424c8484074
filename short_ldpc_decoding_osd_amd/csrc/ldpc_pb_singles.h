// PB-OSD stage 1, pb_singles_kernel: the weight-1 head of the pop sequence, one frame per wavefront, one TEP per lane.  The
// sequence starts with the weight-1 TEPs {63}, {62}, ... while |y'_p| < |y'_62| + |y'_63| (the smallest weight-2 sum).  Two thirds
// of the frames stop here at 2.5 dB; the others are appended to list A, each with ONE 1536-byte record that holds everything its
// search needs (round 4).  72 VGPRs and 4.7 KiB of LDS (FUSED: 70 VGPRs + 4 spilled, 5.7 KiB).
//   mode 0: normal; 1: every frame straight to list A (block kernel); 2: every frame to list B (list replay)
#pragma once
#include "ldpc_pb_common.h"

namespace ldpc {

template <bool FUSED>
struct PbSinglesLdsT {
    SearchLdsLean s;     // no byte LUTs: the kernel evaluates two candidates per frame and lane, and it answers to occupancy
    double cdfA[65], cdfH[65];
    float q[128];
    union {
        float2 pairs[4][64];      // pb_frame_setup's chain operands ...
        float2 tq[64];            // ... then the success rule's factors
    };
};
// FUSED: the OSD front end of the frame runs in this kernel first (ldpc_osd_decode's route: nothing goes through a workspace);
// its scratch lies under the tables that are filled afterwards, the frame's channel row beside it.
template <>
struct PbSinglesLdsT<true> {
    SearchLdsLean s;
    double cdfH[65];
    float yrow[128];
    union {
        FrontLds front;
        struct {
            double cdfA[65];
            float q[128];
            union {
                float2 pairs[4][64];
                float2 tq[64];
            };
        };
    };
};

// (seven wavefronts per SIMD asked of the register allocator: 72 VGPRs, no scratch -- with the loads of a frame's start issued
//  together the kernel took 81 VGPRs and five per SIMD, 89 us instead of 84; at seven 80 us; at eight, 64 VGPRs + 9 spilled, 81 us)
// (one wavefront per workgroup, 4.8 KiB of LDS each: the register count decides how many are resident.  With the searches' 8 KiB
//  of LUTs it was 11.2 KiB and 14 per CU; padded to 10 per CU the kernel took 130 instead of 98 us per 33 k frames.)
template <bool FUSED = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(7))) void pb_singles_kernel(const float *__restrict__ y, const int *__restrict__ index,
                                                         const int *__restrict__ count, long long F,
                                                         const unsigned char *__restrict__ perm_in,
                                                         const u64 *__restrict__ parity_in, const u64 *__restrict__ Gcols, PbParams P, int mode,
                                                         const double *__restrict__ cdf_half,
                                                         int *__restrict__ ctl, int *__restrict__ listA, int *__restrict__ listB, int sub_cap,
                                                         unsigned *__restrict__ recs, PbOut O)
{
    __shared__ PbSinglesLdsT<FUSED> W;
    const int lane = threadIdx.x;
    SearchLdsLean &L = W.s;
    long long nframes = F;
    const long long wave = blockIdx.x;
    if (mode == 2) {   // every frame to the list replay, in frame order
        nframes = frame_count(count, F);
        for (long long f = wave * 64 + lane; f < nframes; f += (long long)gridDim.x * 64) listB[f] = (int)f;
        if (wave == 0 && lane == 0) ctl[kPbCtlLenB] = (int)nframes;
        return;
    }
    // A wavefront serves one frame (two for a few) and half of its life used to be the chain count -> frame number -> permutation
    // and P' -> y (in-kernel stamps, round 4): every load that does not depend on another is now issued before the first
    // is waited for -- the frame's operands are read for f < F (the buffers hold F frames) and dropped if the count says less.
    // (The wave-uniform words -- frame number, count -- go through VECTOR loads, an opaque zero in the address: a scalar load is
    //  waited for where it is issued once its result meets a branch, and three of them in a row were three round trips.)
    int vz = 0;
    asm volatile("" : "+v"(vz));
    for (long long f = wave; f < nframes; f += gridDim.x) {      // (nframes = F until the first frame's loads are out)
        int o1 = 0, o2 = 0;
        u64 Pr = 0;
        if constexpr (!FUSED) { o1 = perm_in[f * 128 + lane]; o2 = perm_in[f * 128 + 64 + lane]; Pr = parity_in[f * 64 + lane]; }
        int srcv = (int)f;
        if (index) srcv = index[f + vz];
        if (f == wave) {
            const double ch = cdf_half[lane], ch64 = cdf_half[64 + vz];
            int cv = 0x7FFFFFFF;
            if (count) cv = count[vz];
            W.cdfH[lane] = ch;
            if (lane == 0) W.cdfH[64] = ch64;
            const long long c = __builtin_amdgcn_readfirstlane(cv);
            nframes = c < F ? c : F;
            wave_fence();
        }
        if (f >= nframes) break;
        const long long src = __builtin_amdgcn_readfirstlane(srcv);
        SearchFrame S;
        if constexpr (FUSED) {
            // the frame's row as it lies in memory (two coalesced loads), the front end on it, then y' = y[perm] out of LDS
            const float ya = y[src * 128 + lane], yb = y[src * 128 + 64 + lane];
            W.yrow[lane] = ya; W.yrow[64 + lane] = yb;
            const FrontResult fr = front_device_vals(W.front, __float_as_uint(ya) & 0x7FFFFFFFu, __float_as_uint(yb) & 0x7FFFFFFFu, Gcols, lane);
            wave_fence();
            S = search_prepare_vals<false>(L, W.yrow[fr.o1], W.yrow[fr.o2], fr.o1, fr.o2, fr.Prow, lane);
        } else {
            S = search_prepare_regs<false>(L, y, src, o1, o2, Pr, lane);
        }
        const float best0 = tep_cost_direct_uniform(L.w, 0.0f, S.d0, lane);
        const PbFrame Fr = pb_frame_setup(L.w, W.q, W.cdfA, P.c4, P.order, P.nmax, lane, best0, &W.pairs[0][0]);
        wave_fence();
        pb_success_terms(W.q, W.tq, lane);
        wave_fence();
        // lane l <-> TEP {63 - l}, visit index l; valid while its weight is below the smallest weight-2 sum
        // (mode 1, the cross-check route "every frame through the chunk kernel from its first TEP": no head at all)
        const int p = 63 - lane;
        const float rs = L.w[p];
        const float s2min = L.w[62] + L.w[63];
        const u64 vmask = mode == 1 ? 0ull : __ballot(P.order == 1 || rs < s2min);
        const int nhead = (~vmask) ? __builtin_ctzll(~vmask) : 64;
        const bool valid = lane < nhead;
        const u64 D = S.d0 ^ L.P[p];
        const float cost = valid ? tep_cost_direct(L.w, rs, D) : __builtin_inff();
        const float incl = wave_incl_min_dpp(cost);
        float before = __shfl_up(incl, 1, 64);
        before = lane == 0 ? best0 : __builtin_fminf(before, best0);
        float w1;
        const bool stop1 = valid && pb_not_promising(rs, before, Fr, P.c4, W.cdfA, W.cdfH, w1);
        const bool newbest = valid && cost < before;
        bool stop2 = false;
        if (newbest) stop2 = pb_success(D, w1, W.tq, Fr);
        const u64 sm = __ballot(stop1 || stop2);
        if (sm == 0 && (P.order > 1 || mode == 1)) {   // no rule fired on the head: the chunk kernel takes the frame, with ONE record
            unsigned *const R = recs + f * kPbR1Words;
            R[lane] = __float_as_uint(L.w[lane]); R[64 + lane] = __float_as_uint(L.w[64 + lane]);
            reinterpret_cast<u64 *>(R + 128)[lane] = L.P[lane];
            if (lane < 2) R[kPbR1Zero + lane] = 0u;
            R[kPbR1Cdf + lane] = __float_as_uint((float)W.cdfA[lane]);
            if (lane < 4) R[kPbR1Cdf + 64 + lane] = lane == 0 ? __float_as_uint((float)W.cdfA[64]) : 0u;
            if (lane < 32) R[kPbR1Perm + lane] = reinterpret_cast<const unsigned *>(L.perm)[lane];
            {   // the head's result: nhead TEPs popped and evaluated, the last improvement among them (if any)
                const u64 nbm = __ballot(newbest);
                float hb = best0;
                u64 hD = S.d0, hE = 0;
                int hidx = 0;
                if (nbm) {
                    const int lb = 63 - __builtin_clzll(nbm);
                    hb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cost), lb));
                    hD = readlane64(D, lb); hE = 1ull << (63 - lb); hidx = lb + 1;
                }
                if (lane == 0) {
                    PbHead h;
                    h.fr = Fr; h.d0 = S.d0; h.hm = S.hm; h.hp = S.hp; h.hbestD = hD; h.hbestE = hE;
                    h.hbest = hb; h.nhead = nhead; h.hsuc2 = __popcll(nbm); h.hbestidx = hidx;
                    *reinterpret_cast<PbHead *>(R + kPbR1Head) = h;
                    const int sl = (int)f & (kPbSub - 1);
                    listA[sl * sub_cap + atomicAdd(&ctl[kPbCtlLenA + kPbCtlLine * sl], 1)] = (int)f;
                }
            }
            continue;
        }
        const int ls = sm ? __builtin_ctzll(sm) : 63;                 // (order 1 without a stop: all 64 TEPs visited)
        const int reason = sm ? (((__ballot(stop1) >> ls) & 1) ? 1 : 2) : 0;
        const int npop = ls + 1;
        const int nev = reason == 1 ? ls : ls + 1;
        const u64 nbm = __ballot(newbest) & (nev >= 64 ? ~0ull : ((1ull << nev) - 1));
        float best = best0;
        u64 bestD = S.d0, bestE = 0;
        int bestidx = 0;
        if (nbm) {
            const int lb = 63 - __builtin_clzll(nbm);
            best = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cost), lb));
            bestD = readlane64(D, lb);
            bestE = 1ull << (63 - lb);
            bestidx = lb + 1;
        }
        // frontier sizes before the pops: 1, 1, 2, 3, ... (order > 1) or always 1 (order 1)
        const int ones = P.order > 1 ? (npop < 2 ? npop : 2) : npop;
        pb_write(L, S, O, f, lane, bestE, bestD, best, bestidx, sm ? npop : P.nmax, 2 * npop - ones, nev, __popcll(nbm), reason);
    }
}

}  // namespace ldpc
