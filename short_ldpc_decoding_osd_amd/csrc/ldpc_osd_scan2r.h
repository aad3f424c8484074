// OSD kernels: the conventional order-2 scan with rotation pairing (the headline configuration) -- osd_search2r_kernel on the
// front-end results of a workspace, osd_fused2r_kernel with the front end in the same wavefront.
// Order-2 scan, second form (the one the launcher uses when the wave_rol probe succeeded):
//  * pairing by ROTATION: in round r = 1..32 lane l meets lane (l -+ r) mod 64, whose low word of P' and weight
//    arrive by two `wave_rol:1` DPP moves of a rotating copy -- no v_readlane (8 issue cycles each, six per
//    round in the triangular pairing of ldpc_osd_scan2.h) and no selects; rounds 1..31 cover every unordered pair once per
//    lane, round 32 pairs l with l +- 32 and only lanes < 32 count;
//  * persistent workgroups (one wavefront each) stride over the frames, and the global inputs of frame
//    f + 2 grid (perm, P' row) and f + grid (channel values, addressed through its perm) are in flight while
//    frame f is scanned, so the ~2 us of dependent global latency of the prologue is hidden;
//  * everything else (two-stage scan with the exact prefix bound, survivor ring, rank-ordered ties) as in ldpc_osd_scan2.h.
#pragma once

#include "ldpc_front.h"
#include "ldpc_osd_scan2.h"

namespace ldpc {

// LDS of the rotation scan: the byte LUT, the survivor ring and the rows of P', 9.5 KiB -> 16 workgroups = 4 wavefronts per
// SIMD (the scan is occupancy-sensitive: 1.75x the time at half the residency).  The parity weights are only needed while
// the LUT is built and the codeword words only after the last survivor batch, so both borrow the ring's memory.
struct __attribute__((aligned(16))) Search2rLds {
    float lut[8][256];   // lut[b][v] = sum of |y'[64+8b+t]| over the set bits t of v, ascending t
    uint2 q[128];        // survivors: prefix metric bits, r * 64 + lane (the candidate is rebuilt from P)
    u64 P[64];           // rows of P' (survivor batches rebuild D = d0 ^ P[l] ^ P[partner])
    __device__ __forceinline__ float *wpar() { return reinterpret_cast<float *>(q); }           // [64], before the scan
    __device__ __forceinline__ u64 *cw() { return reinterpret_cast<u64 *>(q) + 32; }            // [2], after the scan
};
static_assert(sizeof(Search2rLds) <= 10240, "LDS budget of the rotation scan");

__device__ __forceinline__ float cost2r(const Search2rLds &L, float mrb, u64 D)
{
    float acc = mrb;
    acc = acc + lut_byte<0>(L.lut, D); acc = acc + lut_byte<1>(L.lut, D); acc = acc + lut_byte<2>(L.lut, D); acc = acc + lut_byte<3>(L.lut, D);
    acc = acc + lut_byte<4>(L.lut, D); acc = acc + lut_byte<5>(L.lut, D); acc = acc + lut_byte<6>(L.lut, D); acc = acc + lut_byte<7>(L.lut, D);
    return acc;
}

__device__ __forceinline__ int wave_rot1(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x134, 0xF, 0xF, true); }

// (DIR: the probed direction of wave_rol:1, +1 or -1 -- a template parameter of the rotation kernels, so the partner of a
//  survivor is an add or a subtract; as a kernel argument it was a v_mul_lo_u32 per batch and lane)
template <int DIR>
__device__ __forceinline__ void search2r_finish_batch(const Search2rLds &L, uint2 e, bool valid, u64 d0, const int *__restrict__ base2,
                                                      float &best, int &bi, int &bj, u64 &bestD)
{
    static_assert(DIR == 1 || DIR == -1, "wave_rol:1 direction");
    if (!valid) return;
    const int r = (int)(e.y >> 6), l = (int)(e.y & 63), m = (DIR > 0 ? l - r : l + r) & 63;
    const u64 D = d0 ^ L.P[l] ^ L.P[m];
    float acc = __uint_as_float(e.x);
    acc = acc + lut_byte<2>(L.lut, D); acc = acc + lut_byte<3>(L.lut, D); acc = acc + lut_byte<4>(L.lut, D);
    acc = acc + lut_byte<5>(L.lut, D); acc = acc + lut_byte<6>(L.lut, D); acc = acc + lut_byte<7>(L.lut, D);
    if (!(acc <= best)) return;
    search2_take(acc, l < m ? l : m, l < m ? m : l, D, base2, best, bi, bj, bestD);
}

// Stage-1 state of the rotation scan between rounds (wave-uniform: bound, qn)
struct Scan2r {
    float m, t0, t1;     // round r: |y'_l| + |y'_partner| and the LUT terms of parity bytes 0 and 1 (read one round ahead)
    float bound;         // smallest complete metric seen by any lane
    int plo, wr;         // rotating copies of P'.lo and |y'| (bits)
    int qn;              // survivors waiting in q[0 .. qn)
};

// Round R of stage 1.  Software pipeline: the two LUT reads of round R + 1 are issued before round R is finished, so their
// LDS latency (bank conflicts included) overlaps the survivor bookkeeping -- at 4 wavefronts per SIMD nothing else hides
// it.  Returns true when the ring holds a full batch.  (R is a constant: the caller's round loop is unrolled.)
__device__ __forceinline__ bool search2r_round(Search2rLds &LL, Scan2r &s, int R, unsigned dlo, float wl, int lane)
{
    float mn = 0.0f, u0 = 0.0f, u1 = 0.0f;
    if (R < 32) {
        s.plo = wave_rot1(s.plo); s.wr = wave_rot1(s.wr);
        const unsigned Dn = dlo ^ (unsigned)s.plo;
        mn = wl + __int_as_float(s.wr); u0 = lut_byte<0>(LL.lut, Dn); u1 = lut_byte<1>(LL.lut, Dn);
    }
    float acc = s.m + s.t0;                                                   // |y'_i| + |y'_j| (commutative), then byte 0
    acc = acc + s.t1;
    s.m = mn; s.t0 = u0; s.t1 = u1;
    const bool keep = (R < 32 || lane < 32) && !(acc > s.bound);             // round 32: l and l +- 32 meet twice
    const u64 km = __ballot(keep);
    if (!km) return false;
    if (keep) {
        const int slot = wave_lane_rank(km, (unsigned)s.qn);
        LL.q[slot] = make_uint2(__float_as_uint(acc), (unsigned)(R * 64 + lane));
    }
    s.qn += __popcll(km);
    return s.qn >= 64;
}

// Stage 1 carries only what it reads: the low word of the candidate (parity bytes 0 and 1) and the partner's weight travel
// round the wavefront (two DPP moves per round); a survivor is stored as (prefix metric, r * 64 + lane) and its batch rebuilds
// the whole candidate from the P' rows in LDS.  The 32 rounds are unrolled (round number, id and the half-lane rule of round
// 32 are constants, no loop counter, no pipeline copies).  The ring is not circular: a batch takes slots 0..63 and moves the < 64 entries behind them
// down to slot 0, so an append is "slot = qn + mbcnt" with no wrap-around.
template <int DIR>
__device__ __forceinline__ void search2r_device(Search2rLds &LL, const SearchFrame &S, u64 Pl, float wl,
                                                const int *__restrict__ base2, int lane, float &best_out, int &rank_out,
                                                u64 &D_out, u64 &E_out)
{
    Search2rLds &L = LL;
    LL.P[lane] = Pl;     // read only by the survivor batches, after a wave_fence
    float best;
    int bi, bj;
    u64 bestD;
    search2_start([&](float mrb, u64 D) { return cost2r(L, mrb, D); }, S.d0, Pl, wl, lane, best, bi, bj, bestD);
    const unsigned dlo = (unsigned)(S.d0 ^ Pl);
    Scan2r s;
    s.bound = wave_min_f32(best);
    s.qn = 0;
    s.plo = wave_rot1((int)(unsigned)Pl); s.wr = wave_rot1(__float_as_int(wl));
    s.m = wl + __int_as_float(s.wr);
    s.t0 = lut_byte<0>(L.lut, dlo ^ (unsigned)s.plo); s.t1 = lut_byte<1>(L.lut, dlo ^ (unsigned)s.plo);
#pragma unroll
    for (int r = 1; r <= 32; ++r) {
        if (search2r_round(LL, s, r, dlo, wl, lane)) {
            wave_fence();
            const uint2 e = LL.q[lane], rest = LL.q[64 + lane];
            s.qn -= 64;
            if (lane < s.qn) LL.q[lane] = rest;
            search2r_finish_batch<DIR>(L, e, true, S.d0, base2, best, bi, bj, bestD);
            s.bound = wave_min_f32(best);
            wave_fence();
        }
    }
    wave_fence();
    search2r_finish_batch<DIR>(L, LL.q[lane], lane < s.qn, S.d0, base2, best, bi, bj, bestD);
    wave_fence();
    int bestt = tep2_rank(bi, bj, base2);
    u64 bestE = (bi >= 0 ? 1ull << bi : 0ull) | (bj >= 0 ? 1ull << bj : 0ull);
    wave_argmin(best, bestt, bestD, bestE, lane);
    best_out = best; rank_out = bestt; D_out = bestD; E_out = bestE;
}

// The frame body of both rotation-paired order-2 kernels (osd_search2r_kernel, osd_fused2r_kernel): the scan of frame f on
// (o1, o2, P'[lane], y1 = y'[lane], y2 = y'[64 + lane]), its outputs, and -- with counts -- the wrong-codeword counter
// against lab (the label word of lane 0 / 1).
template <int DIR>
__device__ __forceinline__ void search2r_frame(Search2rLds &LL, int o1, int o2, u64 Pl, float y1, float y2, const int *base2,
                                               long long f, u64 lab, int lane, u64 *cw_out, float *metric_out, int *best_out,
                                               int *ntep_out, u64 *counts)
{
    SearchFrame S;
    S.o1 = o1; S.o2 = o2;
    const float w1 = __builtin_fabsf(y1), w2 = __builtin_fabsf(y2);
    LL.wpar()[lane] = w2;
    S.hm = __ballot(!(y1 > 0.0f));
    S.hp = __ballot(!(y2 > 0.0f));
    wave_fence();
    build_byte_luts<8>(LL.lut, LL.wpar(), lane);
    S.d0 = wave_xor64(((S.hm >> lane) & 1) ? Pl : 0ull) ^ S.hp;
    wave_fence();
    float best; int bestt; u64 bestD, bestE;
    search2r_device<DIR>(LL, S, Pl, w1, base2, lane, best, bestt, bestD, bestE);
    {   // search_finish, with the codeword words still in hand for the success test (convention_osd.py:65-66)
        const u64 mrb_bits = S.hm ^ bestE, par_bits = bestD ^ S.hp;
        u64 *const cw = LL.cw();
        if (lane < 2) cw[lane] = 0;
        wave_fence();
        if ((mrb_bits >> lane) & 1) atomicOr(&cw[S.o1 >> 6], 1ull << (S.o1 & 63));
        if ((par_bits >> lane) & 1) atomicOr(&cw[S.o2 >> 6], 1ull << (S.o2 & 63));
        wave_fence();
        const u64 word = lane < 2 ? cw[lane] : 0ull;
        if (lane < 2) cw_out[f * 2 + lane] = word;
        if (counts && __ballot(lane < 2 && word != lab) && lane == 0) atomicAdd(&counts[1], 1ull);
        wave_fence();
    }
    store_results(f, lane, best, bestt, 2081, metric_out, best_out, ntep_out);
}

// The OSD success counters ride along when the caller wants them (ldpc_pipeline_run): {frames, wrong, TEPs};
// frames and TEPs are known up front, a wrong codeword costs one fire-and-forget atomic (~6 % of the frames).
// (Called between the read of *count and the first prefetch.)
__device__ __forceinline__ void count_up_front(u64 *__restrict__ counts, long long nframes, const int *ntep_out, int lane)
{
    if (counts && blockIdx.x == 0 && lane == 0) {
        atomicAdd(&counts[0], (u64)nframes);
        if (ntep_out) atomicAdd(&counts[2], (u64)nframes * 2081ull);       // TEPs only with d_ntep, as osd_counts_kernel
    }
}

// Frame assignment is static (frame = block + k grid).  Dynamic hand-out was measured and dropped: a device-scope
// ticket word saturates at ~88 fetch-adds per us (MI355X_MICROARCH.md, "dequeue") and a returning atomic takes
// microseconds under load -- every frame through ONE ticket word: 551 us; through 16 words on their own 128-byte
// lines, result awaited at once: 213 us; the last 40 % of the frames through 16 words, drawn a whole scan before
// they are looked at: 129 us; static: 102 us (the wavefronts are then alive for ~63 % of the launch: the scan time
// varies with the number of survivors) -- so the balance comes from the hardware dispatcher instead: the grid is 6x
// the resident wavefronts (see the launcher).
template <int DIR>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void osd_search2r_kernel(const float *__restrict__ y,
        const int *__restrict__ index, const int *__restrict__ count, long long F, const unsigned char *__restrict__ perm_in,
        const u64 *__restrict__ parity_in, const int *__restrict__ base2, u64 *__restrict__ cw_out, float *__restrict__ metric_out,
        int *__restrict__ best_out, int *__restrict__ ntep_out, const u64 *__restrict__ label, u64 *__restrict__ counts)
{
    __shared__ Search2rLds LL;
    const int lane = threadIdx.x;
    const long long nframes = frame_count(count, F);
    count_up_front(counts, nframes, ntep_out, lane);
    // software pipeline over the frames of this workgroup: (o, P) two frames ahead, y one frame ahead
    const long long G = gridDim.x;
    long long f0 = blockIdx.x, f1 = f0 + G, f2 = f1 + G;
    int o1a = 0, o2a = 0, o1b = 0, o2b = 0;
    u64 Pa = 0, Pb = 0;
    long long srca = 0, srcb = 0;
    float y1a = 0.0f, y2a = 0.0f;
    if (f0 < nframes) {
        o1a = perm_in[f0 * 128 + lane]; o2a = perm_in[f0 * 128 + 64 + lane]; Pa = parity_in[f0 * 64 + lane];
        srca = index ? index[f0] : f0;
    }
    if (f1 < nframes) {
        o1b = perm_in[f1 * 128 + lane]; o2b = perm_in[f1 * 128 + 64 + lane]; Pb = parity_in[f1 * 64 + lane];
        srcb = index ? index[f1] : f1;
    }
    u64 laba = 0;
    if (f0 < nframes) { y1a = y[srca * 128 + o1a]; y2a = y[srca * 128 + o2a]; if (label && lane < 2) laba = label[srca * 2 + lane]; }
    while (f0 < nframes) {
        // issue the loads of the frames ahead (they are consumed one / two trips later)
        float y1b = 0.0f, y2b = 0.0f;
        u64 labb = 0;
        if (f1 < nframes) { y1b = y[srcb * 128 + o1b]; y2b = y[srcb * 128 + o2b]; if (label && lane < 2) labb = label[srcb * 2 + lane]; }
        int o1c = 0, o2c = 0;
        u64 Pc = 0;
        long long srcc = 0;
        if (f2 < nframes) {
            o1c = perm_in[f2 * 128 + lane]; o2c = perm_in[f2 * 128 + 64 + lane]; Pc = parity_in[f2 * 64 + lane];
            srcc = index ? index[f2] : f2;
        }
        // ---- frame f0
        search2r_frame<DIR>(LL, o1a, o2a, Pa, y1a, y2a, base2, f0, laba, lane, cw_out, metric_out, best_out, ntep_out, counts);
        // ---- rotate the pipeline
        f0 = f1; f1 = f2; f2 += G;
        o1a = o1b; o2a = o2b; Pa = Pb; srca = srcb; y1a = y1b; y2a = y2b; laba = labb;
        o1b = o1c; o2b = o2c; Pb = Pc; srcb = srcc;
    }
}

// ---------------------------------------------------------------------------------------
// ldpc_osd_decode / ldpc_pipeline_run for the conventional order-2 OSD when the caller does not ask for the front-end
// results: front end AND scan of a frame in ONE wavefront, back to back -- the permutation, the rows of P' and the primed
// channel values pass from one to the other in registers and LDS and never touch memory.  Two launches moved 640 B of
// workspace per frame out and in again and read y twice (PMC, round 3: 41 + 49 MB per 33.5 k frames against 18 MB
// algorithmic: 5.1x); this form reads 512 B and writes 24 B per frame.  The front end's 3.1 KiB of LDS lie inside the
// scan's LUT area (built afterwards), the frame's y row in its P' rows (filled afterwards): 9.5 KiB, 16 wavefronts per CU.
// ---------------------------------------------------------------------------------------
template <int DIR>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void osd_fused2r_kernel(const float *__restrict__ y,
        const int *__restrict__ index, const int *__restrict__ count, long long F, const u64 *__restrict__ Gcols,
        const int *__restrict__ base2, u64 *__restrict__ cw_out, float *__restrict__ metric_out, int *__restrict__ best_out,
        int *__restrict__ ntep_out, const u64 *__restrict__ label, u64 *__restrict__ counts)
{
    __shared__ Search2rLds LL;
    static_assert(sizeof(FrontLds) <= sizeof(LL.lut), "the front end works inside the LUT area");
    FrontLds &LF = *reinterpret_cast<FrontLds *>(LL.lut);
    float *const yrow = reinterpret_cast<float *>(LL.P);            // the frame's y row in the P' table (filled by the scan)
    const int lane = threadIdx.x;
    long long nframes = F;      // (frame_count() written out: through the helper this kernel's instructions are scheduled differently)
    if (count) { const long long c = *count; nframes = c < F ? c : F; }
    count_up_front(counts, nframes, ntep_out, lane);
    // software pipeline over the frames of this workgroup: the frame number two frames ahead, the y row one frame ahead
    const long long G = gridDim.x;
    long long f0 = blockIdx.x, f1 = f0 + G, f2 = f1 + G;
    long long srca = 0, srcb = 0;
    float ya1 = 0.0f, ya2 = 0.0f;
    u64 laba = 0;
    if (f0 < nframes) srca = index ? index[f0] : f0;
    if (f1 < nframes) srcb = index ? index[f1] : f1;
    if (f0 < nframes) { ya1 = y[srca * 128 + lane]; ya2 = y[srca * 128 + 64 + lane]; if (label && lane < 2) laba = label[srca * 2 + lane]; }
    while (f0 < nframes) {
        float yb1 = 0.0f, yb2 = 0.0f;
        u64 labb = 0;
        if (f1 < nframes) { yb1 = y[srcb * 128 + lane]; yb2 = y[srcb * 128 + 64 + lane]; if (label && lane < 2) labb = label[srcb * 2 + lane]; }
        long long srcc = 0;
        if (f2 < nframes) srcc = index ? index[f2] : f2;
        // ---- frame f0: front end
        yrow[lane] = ya1; yrow[64 + lane] = ya2;
        const FrontResult fr = front_device_vals(LF, __float_as_uint(ya1) & 0x7FFFFFFFu, __float_as_uint(ya2) & 0x7FFFFFFFu, Gcols, lane);
        const float y1 = yrow[fr.o1], y2 = yrow[fr.o2];            // y'[p] = y[perm[p]]
        wave_fence();
        // ---- scan
        search2r_frame<DIR>(LL, fr.o1, fr.o2, fr.Prow, y1, y2, base2, f0, laba, lane, cw_out, metric_out, best_out, ntep_out, counts);
        f0 = f1; f1 = f2; f2 += G;
        srca = srcb; srcb = srcc; ya1 = yb1; ya2 = yb2; laba = labb;
    }
}

}  // namespace ldpc
