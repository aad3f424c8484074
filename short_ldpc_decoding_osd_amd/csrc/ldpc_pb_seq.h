// PB-OSD stage 3, pb_seq_kernel: literal replay of the frontier list (round-1 kernel), one frame of list B per wavefront (frames
// whose sums tie massively, or every frame when the caller asks for this path as a cross-check): ~1.2 us per TEP.
#pragma once
#include "ldpc_pb_common.h"

namespace ldpc {

// (recs: the singles kernel's records, when the front end ran inside it and left nothing in a workspace: a frame of list B is
//  then set up from its record -- |y'|, P', the permutation, the hard decisions)
__global__ __launch_bounds__(256) void pb_seq_kernel(const float *__restrict__ y, const int *__restrict__ index,
                                                     const unsigned char *__restrict__ perm_in,
                                                     const u64 *__restrict__ parity_in, const unsigned *__restrict__ recs, PbParams P,
                                                     const double *__restrict__ cdf_half,
                                                     PbEntry *__restrict__ spill_all, long long spill_stride,
                                                     int *__restrict__ ctl, const int *__restrict__ listB, PbOut O)
{
    __shared__ SearchLds lds[4];
    __shared__ PbLds pbl[4];
    const int lane = threadIdx.x & 63;
    SearchLds &L = lds[threadIdx.x >> 6];
    PbLds &B = pbl[threadIdx.x >> 6];
    const int nlist = ctl[kPbCtlLenB];
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    PbEntry *spill = spill_all + wave * spill_stride;
    B.cdfH[lane] = cdf_half[lane];
    if (lane == 0) B.cdfH[64] = cdf_half[64];
    wave_fence();

    // frames are handed out through a device counter: run times differ by orders of magnitude between frames
    for (;;) {
        int fq = 0;
        if (lane == 0) fq = atomicAdd(&ctl[kPbCtlTicketB], 1);
        const int tk = __builtin_amdgcn_readfirstlane(fq);
        if (tk >= nlist) break;
        const long long f = listB[tk];
        SearchFrame S;
        if (recs) {
            const unsigned *const R = recs + f * kPbR1Words;
            const PbHead &H = *reinterpret_cast<const PbHead *>(R + kPbR1Head);
            const unsigned char *const pb = reinterpret_cast<const unsigned char *>(R + kPbR1Perm);
            S.o1 = pb[lane]; S.o2 = pb[64 + lane];
            L.perm[lane] = (unsigned char)S.o1; L.perm[lane + 64] = (unsigned char)S.o2;
            L.w[lane] = __uint_as_float(R[lane]); L.w[lane + 64] = __uint_as_float(R[64 + lane]);
            L.P[lane] = reinterpret_cast<const u64 *>(R + 128)[lane];
            if (lane < 2) L.cw[lane] = 0;
            S.hm = H.hm; S.hp = H.hp; S.d0 = H.d0;
            wave_fence();
            build_byte_luts<8>(L.lut, &L.w[64], lane);
            wave_fence();
        } else {
            const long long src = index ? index[f] : f;
            S = search_prepare(L, y, src, perm_in, parity_in, f, lane);
        }
        const PbFrame Fr = pb_frame_setup(L.w, B.q, B.cdfA, P.c4, P.order, P.nmax, lane);
        const float spl = Fr.spl, lrb_mean = Fr.lrb_mean;
        const double p_t_suc = Fr.p_t_suc, p_t_pro = Fr.p_t_pro;
        if (lane == 0) {   // starting point: the single TEP {k-1} (pb_testing.py:109-110)
            PbEntry e0; e0.sum = L.w[63]; e0.pos = 63u | (1u << 24); B.fr[0] = e0;
            PbEntry m0; m0.sum = e0.sum; m0.pos = 0; B.cmin[0] = m0; B.smin[0] = m0;
        }
        wave_fence();
        int nused = 1, nlive = 1, ntep = P.nmax, bestidx = 0, stop = 0, cmp = 0, suc1 = 0, suc2 = 0;
        int tail_ck = 0, tail_ci = 0, tail_sk = 0, tail_si = 0;   // last chunk / super-chunk of the list and their minima
        float tail_cs = L.w[63], tail_ss = L.w[63];
        float best = tep_cost(L, 0.0f, S.d0);
        u64 bestD = S.d0, bestE = 0;
        const PbList FL{&B, spill, P.cmin_off};
        for (int j = 0; j < P.nmax - 1 && nlive > 0; ++j) {
            // first minimum of the list = arg-min on (sum, slot), read off the super-chunk minima
            const int nsuper = (nused + 4095) >> 12;
            float ms = __builtin_inff();
            int mi = 0x7FFFFFFF;
            if (lane < nsuper) { const PbEntry t = B.smin[lane]; ms = t.sum; mi = (int)t.pos; }
            argmin_si(ms, mi, lane);
            cmp += nlive == 1 ? 1 : 2;
            // Both levels of the list that this pop touches are loaded NOW, side by side: the 64 slots of the
            // popped slot's chunk (lane mi & 63 of it is the popped entry itself) and the 64 chunk minima of its
            // super-chunk.  Everything that changes below (the tombstone, children that land in the same chunk,
            // the new chunk minimum) is patched into these registers, so one round trip to the spilled part of the
            // list (global memory) is on the critical path of a TEP instead of three dependent ones.
            const int ck0 = mi >> 6, sk0 = ck0 >> 6;
            PbEntry mys, myc;
            mys.sum = myc.sum = __builtin_inff(); mys.pos = 0; myc.pos = 0x7FFFFFFFu;
            if (ck0 * 64 + lane < nused) mys = FL.slot(ck0 * 64 + lane);
            if ((sk0 * 64 + lane) * 64 < nused) myc = FL.cmin(sk0 * 64 + lane);
            PbEntry e;
            e.sum = ms;
            e.pos = (unsigned)__builtin_amdgcn_readlane((int)mys.pos, mi & 63);
            const int ew = (int)(e.pos >> 24);
            const int p0 = e.pos & 0xFF, pA = (e.pos >> 8) & 0xFF, pB = (e.pos >> 16) & 0xFF;
            const int last = ew == 1 ? p0 : (ew == 2 ? pA : pB);
            const int prev = ew == 2 ? p0 : pA;     // second largest (ew > 1)
            // children (wave-uniform): extended e U {63}, adjacent = largest index moved down by one
            PbEntry c1, c2;
            c1.sum = c2.sum = __builtin_inff(); c1.pos = c2.pos = 0;
            bool has1 = false, has2 = false;
            if (last < 63 && ew < P.order) {
                c1.pos = (e.pos & 0x00FFFFFFu) | (63u << (8 * ew)) | ((unsigned)(ew + 1) << 24);
                c1.sum = e.sum + L.w[63];
                has1 = true;
            }
            if (ew > 1) {
                if (last - prev > 1) {
                    c2.pos = (e.pos & ~(0xFFu << (8 * (ew - 1)))) | ((unsigned)(last - 1) << (8 * (ew - 1)));
                    const int q0 = c2.pos & 0xFF, q1 = (c2.pos >> 8) & 0xFF, q2 = (c2.pos >> 16) & 0xFF;
                    float sacc = L.w[q0] + L.w[q1];
                    if (ew > 2) sacc = sacc + L.w[q2];
                    c2.sum = sacc;
                    has2 = true;
                }
            } else if (last - 1 > -1) {
                c2.pos = (unsigned)(last - 1) | (1u << 24);
                c2.sum = L.w[last - 1];
                has2 = true;
            }
            if (has2 && !has1) { c1 = c2; has1 = true; has2 = false; }      // children in list order: c1 then c2
            const int s1 = nused, s2 = nused + 1;
            if (lane == 0) {
                PbEntry dead;
                dead.sum = __builtin_inff(); dead.pos = 0;
                FL.set_slot(mi, dead);
                if (has1) FL.set_slot(s1, c1);
                if (has2) FL.set_slot(s2, c2);
            }
            nused += (has1 ? 1 : 0) + (has2 ? 1 : 0);
            nlive += (has1 ? 1 : 0) + (has2 ? 1 : 0) - 1;
            // ---- chunk level: the popped slot's chunk from the patched registers; the tail chunk incrementally
            if (lane == (mi & 63)) mys.sum = __builtin_inff();
            if (has1 && (s1 >> 6) == ck0 && lane == (s1 & 63)) mys = c1;
            if (has2 && (s2 >> 6) == ck0 && lane == (s2 & 63)) mys = c2;
            float cs0 = mys.sum;
            int ci0 = ck0 * 64 + lane;
            argmin_si(cs0, ci0, lane);
            if (lane == 0) { PbEntry m; m.sum = cs0; m.pos = (unsigned)ci0; FL.set_cmin(ck0, m); }
            if (ck0 == tail_ck) { tail_cs = cs0; tail_ci = ci0; }
            // ---- super-chunk level, same scheme on the chunk minima (patched as the chunk level changes them)
            if (lane == (ck0 & 63)) { myc.sum = cs0; myc.pos = (unsigned)ci0; }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const bool has = u == 0 ? has1 : has2;
                const int sl = u == 0 ? s1 : s2;
                const float csum = u == 0 ? c1.sum : c2.sum;
                if (!has) continue;
                const int ck = sl >> 6;
                if (ck != tail_ck) { tail_ck = ck; tail_cs = __builtin_inff(); tail_ci = 0x7FFFFFFF; }   // a new chunk starts
                if (ck == ck0) continue;                                   // covered by the reduction above
                if (csum < tail_cs) { tail_cs = csum; tail_ci = sl; }      // (a tie keeps the older, lower slot)
                if (lane == 0) { PbEntry m; m.sum = tail_cs; m.pos = (unsigned)tail_ci; FL.set_cmin(ck, m); }
                if ((ck >> 6) == sk0 && lane == (ck & 63)) { myc.sum = tail_cs; myc.pos = (unsigned)tail_ci; }
            }
            float ss0 = myc.sum;
            int si0 = (int)myc.pos;
            argmin_si(ss0, si0, lane);
            if (lane == 0) { PbEntry m; m.sum = ss0; m.pos = (unsigned)si0; B.smin[sk0] = m; }
            if (sk0 == tail_sk) { tail_ss = ss0; tail_si = si0; }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const bool has = u == 0 ? has1 : has2;
                const int sl = u == 0 ? s1 : s2;
                const float csum = u == 0 ? c1.sum : c2.sum;
                if (!has) continue;
                const int sk = sl >> 12;
                if (sk != tail_sk) { tail_sk = sk; tail_ss = __builtin_inff(); tail_si = 0x7FFFFFFF; }
                if (sk == sk0) continue;
                if (csum < tail_ss) { tail_ss = csum; tail_si = sl; }
                if (lane == 0) { PbEntry m; m.sum = tail_ss; m.pos = (unsigned)tail_si; B.smin[sk] = m; }
            }
            wave_fence();
            // promising-probability rule
            const float rs = e.sum;
            const float w1 = det_expf(P.c4 * rs) * spl, w2 = 1.0f - w1;
            const float bt = __builtin_floorf((best - rs) / lrb_mean);
            const int beta = bt > 0.0f ? (bt < 64.0f ? (int)bt : 64) : 0;
            float bs = 0.0f;
            bs = bs + w1 * (float)B.cdfA[beta];
            bs = bs + w2 * (float)B.cdfH[beta];
            if ((double)bs < p_t_pro) { stop = 1; ntep = j + 1; break; }
            u64 D = S.d0 ^ L.P[p0], E = 1ull << p0;
            if (ew > 1) { D ^= L.P[pA]; E |= 1ull << pA; }
            if (ew > 2) { D ^= L.P[pB]; E |= 1ull << pB; }
            const float cost = tep_cost(L, rs, D);
            ++suc1;
            if (cost < best) {
                best = cost; bestD = D; bestE = E; bestidx = j + 1;
                const float ratio = (1.0f - w1) / w1;
                float prod = 1.0f;
#pragma unroll 4
                for (int p = 0; p < 64; ++p) {
                    const float qp = B.q[64 + p];
                    prod = prod * (((D >> p) & 1) ? 2.0f * qp : 2.0f * (1.0f - qp));
                }
                const float p_suc = 1.0f / (1.0f + ratio / prod);
                ++suc2;
                if (p_suc > (float)p_t_suc) { stop = 2; ntep = j + 1; break; }
            }
        }
        pb_write(L, S, O, f, lane, bestE, bestD, best, bestidx, ntep, cmp, suc1, suc2, stop);
    }
}

}  // namespace ldpc
