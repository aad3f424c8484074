// PB-OSD stage 2, pb_wave_kernel: sorted chunks of the visit order, ONE FRAME of list A PER WAVEFRONT (round 3), continued from the
// head: chunks of <= 832 TEPs (4-byte keys, round 4), each = the members of a sum range walked directly from the sorted reliabilities,
// judged by a sort-free pass (pbw_scan4); what that cannot settle is redone over the same sum range with 8-byte keys, chunks of
// <= 384, and sorted if need be (pbw_redo_range, a real function).  Massive ties go to list B; a search that passes a budget of
// TEPs (chosen on the device from the number of searching frames) leaves with its state.  128 VGPRs (3 more spilled, 272 B of
// scratch), 10 080 B of LDS: four wavefronts per SIMD.  The workgroup kernel's solo path (ldpc_pb_coop.h) runs this code too.
//
// Round 2 ran this stage on 256- and 1024-thread workgroups: ~17 workgroup barriers per chunk, ~15 wave
// instructions per TEP, 60 % of the wave-cycles waiting (profiles/r03/pmc_counters_nms10_pb3_snr1.0_baseline_*).
// Here a frame belongs to ONE wavefront from its first chunk to its stop: no barrier anywhere (phases are
// separated by wave fences), the frame's search state lives in registers, ~9 frames are resident per CU and
// the dispatcher balances them (one wavefront per workgroup, compile-time LDS addresses).
//
// Here: the two real functions of the rare paths (pbw_sorted_chunk, pbw_redo_range) with their call sides, the record a long search
// leaves with (PbCarry) and the kernel.  The chunks and the walk: ldpc_pb_walk.h; the rules of the sort-free pass: ldpc_pb_rules.h;
// the two wavefront scans and the sorted path: ldpc_pb_pass.h.
#pragma once
#include "ldpc_pb_pass.h"

namespace ldpc {

// The sorted path as a FUNCTION (not inlined): it runs for the first chunk or two of a frame that arrives without its head,
// for 0.05 % of the chunks otherwise, and inlined it sets the register peak of every kernel that contains it (key, bucket, start
// and rank arrays of eight entries each).  Arguments and results travel through L.sa, so that nothing is live across the call
// but what the caller chooses to keep (the committed cursors are re-read from L.cur, which holds them after a commit).
template <int CAP>
__device__ __noinline__ void pbw_sorted_chunk(PbWaveLds<CAP> &L)
{
    const int lane = threadIdx.x & 63;
    PbParams P;
    P.order = L.sa.order; P.c4 = L.sa.c4;
    const PbFrame Fr = L.sa.fr;
    const u64 d0 = L.sa.d0;
    const int n = L.sa.n;
    const float mn = L.sa.mn, mx = L.sa.mx;
    PbwState S = L.sa.S;
    int stop = L.sa.stop, ntep = L.sa.ntep;
    wave_fence();
    const int state = pbw_process_chunk<CAP>(L, P, Fr, d0, n, mn, mx, lane, S, stop, ntep);
    wave_fence();
    if (lane == 0) { L.sa.S = S; L.sa.state = state; L.sa.stop = stop; L.sa.ntep = ntep; }
    wave_fence();
}
// caller's side: park, call, take back
template <int CAP>
__device__ __forceinline__ int pbw_sorted_call(PbWaveLds<CAP> &L, const PbParams &P, const PbFrame &Fr, u64 d0, int n, float mn, float mx, int lane,
                                               PbwState &S, int &stop, int &ntep)
{
    wave_fence();
    if (lane == 0) {
        L.sa.S = S; L.sa.fr = Fr; L.sa.d0 = d0; L.sa.mn = mn; L.sa.mx = mx; L.sa.c4 = P.c4; L.sa.n = n; L.sa.order = P.order;
        L.sa.stop = stop; L.sa.ntep = ntep;
    }
    wave_fence();
    pbw_sorted_chunk<CAP>(L);
    wave_fence();
    S = L.sa.S; stop = L.sa.stop; ntep = L.sa.ntep;
    return L.sa.state;
}

// The sums (lo, T] once more with 8-byte keys: chunks of <= CAP keys, the sort-free pass with the keys in registers
// (pbw_scan_chunk) and, where that cannot settle a chunk either, the sorted path.  For a chunk of 4-byte keys that pbw_scan4
// gave up on (many improvement candidates, a tie against a reference key, a frontier that may shrink to one entry) and for the
// workgroup kernel's fallback (coop_solo_range).  L.cur holds the cursors of the range's start; arguments and results in L.ra
// (state 0 / 1 / 2 as in pb_wave_kernel).  A real function: its code (two more passes, the sort) stays out of the hot loop.
template <int CAP>
__device__ __noinline__ void pbw_redo_range(PbWaveLds<CAP> &L)
{
    const int lane = threadIdx.x & 63;
    PbParams P;
    P.order = L.ra.order; P.c4 = L.ra.c4;
    const PbFrame Fr = L.ra.fr;
    const u64 d0 = L.ra.d0;
    const float Tcap = L.ra.T, smax = L.ra.smax;
    const int target = L.ra.target;
    float lo = L.ra.lo;
    int done = L.ra.done;
    const int end = done + L.ra.n;
    const int nall = P.order > 2 ? kPbTabSize : (P.order > 1 ? kPbTriples0 : kPbPairs0);
    PbwState S = L.ra.S;
    int stop = L.ra.stop, ntep = L.ra.ntep;
    wave_fence();
    PbWalk W;
    pbw_cursors_load<CAP>(L, W.ecur, lane);     // (the walk needs nothing but the cursors)
    float tprev = 0.0f, nprev = 0.0f;
    int state = 0;
    while (state == 0 && done < end) {
        float T;
        const int n = pbw_next_chunk<CAP, 0>(L, W, P.order, lo, done, nall, target, lane, T, tprev, nprev, Tcap);
        if (n <= 0) { state = 2; break; }
        wave_fence();
        const float cmn = lo < 0.0f ? L.w[63] : lo, cmx = T < __builtin_inff() ? T : smax;
        state = pbw_scan_chunk<CAP>(L, P, Fr, d0, n, cmn, cmx, lane, S, stop, ntep);
        if (state < 0) { state = pbw_sorted_call<CAP>(L, P, Fr, d0, n, cmn, cmx, lane, S, stop, ntep); pbw_cursors_load<CAP>(L, W.ecur, lane); }
        lo = T;
        done += n;
    }
    wave_fence();
    if (lane == 0) { L.ra.S = S; L.ra.state = state; L.ra.stop = stop; L.ra.ntep = ntep; }
    wave_fence();
}
// caller's side: park, call, take back (the caller has put the range's starting cursors into L.cur)
template <int CAP>
__device__ __forceinline__ int pbw_redo_call(PbWaveLds<CAP> &L, const PbParams &P, const PbFrame &Fr, u64 d0, float lo, float T, float smax, int done, int n,
                                             int lane, PbwState &S, int &stop, int &ntep)
{
    wave_fence();
    if (lane == 0) {
        L.ra.S = S; L.ra.fr = Fr; L.ra.d0 = d0; L.ra.lo = lo; L.ra.T = T; L.ra.smax = smax; L.ra.c4 = P.c4; L.ra.done = done; L.ra.n = n;
        L.ra.order = P.order; L.ra.target = CAP * 13 / 16; L.ra.stop = stop; L.ra.ntep = ntep;
    }
    wave_fence();
    pbw_redo_range<CAP>(L);
    wave_fence();
    S = L.ra.S; stop = L.ra.stop; ntep = L.ra.ntep;
    return L.ra.state;
}

// A long search handed from the chunk kernel to the workgroup kernel: ONE record per frame with everything the search needs,
// so that the receiving workgroup starts after a single wide load (its 1024 threads copy the record into LDS side by side)
// instead of the chain frame number -> source index -> permutation -> y that the chunk kernel went through:
//   words [0, 496)      the frame's tables as they stand in PbWaveLds (pad, w, P, zero row, cdfA, perm, tail, q), verbatim
//   words [496, 1008)   the committed cursors, [8][64]
//   words [1008, ...)   PbCarry: the search state (sums <= lo are visited) and the frame's scalars
struct PbCarry {
    float lo, best;
    int j, nlive, cmp, suc1, suc2, bestidx;
    u64 bestD, bestE;
    PbFrame fr;
    u64 d0, hm, hp;
    long long f;
    float tprev, nprev;      // the last chunk's lower bound and the TEPs before it (the growth exponent for the next bound)
};
constexpr int kPbFarProbe = 8;
constexpr int kPbRecPrefix = 496, kPbRecCur = 496, kPbRecScalars = 1008, kPbRecWords = 1040;
constexpr int kPbRecPerm = 330;       // (the permutation bytes inside the prefix: PbWaveLds::perm)
static_assert(kPbRecScalars * 4 % 8 == 0 && kPbRecScalars * 4 + sizeof(PbCarry) <= kPbRecWords * 4, "record layout");
static_assert(offsetof(PbWaveLds<kPbWaveCap>, cdfH) == kPbRecPrefix * 4 && offsetof(PbWaveLds<kPbWaveCap>, perm) == kPbRecPerm * 4, "the record's first part is the head of PbWaveLds");

// One frame of list A per wavefront, from its first TEP to its stop (or to the end of the table); massive ties go to
// list B (list replay).  Workgroup b serves sub-list b mod 16, entries b / 16, b / 16 + grid / 16, ... -- with the grid the
// launcher uses, ONE frame per workgroup: the hardware dispatcher then hands the next frame to whichever slot frees first.
// (Measured and dropped in round 4: persistent workgroups that draw their frames by ticket and fetch the next frame's list entry
//  and record while the current one is searched.  In-kernel stamps had put ~45 % of a wavefront's life into the dependent round
//  trips list entry -> record at a frame's start and the permutation / result stores at its end, and with the prefetch those
//  phases do vanish from the stamps -- but the launch got SLOWER: 359 -> 423 us at 2.5 dB, 5.03 -> 5.07 ms at 1.0 dB.  A frame
//  bound early to a wavefront that is busy with a long search starts late, and the launch is its tail: 3.4 frames per
//  resident wavefront at 2.5 dB; the other wavefronts of the SIMD had been hiding those round trips anyway.)
// (10 080 B of LDS per frame: 16 workgroups per CU; four wavefronts per SIMD asked of the register allocator: 128 VGPRs)
template <int CAP, int ROT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void pb_wave_kernel(PbParams P,
                                                     const double *__restrict__ cdf_half, int *__restrict__ ctl,
                                                     const int *__restrict__ listA, int *__restrict__ listB, int sub_cap,
                                                     unsigned *__restrict__ carry,
                                                     const unsigned *__restrict__ recs, PbOut O)
{
    __shared__ PbWaveLds<CAP> L;
    const int lane0 = threadIdx.x;
    const int sub = blockIdx.x & (kPbSub - 1);
    // (the sub-list's length and this workgroup's entry of it are asked for together -- entry k0 < sub_cap exists whatever the
    //  length says --, through vector loads: a scalar load whose result meets a branch is waited for where it is issued)
    int vz = 0;
    asm volatile("" : "+v"(vz));
    const int k0 = blockIdx.x >> 4;
    const int lenv = ctl[kPbCtlLenA + kPbCtlLine * sub + vz], f0v = listA[sub * sub_cap + k0 + vz];
    const int len = __builtin_amdgcn_readfirstlane(lenv);
    const int nall = P.order > 2 ? kPbTabSize : (P.order > 1 ? kPbTriples0 : kPbPairs0);      // TEPs of weight 1..order
    // TEPs after which a search may leave for the workgroup kernel: the fewer frames search, the sooner (a lone wavefront
    // takes ~30 us per chunk of ~400 TEPs, the workgroup ~12 us per chunk of ~2700; the schedule and its measurements: launch_pb)
    const int budget0 = len < 128 ? P.budget_s : (len < 448 ? P.budget_m : (len < 1400 ? P.budget : (len < 3000 ? P.budget_l : P.budget_xl)));
    bool have_cdfh = false;
    for (int k = k0; k < len; k += gridDim.x >> 4) {
        // (an opaque copy of the lane number per frame: otherwise every lane-dependent constant of the frame's code -- item
        //  geometry, the rank sort's tie masks -- is hoisted out of this loop, kept in registers for the whole kernel and spilled)
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        if (!have_cdfh) {
            L.cdfH[lane] = (float)cdf_half[lane];
            if (lane == 0) L.cdfH[64] = (float)cdf_half[64];
            if (lane < 4) L.pre[lane] = pbw_nan();
            have_cdfh = true;
        }
        // The launch's TAIL: once the dispatcher has no frame left to hand out, every search that goes on here keeps its CU
        // from idling only by itself -- the launch then lasts as long as the longest of them (measured with the frames sorted by
        // search length, which no product path can do: 260 -> 204 us at 2.5 dB, 3.62 -> 3.18 ms at 1.0 dB).  So the frames count
        // themselves out as they finish, and a search that finds (after a chunk) that fewer frames of its sub-list are unfinished
        // than late_pct % of the chip's wavefront slots -- the sub-lists advance side by side: workgroup b serves entry b / 16 of
        // sub-list b mod 16 -- leaves for the workgroup kernel after budget / late_div TEPs instead of budget.  WHERE a search is
        // handed on depends on timing then; what it returns does not (tests/test_gpu_osd_pb.py runs the kernels under several
        // schedules).
        int *const finished = &ctl[kPbCtlStartA + kPbCtlLine * sub];
        const bool tail_rule = len * kPbSub > P.late_min && len < P.late_maxlen;
        const int tail_budget = budget0 / P.late_div;
        const long long tail_slots = 4096ll * P.late_pct;       // (256 CUs x 16 wavefronts of this kernel, in per cent)
        const long long f = k == k0 ? __builtin_amdgcn_readfirstlane(f0v) : listA[sub * sub_cap + k];
        // ---- per-frame set-up: ONE wide load of the record pb_singles_kernel wrote (|y'|, P', the CDF table, the permutation: 356
        // words, copied into LDS as they are), the frame's scalars by scalar loads; derived here: the cost-bound table, the
        // success-rule factors
        const unsigned *const rec = recs + f * kPbR1Words;
        {
            const uint4 *const r4 = reinterpret_cast<const uint4 *>(rec);
            uint4 *const l4 = reinterpret_cast<uint4 *>(L.w);
            const uint4 a = r4[lane];
            uint4 b = make_uint4(0, 0, 0, 0);
            if (lane < 26) b = r4[64 + lane];
            l4[lane] = a;
            if (lane < 26) l4[64 + lane] = b;
        }
        const PbHead &H = *reinterpret_cast<const PbHead *>(rec + kPbR1Head);
        const PbFrame Fr = H.fr;
        const u64 d0 = H.d0;
        wave_fence();
        {   // pbw_cost_floor's table: every quarter's 16 parity weights in ascending order (rank sort inside the 16-lane row,
            // ties by position; no assumption on the order the caller's front end left them in), their running sums
            const float v = L.w[64 + lane];
            const int g0 = lane & 48;
            int r = 0;
#pragma unroll
            for (int u = 0; u < 16; ++u) { const float o = L.w[64 + g0 + u]; r += (o < v) || (o == v && g0 + u < lane); }
            float *const srt = reinterpret_cast<float *>(L.keys);
            srt[g0 + r] = v;
            L.qpar[lane] = 1.0f / (1.0f + det_expf(-(P.c4 * v)));            // sigmoid(c4 |y'_p|), as pb_frame_setup computes it
            wave_fence();
            float acc = srt[lane];
            acc = acc + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc), 0x111, 0xF, 0xF, true));   // row_shr:1,2,4,8:
            acc = acc + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc), 0x112, 0xF, 0xF, true));   // running sums
            acc = acc + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc), 0x114, 0xF, 0xF, true));   // inside a row
            acc = acc + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc), 0x118, 0xF, 0xF, true));
            L.tail[lane >> 4][(lane & 15) + 1] = acc * 0.99999f;
            if ((lane & 15) == 0) L.tail[lane >> 4][0] = 0.0f;
        }
        wave_fence();
        PbwState S;
        S.best = H.hbest;        // (the order-0 metric, or what the head made of it)
        S.j = 0; S.nlive = 1; S.cmp = 0; S.suc1 = 0; S.suc2 = 0; S.bestidx = 0; S.bestD = d0; S.bestE = 0;
        PbWalk W;
        pbw_walk_init<CAP>(L, W, P.order, lane);
        float lo = -1.0f;
        int done = 0;
        {   // go on where pb_singles_kernel stopped: the nhead least reliable singles are visited (every other sum is larger)
            const int nh = H.nhead;
            if (nh > 0) {
                S.j = nh; S.nlive = nh; S.cmp = 2 * nh - (nh < 2 ? nh : 2); S.suc1 = nh; S.suc2 = H.hsuc2;
                if (H.hsuc2 > 0) { S.bestidx = H.hbestidx; S.bestD = H.hbestD; S.bestE = H.hbestE; }
                lo = L.w[64 - nh]; done = nh;
                if (lane == 63)     // the singles are item 31 of lane 63: its cursor
                    W.ecur[7] = (W.ecur[7] & 0x00FFFFFFu) | ((unsigned)(64 - nh) << 24);
                L.cur[7][lane] = W.ecur[7];
            }
        }
        const float smax = P.order > 2 ? (L.w[0] + L.w[1]) + L.w[2] : (P.order > 1 ? L.w[0] + L.w[1] : L.w[0]);
        int stop = 0, ntep = P.nmax, state = 0;   // state: 0 = searching, 1 = a rule fired, 2 = to the list replay, 3 = to the workgroup kernel
        bool asked = false, firstc = true;       // (firstc: the frame's first chunk here -- its size is tuned apart, many searches end in it)
        float tprev = 0.0f, nprev = 0.0f;
        while (state == 0 && done < nall) {
            float T;
            // (the tail rule's counter, asked for here and looked at after the chunk: the round trip hides behind the walk)
            int nstarted = 0;
            if (tail_rule && !asked) nstarted = __hip_atomic_load(finished, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // a chunk of 4-byte keys (up to 2 CAP + 64 of them); W.ecur keeps the cursors it started from until it is judged
            const int n = pbw_next_chunk<CAP, ROT, true, false>(L, W, P.order, lo, done, nall, firstc ? P.t1 : P.t2, lane, T, tprev, nprev);
            firstc = false;
            if (n < 0) { state = 2; break; }
            if (n == 0) break;
            wave_fence();
            const float cmn = lo < 0.0f ? L.w[63] : lo, cmx = T < __builtin_inff() ? T : smax;
            state = pbw_scan4<CAP>(L, P, Fr, d0, n, cmn, cmx, lane, S, stop, ntep);
            if (state < 0) {     // not settled without a sort: the same sums once more, in chunks of 8-byte keys (a function call)
                pbw_cursors_store<CAP>(L, W.ecur, lane);
                state = pbw_redo_call<CAP>(L, P, Fr, d0, lo, T, smax, done, n, lane, S, stop, ntep);
            }
            pbw_cursors_load<CAP>(L, W.ecur, lane);          // commit (L.cur: the cursors behind the chunk, whoever walked it)
            lo = T;
            done += n;
            const int budget = (tail_rule && (long long)(len - nstarted) * kPbSub * 100 <= tail_slots) ? tail_budget : budget0;
            if (state == 0 && done >= budget && !asked && done < nall && len < P.handoff_maxlen) {
                // a long search: the workgroup kernel takes it over if it still has room (at most kPbCoopHalf frames per half of list C and call)
                asked = true;
                // The workgroup kernel's launch is as long as its last frame: it serves first the searches that will run far.
                // Rule 1 (acquire_prob_promising) against the best so far, at 64 sums between here and the largest sum: a
                // search whose rule cannot fire in the first kPbFarProbe of them goes into the first half of list C (an
                // improvement of the best only shortens a search: the long ones are all there).  Per search call, all in one
                // half / threshold 6 / 8 / 12 (means over four batches x 12 launches: single launches scatter by +-15 %, where a
                // search is handed on depends on timing): 2.5 dB 0.479 / 0.469 / 0.475 / 0.468 ms, 2.0 dB 0.988 / 0.963 / 0.955 / 0.970,
                // 1.0 dB 3.80 / 3.76 / 3.75 / 3.75.
                int far;
                {
                    const float rp = lo + (smax - lo) * ((float)(lane + 1) * (1.0f / 64.0f));
                    float w1;
                    const float bs = pb_promising_bs(rp, S.best, Fr, P.c4, L.cdfA, L.cdfH, w1);
                    const u64 fires = __ballot((double)bs < Fr.p_t_pro);
                    far = (fires ? __builtin_ctzll(fires) : 64) >= kPbFarProbe;
                }
                int slot = 0;
                if (lane == 0) slot = atomicAdd(&ctl[far ? kPbCtlLenC : kPbCtlLenC2], 1);
                slot = __builtin_amdgcn_readfirstlane(slot);
                if (slot < kPbCoopHalf) {
                    if (!far) slot += kPbCoopHalf;
                    unsigned *const crec = carry + (long long)slot * kPbRecWords;
                    const unsigned *const Lw = reinterpret_cast<const unsigned *>(&L);
                    for (int k = lane; k < kPbRecPrefix; k += 64) crec[k] = Lw[k];
#pragma unroll
                    for (int k = 0; k < 8; ++k) crec[kPbRecCur + k * 64 + lane] = W.ecur[k];
                    if (lane == 0) {
                        PbCarry c;
                        c.lo = lo; c.best = S.best; c.j = S.j; c.nlive = S.nlive; c.cmp = S.cmp; c.suc1 = S.suc1; c.suc2 = S.suc2;
                        c.bestidx = S.bestidx; c.bestD = S.bestD; c.bestE = S.bestE;
                        c.fr = Fr; c.d0 = d0; c.hm = H.hm; c.hp = H.hp; c.f = f; c.tprev = tprev; c.nprev = nprev;
                        *reinterpret_cast<PbCarry *>(crec + kPbRecScalars) = c;
                    }
                    state = 3;
                }
            }
        }
        if (state == 2) {   // massive ties: the literal list replay decodes this frame
            if (lane == 0) listB[atomicAdd(&ctl[kPbCtlLenB], 1)] = (int)f;
        } else if (state != 3) {   // candidate (E = flipped MRB positions, D = parity discrepancy) -> codeword in ORIGINAL bit order
            if (lane < 2) L.cw[lane] = 0;
            wave_fence();
            const int o1 = L.perm[lane], o2 = L.perm[64 + lane];       // (original bit index of primed positions lane, 64 + lane)
            const u64 mrb_bits = H.hm ^ S.bestE, par_bits = S.bestD ^ H.hp;
            if ((mrb_bits >> lane) & 1) atomicOr(&L.cw[o1 >> 6], 1ull << (o1 & 63));
            if ((par_bits >> lane) & 1) atomicOr(&L.cw[o2 >> 6], 1ull << (o2 & 63));
            wave_fence();
            if (lane < 2) O.cw[f * 2 + lane] = L.cw[lane];
            if (lane == 0) {
                if (O.metric) O.metric[f] = S.best;
                if (O.best) O.best[f] = S.bestidx;
                if (O.ntep) O.ntep[f] = ntep;
                if (O.aux) { O.aux[f * 4] = S.cmp; O.aux[f * 4 + 1] = S.suc1; O.aux[f * 4 + 2] = S.suc2; O.aux[f * 4 + 3] = stop; }
            }
        }
        if (lane == 0) atomicAdd(finished, 1);
        wave_fence();
    }
}

}  // namespace ldpc
