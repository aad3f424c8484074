// PB-OSD stage 2c, pb_coop_kernel: the long searches pb_wave_kernel hands on, ONE WORKGROUP OF NW WAVEFRONTS PER FRAME (round 3);
// chunks of <= 4096 TEPs counted by bisection and generated once, every wavefront judging the keys it generated; one workgroup
// barrier per count and one per ordinary chunk.  The chunk pass of ldpc_pb_pass.h (above in the translation unit) needs no sort, so a
// chunk is embarrassingly parallel over its keys, and the walk is parallel over the item rows: wavefront v owns 32 / NW of
// the 32 rows (dealt so that light and heavy rows pair up), walks them into the workgroup's ONE key buffer (slots reserved by
// an LDS atomic per trip, so the buffer fills evenly whatever the rows give) and scans every NW-th 64-key slice of it.
// What the wavefronts exchange per chunk is a handful of numbers (counts, frontier growth, the smallest firing sum,
// positions) through LDS words and ~7 workgroup barriers; the order of the keys in the buffer depends on the wavefronts'
// timing, the results do not (the pass takes counts, minima and the candidates ordered by sum, a tie leaves it).  Everything a
// wavefront decides from the exchanged numbers it decides like the others (same values, same arithmetic), so the barriers
// line up by construction: no barrier stands inside control flow that depends on a wavefront's own keys.
// A chunk the sort-free pass cannot settle (a tie against a reference key, > 64 candidates, a frontier that may shrink to
// one entry) is redone by wavefront 0 alone with the single-wavefront code above (sorted path, sub-chunks of <= 512 keys up
// to the same bound), then the co-operation resumes.  Frames arrive from pb_wave_kernel with their search state and cursors.
#pragma once
#include "ldpc_pb_wave.h"

namespace ldpc {

constexpr int kCoopCap = 4096;        // keys of a chunk, all wavefronts together (8192 with a target of 6144 measured in round 4: fewer, longer
                                      // chunks -- per search call 0.428 -> 0.411 ms at 2.5 dB, 0.926 -> 0.941 at 2.0 dB, 3.75 -> 3.84 at 1.0 dB)
constexpr int kCoopMaxCand = 64;
// Wavefronts per frame: 16 (one frame per CU) or 8 (two).  Measured with 8 (round 4), workgroup kernel per
// launch / PB kernels per search call: 2.5 dB 120 -> 151 us / 0.426 -> 0.451 ms (the launch is its longest search, and a chunk
// takes eight wavefronts 1.25 x as long), 2.0 dB 270 -> 200 us / 0.945 -> 0.905 ms (throughput-bound: ~1900 searches),
// 1.5 dB 1.89 -> 1.89 ms, 1.0 dB 245 -> 252 us / 3.75 -> 3.74 ms (its tail again), 3.0 / 3.5 dB 0.287 -> 0.292 / 0.177 -> 0.186 ms.
constexpr int kPbCoopW = 16;
constexpr int kPbCoopGrid = 256 * 16 / kPbCoopW;      // workgroups (frames are handed out by ticket): what the chip holds at once

template <int NW>
struct __attribute__((aligned(16))) PbCoopLds {
    static constexpr int NI = 32 / NW;                    // items per lane
    static constexpr int WK = 2 * kCoopCap / NW;          // keys of a chunk from one wavefront (an NW-th of the items +- 10 % when the chunk is full: half of this)
    PbWaveLds<kPbWaveCap> one;        // the frame's tables (tail, P, w, tq, cdf); the rest of it is wavefront 0's when it works alone
    u64 keys[kCoopCap];
    unsigned short slist[NW][WK];              // a wavefront's keys that the cost bound could not rule out
    uint4 desc[NW][64];                                    // a wavefront's items with members in the chunk (emission)
    u64 ck[kCoopMaxCand], rk[kCoopMaxCand];
    float cc[kCoopMaxCand], rc[kCoopMaxCand];
    int red[8][NW], red2[8][NW];
    int ncand[2], nrec, stop2, tie0, ticket[2];
    PbwState bs;                      // wavefront 0 -> all, after it worked alone
    int bstate, bstop, bntep;
    // What wavefront 0 holds in registers when it leaves for coop_solo_range, parked here and read back afterwards: a value
    // that is live across the call costs a callee-saved register or a scratch slot on EVERY path through the kernel (the
    // call alone took the kernel from 119 VGPRs and no scratch to 128 VGPRs and 101 spilled ones, reloaded inside the walk's
    // loops), a value that is stored before it and loaded after it costs nothing anywhere else.
    int sv[32 / NW][64];
    struct {
        PbFrame fr;
        u64 d0;
        float lo, T, tprev, nprev, smax;
        int done, n, seq, par, it, tk, next_tk;
    } su;
    PbParams sP;
};

template <int NW>
struct CoopRed {
    int (*buf)[NW];
    int seq, wave, lane, par;
};
// sum / minimum of one int per wavefront, the same value in every lane of every wavefront (one barrier; eight rotating slots:
// a slot is rewritten seven barriers after its last reader)
template <int NW>
__device__ __forceinline__ int coop_sum(CoopRed<NW> &R, int x)
{
    int *const s = R.buf[R.seq++ & 7];
    if (R.lane == 0) s[R.wave] = x;
    __syncthreads();
    int a = 0;
#pragma unroll
    for (int v = 0; v < NW; ++v) a += s[v];
    return a;
}
template <int NW>
__device__ __forceinline__ int coop_min(CoopRed<NW> &R, int x)
{
    int *const s = R.buf[R.seq++ & 7];
    if (R.lane == 0) s[R.wave] = x;
    __syncthreads();
    int a = s[0];
#pragma unroll
    for (int v = 1; v < NW; ++v) a = s[v] < a ? s[v] : a;
    return a;
}

// The 2048 items (row q, lane l) are dealt to the wavefronts by (5 l + 3 q) mod 16: every wavefront holds four items of
// every row, spread over the lanes, and a chunk's keys come from the sixteen wavefronts within ~10 % of each other
// (dealing whole rows: the fullest wavefront emits 1.4-1.9 times the mean, the others wait for it at every exchange).
// Item j (0, 1) of lane `lane` in wavefront v:
template <int NW>
__device__ __forceinline__ void coop_item(int v, int j, int lane, int &q, int &l)
{
    static_assert(NW == 16 || NW == 8, "the dealing is written for sixteen or eight wavefronts");
    if constexpr (NW == 16) {
        q = 16 * j + (lane >> 2);
        l = ((13 * (v - 3 * q)) & 15) + 16 * (lane & 3);        // 5 l = v - 3 q (mod 16), 5 * 13 = 1
    } else {            // (5 l + 3 q) mod 8: eight items of every row, four rows of a lane
        q = 8 * j + (lane >> 3);
        l = ((5 * (v - 3 * q)) & 7) + 8 * (lane & 7);           // 5 l = v - 3 q (mod 8), 5 * 5 = 1
    }
}

// A wavefront's items in registers: item j of this lane is (row q, lane l) = coop_item(v, j, lane); sb = the sum of its fixed
// positions, members are m in (base, 63] visited downwards from a - 1 (a = cursor: [a, 64) are visited), key = code | m << sh.
template <int NI>
struct CoopItems {
    float sb[NI];
    int base[NI], sh[NI], a[NI];
    unsigned code[NI];
};
template <int NW>
__device__ __forceinline__ void coop_items_init(CoopItems<32 / NW> &I, const float *w, int order, int lane, int wave)
{
#pragma unroll
    for (int j = 0; j < 32 / NW; ++j) {
        int q, l;
        coop_item<NW>(wave, j, lane, q, l);
        const PbwItem it = pbw_item_rt(q, l);
        const bool live = q < 31 ? order > 2 : (order > 1 || l == 63);
        I.sb[j] = q < 31 ? w[it.i] + w[it.j] : (l <= 62 ? w[l] : 0.0f);
        I.base[j] = live ? it.base : 64;      // (an item the order excludes: no members)
        I.sh[j] = it.sh; I.code[j] = it.code;
    }
}

// The members of every item with sum <= T beyond its cursor: sums fall as the position rises, so they are the positions
// [first, a) and `first` is found by bisection (7 steps of one LDS read, the items of a lane side by side).  Nothing is
// written: the count of a bound is a pure function of the cursors, a bound that gives too many or too few keys costs one
// more count, and the keys are generated once, for the bound that is taken (the round-3 list walk emitted as it went and
// rolled the cursors back: a chain of four dependent LDS round trips per 64 entries, ~2000 cycles each, and a list per wavefront).
template <int NI>
__device__ __forceinline__ void coop_count(const CoopItems<NI> &I, const float *w, float T, int (&first)[NI])
{
    int lo[NI], hi[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) { lo[j] = I.base[j] + 1; hi[j] = I.a[j]; }
#pragma unroll
    for (int s = 0; s < 7; ++s) {
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const bool act = lo[j] < hi[j];
            const int mid = (lo[j] + hi[j]) >> 1;
            const bool f = I.sb[j] + w[mid & 63] <= T;
            hi[j] = act && f ? mid : hi[j];
            lo[j] = act && !f ? mid + 1 : lo[j];
        }
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) first[j] = hi[j];
}

// The next chunk of the workgroup: the same bound T in every wavefront, sized by the SUM of their counts (one barrier per
// count), then the keys of (lo, T] into L.keys[0 .. n) -- wavefront v's behind those of the wavefronts before it, a lane's
// behind those of the lanes before it -- and the cursors advanced.  Returns n, -1: cannot be split, 0: nothing left;
// kbase / kcount: this wavefront's own keys (which it also scans: no barrier between the two).
template <int NW>
__device__ __forceinline__ int coop_next_chunk(PbCoopLds<NW> &L, CoopRed<NW> &R, CoopItems<32 / NW> &I, float lo, int done,
                                               int nall, int target, int lane, int wave, float &Tout, float &tprev, float &nprev, int &kbase, int &kcount)
{
    constexpr int NI = 32 / NW;
    const float inf = __builtin_inff();
    const float *w = L.one.w;
    const float m3 = (w[61] + w[62]) + w[63];
    const float want = (float)(done + target);
    float Tl = lo, Th = inf;
    float T = nall - done <= kCoopCap / 2 ? inf : m3 * pb_bound_guess(want);
    if (tprev > 0.0f && nprev > 0.0f && lo > tprev && (float)done > nprev && T < inf) {
        const float pe = (__builtin_amdgcn_logf((float)done) - __builtin_amdgcn_logf(nprev)) / (__builtin_amdgcn_logf(lo) - __builtin_amdgcn_logf(tprev));
        if (pe > 1.5f && pe < 20.0f) T = lo * __builtin_amdgcn_exp2f((__builtin_amdgcn_logf(want) - __builtin_amdgcn_logf((float)done)) / pe);
    }
    if (!(T > lo)) T = lo > 0.0f ? lo * 1.05f : w[0];
    float tp = lo, np_ = (float)done;
    int first[NI], slot = 0, tot = 0;
    float T_ok = lo;          // the largest bound counted so far that fits (tot_ok keys)
    int tot_ok = 0;
    bool last_ok = false;     // first / slot / tot describe T_ok
    for (int it = 0; it < 48; ++it) {
        coop_count<NI>(I, w, T, first);
        int c = 0;
#pragma unroll
        for (int j = 0; j < NI; ++j) c += I.a[j] - first[j];
        slot = R.seq & 7;
        {
            const int cw = wave_add_i32(c);
            tot = coop_sum<NW>(R, cw > PbCoopLds<NW>::WK ? cw + (1 << 24) : cw);     // (a wavefront scans its own keys: at most WK)
        }
        last_ok = false;
        bool over = false;
        if (tot > kCoopCap) {
            over = true;
            Th = T;
            if (tot_ok > 0 && it >= 3) break;        // (a usable smaller chunk is known: take it rather than search on)
        } else if (tot > 0 && (!(T < inf) || 5 * tot >= 2 * target || it >= 3)) {
            T_ok = T; tot_ok = tot; last_ok = true;
            break;
        } else if (!(T < inf)) {
            return 0;                                // everything that can be visited has been
        } else {
            if (tot > 0) { T_ok = T; tot_ok = tot; last_ok = true; }
            Tl = T;
        }
        float Tn;
        if (over) {
            Tn = Tl > 0.0f ? Tl + (Th - Tl) * 0.5f : Th * 0.9f;
        } else {
            const float totf = (float)(done + tot);
            float p = 6.0f;
            if (tp > 0.0f && np_ > 0.0f && totf != np_ && T != tp) {
                const float pe = (__builtin_amdgcn_logf(totf) - __builtin_amdgcn_logf(np_)) / (__builtin_amdgcn_logf(T) - __builtin_amdgcn_logf(tp));
                if (pe > 1.5f && pe < 20.0f) p = pe;
            }
            if (tot > 0) { tp = T; np_ = totf; }
            Tn = tot > 0 ? T * __builtin_amdgcn_exp2f((__builtin_amdgcn_logf(want) - __builtin_amdgcn_logf(totf)) / p) : T * 1.1f;
            if (it >= 6 || !(Tn > Tl) || !(Tn < Th)) Tn = Th < inf ? Tl + (Th - Tl) * 0.5f : T * 1.2f;
        }
        if (!(Tn > Tl) || !(Tn < Th)) break;
        T = Tn;
    }
    if (tot_ok == 0) return -1;
    if (!last_ok) {     // the bound taken is not the one counted last: count it again (rare)
        coop_count<NI>(I, w, T_ok, first);
        int c = 0;
#pragma unroll
        for (int j = 0; j < NI; ++j) c += I.a[j] - first[j];
        slot = R.seq & 7;
        tot = coop_sum<NW>(R, wave_add_i32(c));
    }
    kbase = 0;
#pragma unroll
    for (int v = 0; v < NW; ++v) kbase += v < wave ? L.red[slot][v] : 0;
    kcount = L.red[slot][wave];
    // ---- the keys.  Offsets: wavefronts before mine (the counts just exchanged), lanes before mine, my items in turn.
    int off = kbase;
    int o[NI], cj[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        cj[j] = I.a[j] - first[j];
        const int inc = wave_incl_add_dpp(cj[j]);
        o[j] = off + inc - cj[j];
        off += __builtin_amdgcn_readlane(inc, 63);
    }
    // Emission.  In a chunk ~26 of a wavefront's 128 items have members, ~6.5 each, at most ~15 (at 2.5 dB): a loop over the
    // member number would run at a quarter of the lanes, a loop over the items at a tenth.  So the items with members leave
    // a 16-byte descriptor in LDS (ballot + mbcnt), and every pass serves EIGHT of them, eight lanes each, a member per lane.
    uint4 *const desc = L.desc[wave];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const u64 am = __ballot(cj[j] > 0);
        const int na = __popcll(am);
        if (cj[j] > 0)
            desc[wave_lane_rank(am)] =
                make_uint4((unsigned)I.a[j] | ((unsigned)cj[j] << 8) | ((unsigned)I.sh[j] << 16), (unsigned)o[j], __float_as_uint(I.sb[j]), I.code[j]);
        wave_fence();
        for (int p0 = 0; p0 < na; p0 += 8) {
            const int it = p0 + (lane >> 3);
            if (it < na) {
                const uint4 d = desc[it];
                const int a_ = (int)(d.x & 255u), c_ = (int)((d.x >> 8) & 255u), sh_ = (int)(d.x >> 16);
                const float sb_ = __uint_as_float(d.z);
                for (int k = lane & 7; k < c_; k += 8) {
                    const int m = a_ - 1 - k;
                    L.keys[(int)d.y + k] = ((u64)__float_as_uint(sb_ + w[m]) << 32) | (d.w | ((unsigned)m << sh_));
                }
            }
        }
        wave_fence();
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) I.a[j] = first[j];
    tprev = lo; nprev = (float)done;
    Tout = T_ok;
    return tot_ok;
}

// pbw_scan_chunk for the workgroup: every wavefront scans the keys it generated (L.keys[kbase .. kbase + kcount)); the
// reductions go through LDS.  Returns 0 / 1 / -1 like pbw_scan_chunk, the same value in every wavefront; -1 leaves the
// state untouched.  The keys are not kept in registers: the ordinary chunk reads each once, the rare paths read them again.
template <int NW>
__device__ __forceinline__ int coop_scan_chunk(PbCoopLds<NW> &L, CoopRed<NW> &R, const PbParams &P, const PbFrame &Fr, u64 d0, int n, int kbase, int kcount,
                                               float mn, float mx, int lane, int wave, PbwState &S, int &stop, int &ntep)
{
    constexpr int CAP = kPbWaveCap, PER = PbCoopLds<NW>::WK / 64;
    const PbWaveLds<CAP> &T0 = L.one;
    if (S.nlive <= 1) return -1;
    const float best0 = S.best;
    const float r_safe = pb_rule1_safe_sum(mn, mx, best0, Fr, P.c4, T0.cdfA, T0.cdfH, lane);      // rule 1 by probes
    const auto parity = [&](const PbTep &t) { return pb_tep_parity(T0.P, d0, t); };
    const auto sumbits = [](u64 key) { return (unsigned)(key >> 32); };
    // a is visited before b (a != b): by sum, equal sums by the list-slot order (pb_visit_less: through the parents).  Round 4: a tie
    // against a reference key used to send the whole chunk, ~2700 keys, to wavefront 0 alone -- 1-4 times per launch at 2.5 dB,
    // 35-135 us each where the launch takes ~150.
    const auto visited_before = [&](u64 a, u64 b) {
        if (sumbits(a) != sumbits(b)) return sumbits(a) < sumbits(b);
        return pb_visit_less(T0.w, pbw_tep((unsigned)a), pbw_tep((unsigned)b));
    };
    const auto key_at = [&](int k) { const int i = k * 64 + lane; return i < kcount ? L.keys[kbase + i] : ~0ull; };   // (an empty slot: all ones, sum NaN)
    int sumdel = 0, neg = 0, nsurv = 0;
    unsigned fs = 0x7FFFFFFFu;     // the smallest sum on which rule 1 fires (against the chunk-start best)
    unsigned short *const slist = L.slist[wave];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (k * 64 < kcount) {      // (uniform: a wavefront holds ~n / NW keys, four or five slices of the eight)
            const u64 key = key_at(k);
            const bool valid = k * 64 + lane < kcount;
            const PbTep t = pbw_tep((unsigned)key);
            const float rs = __uint_as_float(sumbits(key));
            const bool surv = valid && pbw_cost_floor<CAP>(T0, rs, parity(t)) < best0;
            const u64 sm = __ballot(surv);
            if (sm) {
                if (surv) slist[nsurv + wave_lane_rank(sm)] = (unsigned short)(kbase + k * 64 + lane);
                nsurv += __popcll(sm);
            }
            const int dl = valid ? pb_delta(t, P.order) : 0;
            sumdel += dl; neg += dl < 0;
            const bool need = rs > r_safe;      // above the last safe probe (the last chunk of a search): the rule itself
            if (__ballot(need)) {
                float w1;
                if (need && pb_not_promising(rs, best0, Fr, P.c4, T0.cdfA, T0.cdfH, w1) && sumbits(key) < fs) fs = sumbits(key);
            }
        }
    }
    // One exchange settles the ordinary chunk.  (The OTHER candidate counter is reset here: it was last read before the barrier
    // of this chunk's count; this chunk's was reset a chunk ago.)
    const int par = R.par++ & 1;
    if (wave == 0 && lane == 0) L.ncand[par ^ 1] = 0;
    // the survivors' exact costs; candidates (cost below the chunk-start best) go to the workgroup's list
    if (nsurv) {
        // (a wavefront holds one or two survivors, rarely more: eight at a time, eight lanes each -- a lane sums one byte of the
        //  discrepancy pattern in the canonical order (pbw_cost_exact), then the eight byte sums are added in order down the row)
        wave_fence();
        for (int b0 = 0; b0 < nsurv; b0 += 8) {
            const int sidx = b0 + (lane >> 3), byte = lane & 7;
            const bool has = sidx < nsurv;
            const u64 key = has ? L.keys[slist[has ? sidx : 0]] : 0ull;
            const u64 D = parity(pbw_tep((unsigned)key));
            const unsigned v = (unsigned)(D >> (8 * byte)) & 255u;
            float bs = 0.0f;
#pragma unroll
            for (int t = 0; t < 8; ++t) bs = ((v >> t) & 1u) ? bs + T0.w[64 + 8 * byte + t] : bs;
            // acc_b = acc_(b-1) + bs_b, acc_(-1) = the key's sum: seven dependent steps, lane b takes lane b - 1's value (row_shr:1)
            float acc = (byte == 0 ? __uint_as_float((unsigned)(key >> 32)) : 0.0f) + (byte == 0 ? bs : 0.0f);
#pragma unroll
            for (int st = 1; st < 8; ++st) {
                const float prev = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc), 0x111, 0xF, 0xF, true));
                acc = byte == st ? prev + bs : acc;
            }
            const float c = has && byte == 7 ? acc : __builtin_inff();
            const bool cand = c < best0;
            const u64 cm = __ballot(cand);
            if (cm) {
                int base = 0;
                if (lane == 0) base = atomicAdd(&L.ncand[par], __popcll(cm));
                base = __builtin_amdgcn_readfirstlane(base);
                const int idx = base + wave_lane_rank(cm);
                if (cand && idx < kCoopMaxCand) { L.ck[idx] = key; L.cc[idx] = c; }
            }
        }
    }
    // the exchange: frontier growth and the pops that shrink it (per wavefront |growth| <= 2 * WK <= 2^11), the smallest firing sum
    int negtot, deltot;
    unsigned sF;
    {
        const int slot = R.seq++ & 7;
        const int x1 = (wave_add_i32(neg) << 18) + (wave_add_i32(sumdel) + 4096), x2 = wave_min_i32((int)fs);
        if (lane == 0) { L.red[slot][wave] = x1; L.red2[slot][wave] = x2; }
        __syncthreads();
        int a = 0, m = 0x7FFFFFFF;
#pragma unroll
        for (int v = 0; v < NW; ++v) { a += L.red[slot][v]; const int x = L.red2[slot][v]; m = x < m ? x : m; }
        negtot = a >> 18; deltot = (a & 0x3FFFF) - NW * 4096; sF = (unsigned)m;
    }
    const int ncand = L.ncand[par];
    if (S.nlive - negtot <= 1) return -1;
    if (ncand > kCoopMaxCand) return -1;
    if (ncand == 0) {
        // no candidate, no key fires: the whole chunk is visited and nothing else happens
        if (sF == 0x7FFFFFFFu) return pbw_commit_counts(S, 0, 0, 0, n, deltot, stop, ntep);
        // no candidate, rule 1 fires: the search stops at the first key of the smallest firing sum (every key of that sum fires)
        int cs = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (k * 64 < kcount) cs += sumbits(key_at(k)) < sF;
        const int rank_stop = coop_sum<NW>(R, wave_add_i32(cs));      // (pbw_commit_counts(S, 0, 1, rank_stop, ...), written out: the call moves six lines of this kernel)
        S.cmp += 2 * (rank_stop + 1);
        S.suc1 += rank_stop;
        stop = 1; ntep = S.j + rank_stop + 1;
        return 1;
    }
    // ---- candidates: wavefront 0 orders them and finds the records; the others wait
    bool tie = false;
    if (wave == 0) {
        const u64 my = lane < ncand ? L.ck[lane] : ~0ull;
        const float myc = lane < ncand ? L.cc[lane] : 0.0f;
        int rk0 = 0;
        bool t0 = false;
        for (int d = 0; d < ncand; ++d) { const u64 o = L.ck[d]; rk0 += lane < ncand && o != my && visited_before(o, my); }
        wave_fence();
        if (lane < ncand) { L.ck[rk0] = my; L.cc[rk0] = myc; }
        wave_fence();
        int nrec = 0, stop2 = 0;
        if (!__ballot(t0)) {
            float before = best0;
            for (int t = 0; t < ncand && !stop2; ++t) {
                const u64 key = L.ck[t];
                const float c = L.cc[t];
                if (c < before) {
                    if (lane == 0) { L.rk[nrec] = key; L.rc[nrec] = c; }
                    ++nrec;
                    const float w1 = det_expf(P.c4 * __uint_as_float((unsigned)(key >> 32))) * Fr.spl;
                    if (pb_success_q(parity(pbw_tep((unsigned)key)), w1, T0.qpar, Fr)) stop2 = 1;
                    before = c;
                }
            }
        }
        if (lane == 0) { L.nrec = nrec; L.stop2 = stop2; L.tie0 = __ballot(t0) ? 1 : 0; }
    }
    __syncthreads();
    const int nrec = L.nrec, stop2 = L.stop2;
    tie |= L.tie0 != 0;
    // Rule 1 again for the keys from the first record on, each with the best it really sees (the record before it).  A lower
    // best fires sooner (beta falls with it), so a key that the LAST record's cost does not stop is stopped by none: probes
    // with that cost (as above) leave the keys beyond the last safe probe to evaluate -- usually none.  Keys before the first
    // record keep what the chunk-start best said (fs, if it lies before the first record).
    if (nrec > 0) {
        const unsigned s0 = sumbits(L.rk[0]);
        float r_safe2;     // (pb_rule1_safe_sum with the last record's cost, written out: the helper costs this kernel an instruction)
        {
            const float rp = lane == 63 ? mx : mn + (mx - mn) * ((float)(lane + 1) * (1.0f / 64.0f));
            float w1;
            const float bs = pb_promising_bs(rp, L.rc[nrec - 1], Fr, P.c4, T0.cdfA, T0.cdfH, w1);
            const u64 unsafe = ~__ballot((double)bs > Fr.p_t_pro * 1.001);
            const int u = unsafe ? __builtin_ctzll(unsafe) : 64;
            r_safe2 = u == 0 ? -1.0f : __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rp), u - 1));
        }
        fs = fs < s0 ? fs : 0x7FFFFFFFu;
#pragma unroll 1
        for (int k = 0; k < PER; ++k) {
            if (k * 64 < kcount) {
                const u64 key = key_at(k);
                const bool behind = key != ~0ull && sumbits(key) >= s0;
                int t = 0;
                if (behind)
                    for (int u = 0; u < nrec; ++u) { const u64 r = L.rk[u]; t += r != key && visited_before(r, key); }
                const bool need = behind && __uint_as_float(sumbits(key)) > r_safe2;
                if (__ballot(need)) {
                    float w1;      // (the first record itself is judged with the chunk-start best: t = 0)
                    if (need && pb_not_promising(__uint_as_float(sumbits(key)), t > 0 ? L.rc[t - 1] : best0, Fr, P.c4, T0.cdfA, T0.cdfH, w1) && sumbits(key) < fs) fs = sumbits(key);
                }
            }
        }
    }
    sF = (unsigned)coop_min<NW>(R, wave_min_i32((int)fs));
    int reason = 0;
    unsigned sstop = 0;
    if (sF != 0x7FFFFFFFu) {
        reason = 1; sstop = sF;
        // ("the first key of the smallest firing sum stops" holds when every key of that sum sees the same best: not with a
        //  record among them)
        for (int u = 0; u < nrec; ++u) tie |= sumbits(L.rk[u]) == sF;
    }
    if (stop2) {
        const unsigned sR = sumbits(L.rk[nrec - 1]);
        if (reason == 0 || sR < sF) { reason = 2; sstop = sR; }
    }
    // the records that count: all of them without a stop and when the LAST record stops by rule 2 (the records are in visit order,
    // equal sums included -- counting "sums below the stopping record's" dropped a record that ties with it: found by
    // tests/tools/pb_long_fuzz.py on quantised channel values); those below the firing sum when rule 1 stops (a record ON that
    // sum has left the pass above)
    int nbefore = nrec;
    if (reason == 1) {
        nbefore = 0;
        for (int u = 0; u < nrec; ++u) nbefore += sumbits(L.rk[u]) < sstop;
    }
    // positions: the keys below the last record that counts, the keys below the stopping sum; ties (one exchange: 13 + 13 + 1 bits)
    const u64 bk = nbefore > 0 ? L.rk[nbefore - 1] : 0ull;
    const float bcost = nbefore > 0 ? L.rc[nbefore - 1] : 0.0f;
    int cb = 0, cs = 0;
#pragma unroll 1
    for (int k = 0; k < PER; ++k) {
        if (k * 64 < kcount) {
            const u64 key = key_at(k);
            if (nbefore > 0) cb += key != bk && visited_before(key, bk);
            if (reason == 1) cs += sumbits(key) < sstop;
        }
    }
    const int pos = coop_sum<NW>(R, wave_add_i32(cb) + (wave_add_i32(cs) << 13) + (__ballot(tie) ? 1 << 26 : 0));
    // (no barrier here: the candidate / record words are next written behind the NEXT chunk's count exchange, which every
    //  wavefront reaches only after it has left this function)
    if (pos >> 26) return -1;
    const int rank_best = pos & 0x1FFF, rank_stop = reason == 2 ? rank_best : (pos >> 13) & 0x1FFF;
    if (nbefore > 0) {
        const PbTep t = pbw_tep((unsigned)bk);
        u64 E = 1ull << t.p0;          // (pb_tep_mask, written out: with the helper three moves of this kernel change places)
        if (t.wt > 1) E |= 1ull << t.p1;
        if (t.wt > 2) E |= 1ull << t.p2;
        S.best = bcost; S.bestD = parity(t); S.bestE = E;
        S.bestidx = S.j + rank_best + 1;
    }
    return pbw_commit_counts(S, nbefore, reason, rank_stop, n, deltot, stop, ntep);
}

// Wavefront 0 alone over the sums (lo, T] that hold n TEPs: the sorted path, in sub-chunks.  L.one.cur holds the cursors of
// the range's start (all 32 rows); arguments in L.su / L.bs / L.sP, results in L.bs / L.bstate / L.bstop / L.bntep
// (state 0 / 1 / 2 as in pb_wave_kernel).
template <int NW>
__device__ __forceinline__ void coop_solo_range(PbCoopLds<NW> &L)
{
    constexpr int CAP = kPbWaveCap;
    const int lane = threadIdx.x & 63;
    PbwState S = L.bs;
    int stop = L.bstop, ntep = L.bntep;
    PbParams P;
    P.order = L.sP.order; P.c4 = L.sP.c4;
    const int state = pbw_redo_call<CAP>(L.one, P, L.su.fr, L.su.d0, L.su.lo, L.su.T, L.su.smax, L.su.done, L.su.n, lane, S, stop, ntep);
    wave_fence();
    if (lane == 0) { L.bs = S; L.bstate = state; L.bstop = stop; L.bntep = ntep; }
}

template <int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(4))) void pb_coop_kernel(PbParams P, const double *__restrict__ cdf_half, int *__restrict__ ctl, int *__restrict__ listB,
                                                          const unsigned *__restrict__ carry, PbOut O)
{
    // (dynamic LDS: a hipGraph kernel node with more than 64 KiB of STATIC LDS aborts at replay on ROCm 7.2; the size is
    //  registered once in pb_ctx_init)
    extern __shared__ __attribute__((aligned(16))) unsigned char pb_coop_lds[];
    PbCoopLds<NW> &L = *reinterpret_cast<PbCoopLds<NW> *>(pb_coop_lds);
    constexpr int NI = 32 / NW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // list C: ticket t < nfar -> record t (the searches expected to run far), the others -> record kPbCoopHalf + (t - nfar)
    const int lenc = ctl[kPbCtlLenC], lenc2 = ctl[kPbCtlLenC2];
    const int nfar = lenc < kPbCoopHalf ? lenc : kPbCoopHalf;
    const int nlist = nfar + (lenc2 < kPbCoopHalf ? lenc2 : kPbCoopHalf);
    if ((int)blockIdx.x >= nlist) return;      // (more workgroups than frames -- or nothing handed on at all: leave before any set-up)
    const int nall = P.order > 2 ? kPbTabSize : (P.order > 1 ? kPbTriples0 : kPbPairs0);
    if (wave == 0) {
        L.one.cdfH[lane] = (float)cdf_half[lane];
        if (lane == 0) { L.one.cdfH[64] = (float)cdf_half[64]; L.ticket[0] = atomicAdd(&ctl[kPbCtlTicketC], 1); L.sP = P; }
    }
    CoopRed<NW> R{L.red, 0, wave, lane, 0};
    __syncthreads();
    for (int it = 0;; ++it) {
        // frames are handed out by ticket; the NEXT frame's ticket is drawn now and is back long before it is needed
        int tk = L.ticket[it & 1];
        if (tk >= nlist) break;
        int next_tk = 0;      // (drawn now, parked in LDS at the frame's end: the wavefront does not wait for the atomic here)
        if (tid == 0) { next_tk = atomicAdd(&ctl[kPbCtlTicketC], 1); L.ncand[0] = 0; L.ncand[1] = 0; }
        const unsigned *rec = carry + (long long)(tk < nfar ? tk : kPbCoopHalf + (tk - nfar)) * kPbRecWords;
        // the frame's tables: one load per thread (wavefront 0 may still be writing the previous frame's codeword out)
        if (tid >= 64)
            for (int i = tid - 64; i < kPbRecPrefix; i += 64 * NW - 64) reinterpret_cast<unsigned *>(&L.one)[i] = rec[i];
        const PbCarry &c = *reinterpret_cast<const PbCarry *>(rec + kPbRecScalars);
        unsigned po = wave == 0 ? rec[kPbRecPerm + (lane >> 2)] : 0u, po2 = wave == 0 ? rec[kPbRecPerm + 16 + (lane >> 2)] : 0u;      // (the permutation, for the codeword at the end: in flight from here)
        PbFrame Fr = c.fr;
        u64 d0 = c.d0;
        PbwState S;
        S.best = c.best; S.j = c.j; S.nlive = c.nlive; S.cmp = c.cmp; S.suc1 = c.suc1; S.suc2 = c.suc2; S.bestidx = c.bestidx;
        S.bestD = c.bestD; S.bestE = c.bestE;
        float lo = c.lo;
        int done = S.j;
        int a0[NI];            // the cursors the record holds
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            int q, l;
            coop_item<NW>(wave, j, lane, q, l);
            a0[j] = (int)((rec[kPbRecCur + (q >> 2) * 64 + l] >> (8 * (q & 3))) & 255u);
        }
        __syncthreads();
        CoopItems<NI> I;
        coop_items_init<NW>(I, L.one.w, P.order, lane, wave);
#pragma unroll
        for (int j = 0; j < NI; ++j) I.a[j] = a0[j];
        float smax = P.order > 2 ? (L.one.w[0] + L.one.w[1]) + L.one.w[2] : (P.order > 1 ? L.one.w[0] + L.one.w[1] : L.one.w[0]);
        int stop = 0, ntep = P.nmax, state = 0;
        float tprev = c.tprev, nprev = c.nprev;
        while (state == 0 && done < nall) {
            int aprev[NI];
#pragma unroll
            for (int j = 0; j < NI; ++j) aprev[j] = I.a[j];
            float T;
            int kbase = 0, kcount = 0;
            int n = coop_next_chunk<NW>(L, R, I, lo, done, nall, P.t3, lane, wave, T, tprev, nprev, kbase, kcount);
            if (n < 0) { state = 2; break; }
            if (n == 0) break;
            const float cmn = lo < 0.0f ? L.one.w[63] : lo, cmx = T < __builtin_inff() ? T : smax;
            wave_fence();
            state = coop_scan_chunk<NW>(L, R, P, Fr, d0, n, kbase, kcount, cmn, cmx, lane, wave, S, stop, ntep);
            if (state < 0) {
                // (One wavefront redoing ~2700 keys alone takes 35-135 us where the whole launch takes ~150, in-kernel stamps of
                //  round 4.  Measured and dropped: walking the same sums again with a third of the target, all wavefronts
                //  together, until <= 768 keys are left for wavefront 0 -- the failing chunk is walked ~8 times on the way down,
                //  the solo stamp falls from 630 k to 180 k cycles per launch and the launch gets LONGER: 0.479 -> 0.500 ms per
                //  search call at 2.5 dB, no change at 2.0 / 1.0 dB.)
                // wavefront 0 redoes the chunk alone from the cursors the chunk started with
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    int q, l;
                    coop_item<NW>(wave, j, lane, q, l);
                    // (the chunk kernel's code marks an item without members by a cursor of 0; here the cursor stops at base + 1)
                    reinterpret_cast<unsigned char *>(&L.one.cur[q >> 2][l])[q & 3] = (unsigned char)(aprev[j] > I.base[j] + 1 ? aprev[j] : 0);
                }
                __syncthreads();
                if (wave == 0) {
                    // (everything this wavefront needs afterwards is parked in LDS around the call: see PbCoopLds::sv)
#pragma unroll
                    for (int j = 0; j < NI; ++j) L.sv[j][lane] = I.a[j];
                    if (lane == 0) {
                        L.su.fr = Fr; L.su.d0 = d0; L.su.lo = lo; L.su.T = T; L.su.tprev = tprev; L.su.nprev = nprev; L.su.smax = smax;
                        L.su.done = done; L.su.n = n; L.su.seq = R.seq; L.su.par = R.par; L.su.it = it; L.su.tk = tk; L.su.next_tk = next_tk;
                        L.bs = S; L.bstop = stop; L.bntep = ntep;
                    }
                    wave_fence();
                    coop_solo_range<NW>(L);
                    wave_fence();
                    coop_items_init<NW>(I, L.one.w, P.order, lane, wave);
#pragma unroll
                    for (int j = 0; j < NI; ++j) I.a[j] = L.sv[j][lane];
                    Fr = L.su.fr; d0 = L.su.d0; lo = L.su.lo; T = L.su.T; tprev = L.su.tprev; nprev = L.su.nprev; smax = L.su.smax;
                    done = L.su.done; n = L.su.n; R.seq = L.su.seq; R.par = L.su.par; it = L.su.it; tk = L.su.tk;
                    rec = carry + (long long)(tk < nfar ? tk : kPbCoopHalf + (tk - nfar)) * kPbRecWords;
                    po = rec[kPbRecPerm + (lane >> 2)]; po2 = rec[kPbRecPerm + 16 + (lane >> 2)];
                    next_tk = L.su.next_tk;
                }
                __syncthreads();
                S = L.bs; state = L.bstate; stop = L.bstop; ntep = L.bntep;
            }
            lo = T;
            done += n;
        }
        if (tid == 0) L.ticket[(it + 1) & 1] = next_tk;
        __syncthreads();                        // (every wavefront is through with the frame's tables)
        if (wave == 0) {
            if (state == 2) {   // massive ties: the literal list replay decodes this frame
                if (lane == 0) listB[atomicAdd(&ctl[kPbCtlLenB], 1)] = (int)reinterpret_cast<const PbCarry *>(rec + kPbRecScalars)->f;
            } else {
                const PbCarry &c2 = *reinterpret_cast<const PbCarry *>(rec + kPbRecScalars);
                const u64 hm = c2.hm, hp = c2.hp;
                const long long f = c2.f;
                const int o1 = (int)((po >> (8 * (lane & 3))) & 255u), o2 = (int)((po2 >> (8 * (lane & 3))) & 255u);
                if (lane < 2) L.one.cw[lane] = 0;
                wave_fence();
                const u64 mrb_bits = hm ^ S.bestE, par_bits = S.bestD ^ hp;
                if ((mrb_bits >> lane) & 1) atomicOr(&L.one.cw[o1 >> 6], 1ull << (o1 & 63));
                if ((par_bits >> lane) & 1) atomicOr(&L.one.cw[o2 >> 6], 1ull << (o2 & 63));
                wave_fence();
                if (lane < 2) O.cw[f * 2 + lane] = L.one.cw[lane];
                if (lane == 0) {
                    if (O.metric) O.metric[f] = S.best;
                    if (O.best) O.best[f] = S.bestidx;
                    if (O.ntep) O.ntep[f] = ntep;
                    if (O.aux) { O.aux[f * 4] = S.cmp; O.aux[f * 4 + 1] = S.suc1; O.aux[f * 4 + 2] = S.suc2; O.aux[f * 4 + 3] = stop; }
                }
            }
        }
    }
}

}  // namespace ldpc
