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
// Direct enumeration of a sum range.  The MRB positions are sorted by reliability (w[0] >= w[1] >= ...) and float
// addition is monotone, so with the other positions fixed the sum of a TEP is non-increasing in its LAST position m.
// The TEPs are 2017 "items" -- the singles {m}; the pairs {i, m} of one i; the triples {i, j, m} of one (i, j) --
// inside each of which the members appear in the visit order by DESCENDING m.  Every lane owns 32 items:
//   q = 0..30  triples, by the DISTANCE of the two fixed positions: lanes l < 62 - q own (i, j) = (l, l + 1 + q) (distance
//              q + 1), lanes 62 - q .. 62 own (l - 62 + q, l) (distance 62 - q): 62 - q and q + 1 items, 63 together;
//              lane 63 owns none.  In both cases one fixed position is the LANE NUMBER and the other is the lane number
//              plus q + 1 resp. q + 2 modulo 64: the lane's own weight plus a copy of the weights that rotates through the
//              wavefront by one lane per row (DPP wave_rol) -- the fixed sums cost no memory access and no uniform operand.
//              (Rounds 1-3 dealt the rows by i: (q, q + 1 + l) and (61 - q, l): two LDS reads per item for the same sum.)
//   q = 31     lanes 0..62: the pairs of i = l;  lane 63: the singles
// and keeps per item a cursor (members [cursor, 64) are visited; 0 = no member left).  The chunk (lo, T] is produced by a
// WALK: every item's next member (fixed sum + the weight under the cursor) is compared with T, the items that have one are listed,
// those lanes emit it (key = sum bits << 32 | positions; slot = running count + mbcnt of the ballot) and step their
// cursor.  An item costs one compare when it has nothing to give, the members cost one trip each; no binary searches,
// no count-then-write double pass, no block scan.  T can be ANY value -- exactness does not depend on it -- so it is
// sized to the work: first guess from pb_bound_guess / the growth exponent of the last two bounds, a short chunk is
// extended in place (the walk resumes), an overflowing walk is abandoned and retried with a smaller T.
#pragma once
#include "ldpc_pb_common.h"

namespace ldpc {

// uniform search state of a frame (wave-uniform values)
struct PbwState {
    float best;
    int j, nlive, cmp, suc1, suc2, bestidx;
    u64 bestD, bestE;
};
// arguments and results of the sorted path (pbw_sorted_chunk: a real function call, made with nothing live across it)
struct PbSortArgs {
    PbwState S;
    PbFrame fr;
    u64 d0;
    float mn, mx, c4;
    int n, order, state, stop, ntep;
};
// ... and of pbw_redo_range: the sums (lo, T] -- n TEPs, `done` visited before them -- once more, in chunks of 8-byte keys
struct PbRedoArgs {
    PbwState S;
    PbFrame fr;
    u64 d0;
    float lo, T, smax, c4;
    int done, n, order, target, state, stop, ntep;
};

constexpr int kPbMaxTie = 16;
constexpr int kPbWaveCap = 384;   // chunk capacity of the chunk kernel (10 KiB of LDS per frame: four wavefronts per SIMD; 512 = 12 KiB = three)

template <int CAP>
struct __attribute__((aligned(16))) PbWaveLds {
    float pre[4];             // pre[3] = NaN: the "weight" under an exhausted cursor (0) -- its sum compares false with any bound
    float w[128];             // |y'|                                         } words [4, 364): the image of the record
    u64 P[64];                // rows of P'                                   } pb_singles_kernel wrote for the frame
    u64 Pzero;                // = 0: "row 64", what the unused positions of a pair's or a single's key read (no select)
    float cdfA[68];           // P[Bin(64, p1) <= b] ROUNDED TO float32 -- the rules only ever read the table through a
                              // (float) cast (pb_not_promising), so storing the rounded value is the same arithmetic
    unsigned char perm[128];  // original bit index of primed position p (for the codeword at the end)
    unsigned rpad[2];         // (the record's image ends here: 360 words)
    float tail[4][17];        // tail[g][c] <= the sum of the c lightest parity weights of quarter g (pbw_cost_floor)
    float qpar[64];           // q_p = sigmoid(c4 |y'_p|) of the parity positions (the success rule, pb_success_q)
    float cdfH[68];           // P[Bin(64, 1/2) <= b], float32 as cdfA
    // the chunk: as walked (slots 0..n-1), then (sorted path only) grouped by bucket and finally in visit order; 64 entries of
    // slack take the overshoot of the walk's last trip and the "never before me" pad of the rank count.  (Rounds 2-3 skewed
    // the array by one pad entry per eight against the two-bank pattern of lane-consecutive 64-bit accesses in the sorted
    // path, and let a trip overshoot by 128: 1.6 KiB that stood between the kernel and a fourth wavefront per SIMD.)
    u64 keys[CAP + 64];
    union {
        int hist[CAP];        // bucket counts, then cursors; the costs of a chunk
        unsigned list[CAP + 64];   // the walk's work list (one entry per member emitted)
    };
    unsigned cur[8][64];      // tentative cursors of the walk: byte q & 3 of cur[q / 4][lane] = item q of that lane
    union {
        struct {
            u64 ck[16], rk[16];   // sort-free chunk pass: improvement candidates / the records among them (key, cost)
            float cc[16], rc[16];
        };
        PbSortArgs sa;        // (the pass has given up on the chunk when the sorted path is called: its words are free)
        PbRedoArgs ra;        // (read into registers on entry, written on exit: the calls in between use the words)
    };
    u64 cw[2];
};
static_assert(sizeof(PbSortArgs) <= 384 && sizeof(PbRedoArgs) <= 384, "the rare paths' arguments borrow the candidate words");

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

// positions of a key's low word: p0 | p1 << 8 | p2 << 16 | weight << 24 (ascending positions; an unused position is 64, the
// zero row behind P').  Keys made by the chunk kernel's walk carry, in bits 26-27, the frontier growth of the TEP's pop plus
// one (pb_delta + 1 = 0, 1, 2: the walk knows it from the item's geometry; unpacked from the positions it is ~25 instructions)
__device__ __forceinline__ PbTep pbw_tep(unsigned code)
{
    return PbTep{(int)(code & 255u), (int)((code >> 8) & 255u), (int)((code >> 16) & 255u), (int)((code >> 24) & 3u)};
}
constexpr unsigned kPbUnused1 = 64u << 8, kPbUnused2 = 64u << 16;

// the items of a lane (see above).  base: the members are m in (base, 63]; code / sh: a member's key is code | m << sh
struct PbwItem {
    int i, j, base, sh;
    unsigned code;
};
__device__ __forceinline__ PbwItem pbw_item_rt(int q, int l)
{
    PbwItem it;
    const bool tri = q < 31, first = l < 62 - q;
    it.i = tri ? (first ? l : l - 62 + q) : l;
    it.j = tri ? (first ? l + 1 + q : l) : l;
    it.base = tri ? (l <= 62 ? it.j : 63) : (l <= 62 ? l : -1);
    it.code = tri ? ((3u << 24) | ((unsigned)it.j << 8) | (unsigned)it.i) : (l <= 62 ? ((2u << 24) | kPbUnused2 | (unsigned)l) : ((1u << 24) | kPbUnused2 | kPbUnused1));
    it.sh = tri ? 16 : (l <= 62 ? 8 : 0);
    return it;
}

// Walk state.  Registers: the COMMITTED cursors only (one byte per item, four items per register; members [cursor, 64) are
// visited).  LDS: the TENTATIVE cursors L.cur[q / 4][lane] of the chunk being sized -- in the dense phase below a lane works on
// whatever item the list hands it.  The sum of an item's NEXT member is NOT kept (rounds 1-3 held the 32 of them in registers:
// with the chunk's keys that was 225 live VGPRs against the 168 of three wavefronts per SIMD, i.e. 57 registers in scratch,
// re-read and re-written once per walk -- 0.87 GB of HBM writes per launch at 1.0 dB): it is the item's fixed sum plus the weight
// under its cursor, two LDS reads and an add when the walk asks for it.
struct PbWalk {
    unsigned ecur[8];
};

__device__ __forceinline__ float pbw_nan() { return __int_as_float(0x7FC00000); }

template <int CAP>
__device__ __forceinline__ void pbw_cursors_store(PbWaveLds<CAP> &L, const unsigned (&cur)[8], int lane)
{
#pragma unroll
    for (int k = 0; k < 8; ++k) L.cur[k][lane] = cur[k];
}
template <int CAP>
__device__ __forceinline__ void pbw_cursors_load(const PbWaveLds<CAP> &L, unsigned (&cur)[8], int lane)
{
#pragma unroll
    for (int k = 0; k < 8; ++k) cur[k] = L.cur[k][lane];
}

template <int CAP>
__device__ __forceinline__ void pbw_walk_init(PbWaveLds<CAP> &L, PbWalk &W, int order, int lane)
{
    // every cursor at 64 (an item's next member is its last position 63); 0 for the items that do not exist: lane 63's
    // triples, the pairs when the order is 1
#pragma unroll
    for (int k = 0; k < 8; ++k) W.ecur[k] = lane <= 62 ? 0x40404040u : 0u;
    if (lane == 63 || order < 2) W.ecur[7] = lane <= 62 ? 0x00404040u : 0x40000000u;
    pbw_cursors_store<CAP>(L, W.ecur, lane);
}

// w[(lane + 1) & 63] of a register that holds w[lane] in every lane, three ways (ROT: what the context's probe of the
// wave_rol:1 DPP control found: -1 = a lane receives its upper neighbour's value, +1 = its lower neighbour's, 0 = unusable)
template <int ROT>
__device__ __forceinline__ float pbw_rot1(float x)
{
    static_assert(ROT != 0, "no rotation: the caller reads LDS");
    if constexpr (ROT < 0) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x134, 0xF, 0xF, true));   // wave_rol:1
    else return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x13C, 0xF, 0xF, true));                     // wave_ror:1
}

// Emit every member with sum <= T that lies beyond the tentative cursors (L.cur); returns the new running count (> CAP: the
// chunk overflowed, the walk stopped early and the caller puts the committed cursors back).  Two phases:
//   list    one pass over the lane's 32 items.  An item's next member has the sum (w[i] + w[j]) + w[cursor - 1]; one of i, j
//           is the lane number and the other sits q + 1 or q + 2 lanes further (mod 64), so the fixed part is the lane's own
//           weight plus a copy of the weights that moves one lane per row (pbw_rot1); the weight under the cursor is one LDS
//           read (a cursor of 0 reads the NaN in front of the weights: no member left, no separate test); one compare.  The
//           items whose next member is <= T are appended to a work list (ballot + mbcnt, no loop); 86 % have nothing to give;
//   dense   the list, 64 entries per trip, every lane emits one or two members of its entry's item (key = sum bits << 32 |
//           positions; slot = running count + mbcnt), steps that item's cursor in LDS and, if the item's next member is
//           <= T too, appends the entry to the list's tail again -- so a trip runs at full lanes whatever the items' lengths.
// A lane works on whatever item the list hands it, hence the cursors in LDS and the item geometry from run-time (q, lane).
// (Round 3 kept the next-member sums in registers -- 32 VGPRs -- and took them back from the dense phase in a third sweep,
//  "collect", ~9 instructions per item: 57 spilled registers re-read and re-written once per walk.)
// K4 = true: the keys are written as their low words only -- 4 bytes, the positions -- and the pass recomputes a key's sum from
// them (pbw_scan4): the same key memory then holds 2 CAP + 64 keys, and every per-chunk cost (the list pass, the probes, the
// bound arithmetic, the reductions) is paid once per ~680 keys instead of once per ~310.  KCAP: the capacity in keys.
// The work list is a RING of CAP + 64 entries in both forms (an entry is free once its trip has read it).
template <int CAP, bool K4>
struct PbwCaps {
    static constexpr int KCAP = K4 ? 2 * CAP + 64 : CAP;      // keys of a chunk (64 more fit behind them)
    static constexpr int RING = CAP + 64;                      // work-list entries
};
template <int CAP, int ROT, bool K4>
__device__ __forceinline__ int pbw_walk(PbWaveLds<CAP> &L, float T, int cnt, int order, int lane)
{
    constexpr int KCAP = PbwCaps<CAP, K4>::KCAP, RING = PbwCaps<CAP, K4>::RING;
    static_assert(sizeof(L.keys) / (K4 ? 4 : 8) >= KCAP + 64 && CAP >= 128, "a dense trip may write 63 keys past the capacity");
    static_assert(sizeof(L.list) / 4 >= RING, "work-list ring");
    static_assert(offsetof(PbWaveLds<CAP>, w) >= 4 && offsetof(PbWaveLds<CAP>, w) == offsetof(PbWaveLds<CAP>, pre) + 16, "the NaN sits right in front of the weights");
    unsigned *const list = L.list;      // entry: q | owner lane << 5
    const float *const w = L.w;
    int tail = 0;
    {
        // (an opaque copy of the lane number per walk: otherwise lane-dependent addresses are hoisted out of every loop
        //  around the walk, kept for the whole kernel and spilled)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        unsigned cur[8];
        pbw_cursors_load<CAP>(L, cur, ln);
        const float wl = w[ln];
        const char *const wbytes = reinterpret_cast<const char *>(w) - 4;       // + 4 * cursor = the weight under the cursor
        // eight items at a time: the eight sums first (their LDS reads in flight together -- a branch behind every item made
        // the wavefront wait for each read by itself: ~32 exposed LDS latencies per walk), then the eight ballots and appends
        const auto next_sum = [&](int q, float sb) {
            const unsigned a4 = ((cur[q >> 2] >> (8 * (q & 3))) & 255u) << 2;
            return sb + *reinterpret_cast<const float *>(wbytes + a4);
        };
        const auto append = [&](int q, float sv) {
            const bool pend = sv <= T;
            const u64 act = tail <= RING - 64 ? __ballot(pend) : 0ull;      // (more pending items than the ring takes: an overflow already)
            if (act) {
                const int p = tail + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(act >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)act, 0u));
                if (pend) list[p] = (unsigned)q | ((unsigned)ln << 5);
                tail += __popcll(act);
            }
        };
        if (order > 2) {
            // Rows that can have a member <= T at all.  The smallest sum of row q is (w[61 - q] + w[62]) + w[63] (every other
            // member of the row has positions at least as reliable, and float addition is monotone); it grows with q, so the
            // rows with something to give are a PREFIX 0 .. qmax - 1: one compare per row in lane q, one ballot.  Deep rows
            // stay empty for most of a search (a search of 3500 TEPs visits 8 % of the table), at 2.5 dB nearly all of them.
            int qmax;
            {
                const float rmin = (w[(61 - ln) & 63] + w[62]) + w[63];
                qmax = __popcll(__ballot(ln < 31 && rmin <= T));
            }
            float r1;                    // w[(lane + q + 1) & 63]
            if constexpr (ROT != 0) r1 = pbw_rot1<ROT>(wl); else r1 = w[(ln + 1) & 63];
            const float s31 = next_sum(31, ln <= 62 ? wl : 0.0f);      // (the pairs / singles row: always looked at, with group 0)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (8 * g >= qmax) break;
                float sv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int q = 8 * g + u;
                    if (q < 31) {
                        float r2;
                        if constexpr (ROT != 0) r2 = pbw_rot1<ROT>(r1); else r2 = w[(ln + q + 2) & 63];
                        sv[u] = next_sum(q, wl + (ln < 62 - q ? r1 : r2));
                        r1 = r2;
                    } else {
                        sv[u] = pbw_nan();
                    }
                }
                asm volatile("" : "+v"(sv[0]), "+v"(sv[1]), "+v"(sv[2]), "+v"(sv[3]), "+v"(sv[4]), "+v"(sv[5]), "+v"(sv[6]), "+v"(sv[7]));
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (8 * g + u < 31) append(8 * g + u, sv[u]);
            }
            append(31, s31);
        } else {
            append(31, next_sum(31, ln <= 62 ? wl : 0.0f));
        }
    }
    if (tail == 0) return cnt;
    if (tail > RING - 64) return KCAP + 1;
    wave_fence();
    const auto ring = [](int p) { p = p >= RING ? p - RING : p; return p >= RING ? p - RING : p; };      // (p < 3 RING: an entry is a key at least)
    static_assert(3 * RING > KCAP + 128, "ring index");
    int head = 0;
    while (head < tail && cnt <= KCAP) {
        // A trip serves up to 64 entries, two members each.  When fewer than 33 entries wait -- the tail of a walk: a few long
        // items -- every entry gets 2, 4 or 8 lanes, lane u of its group taking the members 2u and 2u + 1 below the cursor:
        // inside an item the sums rise as the position falls, so the members <= T are a PREFIX and every lane judges its two
        // by itself; the group's leader steps the cursor by what the group emitted.  (Two members per entry and trip whatever
        // the list's length: 9.3 trips per chunk at 1.0 dB, half of them at a tenth of the lanes.)
        const int nent = tail - head;
        const int gs = (nent > 32 || cnt > KCAP - 128) ? 0 : (nent > 16 ? 1 : (nent > 8 ? 2 : 3));      // log2 of the lanes per entry
        const int e = head + (lane >> gs), u = lane & ((1 << gs) - 1);
        const bool has = e < tail;
        const unsigned ent = has ? list[ring(e)] : 0u;
        const int q = (int)(ent & 31u), l = (int)((ent >> 5) & 63u);
        int i, j, base, sh;
        unsigned code;
        if (q < 31) {
            const bool first = l < 62 - q;
            i = first ? l : l - 62 + q; j = first ? l + 1 + q : l; base = j; sh = 16;
            code = (3u << 24) | ((unsigned)j << 8) | (unsigned)i;
        } else {
            i = l; j = l; base = l <= 62 ? l : -1; sh = l <= 62 ? 8 : 0;
            code = l <= 62 ? ((2u << 24) | kPbUnused2 | (unsigned)l) : ((1u << 24) | kPbUnused2 | kPbUnused1);
        }
        const int wt = q < 31 ? 3 : (l <= 62 ? 2 : 1);
        unsigned char *const cb = reinterpret_cast<unsigned char *>(&L.cur[q >> 2][l]) + (q & 3);
        const int a = has ? (int)*cb : 1;
        const float sbv = q < 31 ? w[i] + w[j] : (l <= 62 ? w[l] : 0.0f);
        // this lane's two members (the order of the keys inside a chunk is irrelevant: second members follow the first ones)
        const int m = a - 1 - 2 * u;
        const float s = sbv + w[m & 63], s2 = sbv + w[(m - 1) & 63];
        const bool one = has && m > base && (u == 0 || s <= T);                   // (the group's first member is <= T: that is why the item is listed)
        const bool two = one && m - 1 > base && s2 <= T && cnt <= KCAP - 64;       // (no second members in a trip that may end beyond KCAP + 63)
        const u64 act = __ballot(one), act2 = __ballot(two);
        // what the entry's group emitted (a prefix of the item's members below the cursor), its new cursor, and whether the
        // member behind it is <= T too (then the entry is listed again)
        const int gsh = (lane >> gs) << gs;
        const u64 gm = gs == 0 ? 1ull : ((1ull << (1 << gs)) - 1ull);
        const int k = __popcll((act >> gsh) & gm) + __popcll((act2 >> gsh) & gm);
        const int mlast = a - k;                                                  // the lowest position emitted
        const bool left = mlast > base + 1;                                       // the item has members beyond this trip's
        const bool lead = has && u == 0;
        const bool again = lead && left && sbv + w[(mlast - 1) & 63] <= T;
        const int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(act >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)act, (unsigned)cnt));
        const int pos2 = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(act2 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)act2, (unsigned)(cnt + __popcll(act))));
        const u64 more = __ballot(again);
        const int nt = tail + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(more >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)more, 0u));
        wave_fence();                    // (every lane has read its entry: the slots may be written now)
        if (one) {
            const unsigned tmpl = code;       // (the field of the LAST position is zero in it; unused fields hold 64)
            // frontier growth of the pop (pb_delta): the extended child exists below position 63 and below the order, the
            // adjacent child if the last position can move down by one; + 1, in bits 26-27
            const unsigned g1 = (unsigned)((m < 63 && wt < order) + (m > base + 1)) << 26;
            const unsigned g2 = (unsigned)((wt < order) + (m - 1 > base + 1)) << 26;
            if constexpr (K4) {
                unsigned *const codes = reinterpret_cast<unsigned *>(L.keys);
                codes[pos] = tmpl | g1 | ((unsigned)m << sh);
                if (two) codes[pos2] = tmpl | g2 | ((unsigned)(m - 1) << sh);
            } else {
                L.keys[pos] = ((u64)__float_as_uint(s) << 32) | (tmpl | g1 | ((unsigned)m << sh));
                if (two) L.keys[pos2] = ((u64)__float_as_uint(s2) << 32) | (tmpl | g2 | ((unsigned)(m - 1) << sh));
            }
        }
        if (lead) {
            *cb = (unsigned char)(left ? mlast : 0);        // (0: exhausted -- the list pass then reads the NaN)
            if (again) list[ring(nt)] = ent;
        }
        cnt += __popcll(act) + __popcll(act2);
        {
            const int served = 64 >> gs;
            head = head + served < tail ? head + served : tail;
        }
        tail += __popcll(more);
        wave_fence();
        // (the next trip appends at tail .. tail + 63 while the entries head + 64 .. tail - 1 are still unread)
        if (tail - head > RING - 64) { cnt = KCAP + 1; break; }
    }
    return cnt;
}

// Typical bound of the N smallest sums in units of the smallest triple sum m3 = w61 + w62 + w63 (medians over decoding
// failures at 2.5 dB; the ratio is scale-free and tight: +-6 % between the 10th and 90th percentile, where the count
// changes like the ~6th power of the bound).  Only a first guess: pbw_next_chunk corrects it with exact counts.
__device__ __forceinline__ float pb_bound_guess(float n)
{
    const float l = __builtin_amdgcn_logf(n < 64.0f ? 64.0f : n);
    const float x[8] = {8.0f, 9.0f, 10.0f, 11.0f, 12.0f, 13.0f, 14.2877f, 15.4168f};     // log2 of 256 ... 20000, 43744
    const float g[8] = {0.80f, 0.89f, 1.02f, 1.14f, 1.23f, 1.33f, 1.52f, 2.2f};
    if (l <= x[0]) return g[0] * __builtin_amdgcn_exp2f((l - x[0]) / 6.0f);
    float r = g[7];
#pragma unroll
    for (int k = 6; k >= 0; --k) if (l <= x[k + 1]) r = g[k] + (g[k + 1] - g[k]) * (l - x[k]) / (x[k + 1] - x[k]);
    return r;
}

// The next chunk: walks (lo, T] for a T aimed at `target` members, 0 < n <= CAP.  Returns n and T; the chunk's keys are
// L.keys[0..n) and the walk's cursors are committed.  -1: the range cannot be split (massively equal sums: the frame goes
// to the list replay); 0: nothing is left to visit (NaN sums).
// (K4: 4-byte keys, capacity 2 CAP + 64, see pbw_walk.  COMMIT = false: W.ecur keeps the cursors the chunk STARTED from -- the
//  caller commits, pbw_cursors_load, once the chunk is judged, or puts them back, pbw_cursors_store, and redoes the range)
template <int CAP, int ROT, bool K4 = false, bool COMMIT = true>
__device__ __forceinline__ int pbw_next_chunk(PbWaveLds<CAP> &L, PbWalk &W, int order, float lo, int done, int nall, int target, int lane,
                                              float &Tout, float &tprev, float &nprev, float Tcap = __builtin_inff())
{
    constexpr int KCAP = PbwCaps<CAP, K4>::KCAP;
    const float inf = __builtin_inff();
    const float *w = L.w;
    const float m3 = (w[61] + w[62]) + w[63];
    const float want = (float)(done + target);
    float Tl = lo, Th = inf;
    float T = nall - done <= KCAP ? inf : m3 * pb_bound_guess(want);
    if (tprev > 0.0f && nprev > 0.0f && lo > tprev && (float)done > nprev && T < inf) {   // growth exponent of the last two bounds
        const float pe = (__builtin_amdgcn_logf((float)done) - __builtin_amdgcn_logf(nprev)) / (__builtin_amdgcn_logf(lo) - __builtin_amdgcn_logf(tprev));
        if (pe > 1.5f && pe < 20.0f) T = lo * __builtin_amdgcn_exp2f((__builtin_amdgcn_logf(want) - __builtin_amdgcn_logf((float)done)) / pe);
    }
    if (!(T > lo)) T = lo > 0.0f ? lo * 1.05f : w[0];
    if (T > Tcap) T = Tcap;                  // (a caller that wants the chunks to end at a given bound)
    float tp = lo, np_ = (float)done;        // last point with a known count
    int cnt = 0, c_ok = 0;
    float T_ok = lo;
    unsigned a_ok[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int it = 0; it < 48; ++it) {
        cnt = pbw_walk<CAP, ROT, K4>(L, T, cnt, order, lane);
        bool over = false;
        if (cnt > KCAP) {
            if (c_ok > 0) break;
            over = true;
            Th = T;
            pbw_cursors_store<CAP>(L, W.ecur, lane);      // back to the committed cursors
            cnt = 0;
        } else if (cnt > 0 && (!(T < inf) || 5 * cnt >= 2 * target || it >= 3)) {
            c_ok = cnt; T_ok = T;
            break;
        } else if (!(T < inf)) {
            return 0;                         // everything that can be visited has been
        } else {                              // too few so far: keep them and walk on from here
            if (cnt > 0) {
                c_ok = cnt; T_ok = T;
                pbw_cursors_load<CAP>(L, a_ok, lane);
            }
            Tl = T;
        }
        float Tn;
        if (over) {
            Tn = Tl > 0.0f ? Tl + (Th - Tl) * 0.5f : Th * 0.9f;
        } else {
            const float tot = (float)(done + cnt);
            float p = 6.0f;
            if (tp > 0.0f && np_ > 0.0f && tot != np_ && T != tp) {
                const float pe = (__builtin_amdgcn_logf(tot) - __builtin_amdgcn_logf(np_)) / (__builtin_amdgcn_logf(T) - __builtin_amdgcn_logf(tp));
                if (pe > 1.5f && pe < 20.0f) p = pe;
            }
            if (cnt > 0) { tp = T; np_ = tot; }
            Tn = cnt > 0 ? T * __builtin_amdgcn_exp2f((__builtin_amdgcn_logf(want) - __builtin_amdgcn_logf(tot)) / p) : T * 1.1f;
            if (it >= 6 || !(Tn > Tl) || !(Tn < Th)) Tn = Th < inf ? Tl + (Th - Tl) * 0.5f : T * 1.2f;
        }
        if (Tn > Tcap) Tn = Tcap;
        if (!(Tn > Tl) || !(Tn < Th)) break;
        T = Tn;
    }
    if (c_ok == 0) { pbw_cursors_store<CAP>(L, W.ecur, lane); return -1; }
    if (cnt != c_ok) pbw_cursors_store<CAP>(L, a_ok, lane);   // an overflow (or a dead end) after a usable shorter chunk: back to that one
    if constexpr (COMMIT) pbw_cursors_load<CAP>(L, W.ecur, lane);                     // commit
    tprev = lo; nprev = (float)done;
    Tout = T_ok;
    return c_ok;
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
    // Rule 1 by probes.  With the best fixed, the rule's left-hand side bs = H[beta] + (A[beta] - H[beta]) w1 falls as the sum
    // rises (w1 = exp(c4 rs) spl falls, beta -- a floor of a float quotient, monotone as computed -- falls, A >= H); the
    // float32 evaluation follows that to a few units in the last place.  Lane l evaluates it at mn + (mx - mn)(l + 1) / 64:
    // below the last probe that still clears the threshold by 0.1 % no key of the chunk can fire, and none is evaluated --
    // every chunk of a search but its last.  Keys above it get the exact evaluation.
    float r_safe;
    {
        const float rp = lane == 63 ? mx : mn + (mx - mn) * ((float)(lane + 1) * (1.0f / 64.0f));
        float w1;
        const float bs = pb_promising_bs(rp, best0, Fr, P.c4, L.cdfA, L.cdfH, w1);
        const u64 unsafe = ~__ballot((double)bs > Fr.p_t_pro * 1.001);
        const int u = unsafe ? __builtin_ctzll(unsafe) : 64;
        r_safe = u == 0 ? -1.0f : __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rp), u - 1));
    }
    const auto parity = [&](const PbTep &t) {
        u64 D = d0 ^ L.P[t.p0];
        if (t.wt > 1) D ^= L.P[t.p1];
        if (t.wt > 2) D ^= L.P[t.p2];
        return D;
    };
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
                if (surv) slist[nsurv + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(sm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)sm, 0u))] = (unsigned short)(lane + 64 * k);
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
                const int idx = ncand + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(cm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)cm, 0u));
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
        u64 E = 1ull << t.p0;
        if (t.wt > 1) E |= 1ull << t.p1;
        if (t.wt > 2) E |= 1ull << t.p2;
        S.best = L.rc[nbefore - 1]; S.bestD = parity(t); S.bestE = E;
        S.bestidx = S.j + rank_best + 1;
    }
    S.suc2 += nbefore;
    if (reason) {
        S.cmp += 2 * (rank_stop + 1);             // (the frontier never holds a single entry here: no one-comparison pops)
        S.suc1 += reason == 1 ? rank_stop : rank_stop + 1;
        stop = reason; ntep = S.j + rank_stop + 1;
        return 1;
    }
    S.cmp += 2 * n; S.suc1 += n;
    S.j += n; S.nlive += deltot;
    return 0;
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
    float r_safe;                     // rule 1 by probes (pbw_scan_chunk)
    {
        const float rp = lane == 63 ? mx : mn + (mx - mn) * ((float)(lane + 1) * (1.0f / 64.0f));
        float w1;
        const float bs = pb_promising_bs(rp, best0, Fr, P.c4, L.cdfA, L.cdfH, w1);
        const u64 unsafe = ~__ballot((double)bs > Fr.p_t_pro * 1.001);
        const int u = unsafe ? __builtin_ctzll(unsafe) : 64;
        r_safe = u == 0 ? -1.0f : __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rp), u - 1));
    }
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
    const auto parity = [&](const PbTep &t) {
        u64 D = d0 ^ L.P[t.p0];
        if (t.wt > 1) D ^= L.P[t.p1];
        if (t.wt > 2) D ^= L.P[t.p2];
        return D;
    };
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
                if (surv) slist[nsurv + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(sm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)sm, 0u))] = (unsigned short)((k0 + u) * 64 + lane);
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
                const int idx = ncand + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(cm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)cm, 0u));
                if (cand && idx < 16) { L.ck[idx] = ((u64)sbits << 32) | code; L.cc[idx] = c; }
                ncand += __popcll(cm);
            }
        }
        if (ncand > 16) return -1;
    }
    const auto sumbits = [](u64 key) { return (unsigned)(key >> 32); };
    unsigned sF = (unsigned)wave_min_i32((int)fs);
    if (ncand == 0) {
        if (sF == 0x7FFFFFFFu) {     // no candidate, no key fires: the whole chunk is visited and nothing else happens
            S.cmp += 2 * n; S.suc1 += n;
            S.j += n; S.nlive += deltot;
            return 0;
        }
        // no candidate, rule 1 fires: the search stops at the first key of the smallest firing sum (every key of that sum fires)
        int cs = 0;
        for (int k = 0; k < nsl; ++k) { unsigned code, sb; key_at(k, code, sb); cs += sb < sF; }
        const int rank_stop = wave_add_i32(cs);
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
        float r_safe2;
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
        u64 E = 1ull << t.p0;
        if (t.wt > 1) E |= 1ull << t.p1;
        if (t.wt > 2) E |= 1ull << t.p2;
        S.best = L.rc[nbefore - 1]; S.bestD = parity(t); S.bestE = E;
        S.bestidx = S.j + rank_best + 1;
    }
    S.suc2 += nbefore;
    if (reason) {
        S.cmp += 2 * (rank_stop + 1);             // (the frontier never holds a single entry here: no one-comparison pops)
        S.suc1 += reason == 1 ? rank_stop : rank_stop + 1;
        stop = reason; ntep = S.j + rank_stop + 1;
        return 1;
    }
    S.cmp += 2 * n; S.suc1 += n;
    S.j += n; S.nlive += deltot;
    return 0;
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
    const auto parity = [&](const PbTep &t) {
        u64 D = d0 ^ L.P[t.p0];
        if (t.wt > 1) D ^= L.P[t.p1];
        if (t.wt > 2) D ^= L.P[t.p2];
        return D;
    };
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
            const PbTep t = pbw_tep(code);
            u64 E = 1ull << t.p0;
            if (t.wt > 1) E |= 1ull << t.p1;
            if (t.wt > 2) E |= 1ull << t.p2;
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
