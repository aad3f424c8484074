// PB-OSD stage 2, the chunks of the visit order (pb_wave_kernel, and the workgroup kernel's solo path): a frame's tables and chunk in
// LDS (PbWaveLds), the key format, the items and their cursors, the walk that produces a chunk (pbw_walk) and the choice of its
// bound (pb_bound_guess, pbw_next_chunk).  What judges a chunk: ldpc_pb_rules.h, ldpc_pb_pass.h.
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
                const int p = tail + wave_lane_rank(act);
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
        const int pos = wave_lane_rank(act, (unsigned)cnt);
        const int pos2 = wave_lane_rank(act2, (unsigned)(cnt + __popcll(act)));
        const u64 more = __ballot(again);
        const int nt = tail + wave_lane_rank(more);
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

}  // namespace ldpc
