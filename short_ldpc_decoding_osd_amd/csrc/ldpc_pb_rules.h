// PB-OSD, the sort-free pass over a chunk of the visit order: the pieces its three scans share, and where the scans differ on purpose.
//   pbw_scan_chunk   (ldpc_pb_pass.h)  8-byte keys held in registers, one wavefront
//   pbw_scan4        (ldpc_pb_pass.h)  4-byte keys re-read from LDS, one wavefront
//   coop_scan_chunk  (ldpc_pb_coop.h)  8-byte keys, 8 or 16 wavefronts with LDS exchanges
// Each scan keeps its own loop over the keys (how a key is fetched, how many side by side, rolled or unrolled: measured) and
// its own reductions (wave_add_i32 / coop_sum / coop_min).  Behind the loop the three run the same steps: the probes of rule 1,
// the candidates in visit order, the records among them with rule 2, "the stop", the records that count, the commit.  Shared
// here: a TEP's parity discrepancy and error pattern, the probes, and the counters of the commit (pbw_commit_counts).  The
// candidate ordering, the record loop, the stop and the count of the records are written out in each scan: as shared
// functions each of them changed the machine code of its kernel at every site, in the two forms tried
// (profiles/pb_rules/README.md) -- so the INTENDED differences between the copies are listed here, once;
// whatever else differs between them behind the loop is not meant to:
//   ties            the wavefront scans compare sums only: a key whose sum equals that of a key it is counted against (among
//                   the candidates, against a record, against the last record that counts) makes them return -1, and the
//                   caller sorts.  The workgroup scan orders equal sums with pb_visit_less (visited_before): there a tie used
//                   to send ~2700 keys to one wavefront;
//   nbefore         the records that count.  Workgroup scan: all of them when rule 2 stops (the records are in visit order,
//                   equal sums included), those below the firing sum when rule 1 stops.  Wavefront scans: "the records
//                   below the stopping sum, plus one for rule 2" -- a record that ties with the stopping one is dropped by
//                   that count (tests/tools/pb_long_fuzz.py found it in the workgroup scan), and they rely on the tie
//                   above, which sends such a chunk to the sorted path;
//   a record on sF  workgroup scan only: ANY record whose sum is rule 1's smallest firing sum sF is a tie ("the first key of
//                   that sum stops" needs every key of the sum to see the same best).  The wavefront scans flag only the
//                   record on which rule 2 fired;
//   the records     are taken by every lane of a wavefront scan; in the workgroup scan by wavefront 0, which publishes the
//                   outcome through PbCoopLds::nrec / stop2 / tie0 (tie0 is never set since the candidates are ordered by
//                   visited_before: the word keeps the layout);
//   second probe    pbw_scan4 and coop_scan_chunk probe rule 1 again with the last record's cost (r_safe2) before they
//                   re-read their keys; pbw_scan_chunk has its keys in registers and re-evaluates without it.
#pragma once
#include "ldpc_pb_walk.h"

namespace ldpc {

// parity discrepancy of a TEP (d0 ^ the P' rows of its positions; an unused position is not read) / its error pattern on the MRB
__device__ __forceinline__ u64 pb_tep_parity(const u64 *P, u64 d0, const PbTep &t)
{
    u64 D = d0 ^ P[t.p0];
    if (t.wt > 1) D ^= P[t.p1];
    if (t.wt > 2) D ^= P[t.p2];
    return D;
}
__device__ __forceinline__ u64 pb_tep_mask(const PbTep &t)
{
    u64 E = 1ull << t.p0;
    if (t.wt > 1) E |= 1ull << t.p1;
    if (t.wt > 2) E |= 1ull << t.p2;
    return E;
}

// Rule 1 by probes.  With the best fixed, the rule's left-hand side bs = H[beta] + (A[beta] - H[beta]) w1 falls as the sum
// rises (w1 = exp(c4 rs) spl falls, beta -- a floor of a float quotient, monotone as computed -- falls, A >= H); the
// float32 evaluation follows that to a few units in the last place.  Lane l evaluates it at mn + (mx - mn)(l + 1) / 64:
// below the last probe that still clears the threshold by 0.1 % no key of the chunk can fire, and none is evaluated --
// every chunk of a search but its last.  Returns that probe's sum (-1: none); keys above it get the exact evaluation.
// (The second probes of pbw_scan4 and coop_scan_chunk are this function with the last record's cost, written out there.)
template <typename TA>
__device__ __forceinline__ float pb_rule1_safe_sum(float mn, float mx, float best, const PbFrame &Fr, float c4, const TA *cdfA, const TA *cdfH, int lane)
{
    const float rp = lane == 63 ? mx : mn + (mx - mn) * ((float)(lane + 1) * (1.0f / 64.0f));
    float w1;
    const float bs = pb_promising_bs(rp, best, Fr, c4, cdfA, cdfH, w1);
    const u64 unsafe = ~__ballot((double)bs > Fr.p_t_pro * 1.001);
    const int u = unsafe ? __builtin_ctzll(unsafe) : 64;
    return u == 0 ? -1.0f : __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rp), u - 1));
}

// The counters at the end of a pass: nbefore records counted; reason != 0: the search stops behind rank_stop keys of the chunk
// (returns 1, stop / ntep set), otherwise all n keys are visited and the frontier has grown by deltot (returns 0).
// (The frontier never holds a single entry here: no one-comparison pops.)
__device__ __forceinline__ int pbw_commit_counts(PbwState &S, int nbefore, int reason, int rank_stop, int n, int deltot, int &stop, int &ntep)
{
    S.suc2 += nbefore;
    if (reason) {
        S.cmp += 2 * (rank_stop + 1);
        S.suc1 += reason == 1 ? rank_stop : rank_stop + 1;
        stop = reason; ntep = S.j + rank_stop + 1;
        return 1;
    }
    S.cmp += 2 * n; S.suc1 += n;
    S.j += n; S.nlive += deltot;
    return 0;
}

}  // namespace ldpc
