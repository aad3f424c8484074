// Host-only validation shared by the entry points of the three G-form OSD families (ldpc_osd_family.h), ldpc_osd_merge
// (ldpc_util.hip) and ldpc_family_pipeline_run (ldpc_api.hip): everything these calls refuse before their first launch, with no
// kernel in sight, so that the same text also builds into the CPU-only sanitizer library (ldpc_sanitizer_stubs.cpp) and is run
// there by a stand-alone program (ldpc_sanitizer_main.cpp) on contexts made by hand.
#pragma once

#include "ldpc_internal.h"

namespace ldpc {

// the sentence of each family's UNSUPPORTED message
constexpr const char *kOsdxNeeds = "the any-shape OSD kernels need 1 <= k <= 64 and 1 <= n-k <= 64";
constexpr const char *kOsdwNeeds = "the high-rate OSD kernels need 1 <= n-k <= 64 and n <= 128";
constexpr const char *kOsdlNeeds = "the long / low-rate OSD kernels need n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192";

inline int check_order(int order, const char *who)
{
    return order < 0 || order > 3 ? fail(LDPC_E_ARG, "%s: order %d outside 0..3", who, order) : LDPC_OK;
}

// the members of params that only ldpc_osd_search / ldpc_osd_decode serve: flags, y_frames, and d_aux outside PB-OSD
inline int check_scan_extras(const ldpc_osd_params *p, bool aux_allowed, const char *who)
{
    if (p->flags != 0) return fail(LDPC_E_ARG, "%s: flags 0x%x are not served here (flags must be 0)", who, (unsigned)p->flags);
    if (p->d_aux && !aux_allowed) return fail(LDPC_E_ARG, "%s: d_aux is not served here (it must be NULL)", who);
    if (p->y_frames != 0) return fail(LDPC_E_ARG, "%s: y_frames %lld is not served here (it must be 0)", who, (long long)p->y_frames);
    return LDPC_OK;
}

// the params of a scan that takes ldpc_osd_params, for a code with k information bits: its algorithm, an order up to min(3, k),
// and nothing that only ldpc_osd_search / ldpc_osd_decode serve
inline int check_scan_algo(int k, const ldpc_osd_params *p, int algo, const char *algo_name, bool aux_allowed, const char *who)
{
    if (!p) return fail(LDPC_E_ARG, "%s: params is NULL", who);
    if (p->algo != algo) return fail(LDPC_E_ARG, "%s: algo %d is not %s", who, p->algo, algo_name);
    const int omax = k < 3 ? k : 3;
    if (p->order < 0 || p->order > omax) return fail(LDPC_E_ARG, "%s: order %d outside 0..%d", who, p->order, omax);
    return check_scan_extras(p, aux_allowed, who);
}

// ldpc_osd_merge: LDPC_OK with *launch = false where the call has nothing to do
inline int osd_merge_check(const ldpc_ctx *ctx, const uint64_t *d_cw, const int32_t *d_index, const int32_t *d_count, int64_t F,
                           const uint64_t *d_hard, const uint64_t *d_label_bits, const int64_t *d_counts, bool *launch)
{
    *launch = false;
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "ldpc_osd_merge: bad arguments");
    if (F == 0) return LDPC_OK;
    if (int rc = first_null("ldpc_osd_merge", {{"d_cw", d_cw}, {"d_index", d_index}, {"d_count", d_count}})) return rc;
    *launch = d_hard || (d_label_bits && d_counts);   // labels and counters: a pair or neither, as in the family decode calls
    return LDPC_OK;
}

// A family as ldpc_family_pipeline_run's validation sees it: k of its tables in the context (0: the code is not served) and
// the sentence of its refusal.  `family`: LDPC_OSD_FAMILY_X / _W / _L.
struct FamilyGate {
    int k;
    const char *needs;
};
inline FamilyGate family_gate(const ldpc_ctx *ctx, int family)
{
    return family == LDPC_OSD_FAMILY_X ? FamilyGate{ctx->osd_tables.k, kOsdxNeeds}
           : family == LDPC_OSD_FAMILY_W ? FamilyGate{ctx->osdw_tables.k, kOsdwNeeds} : FamilyGate{ctx->osdl_tables.k, kOsdlNeeds};
}

// Everything ldpc_family_pipeline_run refuses, before any launch.  On LDPC_OK with the OSD stage on, *family is the family
// that runs (AUTO resolved: the first of osdx, osdw, osdl that serves the code) and *F the frames the OSD buffers hold.
inline int family_pipeline_check(const ldpc_ctx *ctx, const ldpc_family_pipeline *p, const char *who, int *family, int64_t *F)
{
    *family = LDPC_OSD_FAMILY_AUTO;
    *F = 0;
    if (!ctx || !p) return fail(LDPC_E_ARG, "%s: null argument", who);
    if (p->B < 0 || p->B > 0x7FFFFFFFLL || (p->B > 0 && !p->d_llr)) return fail(LDPC_E_ARG, "%s: d_llr is NULL or B outside 0..2^31-1", who);
    if (p->T < 0 || p->T > kMaxIters) return fail(LDPC_E_ARG, "%s: T=%d outside 0..%d", who, p->T, kMaxIters);
    if (p->T > 0 && !p->alpha) return fail(LDPC_E_ARG, "%s: alpha is NULL", who);
    if (!p->d_hard || !p->d_fail) return fail(LDPC_E_ARG, "%s: d_hard and d_fail are required", who);
    if (p->timing_slot >= LDPC_TIMING_SLOTS || (p->timing_slot >= 0 && !ctx->timing)) return fail(LDPC_E_ARG, "%s: timing_slot %d", who, p->timing_slot);
    if (!p->osd_enable) return LDPC_OK;
    int fam = p->family;
    if (fam == LDPC_OSD_FAMILY_AUTO)
        fam = ctx->osd_tables.k ? LDPC_OSD_FAMILY_X : ctx->osdw_tables.k ? LDPC_OSD_FAMILY_W : LDPC_OSD_FAMILY_L;
    if (fam != LDPC_OSD_FAMILY_X && fam != LDPC_OSD_FAMILY_W && fam != LDPC_OSD_FAMILY_L)
        return fail(LDPC_E_ARG, "%s: family %d is no LDPC_OSD_FAMILY_* value", who, p->family);
    const FamilyGate gate = family_gate(ctx, fam);
    if (!gate.k) return fail(LDPC_E_UNSUPPORTED, "%s; this code is (%d,%d)", gate.needs, ctx->code.n, ctx->code.k);   // (the families' own text)
    int rc;
    switch (p->osd.algo) {
    case LDPC_OSD_CONVENTIONAL:
        if ((rc = check_order(p->osd.order, who)) || (rc = check_scan_extras(&p->osd, false, who))) return rc;
        break;
    case LDPC_OSD_FS:
        if ((rc = check_scan_algo(gate.k, &p->osd, LDPC_OSD_FS, "LDPC_OSD_FS", false, who))) return rc;
        break;
    case LDPC_OSD_PB:
        if ((rc = check_scan_algo(gate.k, &p->osd, LDPC_OSD_PB, "LDPC_OSD_PB", true, who))) return rc;
        break;
    default:
        return fail(LDPC_E_ARG, "%s: algo %d is none of LDPC_OSD_CONVENTIONAL, LDPC_OSD_FS and LDPC_OSD_PB", who, p->osd.algo);
    }
    if (p->osd_capacity < 0) return fail(LDPC_E_ARG, "%s: osd_capacity %lld is negative", who, (long long)p->osd_capacity);
    if ((rc = first_null(who, {{"d_index", p->d_index}, {"d_count", p->d_count}, {"d_perm", p->d_perm}, {"d_parity", p->d_parity},
                               {"d_cw", p->d_cw}}))) return rc;
    *family = fam;
    *F = p->osd_capacity > 0 && p->osd_capacity < p->B ? p->osd_capacity : p->B;
    return LDPC_OK;
}

}  // namespace ldpc
