// Host-only validation of ldpc_dlosd_pipeline_run (ldpc_api.hip), and the sentence with which each H-form family refuses a
// code (the families' own checks in ldpc_hosd.hip and ldpc_hosdl.hip call hosd_family_refusal, so the pipeline's refusal is
// theirs word for word).  As ldpc_family_check.h: no kernel in sight, so the same text builds into the CPU-only sanitizer
// library (ldpc_sanitizer_checks.cpp) and is run there by a stand-alone program (ldpc_sanitizer_main.cpp) on contexts made by hand.
#pragma once

#include "ldpc_internal.h"
#include "ldpc_hosd_limits.h"

namespace ldpc {

// whether the context serves `family` (LDPC_HOSD_FAMILY_128 / _X / _W / _L)
inline bool hosd_family_ok(const ldpc_ctx *ctx, int family)
{
    return family == LDPC_HOSD_FAMILY_128 ? ctx->hosd_ok : family == LDPC_HOSD_FAMILY_X ? ctx->hosdx_ok
           : family == LDPC_HOSD_FAMILY_W ? ctx->hosdw_ok : ctx->hosdl_ok;
}

// LDPC_E_UNSUPPORTED with the sentence of `family`, for the entry point `who`
inline int hosd_family_refusal(const ldpc_ctx *ctx, int family, const char *who)
{
    const ldpc_code &c = ctx->code;
    switch (family) {
    case LDPC_HOSD_FAMILY_128:
        return fail(LDPC_E_UNSUPPORTED, "H-form OSD kernels need n=128, m=k=64; this code is n=%d m=%d k=%d", c.n, c.m, c.k);
    case LDPC_HOSD_FAMILY_X:
        return fail(LDPC_E_UNSUPPORTED, "%s: H-form OSD kernels need 1 <= k <= 64 and an H of exactly n-k <= 64 rows; this H has %d rows, "
                    "n-k = %d, code (%d,%d)", who, c.m, c.n - c.k, c.n, c.k);
    case LDPC_HOSD_FAMILY_W:
        return fail(LDPC_E_UNSUPPORTED, "%s: wide H-form OSD kernels need n <= 128, an H of 1 <= R <= 127 rows and 1 <= n-k <= 64; this H has "
                    "%d rows, n-k = %d, code (%d,%d)", who, c.m, c.n - c.k, c.n, c.k);
    default:
        return fail(LDPC_E_UNSUPPORTED, "%s: long H-form OSD kernels need n <= 384, an H of 1 <= R <= 192 rows, 1 <= n-k <= 192 and "
                    "1 <= k <= 192; this H has %d rows, n-k = %d, code (%d,%d)", who, c.m, c.n - c.k, c.n, c.k);
    }
}

// Everything ldpc_dlosd_pipeline_run refuses, before any launch.  On LDPC_OK with the stage on, *family is the family that
// runs (AUTO resolved: hosd on (128,64), else hosdx, else hosdw, else hosdl) and *F the rows the list buffers hold.
inline int dlosd_pipeline_check(const ldpc_ctx *ctx, const ldpc_dlosd_pipeline *p, const char *who, int *family, int64_t *F)
{
    *family = LDPC_HOSD_FAMILY_AUTO;
    *F = 0;
    if (!ctx || !p) return fail(LDPC_E_ARG, "%s: null argument", who);
    if (p->B < 0 || p->B > 0x7FFFFFFFLL || (p->B > 0 && !p->d_llr)) return fail(LDPC_E_ARG, "%s: d_llr is NULL or B outside 0..2^31-1", who);
    if (p->T < 0 || p->T > kMaxIters) return fail(LDPC_E_ARG, "%s: T=%d outside 0..%d", who, p->T, kMaxIters);
    if (p->T > 0 && !p->alpha) return fail(LDPC_E_ARG, "%s: alpha is NULL", who);
    if (!p->d_hard || !p->d_fail) return fail(LDPC_E_ARG, "%s: d_hard and d_fail are required", who);
    if (p->timing_slot >= LDPC_TIMING_SLOTS || (p->timing_slot >= 0 && !ctx->timing)) return fail(LDPC_E_ARG, "%s: timing_slot %d", who, p->timing_slot);
    if (!p->osd_enable) return LDPC_OK;
    int fam = p->family;
    if (fam == LDPC_HOSD_FAMILY_AUTO)
        fam = ctx->hosd_ok ? LDPC_HOSD_FAMILY_128 : ctx->hosdx_ok ? LDPC_HOSD_FAMILY_X : ctx->hosdw_ok ? LDPC_HOSD_FAMILY_W : LDPC_HOSD_FAMILY_L;
    if (fam < LDPC_HOSD_FAMILY_128 || fam > LDPC_HOSD_FAMILY_L)
        return fail(LDPC_E_ARG, "%s: family %d is no LDPC_HOSD_FAMILY_* value", who, p->family);
    if (!hosd_family_ok(ctx, fam)) return hosd_family_refusal(ctx, fam, who);
    if (p->osd_capacity < 0) return fail(LDPC_E_ARG, "%s: osd_capacity %lld is negative", who, (long long)p->osd_capacity);
    if (p->win < 1 || p->win > kSlideMaxWin) return fail(LDPC_E_ARG, "%s: win %d outside 1..%d", who, p->win, kSlideMaxWin);
    if (p->nblk < p->win) return fail(LDPC_E_ARG, "%s: nblk %d is below win %d", who, p->nblk, p->win);
    if (p->nblk > kHosdMaxBlocks) return fail(LDPC_E_UNSUPPORTED, "%s: nblk %d TEP blocks, at most %d", who, p->nblk, kHosdMaxBlocks);
    if (p->group < 0) return fail(LDPC_E_ARG, "%s: group %d is negative", who, p->group);
    int rc;
    if ((rc = first_null(who, {{"fcn_weights", p->fcn_weights}}))) return rc;
    if (p->n_fcn_weights != fcn_weight_count(p->win))
        return fail(LDPC_E_ARG, "%s: n_fcn_weights %d, a window of %d takes %d", who, p->n_fcn_weights, p->win, fcn_weight_count(p->win));
    if (p->cnn_weights) {
        const int L = p->T + 1;
        if (L < 7) return fail(LDPC_E_ARG, "%s: cnn_weights with T %d (the CNN needs T + 1 >= 7 rows)", who, p->T);
        if (p->n_cnn_weights != dia_weight_count(L))
            return fail(LDPC_E_ARG, "%s: n_cnn_weights %d, T + 1 = %d rows take %d", who, p->n_cnn_weights, L, dia_weight_count(L));
        if ((rc = first_null(who, {{"d_rows", p->d_rows}, {"d_order_llr", p->d_order_llr}}))) return rc;
    }
    if ((rc = first_null(who, {{"d_index", p->d_index}, {"d_count", p->d_count}, {"d_teps", p->d_teps}, {"d_block_off", p->d_block_off},
                               {"d_metric_llr", p->d_metric_llr}, {"d_lri", p->d_lri}, {"d_uidx", p->d_uidx}, {"d_M", p->d_M},
                               {"d_cw", p->d_cw}}))) return rc;
    if (p->d_label_bits && !p->d_list_labels) return fail(LDPC_E_ARG, "%s: d_list_labels is NULL (required with d_label_bits)", who);
    if (p->d_dl_counts && !p->d_deep_limit) return fail(LDPC_E_ARG, "%s: d_deep_limit is NULL (required with d_dl_counts)", who);
    *family = fam;
    *F = p->osd_capacity > 0 && p->osd_capacity < p->B ? p->osd_capacity : p->B;
    return LDPC_OK;
}

}  // namespace ldpc
