// The host side that the any-shape family (ldpc_osdx_*, ldpc_osdx.hip), the high-rate family (ldpc_osdw_*, ldpc_osdw.hip) and
// the long / low-rate family (ldpc_osdl_*, ldpc_osdl.hip) share: validation, launches and the bodies of their entry points,
// written once.  Host code only; included after the family's kernel headers.  A family is a traits struct FAM with
//   tables(ctx)                     its tables in the context (OsdTables / OsdwTables / OsdlTables: n, k, d_Gcols, d_tep, ntep
//                                   and, where the family has FS-OSD, d_tep_fs, fs_off, fs_cnt under the same names); k = 0:
//                                   the code is not served
//   needs                           the sentence of its UNSUPPORTED message
//   perm_t                          the element of d_perm (uint8_t while n <= 128, uint16_t beyond); the strides of d_perm and
//                                   d_parity follow from n and k inside the kernels
//   front(t), search(t)             its front-end and scan kernels for the shape of the tables t (one kernel in the first two
//                                   families, an instantiation per shape class in the third); the same argument lists in all
//   fs(t), tep_eval(t)              its FS-OSD and one-TEP kernels, likewise
// `who` is the name of the extern "C" entry point, for the error texts.
// There is no library workspace: the decode entry points run their two launches through the caller's d_perm / d_parity, so the
// calls hold no per-stream state, allocate nothing and are graph-capturable as they are.
#pragma once

#include "ldpc_internal.h"
#include "ldpc_family_check.h"   // check_order, check_scan_algo: the validation without a kernel in sight

namespace ldpc {

// the frames of a call and the per-frame results of a scan, as the entry points receive them
struct OsdFrames {
    const float *y;
    const int32_t *index, *count;
    int64_t F;
};
struct OsdScanOut {
    uint64_t *cw;
    float *metric;
    int32_t *best, *ntep;
};

// the fused counters of a scan: only with the labels AND the counters, otherwise neither
struct OsdCounting {
    const u64 *label = nullptr;
    u64 *counts = nullptr;
};
inline OsdCounting osd_counting(const uint64_t *d_label, int64_t *d_counts)
{
    if (!d_label || !d_counts) return {};
    return {reinterpret_cast<const u64 *>(d_label), reinterpret_cast<u64 *>(d_counts)};
}

// the first checks of every entry point: the context, the frame count, whether the family serves the code
template <class FAM>
int family_open(const ldpc_ctx *ctx, int64_t F, const char *who)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "%s: bad arguments", who);
    return FAM::tables(ctx).k ? LDPC_OK : fail(LDPC_E_UNSUPPORTED, "%s; this code is (%d,%d)", FAM::needs, ctx->code.n, ctx->code.k);
}

// the pointers every scan with F > 0 needs
inline int scan_required(const OsdFrames &fr, const void *d_perm, const uint64_t *d_parity, const OsdScanOut &o, const char *who)
{
    return first_null(who, {{"d_y", fr.y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_cw", o.cw}});
}

template <class FAM>
int family_launch_front(const ldpc_ctx *ctx, const OsdFrames &fr, typename FAM::perm_t *d_perm, uint64_t *d_parity, int32_t *d_nswaps, hipStream_t s)
{
    const auto &t = FAM::tables(ctx);
    hipLaunchKernelGGL(FAM::front(t), dim3(frame_grid(fr.F)), dim3(64), 0, s, fr.y, fr.index, fr.count, (long long)fr.F, t.n, t.k, t.d_Gcols,
                       d_perm, reinterpret_cast<u64 *>(d_parity), d_nswaps);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

template <class FAM>
int family_launch_search(const ldpc_ctx *ctx, const OsdFrames &fr, const typename FAM::perm_t *d_perm, const uint64_t *d_parity, int order,
                         const OsdScanOut &o, OsdCounting c, hipStream_t s)
{
    const auto &t = FAM::tables(ctx);
    hipLaunchKernelGGL(FAM::search(t), dim3(frame_grid(fr.F)), dim3(64), 0, s, fr.y, fr.index, fr.count, (long long)fr.F, t.n, t.k, d_perm,
                       reinterpret_cast<const u64 *>(d_parity), t.d_tep, (int)t.ntep[order], reinterpret_cast<u64 *>(o.cw), o.metric,
                       o.best, o.ntep, c.label, c.counts);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

template <class FAM>
int family_launch_fs(const ldpc_ctx *ctx, const OsdFrames &fr, const typename FAM::perm_t *d_perm, const uint64_t *d_parity,
                     const ldpc_osd_params *p, const OsdScanOut &o, OsdCounting c, hipStream_t s)
{
    const auto &t = FAM::tables(ctx);
    hipLaunchKernelGGL(FAM::fs(t), dim3(frame_grid(fr.F)), dim3(64), 0, s, fr.y, fr.index, fr.count, (long long)fr.F, t.n, t.k, d_perm,
                       reinterpret_cast<const u64 *>(d_parity), t.d_tep_fs, fs_params(p, t.n, t.k, t.fs_off, t.fs_cnt),
                       reinterpret_cast<u64 *>(o.cw), o.metric, o.best, o.ntep, c.label, c.counts);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

template <class FAM>
int family_front(ldpc_ctx *ctx, const OsdFrames &fr, typename FAM::perm_t *d_perm, uint64_t *d_parity, int32_t *d_nswaps, void *stream, const char *who)
{
    if (int rc = family_open<FAM>(ctx, fr.F, who)) return rc;
    if (fr.F == 0) return LDPC_OK;
    if (int rc = first_null(who, {{"d_y", fr.y}, {"d_perm", d_perm}, {"d_parity", d_parity}})) return rc;
    return family_launch_front<FAM>(ctx, fr, d_perm, d_parity, d_nswaps, (hipStream_t)stream);
}

template <class FAM>
int family_search(ldpc_ctx *ctx, const OsdFrames &fr, const typename FAM::perm_t *d_perm, const uint64_t *d_parity, int32_t order, const OsdScanOut &o,
                  void *stream, const char *who)
{
    if (int rc = family_open<FAM>(ctx, fr.F, who)) return rc;
    if (int rc = check_order(order, who)) return rc;
    if (fr.F == 0) return LDPC_OK;
    if (int rc = scan_required(fr, d_perm, d_parity, o, who)) return rc;
    return family_launch_search<FAM>(ctx, fr, d_perm, d_parity, order, o, {}, (hipStream_t)stream);
}

template <class FAM>
int family_decode(ldpc_ctx *ctx, const OsdFrames &fr, int32_t order, typename FAM::perm_t *d_perm, uint64_t *d_parity, const OsdScanOut &o,
                  OsdCounting c, void *stream, const char *who)
{
    if (int rc = family_open<FAM>(ctx, fr.F, who)) return rc;
    if (int rc = check_order(order, who)) return rc;
    if (fr.F == 0) return LDPC_OK;
    if (int rc = scan_required(fr, d_perm, d_parity, o, who)) return rc;
    if (int rc = family_launch_front<FAM>(ctx, fr, d_perm, d_parity, nullptr, (hipStream_t)stream)) return rc;
    return family_launch_search<FAM>(ctx, fr, d_perm, d_parity, order, o, c, (hipStream_t)stream);
}

// A scan that takes ldpc_osd_params (FS-OSD in every family, PB-OSD in the first two; each family launches its own PB kernel):
// what its entry points check and launch.  PERM: the family's perm_t.
template <class PERM>
struct OsdScan {
    int algo;
    const char *algo_name;
    bool aux_allowed;   // the scan writes params->d_aux
    int (*launch)(const ldpc_ctx *, const OsdFrames &, const PERM *, const uint64_t *, const ldpc_osd_params *, const OsdScanOut &,
                  OsdCounting, hipStream_t);
};
template <class FAM>
constexpr OsdScan<typename FAM::perm_t> fs_scan{LDPC_OSD_FS, "LDPC_OSD_FS", false, family_launch_fs<FAM>};

// the params of the entry points of `scan` for a code with k information bits: its algorithm, an order up to min(3, k), and
// nothing that only ldpc_osd_search / ldpc_osd_decode serve
template <class PERM>
int check_scan_params(int k, const ldpc_osd_params *p, const OsdScan<PERM> &scan, const char *who)
{
    return check_scan_algo(k, p, scan.algo, scan.algo_name, scan.aux_allowed, who);
}

template <class FAM>
int family_scan_search(ldpc_ctx *ctx, const OsdFrames &fr, const typename FAM::perm_t *d_perm, const uint64_t *d_parity,
                       const ldpc_osd_params *params, const OsdScan<typename FAM::perm_t> &scan, const OsdScanOut &o, void *stream, const char *who)
{
    if (int rc = family_open<FAM>(ctx, fr.F, who)) return rc;
    if (int rc = check_scan_params(FAM::tables(ctx).k, params, scan, who)) return rc;
    if (fr.F == 0) return LDPC_OK;
    if (int rc = scan_required(fr, d_perm, d_parity, o, who)) return rc;
    return scan.launch(ctx, fr, d_perm, d_parity, params, o, {}, (hipStream_t)stream);
}

template <class FAM>
int family_scan_decode(ldpc_ctx *ctx, const OsdFrames &fr, const ldpc_osd_params *params, const OsdScan<typename FAM::perm_t> &scan,
                       typename FAM::perm_t *d_perm, uint64_t *d_parity, const OsdScanOut &o, OsdCounting c, void *stream, const char *who)
{
    if (int rc = family_open<FAM>(ctx, fr.F, who)) return rc;
    if (int rc = check_scan_params(FAM::tables(ctx).k, params, scan, who)) return rc;
    if (fr.F == 0) return LDPC_OK;
    if (int rc = scan_required(fr, d_perm, d_parity, o, who)) return rc;
    if (int rc = family_launch_front<FAM>(ctx, fr, d_perm, d_parity, nullptr, (hipStream_t)stream)) return rc;
    return scan.launch(ctx, fr, d_perm, d_parity, params, o, c, (hipStream_t)stream);
}

template <class FAM>
int family_tep_eval(ldpc_ctx *ctx, const OsdFrames &fr, const typename FAM::perm_t *d_perm, const uint64_t *d_parity, const uint64_t *d_mask,
                    uint64_t *d_cw, float *d_metric, int32_t *d_hd, void *stream, const char *who)
{
    if (int rc = family_open<FAM>(ctx, fr.F, who)) return rc;
    if (fr.F == 0) return LDPC_OK;
    if (int rc = first_null(who, {{"d_y", fr.y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_mask", d_mask}, {"d_cw", d_cw}})) return rc;
    const auto &t = FAM::tables(ctx);
    hipLaunchKernelGGL(FAM::tep_eval(t), dim3(frame_grid(fr.F)), dim3(64), 0, (hipStream_t)stream, fr.y, fr.index, fr.count, (long long)fr.F,
                       t.n, t.k, d_perm, reinterpret_cast<const u64 *>(d_parity), reinterpret_cast<const u64 *>(d_mask),
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_hd);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

// ---------------------------------------------------------------------------------------
// The OSD stage of ldpc_family_pipeline_run (ldpc_api.hip) on one family: its two launches, front end and scan apart (the
// pipeline records a timing event in between), behind one signature.  d_perm travels as void *: its element is the family's
// perm_t.  PB: the family's PB scan (each family launches its own kernel).  The checks are family_pipeline_check's
// (ldpc_family_check.h), which needs no kernel.
// ---------------------------------------------------------------------------------------
struct FamilyStage {
    int (*front)(const ldpc_ctx *, const OsdFrames &, void *d_perm, uint64_t *d_parity, hipStream_t);
    int (*scan)(const ldpc_ctx *, const OsdFrames &, const void *d_perm, const uint64_t *d_parity, const ldpc_osd_params *, const OsdScanOut &,
                OsdCounting, hipStream_t);
};

template <class FAM, const OsdScan<typename FAM::perm_t> &PB>
struct FamilyStageOf {
    using perm_t = typename FAM::perm_t;
    static int front(const ldpc_ctx *ctx, const OsdFrames &fr, void *d_perm, uint64_t *d_parity, hipStream_t s)
    {
        return family_launch_front<FAM>(ctx, fr, static_cast<perm_t *>(d_perm), d_parity, nullptr, s);
    }
    static int scan(const ldpc_ctx *ctx, const OsdFrames &fr, const void *d_perm, const uint64_t *d_parity, const ldpc_osd_params *p,
                    const OsdScanOut &o, OsdCounting c, hipStream_t s)
    {
        const perm_t *perm = static_cast<const perm_t *>(d_perm);
        if (p->algo == LDPC_OSD_FS) return family_launch_fs<FAM>(ctx, fr, perm, d_parity, p, o, c, s);
        if (p->algo == LDPC_OSD_PB) return PB.launch(ctx, fr, perm, d_parity, p, o, c, s);
        return family_launch_search<FAM>(ctx, fr, perm, d_parity, p->order, o, c, s);
    }
    static FamilyStage make() { return {front, scan}; }
};
// one per family, each beside the family's PB scan: ldpc_osdx.hip, ldpc_osdw.hip, ldpc_osdl_pb.hip
const FamilyStage &osdx_stage();
const FamilyStage &osdw_stage();
const FamilyStage &osdl_stage();

}  // namespace ldpc
