// OSD for high-rate short codes: the host side of ldpc_osdw_* (validation, launches; device code: ldpc_osdw.h).
// For every code with n <= 128 and 1 <= n - k <= 64, hence k up to 127: the front end, the conventional order-p scan (device
// code: ldpc_osdw.h), FS-OSD and the one-TEP primitive (ldpc_osdw_fs.h).
// PB-OSD stays with ldpc_osdx_pb_* (k <= 64), the one-call pipeline with the (128,64) kernels.
// The two-word G columns and the TEP tables of k are the context's OsdwTables (ldpc_osd_tables.h), uploaded by ldpc_ctx_create.
// There is no library workspace: the decode entry points run their two launches through the caller's d_perm / d_parity, so the
// calls hold no per-stream state, allocate nothing and are graph-capturable as they are.
#include "ldpc_osdw_fs.h"

namespace ldpc {

static int need_osdw(const ldpc_ctx *ctx)
{
    return ctx->osdw_tables.k ? LDPC_OK
                              : fail(LDPC_E_UNSUPPORTED, "the high-rate OSD kernels need 1 <= n-k <= 64 and n <= 128; this code is (%d,%d)",
                                     ctx->code.n, ctx->code.k);
}

// one wavefront per workgroup, a workgroup per frame up to 65536 (then strided: a wavefront decodes several frames in turn)
static unsigned osdw_grid(int64_t F) { return (unsigned)(F < 65536 ? F : 65536); }

static int osdw_launch_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, uint8_t *d_perm,
                             uint64_t *d_parity, int32_t *d_nswaps, hipStream_t s)
{
    const OsdwTables &t = ctx->osdw_tables;
    hipLaunchKernelGGL(osdw_front_kernel, dim3(osdw_grid(F)), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, t.n, t.k, t.d_Gcols,
                       d_perm, reinterpret_cast<u64 *>(d_parity), d_nswaps);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

// label / counts: the fused counters of the scan, only with the labels AND the counters, otherwise neither
static int osdw_launch_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                              const uint8_t *d_perm, const uint64_t *d_parity, int order, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                              int32_t *d_ntep, const uint64_t *d_label, int64_t *d_counts, hipStream_t s)
{
    const OsdwTables &t = ctx->osdw_tables;
    const bool counting = d_label && d_counts;
    hipLaunchKernelGGL(osdw_search_kernel, dim3(osdw_grid(F)), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, t.n, t.k, d_perm,
                       reinterpret_cast<const u64 *>(d_parity), t.d_tep, (int)t.ntep[order], reinterpret_cast<u64 *>(d_cw), d_metric,
                       d_best, d_ntep, counting ? reinterpret_cast<const u64 *>(d_label) : nullptr,
                       counting ? reinterpret_cast<u64 *>(d_counts) : nullptr);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

// every check of the FS entry points before a launch (osdx_fs_check, ldpc_osdx.hip, with the limits of this family);
// `required`: the pointers a call with F > 0 needs
static int osdw_fs_check(const ldpc_ctx *ctx, const ldpc_osd_params *p, int64_t F, std::initializer_list<NamedPtr> required, const char *who)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "%s: bad arguments", who);
    if (int rc = need_osdw(ctx)) return rc;
    if (!p) return fail(LDPC_E_ARG, "%s: params is NULL", who);
    if (p->algo != LDPC_OSD_FS) return fail(LDPC_E_ARG, "%s: algo %d is not LDPC_OSD_FS", who, p->algo);
    const int omax = ctx->osdw_tables.k < 3 ? ctx->osdw_tables.k : 3;
    if (p->order < 0 || p->order > omax) return fail(LDPC_E_ARG, "%s: order %d outside 0..%d", who, p->order, omax);
    if (p->flags != 0) return fail(LDPC_E_ARG, "%s: flags 0x%x are not served here (flags must be 0)", who, (unsigned)p->flags);
    if (p->d_aux) return fail(LDPC_E_ARG, "%s: d_aux is not served here (it must be NULL)", who);
    if (p->y_frames != 0) return fail(LDPC_E_ARG, "%s: y_frames %lld is not served here (it must be 0)", who, (long long)p->y_frames);
    return F > 0 ? first_null(who, required) : LDPC_OK;
}

static int osdw_launch_fs(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                          const uint8_t *d_perm, const uint64_t *d_parity, const ldpc_osd_params *p, uint64_t *d_cw, float *d_metric,
                          int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label, int64_t *d_counts, hipStream_t s)
{
    const OsdwTables &t = ctx->osdw_tables;
    const bool counting = d_label && d_counts;
    hipLaunchKernelGGL(osdw_fs_kernel, dim3(osdw_grid(F)), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, t.n, t.k, d_perm,
                       reinterpret_cast<const u64 *>(d_parity), t.d_tep_fs, fs_params(p, t.n, t.k, t.fs_off, t.fs_cnt),
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_best, d_ntep, counting ? reinterpret_cast<const u64 *>(d_label) : nullptr,
                       counting ? reinterpret_cast<u64 *>(d_counts) : nullptr);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // namespace ldpc

using namespace ldpc;

extern "C" {

int ldpc_osdw_supported(const ldpc_ctx *ctx) { return ctx && ctx->osdw_tables.k ? 1 : 0; }

int ldpc_osdw_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, uint8_t *d_perm,
                    uint64_t *d_parity, int32_t *d_nswaps, void *stream)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "ldpc_osdw_front: bad arguments");
    if (int rc = need_osdw(ctx)) return rc;
    if (F == 0) return LDPC_OK;
    if (int rc = first_null("ldpc_osdw_front", {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}})) return rc;
    return osdw_launch_front(ctx, d_y, d_index, d_count, F, d_perm, d_parity, d_nswaps, (hipStream_t)stream);
}

int ldpc_osdw_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                     const uint64_t *d_parity, int32_t order, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
                     void *stream)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "ldpc_osdw_search: bad arguments");
    if (int rc = need_osdw(ctx)) return rc;
    if (order < 0 || order > 3) return fail(LDPC_E_ARG, "ldpc_osdw_search: order %d outside 0..3", order);
    if (F == 0) return LDPC_OK;
    if (int rc = first_null("ldpc_osdw_search", {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_cw", d_cw}})) return rc;
    return osdw_launch_search(ctx, d_y, d_index, d_count, F, d_perm, d_parity, order, d_cw, d_metric, d_best, d_ntep, nullptr, nullptr,
                              (hipStream_t)stream);
}

int ldpc_osdw_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, int32_t order,
                     uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
                     const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "ldpc_osdw_decode: bad arguments");
    if (int rc = need_osdw(ctx)) return rc;
    if (order < 0 || order > 3) return fail(LDPC_E_ARG, "ldpc_osdw_decode: order %d outside 0..3", order);
    if (F == 0) return LDPC_OK;
    if (int rc = first_null("ldpc_osdw_decode", {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_cw", d_cw}})) return rc;
    if (int rc = osdw_launch_front(ctx, d_y, d_index, d_count, F, d_perm, d_parity, nullptr, (hipStream_t)stream)) return rc;
    return osdw_launch_search(ctx, d_y, d_index, d_count, F, d_perm, d_parity, order, d_cw, d_metric, d_best, d_ntep, d_label_bits,
                              d_counts, (hipStream_t)stream);
}

int ldpc_osdw_fs_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                        const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                        int32_t *d_ntep, void *stream)
{
    if (int rc = osdw_fs_check(ctx, params, F, {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_cw", d_cw}},
                               "ldpc_osdw_fs_search")) return rc;
    if (F == 0) return LDPC_OK;
    return osdw_launch_fs(ctx, d_y, d_index, d_count, F, d_perm, d_parity, params, d_cw, d_metric, d_best, d_ntep, nullptr, nullptr,
                          (hipStream_t)stream);
}

int ldpc_osdw_fs_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric,
                        int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    if (int rc = osdw_fs_check(ctx, params, F, {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_cw", d_cw}},
                               "ldpc_osdw_fs_decode")) return rc;
    if (F == 0) return LDPC_OK;
    if (int rc = osdw_launch_front(ctx, d_y, d_index, d_count, F, d_perm, d_parity, nullptr, (hipStream_t)stream)) return rc;
    return osdw_launch_fs(ctx, d_y, d_index, d_count, F, d_perm, d_parity, params, d_cw, d_metric, d_best, d_ntep, d_label_bits, d_counts,
                          (hipStream_t)stream);
}

int ldpc_osdw_tep_eval(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                       const uint64_t *d_parity, const uint64_t *d_mask, uint64_t *d_cw, float *d_metric, int32_t *d_hd, void *stream)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "ldpc_osdw_tep_eval: bad arguments");
    if (int rc = need_osdw(ctx)) return rc;
    if (F == 0) return LDPC_OK;
    if (int rc = first_null("ldpc_osdw_tep_eval", {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_mask", d_mask}, {"d_cw", d_cw}}))
        return rc;
    hipLaunchKernelGGL(osdw_tep_eval_kernel, dim3(osdw_grid(F)), dim3(64), 0, (hipStream_t)stream, d_y, d_index, d_count, (long long)F,
                       ctx->osdw_tables.n, ctx->osdw_tables.k, d_perm, reinterpret_cast<const u64 *>(d_parity),
                       reinterpret_cast<const u64 *>(d_mask), reinterpret_cast<u64 *>(d_cw), d_metric, d_hd);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // extern "C"
