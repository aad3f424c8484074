// OSD for short codes of any shape: the host side of ldpc_osdx_* (context tables, validation, launches).
// For every code with 1 <= k <= 64 and 1 <= n - k <= 64: the front end, the conventional order-p scan (device code:
// ldpc_osdx.h), FS-OSD and the one-TEP primitive (ldpc_osdx_fs.h) and PB-OSD (ldpc_osdx_pb.h).  The PB tuning and routes and the
// one-call pipeline stay with the (128,64) kernels of ldpc_osd.hip / ldpc_osd_pb.hip.
// The G columns and the TEP tables are the context's OsdTables (ldpc_osd_tables.h), the set the (128,64) kernels read as well.
// There is no library workspace: the decode entry points run their two launches through the caller's d_perm / d_parity, so the
// calls hold no per-stream state, allocate nothing and are graph-capturable as they are.
#include <cmath>

#include "ldpc_osdx_fs.h"
#include "ldpc_osdx_pb.h"

namespace ldpc {

static int need_osdx(const ldpc_ctx *ctx)
{
    return ctx->osd_tables.k ? LDPC_OK
                             : fail(LDPC_E_UNSUPPORTED, "the any-shape OSD kernels need 1 <= k <= 64 and 1 <= n-k <= 64; this code is (%d,%d)",
                                    ctx->code.n, ctx->code.k);
}

// one wavefront per workgroup, a workgroup per frame up to 65536 (then strided: a wavefront decodes several frames in turn)
static unsigned osdx_grid(int64_t F) { return (unsigned)(F < 65536 ? F : 65536); }

// the fused counters of a scan: only with the labels AND the counters, otherwise neither
struct OsdxCounting {
    const u64 *label = nullptr;
    u64 *counts = nullptr;
};
static OsdxCounting osdx_counting(const uint64_t *d_label, int64_t *d_counts)
{
    if (!d_label || !d_counts) return {};
    return {reinterpret_cast<const u64 *>(d_label), reinterpret_cast<u64 *>(d_counts)};
}

static int osdx_launch_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, uint8_t *d_perm,
                             uint64_t *d_parity, int32_t *d_nswaps, hipStream_t s)
{
    const OsdTables &t = ctx->osd_tables;
    hipLaunchKernelGGL(osdx_front_kernel, dim3(osdx_grid(F)), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, t.n, t.k, t.d_Gcols,
                       d_perm, reinterpret_cast<u64 *>(d_parity), d_nswaps);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

static int osdx_launch_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                              const uint8_t *d_perm, const uint64_t *d_parity, int order, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                              int32_t *d_ntep, OsdxCounting c, hipStream_t s)
{
    const OsdTables &t = ctx->osd_tables;
    hipLaunchKernelGGL(osdx_search_kernel, dim3(osdx_grid(F)), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, t.n, t.k, d_perm,
                       reinterpret_cast<const u64 *>(d_parity), t.d_tep, (int)t.ntep[order], reinterpret_cast<u64 *>(d_cw), d_metric,
                       d_best, d_ntep, c.label, c.counts);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

// every check of the FS entry points before a launch; `required`: the pointers a call with F > 0 needs
static int osdx_fs_check(const ldpc_ctx *ctx, const ldpc_osd_params *p, int64_t F, std::initializer_list<NamedPtr> required, const char *who)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "%s: bad arguments", who);
    if (int rc = need_osdx(ctx)) return rc;
    if (!p) return fail(LDPC_E_ARG, "%s: params is NULL", who);
    if (p->algo != LDPC_OSD_FS) return fail(LDPC_E_ARG, "%s: algo %d is not LDPC_OSD_FS", who, p->algo);
    const int omax = ctx->osd_tables.k < 3 ? ctx->osd_tables.k : 3;
    if (p->order < 0 || p->order > omax) return fail(LDPC_E_ARG, "%s: order %d outside 0..%d", who, p->order, omax);
    if (p->flags != 0) return fail(LDPC_E_ARG, "%s: flags 0x%x are not served here (flags must be 0)", who, (unsigned)p->flags);
    if (p->d_aux) return fail(LDPC_E_ARG, "%s: d_aux is not served here (it must be NULL)", who);
    if (p->y_frames != 0) return fail(LDPC_E_ARG, "%s: y_frames %lld is not served here (it must be 0)", who, (long long)p->y_frames);
    return F > 0 ? first_null(who, required) : LDPC_OK;
}

static int osdx_launch_fs(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                          const uint8_t *d_perm, const uint64_t *d_parity, const ldpc_osd_params *p, uint64_t *d_cw, float *d_metric,
                          int32_t *d_best, int32_t *d_ntep, OsdxCounting c, hipStream_t s)
{
    const OsdTables &t = ctx->osd_tables;
    hipLaunchKernelGGL(osdx_fs_kernel, dim3(osdx_grid(F)), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, t.n, t.k, d_perm,
                       reinterpret_cast<const u64 *>(d_parity), t.d_tep_fs, fs_params(p, t.n, t.k, t.fs_off, t.fs_cnt),
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_best, d_ntep, c.label, c.counts);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

// every check of the PB entry points before a launch; `required`: the pointers a call with F > 0 needs
static int osdx_pb_check(const ldpc_ctx *ctx, const ldpc_osd_params *p, int64_t F, std::initializer_list<NamedPtr> required, const char *who)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "%s: bad arguments", who);
    if (int rc = need_osdx(ctx)) return rc;
    if (!p) return fail(LDPC_E_ARG, "%s: params is NULL", who);
    if (p->algo != LDPC_OSD_PB) return fail(LDPC_E_ARG, "%s: algo %d is not LDPC_OSD_PB", who, p->algo);
    const int omax = ctx->osd_tables.k < 3 ? ctx->osd_tables.k : 3;
    if (p->order < 0 || p->order > omax) return fail(LDPC_E_ARG, "%s: order %d outside 0..%d", who, p->order, omax);
    if (p->flags != 0) return fail(LDPC_E_ARG, "%s: flags 0x%x are not served here (flags must be 0)", who, (unsigned)p->flags);
    if (p->y_frames != 0) return fail(LDPC_E_ARG, "%s: y_frames %lld is not served here (it must be 0)", who, (long long)p->y_frames);
    return F > 0 ? first_null(who, required) : LDPC_OK;
}

static int osdx_launch_pb(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                          const uint8_t *d_perm, const uint64_t *d_parity, const ldpc_osd_params *p, uint64_t *d_cw, float *d_metric,
                          int32_t *d_best, int32_t *d_ntep, OsdxCounting c, hipStream_t s)
{
    const OsdTables &t = ctx->osd_tables;
    PbxParams pp;
    pp.order = p->order;
    pp.nmax = (int)t.ntep[p->order];
    pp.c4 = (float)(-4.0 * (1.0 / pow(10.0, (double)p->snr_db / 10.0)));    // -4 * noise_variance, pb_testing.py:50-52
    // the frontier's LDS is sized by the order: 64 slots up to order 2, 2048 for order 3
    const auto kern = p->order == 3 ? osdx_pb_kernel<true> : osdx_pb_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(osdx_grid(F)), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, t.n, t.k, d_perm,
                       reinterpret_cast<const u64 *>(d_parity), t.d_pb, pp, reinterpret_cast<u64 *>(d_cw), d_metric, d_best, d_ntep,
                       static_cast<int *>(p->d_aux), c.label, c.counts);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // namespace ldpc

using namespace ldpc;

extern "C" {

int ldpc_osdx_supported(const ldpc_ctx *ctx) { return ctx && ctx->osd_tables.k ? 1 : 0; }

int ldpc_osdx_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, uint8_t *d_perm,
                    uint64_t *d_parity, int32_t *d_nswaps, void *stream)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "ldpc_osdx_front: bad arguments");
    if (int rc = need_osdx(ctx)) return rc;
    if (F == 0) return LDPC_OK;
    if (int rc = first_null("ldpc_osdx_front", {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}})) return rc;
    return osdx_launch_front(ctx, d_y, d_index, d_count, F, d_perm, d_parity, d_nswaps, (hipStream_t)stream);
}

int ldpc_osdx_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                     const uint64_t *d_parity, int32_t order, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
                     void *stream)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "ldpc_osdx_search: bad arguments");
    if (int rc = need_osdx(ctx)) return rc;
    if (order < 0 || order > 3) return fail(LDPC_E_ARG, "ldpc_osdx_search: order %d outside 0..3", order);
    if (F == 0) return LDPC_OK;
    if (int rc = first_null("ldpc_osdx_search", {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_cw", d_cw}})) return rc;
    return osdx_launch_search(ctx, d_y, d_index, d_count, F, d_perm, d_parity, order, d_cw, d_metric, d_best, d_ntep, {}, (hipStream_t)stream);
}

int ldpc_osdx_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, int32_t order,
                     uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
                     const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "ldpc_osdx_decode: bad arguments");
    if (int rc = need_osdx(ctx)) return rc;
    if (order < 0 || order > 3) return fail(LDPC_E_ARG, "ldpc_osdx_decode: order %d outside 0..3", order);
    if (F == 0) return LDPC_OK;
    if (int rc = first_null("ldpc_osdx_decode", {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_cw", d_cw}})) return rc;
    if (int rc = osdx_launch_front(ctx, d_y, d_index, d_count, F, d_perm, d_parity, nullptr, (hipStream_t)stream)) return rc;
    return osdx_launch_search(ctx, d_y, d_index, d_count, F, d_perm, d_parity, order, d_cw, d_metric, d_best, d_ntep,
                              osdx_counting(d_label_bits, d_counts), (hipStream_t)stream);
}

int ldpc_osdx_fs_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                        const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                        int32_t *d_ntep, void *stream)
{
    if (int rc = osdx_fs_check(ctx, params, F, {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_cw", d_cw}},
                               "ldpc_osdx_fs_search")) return rc;
    if (F == 0) return LDPC_OK;
    return osdx_launch_fs(ctx, d_y, d_index, d_count, F, d_perm, d_parity, params, d_cw, d_metric, d_best, d_ntep, {}, (hipStream_t)stream);
}

int ldpc_osdx_fs_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric,
                        int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    if (int rc = osdx_fs_check(ctx, params, F, {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_cw", d_cw}},
                               "ldpc_osdx_fs_decode")) return rc;
    if (F == 0) return LDPC_OK;
    if (int rc = osdx_launch_front(ctx, d_y, d_index, d_count, F, d_perm, d_parity, nullptr, (hipStream_t)stream)) return rc;
    return osdx_launch_fs(ctx, d_y, d_index, d_count, F, d_perm, d_parity, params, d_cw, d_metric, d_best, d_ntep,
                          osdx_counting(d_label_bits, d_counts), (hipStream_t)stream);
}

int ldpc_osdx_pb_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                        const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                        int32_t *d_ntep, void *stream)
{
    if (int rc = osdx_pb_check(ctx, params, F, {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_cw", d_cw}},
                               "ldpc_osdx_pb_search")) return rc;
    if (F == 0) return LDPC_OK;
    return osdx_launch_pb(ctx, d_y, d_index, d_count, F, d_perm, d_parity, params, d_cw, d_metric, d_best, d_ntep, {}, (hipStream_t)stream);
}

int ldpc_osdx_pb_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric,
                        int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    if (int rc = osdx_pb_check(ctx, params, F, {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_cw", d_cw}},
                               "ldpc_osdx_pb_decode")) return rc;
    if (F == 0) return LDPC_OK;
    if (int rc = osdx_launch_front(ctx, d_y, d_index, d_count, F, d_perm, d_parity, nullptr, (hipStream_t)stream)) return rc;
    return osdx_launch_pb(ctx, d_y, d_index, d_count, F, d_perm, d_parity, params, d_cw, d_metric, d_best, d_ntep,
                          osdx_counting(d_label_bits, d_counts), (hipStream_t)stream);
}

int ldpc_osdx_tep_eval(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                       const uint64_t *d_parity, const uint64_t *d_mask, uint64_t *d_cw, float *d_metric, int32_t *d_hd, void *stream)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "ldpc_osdx_tep_eval: bad arguments");
    if (int rc = need_osdx(ctx)) return rc;
    if (F == 0) return LDPC_OK;
    if (int rc = first_null("ldpc_osdx_tep_eval", {{"d_y", d_y}, {"d_perm", d_perm}, {"d_parity", d_parity}, {"d_mask", d_mask}, {"d_cw", d_cw}}))
        return rc;
    hipLaunchKernelGGL(osdx_tep_eval_kernel, dim3(osdx_grid(F)), dim3(64), 0, (hipStream_t)stream, d_y, d_index, d_count, (long long)F,
                       ctx->osd_tables.n, ctx->osd_tables.k, d_perm, reinterpret_cast<const u64 *>(d_parity),
                       reinterpret_cast<const u64 *>(d_mask),
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_hd);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // extern "C"
