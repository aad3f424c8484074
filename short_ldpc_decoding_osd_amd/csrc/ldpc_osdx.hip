// OSD for short codes of any shape: the host side of ldpc_osdx_* (context tables, validation, launches).
// For every code with 1 <= k <= 64 and 1 <= n - k <= 64: the front end, the conventional order-p scan (device code:
// ldpc_osdx.h), FS-OSD and the one-TEP primitive (ldpc_osdx_fs.h).  PB-OSD and the one-call pipeline stay with the (128,64)
// kernels of ldpc_osd.hip / ldpc_osd_pb.hip.
// There is no library workspace: the decode entry points run their two launches through the caller's d_perm / d_parity, so the
// calls hold no per-stream state, allocate nothing and are graph-capturable as they are.
#include "ldpc_osdx_fs.h"

namespace ldpc {

struct OsdxState {
    u64 *d_Gcols = nullptr;      // [n] column v of G as a k-bit word (bit r = G[r][v])
    uchar4 *d_tep = nullptr;     // the order-3 TEP table for this k: (i, j, l, weight); orders 0..2 are its prefixes
    int64_t ntep[4] = {0, 0, 0, 0};
    uchar4 *d_tep_fs = nullptr;  // FS-OSD visit order (generate_sequential_teps) of this k: weight classes 1..min(3, k) back to back
    int fs_off[4] = {0, 0, 0, 0}, fs_cnt[4] = {0, 0, 0, 0};
};

static inline OsdxState *xstate(const ldpc_ctx *ctx) { return reinterpret_cast<OsdxState *>(ctx->osdx_state); }

static bool osdx_shape_ok(const ldpc_code &c) { return c.k >= 1 && c.k <= 64 && c.n - c.k >= 1 && c.n - c.k <= 64; }

// tables of every eligible shape, uploaded with the context (nothing is allocated by a decode call)
int osdx_ctx_init(ldpc_ctx *ctx)
{
    const ldpc_code &c = ctx->code;
    ctx->osdx_state = nullptr;
    if (!osdx_shape_ok(c) || c.G.size() != (size_t)c.k * c.n) return LDPC_OK;   // the entry points will report UNSUPPORTED
    OsdxState *st = new OsdxState();
    ctx->osdx_state = st;
    std::vector<u64> cols(c.n, 0);
    for (int r = 0; r < c.k; ++r)
        for (int v = 0; v < c.n; ++v)
            if (c.G[(size_t)r * c.n + v]) cols[v] |= 1ull << r;
    LDPC_HIP(hipMalloc((void **)&st->d_Gcols, sizeof(u64) * c.n));
    LDPC_HIP(hipMemcpy(st->d_Gcols, cols.data(), sizeof(u64) * c.n, hipMemcpyHostToDevice));
    int64_t bounds[4];
    const int64_t total = tep_table(c.k, 3, nullptr, bounds);
    if (total < 0) return (int)total;
    std::vector<uint8_t> sup((size_t)total * 3), packed((size_t)total * 4);
    tep_table(c.k, 3, sup.data(), nullptr);
    for (int64_t t = 0; t < total; ++t) {
        int w = 0;
        for (int q = 0; q < 3; ++q) { packed[4 * t + q] = sup[3 * t + q] == 0xFF ? 0 : sup[3 * t + q]; w += sup[3 * t + q] != 0xFF; }
        packed[4 * t + 3] = (uint8_t)w;
    }
    for (int o = 0; o < 4; ++o) st->ntep[o] = bounds[o];
    LDPC_HIP(hipMalloc((void **)&st->d_tep, packed.size()));
    LDPC_HIP(hipMemcpy(st->d_tep, packed.data(), packed.size(), hipMemcpyHostToDevice));
    std::vector<uint8_t> fs;   // supports stored ascending, packed as the (128,64) table of osd_ctx_init
    int off = 0;
    for (int w = 1; w <= 3 && w <= c.k; ++w) {
        const int64_t cnt = tep_table_fs(c.k, w, nullptr);
        if (cnt < 0) return (int)cnt;
        std::vector<uint8_t> sup3((size_t)cnt * 3);
        tep_table_fs(c.k, w, sup3.data());
        st->fs_off[w] = off; st->fs_cnt[w] = (int)cnt;
        for (int64_t t = 0; t < cnt; ++t) {
            for (int q = 0; q < 3; ++q) fs.push_back(sup3[3 * t + q] == 0xFF ? 0 : sup3[3 * t + q]);
            fs.push_back((uint8_t)w);
        }
        off += (int)cnt;
    }
    LDPC_HIP(hipMalloc((void **)&st->d_tep_fs, fs.size()));
    LDPC_HIP(hipMemcpy(st->d_tep_fs, fs.data(), fs.size(), hipMemcpyHostToDevice));
    return LDPC_OK;
}

void osdx_ctx_release(ldpc_ctx *ctx)
{
    if (OsdxState *st = xstate(ctx)) {
        (void)hipFree(st->d_Gcols);
        (void)hipFree(st->d_tep);
        (void)hipFree(st->d_tep_fs);
        delete st;
    }
    ctx->osdx_state = nullptr;
}

static int need_osdx(const ldpc_ctx *ctx)
{
    return xstate(ctx) ? LDPC_OK
                       : fail(LDPC_E_UNSUPPORTED, "the any-shape OSD kernels need 1 <= k <= 64 and 1 <= n-k <= 64; this code is (%d,%d)",
                              ctx->code.n, ctx->code.k);
}

// one wavefront per workgroup, a workgroup per frame up to 65536 (then strided: a wavefront decodes several frames in turn)
static unsigned osdx_grid(int64_t F) { return (unsigned)(F < 65536 ? F : 65536); }

static int osdx_launch_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, uint8_t *d_perm,
                             uint64_t *d_parity, int32_t *d_nswaps, hipStream_t s)
{
    const OsdxState *st = xstate(ctx);
    hipLaunchKernelGGL(osdx_front_kernel, dim3(osdx_grid(F)), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, ctx->code.n,
                       ctx->code.k, st->d_Gcols, d_perm, reinterpret_cast<u64 *>(d_parity), d_nswaps);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

static int osdx_launch_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                              const uint8_t *d_perm, const uint64_t *d_parity, int order, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                              int32_t *d_ntep, const uint64_t *d_label, int64_t *d_counts, hipStream_t s)
{
    const OsdxState *st = xstate(ctx);
    const bool counting = d_label && d_counts;
    hipLaunchKernelGGL(osdx_search_kernel, dim3(osdx_grid(F)), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, ctx->code.n,
                       ctx->code.k, d_perm, reinterpret_cast<const u64 *>(d_parity), st->d_tep, (int)st->ntep[order],
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_best, d_ntep,
                       counting ? reinterpret_cast<const u64 *>(d_label) : nullptr, counting ? reinterpret_cast<u64 *>(d_counts) : nullptr);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

// every check of the FS entry points before a launch; `required` names the first NULL among the required pointers (or is NULL)
static int osdx_fs_check(const ldpc_ctx *ctx, const ldpc_osd_params *p, int64_t F, const char *required, const char *who)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "%s: bad arguments", who);
    if (int rc = need_osdx(ctx)) return rc;
    if (!p) return fail(LDPC_E_ARG, "%s: params is NULL", who);
    if (p->algo != LDPC_OSD_FS) return fail(LDPC_E_ARG, "%s: algo %d is not LDPC_OSD_FS", who, p->algo);
    const int omax = ctx->code.k < 3 ? ctx->code.k : 3;
    if (p->order < 0 || p->order > omax) return fail(LDPC_E_ARG, "%s: order %d outside 0..%d", who, p->order, omax);
    if (p->flags != 0) return fail(LDPC_E_ARG, "%s: flags 0x%x are not served here (flags must be 0)", who, (unsigned)p->flags);
    if (p->d_aux) return fail(LDPC_E_ARG, "%s: d_aux is not served here (it must be NULL)", who);
    if (p->y_frames != 0) return fail(LDPC_E_ARG, "%s: y_frames %lld is not served here (it must be 0)", who, (long long)p->y_frames);
    if (F > 0 && required) return fail(LDPC_E_ARG, "%s: %s is NULL", who, required);
    return LDPC_OK;
}

static int osdx_launch_fs(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                          const uint8_t *d_perm, const uint64_t *d_parity, const ldpc_osd_params *p, uint64_t *d_cw, float *d_metric,
                          int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label, int64_t *d_counts, hipStream_t s)
{
    const OsdxState *st = xstate(ctx);
    const bool counting = d_label && d_counts;
    OsdxFsParams fp;
    fp.order = p->order; fp.quirk = p->fs_reference_quirk != 0;
    fp.beta_term = (float)((double)p->fs_beta * (double)(ctx->code.n - ctx->code.k));   // fs_testing.py:138
    fp.tau_e = p->fs_tau_e; fp.tau_psc = p->fs_tau_psc;
    for (int w = 0; w < 4; ++w) { fp.cls_off[w] = st->fs_off[w]; fp.cls_cnt[w] = st->fs_cnt[w]; }
    hipLaunchKernelGGL(osdx_fs_kernel, dim3(osdx_grid(F)), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, ctx->code.n, ctx->code.k,
                       d_perm, reinterpret_cast<const u64 *>(d_parity), st->d_tep_fs, fp, reinterpret_cast<u64 *>(d_cw), d_metric, d_best,
                       d_ntep, counting ? reinterpret_cast<const u64 *>(d_label) : nullptr,
                       counting ? reinterpret_cast<u64 *>(d_counts) : nullptr);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // namespace ldpc

using namespace ldpc;

extern "C" {

int ldpc_osdx_supported(const ldpc_ctx *ctx) { return ctx && xstate(ctx) ? 1 : 0; }

int ldpc_osdx_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, uint8_t *d_perm,
                    uint64_t *d_parity, int32_t *d_nswaps, void *stream)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "ldpc_osdx_front: bad arguments");
    if (int rc = need_osdx(ctx)) return rc;
    if (F > 0 && (!d_y || !d_perm || !d_parity))
        return fail(LDPC_E_ARG, "ldpc_osdx_front: %s is NULL", !d_y ? "d_y" : (!d_perm ? "d_perm" : "d_parity"));
    if (F == 0) return LDPC_OK;
    return osdx_launch_front(ctx, d_y, d_index, d_count, F, d_perm, d_parity, d_nswaps, (hipStream_t)stream);
}

int ldpc_osdx_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                     const uint64_t *d_parity, int32_t order, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
                     void *stream)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "ldpc_osdx_search: bad arguments");
    if (int rc = need_osdx(ctx)) return rc;
    if (order < 0 || order > 3) return fail(LDPC_E_ARG, "ldpc_osdx_search: order %d outside 0..3", order);
    if (F > 0 && (!d_y || !d_perm || !d_parity || !d_cw))
        return fail(LDPC_E_ARG, "ldpc_osdx_search: %s is NULL", !d_y ? "d_y" : (!d_perm ? "d_perm" : (!d_parity ? "d_parity" : "d_cw")));
    if (F == 0) return LDPC_OK;
    return osdx_launch_search(ctx, d_y, d_index, d_count, F, d_perm, d_parity, order, d_cw, d_metric, d_best, d_ntep, nullptr, nullptr,
                              (hipStream_t)stream);
}

int ldpc_osdx_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, int32_t order,
                     uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
                     const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "ldpc_osdx_decode: bad arguments");
    if (int rc = need_osdx(ctx)) return rc;
    if (order < 0 || order > 3) return fail(LDPC_E_ARG, "ldpc_osdx_decode: order %d outside 0..3", order);
    if (F > 0 && (!d_y || !d_perm || !d_parity || !d_cw))
        return fail(LDPC_E_ARG, "ldpc_osdx_decode: %s is NULL", !d_y ? "d_y" : (!d_perm ? "d_perm" : (!d_parity ? "d_parity" : "d_cw")));
    if (F == 0) return LDPC_OK;
    if (int rc = osdx_launch_front(ctx, d_y, d_index, d_count, F, d_perm, d_parity, nullptr, (hipStream_t)stream)) return rc;
    return osdx_launch_search(ctx, d_y, d_index, d_count, F, d_perm, d_parity, order, d_cw, d_metric, d_best, d_ntep, d_label_bits,
                              d_counts, (hipStream_t)stream);
}

int ldpc_osdx_fs_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                        const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                        int32_t *d_ntep, void *stream)
{
    const char *null = !d_y ? "d_y" : (!d_perm ? "d_perm" : (!d_parity ? "d_parity" : (!d_cw ? "d_cw" : nullptr)));
    if (int rc = osdx_fs_check(ctx, params, F, null, "ldpc_osdx_fs_search")) return rc;
    if (F == 0) return LDPC_OK;
    return osdx_launch_fs(ctx, d_y, d_index, d_count, F, d_perm, d_parity, params, d_cw, d_metric, d_best, d_ntep, nullptr, nullptr,
                          (hipStream_t)stream);
}

int ldpc_osdx_fs_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric,
                        int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    const char *null = !d_y ? "d_y" : (!d_perm ? "d_perm" : (!d_parity ? "d_parity" : (!d_cw ? "d_cw" : nullptr)));
    if (int rc = osdx_fs_check(ctx, params, F, null, "ldpc_osdx_fs_decode")) return rc;
    if (F == 0) return LDPC_OK;
    if (int rc = osdx_launch_front(ctx, d_y, d_index, d_count, F, d_perm, d_parity, nullptr, (hipStream_t)stream)) return rc;
    return osdx_launch_fs(ctx, d_y, d_index, d_count, F, d_perm, d_parity, params, d_cw, d_metric, d_best, d_ntep, d_label_bits, d_counts,
                          (hipStream_t)stream);
}

int ldpc_osdx_tep_eval(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                       const uint64_t *d_parity, const uint64_t *d_mask, uint64_t *d_cw, float *d_metric, int32_t *d_hd, void *stream)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "ldpc_osdx_tep_eval: bad arguments");
    if (int rc = need_osdx(ctx)) return rc;
    if (F > 0 && (!d_y || !d_perm || !d_parity || !d_mask || !d_cw))
        return fail(LDPC_E_ARG, "ldpc_osdx_tep_eval: %s is NULL",
                    !d_y ? "d_y" : (!d_perm ? "d_perm" : (!d_parity ? "d_parity" : (!d_mask ? "d_mask" : "d_cw"))));
    if (F == 0) return LDPC_OK;
    hipLaunchKernelGGL(osdx_tep_eval_kernel, dim3(osdx_grid(F)), dim3(64), 0, (hipStream_t)stream, d_y, d_index, d_count, (long long)F,
                       ctx->code.n, ctx->code.k, d_perm, reinterpret_cast<const u64 *>(d_parity), reinterpret_cast<const u64 *>(d_mask),
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_hd);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // extern "C"
