// H-form ordered-statistics primitives for longer and low-rate codes (ldpc_hosdl_*: n <= 384, an H of R <= 192 rows of rank
// n - k <= 192, k <= 192): the context's H columns, the routing of a code to the instantiations of ldpc_hosdl.h and the host
// side of the entry points.  The checks, their order and their messages are those of hosd_front / hosd_search / hosd_sliding
// in ldpc_hosd.hip, whose templates are tied to 8-bit index buffers and to kernels without template arguments: this unit
// carries a thin copy over 16-bit indices and a (words of discrepancy, words of a column) dispatch.
#include <tuple>
#include <type_traits>

#include "ldpc_internal.h"
#include "ldpc_wave.h"
#include "ldpc_hosdl.h"
#include "ldpc_dlosd_check.h"   // hosd_family_refusal: the sentence of each family
#include "ldpc_dlosd_stage.h"   // HosdStage: the counted launches of ldpc_dlosd_pipeline_run

namespace ldpc {

// Column v < n of H as given, rows 0..63 / 64..127 / 128..191, [384][3]; with hosdl_ok only.
int hosdl_ctx_init(ldpc_ctx *ctx)
{
    const ldpc_code &c = ctx->code;
    ctx->hosdl_ok = false;
    const int rank = c.n - c.k;
    if (c.n > kHosdlN || c.m < 1 || c.m > kHosdlM || rank < 1 || rank > c.m || c.k < 1 || c.k > kHosdlK) return LDPC_OK;
    std::vector<u64> cols((size_t)kHosdlN * 3, 0);
    for (int r = 0; r < c.m; ++r)
        for (int v = 0; v < c.n; ++v)
            if (c.H[(size_t)r * c.n + v]) cols[3 * v + (r >> 6)] |= 1ull << (r & 63);
    LDPC_HIP(hipMalloc((void **)&ctx->d_HcolsL, sizeof(u64) * cols.size()));
    LDPC_HIP(hipMemcpy(ctx->d_HcolsL, cols.data(), sizeof(u64) * cols.size(), hipMemcpyHostToDevice));
    ctx->hosdl_ok = true;
    return LDPC_OK;
}

void hosdl_ctx_release(ldpc_ctx *ctx)
{
    (void)hipFree(ctx->d_HcolsL);
    ctx->d_HcolsL = nullptr;
}

static int hosdl_check(const ldpc_ctx *ctx, const char *who)
{
    if (ctx->hosdl_ok) return LDPC_OK;
    return hosd_family_refusal(ctx, LDPC_HOSD_FAMILY_L, who);
}

static unsigned hosdl_grid(int64_t F, int cap) { return (unsigned)(F < 1 ? 1 : (F < cap ? F : cap)); }

// kernel(args...) on `grid` workgroups of `threads`: one argument list for a kernel and its counted form (the count appended)
template <class K, class... A>
static void hosdl_launch(K kernel, dim3 grid, int threads, void *stream, const std::tuple<A...> &args)
{
    std::apply([&](const auto &...a) { hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, (hipStream_t)stream, a...); }, args);
}

static const u64 *w64(const uint64_t *p) { return reinterpret_cast<const u64 *>(p); }
static u64 *w64(uint64_t *p) { return reinterpret_cast<u64 *>(p); }

// fn(integral_constant a, integral_constant b) for the run-time pair (a, b) among the listed ones; false if it is not listed
#define HOSDL_FRONT_SHAPES(X) X(2, 1) X(2, 2) X(2, 3) X(4, 1) X(4, 2) X(4, 3) X(6, 1) X(6, 2) X(6, 3)
#define HOSDL_SCAN_SHAPES(X) X(1, 1) X(2, 1) X(2, 2) X(3, 1) X(3, 2) X(3, 3) X(4, 1) X(4, 2) X(4, 3) X(5, 1) X(5, 2) X(5, 3) X(6, 1) X(6, 2) X(6, 3)
#define HOSDL_CASE(a, b) case (a) * 4 + (b): fn(std::integral_constant<int, a>(), std::integral_constant<int, b>()); return true;
template <class FN>
static bool front_dispatch(int S, int W, FN &&fn)
{
    switch (S * 4 + W) { HOSDL_FRONT_SHAPES(HOSDL_CASE) }
    return false;
}
template <class FN>
static bool scan_dispatch(int NW, int MW, FN &&fn)
{
    switch (NW * 4 + MW) { HOSDL_SCAN_SHAPES(HOSDL_CASE) }
    return false;
}

static SlideFcnArg slide_fcn_arg(const float *fcn_weights, int win)
{
    const int d = win + 1;
    SlideFcnArg w = {};
    for (int i = 0; i < d * d; ++i) w.w1[i] = fcn_weights[i];
    for (int i = 0; i < 2 * d; ++i) w.w2[i] = fcn_weights[d * d + i];
    return w;
}

// The host side of ldpc_hosdl_front and ldpc_hosdl_sliding; with d_count the counted form, on min(*d_count, F) frames
// (ldpc_dlosd_pipeline_run alone).  Defined below, each after its entry point.
static int hosdl_front(const char *who, ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint16_t *d_lri, uint16_t *d_uidx, uint64_t *d_M,
                       int32_t *d_nswaps, void *stream, const int32_t *d_count = nullptr);
static int hosdl_sliding(const char *who, ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint16_t *d_lri,
                         const uint16_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off, int32_t nblk,
                         int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights, int32_t group,
                         const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min, float *d_truth, uint8_t *d_success,
                         uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_teps_evaluated, void *stream,
                         const int32_t *d_count = nullptr);

}  // namespace ldpc

using namespace ldpc;

extern "C" {

int ldpc_hosdl_supported(const ldpc_ctx *ctx) { return ctx && ctx->hosdl_ok ? 1 : 0; }

int ldpc_hosdl_front(ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint16_t *d_lri, uint16_t *d_uidx, uint64_t *d_M,
                     int32_t *d_nswaps, void *stream)
{
    return hosdl_front("ldpc_hosdl_front", ctx, d_order_llr, F, d_lri, d_uidx, d_M, d_nswaps, stream);
}

}  // extern "C"

namespace ldpc {

static int hosdl_front(const char *who, ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint16_t *d_lri, uint16_t *d_uidx, uint64_t *d_M,
                       int32_t *d_nswaps, void *stream, const int32_t *d_count)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "%s: bad arguments (ctx %p, F %lld)", who, (void *)ctx, (long long)F);
    if (F > 0)
        if (int rc = first_null(who, {{"d_order_llr", d_order_llr}, {"d_lri", d_lri}, {"d_uidx", d_uidx}, {"d_M", d_M}})) return rc;
    if (int rc = hosdl_check(ctx, who)) return rc;
    if (F == 0) return LDPC_OK;
    const ldpc_code &c = ctx->code;
    const int S = 2 * ((c.n + 127) / 128), W = (c.m + 63) / 64;       // slots rounded up to 2, 4 or 6; row words of H as given
    const bool ok = front_dispatch(S, W, [&](auto s, auto w) {
        constexpr int SS = decltype(s)::value, WW = decltype(w)::value;
        const auto args = std::make_tuple(d_order_llr, (long long)F, c.n, c.m, c.n - c.k, w64(ctx->d_HcolsL), d_lri, d_uidx, w64(d_M), d_nswaps);
        const dim3 grid(hosdl_grid(F, kHosdlFrontGrid));
        if (d_count) hosdl_launch(hosdl_front_kernel<SS, WW, const int *>, grid, 64, stream, std::tuple_cat(args, std::make_tuple((const int *)d_count)));
        else hosdl_launch(hosdl_front_kernel<SS, WW>, grid, 64, stream, args);
    });
    if (!ok) return fail(LDPC_E_UNSUPPORTED, "%s: no kernel for %d slots, %d row words", who, S, W);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // namespace ldpc

extern "C" {

int ldpc_hosdl_search(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint16_t *d_lri,
                      const uint16_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off, int32_t nblk,
                      const uint64_t *d_label_bits, float *d_block_min, int32_t *d_block_arg, float *d_truth, uint64_t *d_cw,
                      float *d_metric, int32_t *d_best, void *stream)
{
    static const char who[] = "ldpc_hosdl_search";
    if (!ctx || F < 0 || nblk < 0)
        return fail(LDPC_E_ARG, "%s: bad arguments (ctx %p, F %lld, nblk %d)", who, (void *)ctx, (long long)F, (int)nblk);
    if (F > 0) {
        if (int rc = first_null(who, {{"d_order_llr", d_order_llr}, {"d_metric_llr", d_metric_llr}, {"d_lri", d_lri},
                                      {"d_uidx", d_uidx}, {"d_M", d_M}, {"d_block_off", d_block_off}})) return rc;
        if (nblk > 0)     // (the kernels read d_teps[0 .. d_block_off[nblk]), device data)
            if (int rc = first_null(who, {{"d_teps", d_teps}, {"d_block_min", d_block_min}})) return rc;
    }
    if (d_truth && !d_label_bits) return fail(LDPC_E_ARG, "%s: d_truth needs d_label_bits", who);
    if (int rc = hosdl_check(ctx, who)) return rc;
    if (nblk > kHosdMaxBlocks) return fail(LDPC_E_UNSUPPORTED, "%s: %d TEP blocks, at most %d", who, nblk, kHosdMaxBlocks);
    if (F == 0) return LDPC_OK;
    const ldpc_code &c = ctx->code;
    const int n = c.n, m = c.n - c.k;
    // (the TEP table's size is device data: both forms are launched and one of them returns at once)
    const bool ok = scan_dispatch((n + 63) / 64, (m + 63) / 64, [&](auto nw, auto mw) {
        constexpr int NW = decltype(nw)::value, MW = decltype(mw)::value;
        const dim3 grid(hosdl_grid(F, kHosdlScanGrid));
        hipLaunchKernelGGL((hosdl_search_kernel<NW, MW, true>), grid, dim3(256), 0, (hipStream_t)stream, d_order_llr, d_metric_llr, (long long)F,
                           n, m, d_lri, d_uidx, w64(d_M), reinterpret_cast<const uchar4 *>(d_teps), d_block_off, (int)nblk, w64(d_label_bits),
                           d_block_min, d_block_arg, d_truth, w64(d_cw), d_metric, d_best);
        hipLaunchKernelGGL((hosdl_search_kernel<NW, MW, false>), grid, dim3(256), 0, (hipStream_t)stream, d_order_llr, d_metric_llr, (long long)F,
                           n, m, d_lri, d_uidx, w64(d_M), reinterpret_cast<const uchar4 *>(d_teps), d_block_off, (int)nblk, w64(d_label_bits),
                           d_block_min, d_block_arg, d_truth, w64(d_cw), d_metric, d_best);
    });
    if (!ok) return fail(LDPC_E_UNSUPPORTED, "%s: no kernel for n = %d, n-k = %d", who, n, m);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_hosdl_sliding(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint16_t *d_lri,
                       const uint16_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off, int32_t nblk,
                       int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights, int32_t group,
                       const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min, float *d_truth, uint8_t *d_success,
                       uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_teps_evaluated, void *stream)
{
    return hosdl_sliding("ldpc_hosdl_sliding", ctx, d_order_llr, d_metric_llr, F, d_lri, d_uidx, d_M, d_teps, d_block_off, nblk, win,
                         soft_margin, fcn_weights, n_weights, group, d_label_bits, d_deep_limit, d_global_min, d_truth, d_success, d_cw,
                         d_metric, d_best, d_teps_evaluated, stream);
}

}  // extern "C"

namespace ldpc {

static int hosdl_sliding(const char *who, ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint16_t *d_lri,
                         const uint16_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off, int32_t nblk,
                         int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights, int32_t group,
                         const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min, float *d_truth, uint8_t *d_success,
                         uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_teps_evaluated, void *stream, const int32_t *d_count)
{
    if (!ctx || F < 0 || win < 1 || win > kSlideMaxWin || nblk < win || group < 0)
        return fail(LDPC_E_ARG, "%s: bad arguments (ctx %p, F %lld, win %d, nblk %d, group %d)", who, (void *)ctx, (long long)F,
                    (int)win, (int)nblk, (int)group);
    if (int rc = first_null(who, {{"fcn_weights", fcn_weights}})) return rc;
    if (F > 0)
        if (int rc = first_null(who, {{"d_order_llr", d_order_llr}, {"d_metric_llr", d_metric_llr}, {"d_lri", d_lri},
                                      {"d_uidx", d_uidx}, {"d_M", d_M}, {"d_teps", d_teps}, {"d_block_off", d_block_off}})) return rc;
    if (n_weights != fcn_weight_count(win))
        return fail(LDPC_E_ARG, "%s: %d classifier weights, a window of %d takes %d", who, (int)n_weights, (int)win, fcn_weight_count(win));
    if ((d_truth || d_success) && !d_label_bits) return fail(LDPC_E_ARG, "%s: d_truth / d_success need d_label_bits", who);
    if (int rc = hosdl_check(ctx, who)) return rc;
    if (nblk > kHosdMaxBlocks) return fail(LDPC_E_UNSUPPORTED, "%s: %d TEP blocks, at most %d", who, nblk, kHosdMaxBlocks);
    if (F == 0) return LDPC_OK;
    const ldpc_code &c = ctx->code;
    const int n = c.n, m = c.n - c.k;
    const SlideFcnArg fcn = slide_fcn_arg(fcn_weights, win);
    const bool ok = scan_dispatch((n + 63) / 64, (m + 63) / 64, [&](auto nw, auto mw) {
        constexpr int NW = decltype(nw)::value, MW = decltype(mw)::value;
        const auto args = std::make_tuple(d_order_llr, d_metric_llr, (long long)F, n, m, d_lri, d_uidx, w64(d_M), reinterpret_cast<const uchar4 *>(d_teps),
                                          d_block_off, (int)nblk, (int)win, soft_margin, fcn, (int)group, w64(d_label_bits), d_deep_limit,
                                          d_global_min, d_truth, d_success, w64(d_cw), d_metric, d_best, d_teps_evaluated);
        const dim3 grid(hosdl_grid(F, kHosdlScanGrid));
        if (d_count) hosdl_launch(hosdl_sliding_kernel<NW, MW, const int *>, grid, 256, stream, std::tuple_cat(args, std::make_tuple((const int *)d_count)));
        else hosdl_launch(hosdl_sliding_kernel<NW, MW>, grid, 256, stream, args);
    });
    if (!ok) return fail(LDPC_E_UNSUPPORTED, "%s: no kernel for n = %d, n-k = %d", who, n, m);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

// the long family as ldpc_dlosd_pipeline_run sees it
static int hosdl_stage_front(ldpc_ctx *ctx, const float *xo, const int32_t *d_count, int64_t F, void *d_lri, void *d_uidx, uint64_t *d_M,
                             int32_t *d_nswaps, hipStream_t s)
{
    return hosdl_front(kDlosdWho, ctx, xo, F, static_cast<uint16_t *>(d_lri), static_cast<uint16_t *>(d_uidx), d_M, d_nswaps, s, d_count);
}
static int hosdl_stage_sliding(ldpc_ctx *ctx, const float *xo, const float *xm, const int32_t *d_count, int64_t F, const ldpc_dlosd_pipeline *p,
                               const uint64_t *d_label, hipStream_t s)
{
    return hosdl_sliding(kDlosdWho, ctx, xo, xm, F, static_cast<const uint16_t *>(p->d_lri), static_cast<const uint16_t *>(p->d_uidx), p->d_M,
                         p->d_teps, p->d_block_off, p->nblk, p->win, p->soft_margin, p->fcn_weights, p->n_fcn_weights, p->group, d_label,
                         p->d_deep_limit, p->d_global_min, d_label ? p->d_truth : nullptr, d_label ? p->d_success : nullptr, p->d_cw,
                         p->d_metric, p->d_best, p->d_teps_evaluated, s, d_count);
}
const HosdStage &hosdl_stage()
{
    static const HosdStage st{hosdl_stage_front, hosdl_stage_sliding};
    return st;
}

}  // namespace ldpc
