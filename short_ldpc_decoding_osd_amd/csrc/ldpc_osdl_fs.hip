// OSD for longer and low-rate codes: the ldpc_osdl_fs_* and ldpc_osdl_tep_eval entry points.
// For every code with n <= 384, 1 <= k <= 192 and 1 <= n - k <= 192: FS-OSD and the one-TEP primitive (device code:
// ldpc_osdl_fs.h) on the front-end results of ldpc_osdl_front (ldpc_osdl.hip), which ldpc_osdl_fs_decode launches through
// Osdl::front.  A translation unit of its own, so that ldpc_osdl.hip stays the code object of the front end and the conventional scan.
// The FS visit-order table of k is in the context's OsdlTables (ldpc_osd_tables.h).  Validation, launches and the bodies of the
// entry points are those of ldpc_osd_family.h, shared with ldpc_osdx.hip and ldpc_osdw.hip.
#include "ldpc_osdl_fs.h"
#include "ldpc_osdl_family.h"

namespace ldpc {

Osdl::fs_fn Osdl::fs(const OsdlTables &t)
{
    const int Wp = (t.n - t.k + 63) / 64;
    return Wp == 1 ? osdl_fs_kernel<1> : Wp == 2 ? osdl_fs_kernel<2> : osdl_fs_kernel<3>;
}

Osdl::tep_eval_fn Osdl::tep_eval(const OsdlTables &t)
{
    const int Wp = (t.n - t.k + 63) / 64;
    return Wp == 1 ? osdl_tep_eval_kernel<1> : Wp == 2 ? osdl_tep_eval_kernel<2> : osdl_tep_eval_kernel<3>;
}

}  // namespace ldpc

using namespace ldpc;

extern "C" {

int ldpc_osdl_fs_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint16_t *d_perm,
                        const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                        int32_t *d_ntep, void *stream)
{
    return family_scan_search<Osdl>(ctx, {d_y, d_index, d_count, F}, d_perm, d_parity, params, fs_scan<Osdl>,
                                    {d_cw, d_metric, d_best, d_ntep}, stream, "ldpc_osdl_fs_search");
}

int ldpc_osdl_fs_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint16_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric,
                        int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    return family_scan_decode<Osdl>(ctx, {d_y, d_index, d_count, F}, params, fs_scan<Osdl>, d_perm, d_parity,
                                    {d_cw, d_metric, d_best, d_ntep}, osd_counting(d_label_bits, d_counts), stream, "ldpc_osdl_fs_decode");
}

int ldpc_osdl_tep_eval(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint16_t *d_perm,
                       const uint64_t *d_parity, const uint64_t *d_mask, uint64_t *d_cw, float *d_metric, int32_t *d_hd, void *stream)
{
    return family_tep_eval<Osdl>(ctx, {d_y, d_index, d_count, F}, d_perm, d_parity, d_mask, d_cw, d_metric, d_hd, stream,
                                 "ldpc_osdl_tep_eval");
}

}  // extern "C"
