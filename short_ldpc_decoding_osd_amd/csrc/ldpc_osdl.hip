// OSD for longer and low-rate codes: the ldpc_osdl_* entry points.
// For every code with n <= 384, 1 <= k <= 192 and 1 <= n - k <= 192: the front end and the conventional order-p scan (device
// code: ldpc_osdl.h).  FS-OSD and the one-TEP primitive of the family are in ldpc_osdl_fs.hip, PB-OSD and the family's
// stage of ldpc_family_pipeline_run in ldpc_osdl_pb.hip.
// The W-word G columns and the TEP tables of k are the context's OsdlTables (ldpc_osd_tables.h), uploaded by ldpc_ctx_create.
// Validation, launches and the bodies of the entry points are those of ldpc_osd_family.h, shared with ldpc_osdx.hip and
// ldpc_osdw.hip; this family's d_perm is uint16_t and its kernels are instantiations chosen by the shape (ldpc_osdl_family.h).
#include "ldpc_osdl_family.h"

namespace ldpc {

// the front end for S = ceil(n / 64) rounded up to 2, 4 or 6 slots and W = ceil(k / 64) row words
template <int S>
static Osdl::front_fn osdl_front_w(int W) { return W == 1 ? osdl_front_kernel<S, 1> : W == 2 ? osdl_front_kernel<S, 2> : osdl_front_kernel<S, 3>; }

Osdl::front_fn Osdl::front(const OsdlTables &t)
{
    const int S = (t.n + 63) / 64, W = (t.k + 63) / 64;
    // (two slots hold k <= 127: W = 3 starts at four)
    return S <= 2 ? (W == 1 ? osdl_front_kernel<2, 1> : osdl_front_kernel<2, 2>) : S <= 4 ? osdl_front_w<4>(W) : osdl_front_w<6>(W);
}

// the scan for Wp = ceil((n - k) / 64) words of discrepancy
Osdl::search_fn Osdl::search(const OsdlTables &t)
{
    const int Wp = (t.n - t.k + 63) / 64;
    return Wp == 1 ? osdl_search_kernel<1> : Wp == 2 ? osdl_search_kernel<2> : osdl_search_kernel<3>;
}

}  // namespace ldpc

using namespace ldpc;

extern "C" {

int ldpc_osdl_supported(const ldpc_ctx *ctx) { return ctx && ctx->osdl_tables.k ? 1 : 0; }

int ldpc_osdl_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, uint16_t *d_perm,
                    uint64_t *d_parity, int32_t *d_nswaps, void *stream)
{
    return family_front<Osdl>(ctx, {d_y, d_index, d_count, F}, d_perm, d_parity, d_nswaps, stream, "ldpc_osdl_front");
}

int ldpc_osdl_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint16_t *d_perm,
                     const uint64_t *d_parity, int32_t order, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
                     void *stream)
{
    return family_search<Osdl>(ctx, {d_y, d_index, d_count, F}, d_perm, d_parity, order, {d_cw, d_metric, d_best, d_ntep}, stream,
                               "ldpc_osdl_search");
}

int ldpc_osdl_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, int32_t order,
                     uint16_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
                     const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    return family_decode<Osdl>(ctx, {d_y, d_index, d_count, F}, order, d_perm, d_parity, {d_cw, d_metric, d_best, d_ntep},
                               osd_counting(d_label_bits, d_counts), stream, "ldpc_osdl_decode");
}

}  // extern "C"
