// OSD for longer and low-rate codes: the ldpc_osdl_pb_* entry points.
// For every code with n <= 384, 1 <= k <= 192 and 1 <= n - k <= 192: PB-OSD (device code: ldpc_osdl_pb.h) on the front-end
// results of ldpc_osdl_front (ldpc_osdl.hip), which ldpc_osdl_pb_decode launches through Osdl::front.  A translation unit and a
// code object of its own: ldpc_osdl.hip and ldpc_osdl_fs.hip keep the ones their register counts were measured on.
// The PB constants of (n, k) are in the context's OsdlTables (ldpc_osd_tables.h, the kPbl* layout).  Validation and the bodies
// of the entry points are those of ldpc_osd_family.h, shared with ldpc_osdx.hip and ldpc_osdw.hip; PB-OSD has a kernel per
// family, so each family launches its own.  The PB tuning and routes stay with the (128,64) kernels of ldpc_osd_pb.hip.
#include <cmath>

#include "ldpc_osdl_pb.h"
#include "ldpc_osdl_family.h"

namespace ldpc {

// the frontier's LDS is sized by the order and, at order 3, by k: 192 slots up to order 2, then the smallest of 2048 (k <= 64),
// 4096 (k <= 91), 8064 (k <= 127) and 18 368 (k <= 192) that holds the k + C(k-1, 2) runs (occupancy: ldpc_osdl_pb.h)
template <int WP>
static Osdl::pb_fn osdl_pb_pick(int order, int slots)
{
    return order < 3       ? osdl_pb_kernel<WP, false, 192>
           : slots <= 2048 ? osdl_pb_kernel<WP, true, 2048>
           : slots <= 4096 ? osdl_pb_kernel<WP, true, 4096>
           : slots <= 8064 ? osdl_pb_kernel<WP, true, 8064>
                           : osdl_pb_kernel<WP, true, 18368>;
}

Osdl::pb_fn Osdl::pb(const OsdlTables &t, int order)
{
    const int Wp = (t.n - t.k + 63) / 64, slots = pbl_slots3(t.k);
    return Wp == 1 ? osdl_pb_pick<1>(order, slots) : Wp == 2 ? osdl_pb_pick<2>(order, slots) : osdl_pb_pick<3>(order, slots);
}

static int osdl_launch_pb(const ldpc_ctx *ctx, const OsdFrames &fr, const uint16_t *d_perm, const uint64_t *d_parity, const ldpc_osd_params *p,
                          const OsdScanOut &o, OsdCounting c, hipStream_t s)
{
    const OsdlTables &t = ctx->osdl_tables;
    PbxParams pp;
    pp.order = p->order;
    pp.nmax = (int)t.ntep[p->order];
    pp.c4 = (float)(-4.0 * (1.0 / pow(10.0, (double)p->snr_db / 10.0)));    // -4 * noise_variance, pb_testing.py:50-52
    hipLaunchKernelGGL(Osdl::pb(t, p->order), dim3(frame_grid(fr.F)), dim3(64), 0, s, fr.y, fr.index, fr.count, (long long)fr.F, t.n, t.k,
                       d_perm, reinterpret_cast<const u64 *>(d_parity), t.d_pb, pp, reinterpret_cast<u64 *>(o.cw), o.metric, o.best,
                       o.ntep, static_cast<int *>(p->d_aux), c.label, c.counts);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}
constexpr OsdScan<uint16_t> osdl_pb_scan{LDPC_OSD_PB, "LDPC_OSD_PB", true, osdl_launch_pb};
const FamilyStage &osdl_stage() { static const FamilyStage st = FamilyStageOf<Osdl, osdl_pb_scan>::make(); return st; }   // ldpc_family_pipeline_run

}  // namespace ldpc

using namespace ldpc;

extern "C" {

int ldpc_osdl_pb_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint16_t *d_perm,
                        const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                        int32_t *d_ntep, void *stream)
{
    return family_scan_search<Osdl>(ctx, {d_y, d_index, d_count, F}, d_perm, d_parity, params, osdl_pb_scan,
                                    {d_cw, d_metric, d_best, d_ntep}, stream, "ldpc_osdl_pb_search");
}

int ldpc_osdl_pb_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint16_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric,
                        int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    return family_scan_decode<Osdl>(ctx, {d_y, d_index, d_count, F}, params, osdl_pb_scan, d_perm, d_parity,
                                    {d_cw, d_metric, d_best, d_ntep}, osd_counting(d_label_bits, d_counts), stream, "ldpc_osdl_pb_decode");
}

}  // extern "C"
