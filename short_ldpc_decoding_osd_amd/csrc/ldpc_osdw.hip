// OSD for high-rate short codes: the ldpc_osdw_* entry points.
// For every code with n <= 128 and 1 <= n - k <= 64, hence k up to 127: the front end, the conventional order-p scan (device
// code: ldpc_osdw.h), FS-OSD and the one-TEP primitive (ldpc_osdw_fs.h) and PB-OSD (ldpc_osdw_pb.h).  The PB tuning and routes and
// ldpc_pipeline_run stay with the (128,64) kernels of ldpc_osd.hip / ldpc_osd_pb.hip; osdw_stage() is this family's OSD stage of
// ldpc_family_pipeline_run (ldpc_api.hip).
// The two-word G columns and the TEP tables of k are the context's OsdwTables (ldpc_osd_tables.h), uploaded by ldpc_ctx_create.
// Validation, launches and the bodies of the entry points are those of ldpc_osd_family.h, shared with ldpc_osdx.hip; PB-OSD has a
// kernel per family, so each family launches its own.
#include <cmath>

#include "ldpc_osdw_fs.h"
#include "ldpc_osdw_pb.h"
#include "ldpc_osd_family.h"

namespace ldpc {

struct Osdw {
    static const OsdwTables &tables(const ldpc_ctx *ctx) { return ctx->osdw_tables; }
    static constexpr const char *needs = kOsdwNeeds;
    using perm_t = uint8_t;
    static constexpr auto front(const OsdwTables &) { return osdw_front_kernel; }
    static constexpr auto search(const OsdwTables &) { return osdw_search_kernel; }
    static constexpr auto fs(const OsdwTables &) { return osdw_fs_kernel; }
    static constexpr auto tep_eval(const OsdwTables &) { return osdw_tep_eval_kernel; }
};

static int osdw_launch_pb(const ldpc_ctx *ctx, const OsdFrames &fr, const uint8_t *d_perm, const uint64_t *d_parity, const ldpc_osd_params *p,
                          const OsdScanOut &o, OsdCounting c, hipStream_t s)
{
    const OsdwTables &t = ctx->osdw_tables;
    PbxParams pp;
    pp.order = p->order;
    pp.nmax = (int)t.ntep[p->order];
    pp.c4 = (float)(-4.0 * (1.0 / pow(10.0, (double)p->snr_db / 10.0)));    // -4 * noise_variance, pb_testing.py:50-52
    // the frontier's LDS is sized by the order and, at order 3, by k: 128 slots up to order 2, then the smallest of 2048 (k <= 64),
    // 4096 (k <= 91) and 8064 (k <= 127) that holds the k + C(k-1, 2) runs (occupancy: ldpc_osdw_pb.h)
    const int slots = pbw_slots3(t.k);
    const auto kern = p->order < 3   ? osdw_pb_kernel<false, 128>
                      : slots <= 2048 ? osdw_pb_kernel<true, 2048>
                      : slots <= 4096 ? osdw_pb_kernel<true, 4096>
                                      : osdw_pb_kernel<true, 8064>;
    hipLaunchKernelGGL(kern, dim3(frame_grid(fr.F)), dim3(64), 0, s, fr.y, fr.index, fr.count, (long long)fr.F, t.n, t.k, d_perm,
                       reinterpret_cast<const u64 *>(d_parity), t.d_pb, pp, reinterpret_cast<u64 *>(o.cw), o.metric, o.best, o.ntep,
                       static_cast<int *>(p->d_aux), c.label, c.counts);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}
constexpr OsdScan<uint8_t> osdw_pb_scan{LDPC_OSD_PB, "LDPC_OSD_PB", true, osdw_launch_pb};
const FamilyStage &osdw_stage() { static const FamilyStage st = FamilyStageOf<Osdw, osdw_pb_scan>::make(); return st; }   // ldpc_family_pipeline_run

}  // namespace ldpc

using namespace ldpc;

extern "C" {

int ldpc_osdw_supported(const ldpc_ctx *ctx) { return ctx && ctx->osdw_tables.k ? 1 : 0; }

int ldpc_osdw_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, uint8_t *d_perm,
                    uint64_t *d_parity, int32_t *d_nswaps, void *stream)
{
    return family_front<Osdw>(ctx, {d_y, d_index, d_count, F}, d_perm, d_parity, d_nswaps, stream, "ldpc_osdw_front");
}

int ldpc_osdw_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                     const uint64_t *d_parity, int32_t order, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
                     void *stream)
{
    return family_search<Osdw>(ctx, {d_y, d_index, d_count, F}, d_perm, d_parity, order, {d_cw, d_metric, d_best, d_ntep}, stream,
                               "ldpc_osdw_search");
}

int ldpc_osdw_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, int32_t order,
                     uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
                     const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    return family_decode<Osdw>(ctx, {d_y, d_index, d_count, F}, order, d_perm, d_parity, {d_cw, d_metric, d_best, d_ntep},
                               osd_counting(d_label_bits, d_counts), stream, "ldpc_osdw_decode");
}

int ldpc_osdw_fs_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                        const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                        int32_t *d_ntep, void *stream)
{
    return family_scan_search<Osdw>(ctx, {d_y, d_index, d_count, F}, d_perm, d_parity, params, fs_scan<Osdw>,
                                    {d_cw, d_metric, d_best, d_ntep}, stream, "ldpc_osdw_fs_search");
}

int ldpc_osdw_fs_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric,
                        int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    return family_scan_decode<Osdw>(ctx, {d_y, d_index, d_count, F}, params, fs_scan<Osdw>, d_perm, d_parity,
                                    {d_cw, d_metric, d_best, d_ntep}, osd_counting(d_label_bits, d_counts), stream, "ldpc_osdw_fs_decode");
}

int ldpc_osdw_pb_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                        const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                        int32_t *d_ntep, void *stream)
{
    return family_scan_search<Osdw>(ctx, {d_y, d_index, d_count, F}, d_perm, d_parity, params, osdw_pb_scan,
                                    {d_cw, d_metric, d_best, d_ntep}, stream, "ldpc_osdw_pb_search");
}

int ldpc_osdw_pb_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric,
                        int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    return family_scan_decode<Osdw>(ctx, {d_y, d_index, d_count, F}, params, osdw_pb_scan, d_perm, d_parity,
                                    {d_cw, d_metric, d_best, d_ntep}, osd_counting(d_label_bits, d_counts), stream, "ldpc_osdw_pb_decode");
}

int ldpc_osdw_tep_eval(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
                       const uint64_t *d_parity, const uint64_t *d_mask, uint64_t *d_cw, float *d_metric, int32_t *d_hd, void *stream)
{
    return family_tep_eval<Osdw>(ctx, {d_y, d_index, d_count, F}, d_perm, d_parity, d_mask, d_cw, d_metric, d_hd, stream,
                                 "ldpc_osdw_tep_eval");
}

}  // extern "C"
