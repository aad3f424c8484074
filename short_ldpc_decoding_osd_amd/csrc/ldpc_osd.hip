// Ordered-statistics decoding for (128,64) codes on gfx950 (MI355X): the translation unit of the conventional and FS side.
// Here: the host side (the (128,64) constants of a context, per-stream workspace, validation, route selection, osd_launch, fs_params,
// the entry points).  G columns and TEP tables: the context's OsdTables (ldpc_osd_tables.h), shared with ldpc_osdx.hip.
// Reference (paths relative to LDPC_128/ of the reference):
//   swapped_info / identify_mrb / full_gf2elim   PB_OSD/pb_testing.py:231-320 (== FS_OSD/fs_testing.py:233-322)
//   generate_teps / convention_osd_main           FS_OSD/convention_osd.py:13-76
// The device code lies in five headers, included in the order the kernels had in this file (ONE translation unit on purpose:
// the kernels share inlined device code, and the order of the definitions is the order of the code object):
//   ldpc_osd_small.h   osd_ge_kernel, osd_front_kernel, osd_search_kernel<WAVES> (the table scan)
//   ldpc_osd_scan2.h   osd_search2_kernel (order 2, v_readlane pairing); tep2_rank and the pieces both order-2 scans share
//   ldpc_osd_scan2r.h  osd_search2r_kernel, osd_fused2r_kernel (order 2, rotation pairing: the headline configuration)
//   ldpc_osd_fs.h      osd_fs_kernel
//   ldpc_osd_aux.h     osd_tep_eval_kernel, osd_counts_kernel, index_guard_kernel
// (PB-OSD: ldpc_osd_pb.hip, the host side, and ldpc_pb_*.h, its kernels; shared per-frame device code: ldpc_front.h, ldpc_search.h,
//  ldpc_wave.h; host state: ldpc_osd_state.h)
#include <math.h>
#include <stdlib.h>

#include "ldpc_osd_small.h"
#include "ldpc_osd_scan2.h"
#include "ldpc_osd_scan2r.h"
#include "ldpc_osd_fs.h"
#include "ldpc_osd_aux.h"
#include "ldpc_osd_state.h"

namespace ldpc {

// ---------------------------------------------------------------------------------------
// context pieces: the constants of the (128,64) kernels beside the context's OsdTables, front-end workspace
// ---------------------------------------------------------------------------------------
int osd_ctx_init(ldpc_ctx *ctx)
{
    const OsdTables &t = ctx->osd_tables;
    ctx->osd_ok = false;
    if (t.n != kOsdN || t.k != kOsdK) return LDPC_OK;  // OSD entry points will report UNSUPPORTED
    OsdState *st = new OsdState();
    ctx->osd_state = st;
    {
        int base2[127];
        auto npairs = [](int t) { return (t - 1) / 2 - (t > 63 ? t - 63 : 0) + 1; };
        for (int sidx = 0; sidx < 127; ++sidx) {
            int acc = 0;
            for (int t = sidx + 1; t <= 125; ++t) acc += npairs(t);
            base2[sidx] = acc;
        }
        LDPC_HIP(hipMalloc((void **)&st->d_base2, sizeof(base2)));
        LDPC_HIP(hipMemcpy(st->d_base2, base2, sizeof(base2), hipMemcpyHostToDevice));
    }
    // PB-OSD constants, same float64 recurrence as the kernel / oracle
    {
        double coef[64], cdf[65], t = 0.5;
        for (int i = 0; i < 64; ++i) coef[i] = (double)(64 - i) / (double)(i + 1);
        for (int q = 0; q < 6; ++q) t = t * t;
        double acc = t;
        cdf[0] = acc;
        for (int i = 0; i < 64; ++i) { t = t * coef[i] * (0.5 / 0.5); acc = acc + t; cdf[i + 1] = acc; }
        LDPC_HIP(hipMalloc((void **)&st->d_cdf_half, sizeof(cdf)));
        LDPC_HIP(hipMemcpy(st->d_cdf_half, cdf, sizeof(cdf), hipMemcpyHostToDevice));
    }
    LDPC_HIP(hipMalloc((void **)&st->d_index_errors, sizeof(unsigned long long)));
    LDPC_HIP(hipMemset(st->d_index_errors, 0, sizeof(unsigned long long)));
    if (int rc = pb_ctx_init(ctx)) return rc;
    ctx->osd_ok = true;
    return LDPC_OK;
}

static void free_stream_ws(StreamWs &w)
{
    (void)hipFree(w.d_perm); (void)hipFree(w.d_parity); (void)hipFree(w.d_index_safe);
    (void)hipFree(w.d_pb_ctl); (void)hipFree(w.d_pb_list); (void)hipFree(w.d_pb_spill); (void)hipFree(w.d_pb_prep);
    (void)hipFree(w.d_pb_carry);
    w = StreamWs();
}

void osd_ctx_release(ldpc_ctx *ctx)
{
    if (OsdState *st = state(ctx)) {
        for (auto &kv : st->ws) free_stream_ws(kv.second);
        (void)hipFree(st->d_base2);
        (void)hipFree(st->d_cdf_half);
        (void)hipFree(st->d_index_errors);
        delete st;
    }
    ctx->osd_state = nullptr;
}

bool stream_capturing(hipStream_t s)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// the workspace of `s` with room for the front-end results of `frames` frames (0: just look it up);
// allocation happens on a stream's first call or when a call outgrows it -- never while `s` is capturing, and never
// again once a graph was captured on `s` (the graph's nodes hold the buffer addresses: ADVICE r02)
static int stream_ws(ldpc_ctx *ctx, hipStream_t s, int64_t frames, StreamWs **out)
{
    OsdState *st = state(ctx);
    std::lock_guard<std::mutex> lock(st->mu);
    StreamWs &w = st->ws[s];
    if (frames > 0 && frames < st->reserve_frames) frames = st->reserve_frames;
    const bool capturing = stream_capturing(s);
    if (frames > w.cap) {
        if (capturing)
            return fail(LDPC_E_NOMEM, "OSD workspace of this stream holds %lld frames, %lld needed: run one call (or "
                        "ldpc_osd_reserve_stream) on the stream before capturing", (long long)w.cap, (long long)frames);
        if (w.captured)
            return fail(LDPC_E_NOMEM, "OSD workspace of this stream (%lld frames) is referenced by a captured graph and cannot grow to "
                        "%lld: destroy the graph and call ldpc_osd_release_stream, or reserve the larger size before capturing",
                        (long long)w.cap, (long long)frames);
        (void)hipFree(w.d_perm); (void)hipFree(w.d_parity);
        w.d_perm = nullptr; w.d_parity = nullptr; w.cap = 0;
        if (hipMalloc((void **)&w.d_perm, (size_t)frames * 128) != hipSuccess ||
            hipMalloc((void **)&w.d_parity, (size_t)frames * 64 * sizeof(u64)) != hipSuccess)
            return fail(LDPC_E_NOMEM, "OSD workspace for %lld frames could not be allocated", (long long)frames);
        w.cap = frames;
    }
    if (capturing) w.captured = true;
    *out = &w;
    return LDPC_OK;
}
// returns the list the kernels should use: d_index itself, or its sanitised copy in the stream's workspace
static int guarded_index(ldpc_ctx *ctx, const ldpc_osd_params *p, const int32_t *d_index, const int32_t *d_count, int64_t F, hipStream_t s,
                         const int32_t **out)
{
    *out = d_index;
    if (!d_index || p->y_frames <= 0 || F <= 0) return LDPC_OK;
    OsdState *st = state(ctx);
    int *safe;
    {
        std::lock_guard<std::mutex> lock(st->mu);
        StreamWs &w = st->ws[s];
        if (F > w.index_cap) {
            if (stream_capturing(s) || w.captured)
                return fail(LDPC_E_NOMEM, "ldpc_osd_params.y_frames: the checked frame list of this stream holds %lld entries, %lld needed; "
                            "it cannot grow during or after a capture", (long long)w.index_cap, (long long)F);
            (void)hipFree(w.d_index_safe); w.d_index_safe = nullptr; w.index_cap = 0;
            if (hipMalloc((void **)&w.d_index_safe, sizeof(int) * (size_t)F) != hipSuccess)
                return fail(LDPC_E_NOMEM, "checked frame list for %lld frames could not be allocated", (long long)F);
            w.index_cap = F;
        }
        if (stream_capturing(s)) w.captured = true;
        safe = w.d_index_safe;
    }
    const int64_t g = (F + 255) / 256;
    hipLaunchKernelGGL(index_guard_kernel, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(256), 0, s, d_index, d_count, (long long)F,
                       (long long)p->y_frames, safe, st->d_index_errors);
    LDPC_HIP(hipGetLastError());
    *out = safe;
    return LDPC_OK;
}

// ---- grid sizes.  osd_grid: persistent, enough blocks to fill 256 CUs a few times over, frames are strided over waves (4 per workgroup)
static unsigned osd_grid(int64_t F)
{
    const int64_t want = (F + 3) / 4;
    return (unsigned)(want < 1 ? 1 : (want < 4096 ? want : 4096));
}

// (frame_grid, one wavefront per workgroup, and front_grid, the front end's frame pipeline: ldpc_internal.h)

// the rotation-paired kernels: 4 wavefronts per SIMD are resident (10 KiB of LDS each); the grid is 6x that, ~1.5 frames per
// workgroup at the headline size: the dispatcher then evens out the different scan times, and the prefetch still covers the
// second frame (measured, 33 487 frames: 1x 119 us, 2x 117, 3x 108, 4x 107, 6x 100, 9x 102 per call incl. events)
static unsigned grid2r(const ldpc_ctx *ctx, int64_t F) { const int64_t g = (int64_t)ctx->cu_count * 16 * 6; return (unsigned)(F < g ? F : g); }

static void launch_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, uint8_t *d_perm,
                         u64 *d_parity, int32_t *d_nswaps, hipStream_t s)
{
    hipLaunchKernelGGL(osd_front_kernel, dim3(front_grid(ctx->cu_count, F)), dim3(64), 0, s, d_y, d_index, d_count, (long long)F,
                       ctx->osd_tables.d_Gcols, d_perm, d_parity, d_nswaps);
}

static int need_osd(const ldpc_ctx *ctx)
{
    return ctx->osd_ok ? LDPC_OK : fail(LDPC_E_UNSUPPORTED, "OSD kernels need an (n=128, k=64) code; this one is (%d,%d)", ctx->code.n, ctx->code.k);
}

static const char *flag_name(unsigned f)   // the lowest LDPC_OSD_F_* flag in f
{
    if (f & LDPC_OSD_F_TABLE_SCAN) return "LDPC_OSD_F_TABLE_SCAN";
    if (f & LDPC_OSD_F_PB_BLOCK) return "LDPC_OSD_F_PB_BLOCK";
    if (f & LDPC_OSD_F_PB_REPLAY) return "LDPC_OSD_F_PB_REPLAY";
    if (f & LDPC_OSD_F_READLANE_SCAN) return "LDPC_OSD_F_READLANE_SCAN";
    return "LDPC_OSD_F_PB_FRONT_INSIDE";
}

int check_params(ldpc_ctx *ctx, const ldpc_osd_params *p, bool front_outside, const char *who)
{
    if (int rc = need_osd(ctx)) return rc;
    if (p->order < 0 || p->order > 3) return fail(LDPC_E_ARG, "%s: order %d outside 0..3", who, p->order);
    if (p->algo != LDPC_OSD_CONVENTIONAL && p->algo != LDPC_OSD_FS && p->algo != LDPC_OSD_PB)
        return fail(LDPC_E_ARG, "%s: unknown search algorithm %d", who, p->algo);
    if (p->algo == LDPC_OSD_PB && p->order < 1) return fail(LDPC_E_ARG, "%s: PB-OSD needs order >= 1", who);
    const unsigned f = (unsigned)p->flags;
    const unsigned conv = LDPC_OSD_F_TABLE_SCAN | LDPC_OSD_F_READLANE_SCAN;
    const unsigned pb = LDPC_OSD_F_PB_BLOCK | LDPC_OSD_F_PB_REPLAY | LDPC_OSD_F_PB_FRONT_INSIDE;
    if (f & ~(conv | pb)) return fail(LDPC_E_ARG, "%s: flags 0x%x are no LDPC_OSD_F_* flag", who, f & ~(conv | pb));
    if ((f & conv) && p->algo != LDPC_OSD_CONVENTIONAL)
        return fail(LDPC_E_ARG, "%s: %s needs the conventional algorithm, not %d", who, flag_name(f & conv), p->algo);
    if ((f & LDPC_OSD_F_READLANE_SCAN) && (p->order != 2 || (f & LDPC_OSD_F_TABLE_SCAN)))
        return fail(LDPC_E_ARG, "%s: LDPC_OSD_F_READLANE_SCAN needs order 2 (not %d) and no LDPC_OSD_F_TABLE_SCAN", who, p->order);
    if ((f & pb) && p->algo != LDPC_OSD_PB)
        return fail(LDPC_E_ARG, "%s: %s needs the PB algorithm, not %d", who, flag_name(f & pb), p->algo);
    if ((f & LDPC_OSD_F_PB_REPLAY) && (f & (LDPC_OSD_F_PB_BLOCK | LDPC_OSD_F_PB_FRONT_INSIDE)))
        return fail(LDPC_E_ARG, "%s: LDPC_OSD_F_PB_REPLAY excludes %s", who, flag_name(f & (LDPC_OSD_F_PB_BLOCK | LDPC_OSD_F_PB_FRONT_INSIDE)));
    if ((f & LDPC_OSD_F_PB_FRONT_INSIDE) && front_outside)
        return fail(LDPC_E_ARG, "%s: LDPC_OSD_F_PB_FRONT_INSIDE keeps the front-end results inside the PB kernels, and this call "
                    "supplies or wants them", who);
    return LDPC_OK;
}

OsdPlan select_route(const ldpc_ctx *ctx, const ldpc_osd_params *p, bool front_outside)
{
    const unsigned f = (unsigned)p->flags;
    if (p->algo == LDPC_OSD_FS) return {OsdRoute::Fs, 0};
    if (p->algo == LDPC_OSD_PB)
        return {(f & LDPC_OSD_F_PB_FRONT_INSIDE) ? OsdRoute::PbFrontInside : OsdRoute::PbStaged,
                (f & LDPC_OSD_F_PB_REPLAY) ? 2 : ((f & LDPC_OSD_F_PB_BLOCK) ? 1 : 0)};
    if (p->order != 2 || (f & LDPC_OSD_F_TABLE_SCAN)) return {OsdRoute::Table, 0};
    // the rotation-paired kernels need the probed wave_rol:1 direction
    if ((f & LDPC_OSD_F_READLANE_SCAN) || ctx->dpp_wave_rol_dir == 0) return {OsdRoute::Search2, 0};
    return {front_outside ? OsdRoute::Search2r : OsdRoute::Fused2r, 0};
}

int osd_launch(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
               const uint64_t *d_parity, const ldpc_osd_params *p, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
               const uint64_t *d_label, int64_t *d_counts, hipStream_t s, bool *counted)
{
    *counted = false;
    const OsdPlan r = select_route(ctx, p, d_perm != nullptr);
    OsdState *st = state(ctx);
    const OsdTables &t = ctx->osd_tables;
    int rc;
    if ((rc = guarded_index(ctx, p, d_index, d_count, F, s, &d_index))) return rc;
    if (!d_perm && r.route != OsdRoute::Fused2r && r.route != OsdRoute::PbFrontInside) {   // the front end into the stream's workspace
        StreamWs *w;
        if ((rc = stream_ws(ctx, s, F, &w))) return rc;
        launch_front(ctx, d_y, d_index, d_count, F, w->d_perm, w->d_parity, nullptr, s);
        d_perm = w->d_perm; d_parity = reinterpret_cast<const uint64_t *>(w->d_parity);
    }
    const u64 *const parity = reinterpret_cast<const u64 *>(d_parity);
    u64 *const cw = reinterpret_cast<u64 *>(d_cw);
    const u64 *const label = d_label && d_counts ? reinterpret_cast<const u64 *>(d_label) : nullptr;
    u64 *const counts = label ? reinterpret_cast<u64 *>(d_counts) : nullptr;
    const unsigned g2r = grid2r(ctx, F), g64 = frame_grid(F);
    switch (r.route) {
    case OsdRoute::Fused2r: {
        // (the probed wave_rol:1 direction picks the instantiation; select_route leaves 0 to the read-lane scan)
        const auto kernel = ctx->dpp_wave_rol_dir > 0 ? osd_fused2r_kernel<1> : osd_fused2r_kernel<-1>;
        hipLaunchKernelGGL(kernel, dim3(g2r), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, t.d_Gcols, st->d_base2, cw, d_metric,
                           d_best, d_ntep, label, counts);
        *counted = label != nullptr;
        break;
    }
    case OsdRoute::Search2r: {
        const auto kernel = ctx->dpp_wave_rol_dir > 0 ? osd_search2r_kernel<1> : osd_search2r_kernel<-1>;
        hipLaunchKernelGGL(kernel, dim3(g2r), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, d_perm, parity, st->d_base2, cw, d_metric,
                           d_best, d_ntep, label, counts);
        *counted = label != nullptr;
        break;
    }
    case OsdRoute::Search2:
        hipLaunchKernelGGL(osd_search2_kernel, dim3(g64), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, d_perm, parity, st->d_base2,
                           cw, d_metric, d_best, d_ntep);
        break;
    case OsdRoute::Table:
        if (p->order >= 2)
            hipLaunchKernelGGL(osd_search_kernel<1>, dim3(g64), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, d_perm, parity,
                               t.d_tep, (int)t.ntep[p->order], cw, d_metric, d_best, d_ntep);
        else
            hipLaunchKernelGGL(osd_search_kernel<4>, dim3(osd_grid(F)), dim3(256), 0, s, d_y, d_index, d_count, (long long)F, d_perm, parity,
                               t.d_tep, (int)t.ntep[p->order], cw, d_metric, d_best, d_ntep);
        break;
    case OsdRoute::Fs:
        hipLaunchKernelGGL(osd_fs_kernel, dim3(g64), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, d_perm, parity, t.d_tep_fs,
                           fs_params(p, t.n, t.k, t.fs_off, t.fs_cnt), cw, d_metric, d_best, d_ntep);
        break;
    case OsdRoute::PbStaged:
        return launch_pb(ctx, d_y, d_index, d_count, F, d_perm, parity, p, r.pb_mode, false, d_cw, d_metric, d_best, d_ntep, s);
    // The front end INSIDE the first PB kernel, nothing through a workspace (not the list replay, which needs records to set a
    // frame up from).  Measured against the two kernels (osd_front + pb_singles, per 131 072-frame step): 170 against 164 us at
    // 2.5 dB, 507 against 481 us at 1.0 dB, 58 against 102 MB and 236 against 400 MB of HBM traffic -- the path is
    // instruction-bound, the traffic was never its limiter: an option, not the default.
    case OsdRoute::PbFrontInside:
        return launch_pb(ctx, d_y, d_index, d_count, F, nullptr, nullptr, p, r.pb_mode, true, d_cw, d_metric, d_best, d_ntep, s);
    }
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

FsParams fs_params(const ldpc_osd_params *p, int n, int k, const int (&fs_off)[4], const int (&fs_cnt)[4])
{
    FsParams fp;
    fp.order = p->order; fp.quirk = p->fs_reference_quirk != 0;
    fp.beta_term = (float)((double)p->fs_beta * (double)(n - k));   // fs_testing.py:138
    fp.tau_e = p->fs_tau_e; fp.tau_psc = p->fs_tau_psc;
    for (int w = 0; w < 4; ++w) { fp.cls_off[w] = fs_off[w]; fp.cls_cnt[w] = fs_cnt[w]; }
    return fp;
}

}  // namespace ldpc

using namespace ldpc;

extern "C" {

int ldpc_osd_reserve(ldpc_ctx *ctx, int64_t max_frames)
{
    if (!ctx || max_frames < 0) return fail(LDPC_E_ARG, "ldpc_osd_reserve: bad arguments");
    if (int rc = need_osd(ctx)) return rc;
    {
        OsdState *st = state(ctx);
        std::lock_guard<std::mutex> lock(st->mu);
        if (max_frames > st->reserve_frames) st->reserve_frames = max_frames;
    }
    StreamWs *w;
    return stream_ws(ctx, nullptr, max_frames, &w);   // the NULL stream's workspace now; other streams on their first call
}

int ldpc_osd_reserve_stream(ldpc_ctx *ctx, int64_t max_frames, const ldpc_osd_params *params, void *stream)
{
    if (!ctx || max_frames < 0) return fail(LDPC_E_ARG, "ldpc_osd_reserve_stream: bad arguments");
    int rc;
    if ((rc = need_osd(ctx))) return rc;
    if (params && (rc = check_params(ctx, params, false, "ldpc_osd_reserve_stream"))) return rc;
    StreamWs *w;
    if ((rc = stream_ws(ctx, (hipStream_t)stream, max_frames, &w)) || !params) return rc;
    if (params->algo == LDPC_OSD_PB && max_frames > 0) return pb_reserve(ctx, (hipStream_t)stream, max_frames, params->order);
    return LDPC_OK;
}

int ldpc_osd_release_stream(ldpc_ctx *ctx, void *stream)
{
    if (!ctx) return fail(LDPC_E_ARG, "ldpc_osd_release_stream: null ctx");
    OsdState *st = state(ctx);
    if (!st) return LDPC_OK;
    if (stream_capturing((hipStream_t)stream)) return fail(LDPC_E_ARG, "ldpc_osd_release_stream: the stream is capturing");
    std::lock_guard<std::mutex> lock(st->mu);
    auto it = st->ws.find((hipStream_t)stream);
    if (it != st->ws.end()) { free_stream_ws(it->second); st->ws.erase(it); }
    return LDPC_OK;
}

int ldpc_osd_ge(ldpc_ctx *ctx, const uint64_t *d_rows_in, int64_t F, uint64_t *d_rows_out, uint8_t *d_swaps,
                int32_t *d_nswaps, void *stream)
{
    if (!ctx || F < 0 || (F > 0 && (!d_rows_in || !d_rows_out))) return fail(LDPC_E_ARG, "ldpc_osd_ge: bad arguments");
    if (int rc = need_osd(ctx)) return rc;
    if (F == 0) return LDPC_OK;
    hipLaunchKernelGGL(osd_ge_kernel, dim3(osd_grid(F)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const u64 *>(d_rows_in), (long long)F, reinterpret_cast<u64 *>(d_rows_out), d_swaps,
                       d_nswaps);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_osd_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                   uint8_t *d_perm, uint64_t *d_parity, int32_t *d_nswaps, void *stream)
{
    if (!ctx || F < 0 || (F > 0 && (!d_y || !d_perm || !d_parity))) return fail(LDPC_E_ARG, "ldpc_osd_front: bad arguments");
    if (int rc = need_osd(ctx)) return rc;
    if (F == 0) return LDPC_OK;
    launch_front(ctx, d_y, d_index, d_count, F, d_perm, reinterpret_cast<u64 *>(d_parity), d_nswaps, (hipStream_t)stream);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_osd_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                    const uint8_t *d_perm, const uint64_t *d_parity, const ldpc_osd_params *p, uint64_t *d_cw,
                    float *d_metric, int32_t *d_best, int32_t *d_ntep, void *stream)
{
    if (!ctx || !p || F < 0 || (F > 0 && (!d_y || !d_cw || !d_perm || !d_parity)))
        return fail(LDPC_E_ARG, "ldpc_osd_search: bad arguments");
    int rc = check_params(ctx, p, true, "ldpc_osd_search");
    if (rc || F == 0) return rc;
    bool counted;
    return osd_launch(ctx, d_y, d_index, d_count, F, d_perm, d_parity, p, d_cw, d_metric, d_best, d_ntep, nullptr, nullptr,
                      (hipStream_t)stream, &counted);
}

int ldpc_osd_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                    const ldpc_osd_params *p, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
                    void *stream)
{
    if (!ctx || !p || F < 0 || (F > 0 && (!d_y || !d_cw))) return fail(LDPC_E_ARG, "ldpc_osd_decode: bad arguments");
    int rc = check_params(ctx, p, false, "ldpc_osd_decode");
    if (rc || F == 0) return rc;
    bool counted;
    return osd_launch(ctx, d_y, d_index, d_count, F, nullptr, nullptr, p, d_cw, d_metric, d_best, d_ntep, nullptr, nullptr,
                      (hipStream_t)stream, &counted);
}

int ldpc_osd_index_errors(ldpc_ctx *ctx, int64_t *count)
{
    if (!ctx || !count) return fail(LDPC_E_ARG, "ldpc_osd_index_errors: null argument");
    *count = 0;
    OsdState *st = state(ctx);
    if (!st || !st->d_index_errors) return LDPC_OK;
    unsigned long long v = 0;
    LDPC_HIP(hipMemcpy(&v, st->d_index_errors, sizeof(v), hipMemcpyDeviceToHost));   // (synchronises the device)
    *count = (int64_t)v;
    return LDPC_OK;
}

int ldpc_osd_tep_eval(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                      const uint8_t *d_perm, const uint64_t *d_parity, const uint64_t *d_mask, uint64_t *d_cw, float *d_metric,
                      int32_t *d_hd, void *stream)
{
    if (!ctx || F < 0 || (F > 0 && (!d_y || !d_perm || !d_parity || !d_mask || !d_cw)))
        return fail(LDPC_E_ARG, "ldpc_osd_tep_eval: bad arguments");
    if (int rc = need_osd(ctx)) return rc;
    if (F == 0) return LDPC_OK;
    hipLaunchKernelGGL(osd_tep_eval_kernel, dim3(osd_grid(F)), dim3(256), 0, (hipStream_t)stream, d_y, d_index, d_count, (long long)F,
                       d_perm, reinterpret_cast<const u64 *>(d_parity), reinterpret_cast<const u64 *>(d_mask),
                       reinterpret_cast<u64 *>(d_cw), d_metric, d_hd);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_osd_counts(ldpc_ctx *ctx, const uint64_t *d_cw, const uint64_t *d_label_bits, const int32_t *d_index,
                    const int32_t *d_count, const int32_t *d_ntep, int64_t F, int64_t *d_counts, void *stream)
{
    if (!ctx || F < 0 || !d_counts || (F > 0 && (!d_cw || !d_label_bits))) return fail(LDPC_E_ARG, "ldpc_osd_counts: bad arguments");
    if (F == 0) return LDPC_OK;
    int64_t g = (F + 1023) / 1024;
    hipLaunchKernelGGL(osd_counts_kernel, dim3((unsigned)(g < 128 ? g : 128)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const u64 *>(d_cw), reinterpret_cast<const u64 *>(d_label_bits), d_index, d_count,
                       d_ntep, (long long)F, reinterpret_cast<u64 *>(d_counts));
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // extern "C"
