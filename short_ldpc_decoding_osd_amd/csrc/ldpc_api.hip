// Context management and the NMS entry point of the C ABI (include/ldpc_osd.h).
#include <string.h>

#include "ldpc_internal.h"
#include "ldpc_osd_family.h"   // FamilyStage: the OSD stage of ldpc_family_pipeline_run
#include "ldpc_dlosd_check.h"  // dlosd_pipeline_check
#include "ldpc_dlosd_stage.h"  // HosdStage and the other launches of ldpc_dlosd_pipeline_run

using namespace ldpc;

namespace ldpc {
int osd_ctx_init(ldpc_ctx *ctx);      // ldpc_osd.hip
void osd_ctx_release(ldpc_ctx *ctx);  // ldpc_osd.hip
int hosd_ctx_init(ldpc_ctx *ctx);     // ldpc_hosd.hip
void hosd_ctx_release(ldpc_ctx *ctx); // ldpc_hosd.hip
int hosdl_ctx_init(ldpc_ctx *ctx);    // ldpc_hosdl.hip
void hosdl_ctx_release(ldpc_ctx *ctx); // ldpc_hosdl.hip
}  // namespace ldpc

template <typename T>
static int upload(const std::vector<T> &v, T **dst)
{
    LDPC_HIP(hipMalloc((void **)dst, sizeof(T) * (v.size() ? v.size() : 1)));
    if (!v.empty()) LDPC_HIP(hipMemcpy(*dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return LDPC_OK;
}

extern "C" {

int ldpc_ctx_create(const ldpc_code *code, int32_t device, ldpc_ctx **out)
{
    if (!code || !out) return fail(LDPC_E_ARG, "ldpc_ctx_create: null argument");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(LDPC_E_HIP, "ldpc_ctx_create: no HIP device visible (%s) -- this library has no CPU path",
                    hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(LDPC_E_ARG, "ldpc_ctx_create: device %d of %d", device, ndev);
    int prev = 0;
    LDPC_HIP(hipGetDevice(&prev));
    LDPC_HIP(hipSetDevice(device));
    ldpc_ctx *ctx = new ldpc_ctx();
    ctx->device = device;
    ctx->code = *code;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ctx->cu_count = prop.multiProcessorCount;
    }
    int rc = LDPC_OK;
    do {
        if ((rc = upload(code->chk_ptr, &ctx->d_chk_ptr))) break;
        if ((rc = upload(code->chk_var, &ctx->d_chk_var))) break;
        if ((rc = upload(code->var_ptr, &ctx->d_var_ptr))) break;
        if ((rc = upload(code->var_edge, &ctx->d_var_edge))) break;
        {   // the OSD tables of every shape they exist for (ldpc_osd_tables.h); osd_ctx_init finds them in place
            OsdTables &t = ctx->osd_tables;
            OsdTablesHost host;
            if ((rc = pack_osd_tables(ctx->code, t, host))) break;
            if (t.k && ((rc = upload(host.Gcols, &t.d_Gcols)) || (rc = upload(host.tep, &t.d_tep)) ||
                        (rc = upload(host.tep_fs, &t.d_tep_fs)) || (rc = upload(host.pb, &t.d_pb)))) break;
        }
        {   // the tables of the high-rate family (ldpc_osdw.hip); the TEP tables of a k <= 64 are the ones uploaded above
            OsdwTables &w = ctx->osdw_tables;
            OsdwTablesHost host;
            if ((rc = pack_osdw_tables(ctx->code, ctx->osd_tables, w, host))) break;
            if (w.k && (rc = upload(host.Gcols, &w.d_Gcols))) break;
            if (w.k && w.own_tep && ((rc = upload(host.tep, &w.d_tep)) || (rc = upload(host.tep_fs, &w.d_tep_fs)) ||
                                       (rc = upload(host.pb, &w.d_pb)))) break;
            if (w.k && !w.own_tep) { w.d_tep = ctx->osd_tables.d_tep; w.d_tep_fs = ctx->osd_tables.d_tep_fs; w.d_pb = ctx->osd_tables.d_pb; }
        }
        {   // the tables of the long / low-rate family (ldpc_osdl.hip, ldpc_osdl_fs.hip, ldpc_osdl_pb.hip); the TEP tables of a code the high-rate family serves are the ones above
            OsdlTables &l = ctx->osdl_tables;
            OsdlTablesHost host;
            if ((rc = pack_osdl_tables(ctx->code, ctx->osdw_tables, l, host))) break;
            if (l.k && (rc = upload(host.Gcols, &l.d_Gcols))) break;
            if (l.k && l.own_tep && ((rc = upload(host.tep, &l.d_tep)) || (rc = upload(host.tep_fs, &l.d_tep_fs)))) break;
            if (l.k && !l.own_tep) { l.d_tep = ctx->osdw_tables.d_tep; l.d_tep_fs = ctx->osdw_tables.d_tep_fs; }
            if (l.k && (rc = upload(host.pb, &l.d_pb))) break;
        }
        if ((rc = probe_dpp(&ctx->dpp_ror_up, &ctx->dpp_wave_rol_dir))) break;
        // event pool of ldpc_pipeline_run's timing slots: created (and recorded once: the first record of an
        // event sets up its signal and is slow) here, so that decode calls never create anything.  The warm-up
        // records go to a private stream -- the legacy NULL stream would synchronise with every blocking stream
        // of the process and break a capture in progress elsewhere.
        ctx->timing = new hipEvent_t[LDPC_TIMING_SLOTS * 6]();
        hipStream_t warm = nullptr;
        if (hipStreamCreateWithFlags(&warm, hipStreamNonBlocking) != hipSuccess) { rc = fail(LDPC_E_HIP, "ldpc_ctx_create: stream creation failed"); break; }
        for (int i = 0; i < LDPC_TIMING_SLOTS * 6 && !rc; ++i) {
            hipError_t he = hipEventCreate(&ctx->timing[i]);
            if (he == hipSuccess) he = hipEventRecord(ctx->timing[i], warm);
            if (he != hipSuccess) rc = hip_fail(he, "timing event pool");
        }
        if (!rc && hipStreamSynchronize(warm) != hipSuccess) rc = fail(LDPC_E_HIP, "ldpc_ctx_create: stream sync failed");
        (void)hipStreamDestroy(warm);
        if (rc) break;
        if ((rc = osd_ctx_init(ctx))) break;
        if ((rc = hosd_ctx_init(ctx))) break;
        if ((rc = hosdl_ctx_init(ctx))) break;
        if ((rc = gen_ctx_init(ctx))) break;
    } while (0);
    (void)hipSetDevice(prev);
    if (rc) { ldpc_ctx_destroy(ctx); return rc; }
    *out = ctx;
    return LDPC_OK;
}

void ldpc_ctx_destroy(ldpc_ctx *ctx)
{
    if (!ctx) return;
    osd_ctx_release(ctx);
    hosd_ctx_release(ctx);
    hosdl_ctx_release(ctx);
    gen_ctx_release(ctx);
    (void)hipFree(ctx->osd_tables.d_Gcols); (void)hipFree(ctx->osd_tables.d_tep); (void)hipFree(ctx->osd_tables.d_tep_fs);
    (void)hipFree(ctx->osd_tables.d_pb);
    (void)hipFree(ctx->osdw_tables.d_Gcols);
    if (ctx->osdw_tables.own_tep) {
        (void)hipFree(ctx->osdw_tables.d_tep); (void)hipFree(ctx->osdw_tables.d_tep_fs); (void)hipFree(ctx->osdw_tables.d_pb);
    }
    (void)hipFree(ctx->osdl_tables.d_Gcols); (void)hipFree(ctx->osdl_tables.d_pb);
    if (ctx->osdl_tables.own_tep) { (void)hipFree(ctx->osdl_tables.d_tep); (void)hipFree(ctx->osdl_tables.d_tep_fs); }
    (void)hipFree(ctx->d_chk_ptr); (void)hipFree(ctx->d_chk_var);
    (void)hipFree(ctx->d_var_ptr); (void)hipFree(ctx->d_var_edge);
    if (ctx->timing) {
        for (int i = 0; i < LDPC_TIMING_SLOTS * 6; ++i) if (ctx->timing[i]) (void)hipEventDestroy(ctx->timing[i]);
        delete[] ctx->timing;
    }
    delete ctx;
}

int ldpc_ctx_nms_kernel(const ldpc_ctx *ctx)
{
    if (!ctx) return fail(LDPC_E_ARG, "ldpc_ctx_nms_kernel: null ctx");
    return ctx->code.qc16_ccsds ? LDPC_NMS_QC16 : LDPC_NMS_GENERIC;
}

int ldpc_gen_frames(ldpc_ctx *ctx, const ldpc_gen_params *p, int64_t B, float *d_y, uint64_t *d_label_bits, void *stream)
{
    if (!ctx) return fail(LDPC_E_ARG, "ldpc_gen_frames: ctx is NULL");
    if (!p) return fail(LDPC_E_ARG, "ldpc_gen_frames: p is NULL");
    if (B < 0) return fail(LDPC_E_ARG, "ldpc_gen_frames: B = %lld is negative", (long long)B);
    if (p->frame0 < 0) return fail(LDPC_E_ARG, "ldpc_gen_frames: frame0 = %lld is negative", (long long)p->frame0);
    if (!(p->sigma >= 0.0f) || !(p->sigma <= 3.402823466e+38f))   // (NaN fails both comparisons)
        return fail(LDPC_E_ARG, "ldpc_gen_frames: sigma = %g is not a finite value >= 0", (double)p->sigma);
    if (p->flags & ~(uint32_t)(LDPC_GEN_F_ALL_ZEROS | LDPC_GEN_F_RAYLEIGH))
        return fail(LDPC_E_ARG, "ldpc_gen_frames: unknown flag bits 0x%x", p->flags & ~(uint32_t)(LDPC_GEN_F_ALL_ZEROS | LDPC_GEN_F_RAYLEIGH));
    if ((p->flags & LDPC_GEN_F_RAYLEIGH) && p->fade_len < 1)
        return fail(LDPC_E_ARG, "ldpc_gen_frames: fade_len = %d with LDPC_GEN_F_RAYLEIGH (want >= 1)", p->fade_len);
    if (B == 0 || (!d_y && !d_label_bits)) return LDPC_OK;
    return launch_gen(ctx, p, B, d_y, d_label_bits, (hipStream_t)stream);
}

int ldpc_nms_decode(ldpc_ctx *ctx, const float *d_llr, int64_t B, int32_t T, const float *alpha, float w_in,
                    float w_out, float *d_soft, float *d_traj, uint64_t *d_hard, uint8_t *d_fail, int32_t kernel,
                    void *stream)
{
    if (!ctx || B < 0 || (!d_llr && B > 0)) return fail(LDPC_E_ARG, "ldpc_nms_decode: bad arguments");
    if (T < 0 || T > kMaxIters) return fail(LDPC_E_ARG, "ldpc_nms_decode: T=%d outside 0..%d", T, kMaxIters);
    if (T > 0 && !alpha) return fail(LDPC_E_ARG, "ldpc_nms_decode: alpha is NULL");
    if (B == 0) return LDPC_OK;
    return launch_nms(ctx, d_llr, B, T, alpha, w_in, w_out, d_soft, d_traj, d_hard, d_fail, kernel, (hipStream_t)stream);
}

int ldpc_nms_traj_rows(ldpc_ctx *ctx, const float *d_llr, const int32_t *d_index, const int32_t *d_count, int64_t F, int32_t T,
                       const float *alpha, float w_in, float w_out, float *d_rows, int32_t kernel, void *stream)
{
    if (!ctx || F < 0 || ((!d_llr || !d_index || !d_rows) && F > 0)) return fail(LDPC_E_ARG, "ldpc_nms_traj_rows: bad arguments");
    if (T < 0 || T > kMaxIters) return fail(LDPC_E_ARG, "ldpc_nms_traj_rows: T=%d outside 0..%d", T, kMaxIters);
    if (T > 0 && !alpha) return fail(LDPC_E_ARG, "ldpc_nms_traj_rows: alpha is NULL");
    if (!d_count) return fail(LDPC_E_ARG, "ldpc_nms_traj_rows: d_count is NULL (the number of listed frames is device data)");
    if (F == 0) return LDPC_OK;
    return launch_nms(ctx, d_llr, F, T, alpha, w_in, w_out, nullptr, nullptr, nullptr, nullptr, kernel, (hipStream_t)stream, d_index, d_count, d_rows);
}

int ldpc_nms_train_grad(ldpc_ctx *ctx, const float *d_llr, const uint64_t *d_label_bits, int64_t B, int32_t T, const float *alpha,
                        float w_in, float w_out, float *d_loss, float *d_grad, double *d_loss_sum, double *d_grad_sum, float *d_traj,
                        uint64_t *d_hard, uint8_t *d_fail, void *stream)
{
    if (!ctx || B < 0 || ((!d_llr || !d_label_bits) && B > 0)) return fail(LDPC_E_ARG, "ldpc_nms_train_grad: bad arguments");
    if (T < 0 || T > kMaxIters) return fail(LDPC_E_ARG, "ldpc_nms_train_grad: T=%d outside 0..%d", T, kMaxIters);
    if (T > 0 && !alpha) return fail(LDPC_E_ARG, "ldpc_nms_train_grad: alpha is NULL");
    if (B == 0) return LDPC_OK;
    return launch_nms_train(ctx, d_llr, d_label_bits, B, T, alpha, w_in, w_out, d_loss, d_grad, d_loss_sum, d_grad_sum, d_traj,
                            d_hard, d_fail, (hipStream_t)stream);
}

int ldpc_pipeline_run(ldpc_ctx *ctx, const ldpc_pipeline *p, void *stream)
{
    if (!ctx || !p) return fail(LDPC_E_ARG, "ldpc_pipeline_run: null argument");
    if (p->B < 0 || (p->B > 0 && !p->d_llr)) return fail(LDPC_E_ARG, "ldpc_pipeline_run: d_llr is NULL or B < 0");
    if (p->T > 0 && !p->alpha) return fail(LDPC_E_ARG, "ldpc_pipeline_run: alpha is NULL");
    if (!p->d_hard || !p->d_fail) return fail(LDPC_E_ARG, "ldpc_pipeline_run: d_hard and d_fail are required");
    const bool front = p->d_perm && p->d_parity;   // the caller wants the front-end results: front end and search apart
    int rc;
    if (p->osd_enable) {
        if (!p->d_index || !p->d_count || !p->d_cw)
            return fail(LDPC_E_ARG, "ldpc_pipeline_run: OSD stage needs d_index, d_count, d_cw");
        if (!p->d_perm != !p->d_parity)
            return fail(LDPC_E_ARG, "ldpc_pipeline_run: d_perm and d_parity go together (both, or both NULL); %s is NULL",
                        p->d_perm ? "d_parity" : "d_perm");
        if ((rc = check_params(ctx, &p->osd, front, "ldpc_pipeline_run"))) return rc;
    }
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t *ev = nullptr;
    unsigned *rec = nullptr;            // which of the slot's events THIS run records (ldpc_pipeline_timing reads only those)
    if (p->timing_slot >= 0) {
        if (p->timing_slot >= LDPC_TIMING_SLOTS || !ctx->timing) return fail(LDPC_E_ARG, "ldpc_pipeline_run: timing_slot %d", p->timing_slot);
        ev = ctx->timing + p->timing_slot * 6;
        rec = &ctx->timing_recorded[p->timing_slot];
        *rec = 0;
    }
#define LDPC_EV(i) do { if (ev) { LDPC_HIP(hipEventRecord(ev[i], s)); *rec |= 1u << (i); } } while (0)
    LDPC_EV(0);
    if ((rc = ldpc_nms_decode(ctx, p->d_llr, p->B, p->T, p->alpha, p->w_in, p->w_out, p->d_soft, nullptr, p->d_hard,
                              p->d_fail, p->nms_kernel, stream))) return rc;
    LDPC_EV(1);
    const bool want_eval = p->d_label_bits && p->d_nms_counts;
    if (!p->osd_enable) {
        if (want_eval && (rc = ldpc_eval_counts(ctx, p->d_hard, p->d_label_bits, p->d_fail, p->B, p->d_nms_counts, stream))) return rc;
        return LDPC_OK;
    }
    if (want_eval && p->B > 0) {   // counters and the compaction's counting pass share one kernel
        if ((rc = eval_and_compact(ctx, p->d_hard, p->d_label_bits, p->d_fail, p->B, p->d_nms_counts, p->d_index,
                                   p->d_count, s))) return rc;
    } else if ((rc = ldpc_compact(ctx, p->d_fail, p->B, p->d_index, p->d_count, stream))) return rc;
    LDPC_EV(2);
    if (front && (rc = ldpc_osd_front(ctx, p->d_llr, p->d_index, p->d_count, p->B, p->d_perm, p->d_parity, nullptr, stream))) return rc;
    LDPC_EV(3);
    // the search kernel counts its own successes where it can (rotation-paired order-2 scan); otherwise the counting launch
    // follows the search's closing event, so that ms[2] is the search alone for every route
    const bool counts = p->d_label_bits && p->d_osd_counts;
    bool counted = false;
    if (p->B > 0 && (rc = osd_launch(ctx, p->d_llr, p->d_index, p->d_count, p->B, front ? p->d_perm : nullptr, front ? p->d_parity : nullptr,
                                     &p->osd, p->d_cw, p->d_metric, p->d_best, p->d_ntep, counts ? p->d_label_bits : nullptr,
                                     counts ? p->d_osd_counts : nullptr, s, &counted))) return rc;
    LDPC_EV(4);
    if (counts && !counted &&
        (rc = ldpc_osd_counts(ctx, p->d_cw, p->d_label_bits, p->d_index, p->d_count, p->d_ntep, p->B, p->d_osd_counts, stream))) return rc;
#undef LDPC_EV
    return LDPC_OK;
}

int ldpc_family_pipeline_run(ldpc_ctx *ctx, const ldpc_family_pipeline *p, void *stream)
{
    static const char who[] = "ldpc_family_pipeline_run";
    int family, rc;
    int64_t F;                          // the frames the OSD buffers hold
    if ((rc = family_pipeline_check(ctx, p, who, &family, &F))) return rc;
    const FamilyStage *fam = family == LDPC_OSD_FAMILY_X ? &osdx_stage() : family == LDPC_OSD_FAMILY_W ? &osdw_stage() : &osdl_stage();
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t *ev = nullptr;
    unsigned *rec = nullptr;            // which of the slot's events THIS run records (ldpc_pipeline_timing reads only those)
    if (p->timing_slot >= 0) {
        ev = ctx->timing + p->timing_slot * 6;
        rec = &ctx->timing_recorded[p->timing_slot];
        *rec = 0;
    }
#define LDPC_EV(i) do { if (ev) { LDPC_HIP(hipEventRecord(ev[i], s)); *rec |= 1u << (i); } } while (0)
    LDPC_EV(0);
    if ((rc = ldpc_nms_decode(ctx, p->d_llr, p->B, p->T, p->alpha, p->w_in, p->w_out, p->d_soft, nullptr, p->d_hard,
                              p->d_fail, p->nms_kernel, stream))) return rc;
    LDPC_EV(1);
    const bool want_eval = p->d_label_bits && p->d_nms_counts;
    if (!p->osd_enable) {
        if (want_eval && (rc = ldpc_eval_counts(ctx, p->d_hard, p->d_label_bits, p->d_fail, p->B, p->d_nms_counts, stream))) return rc;
        return LDPC_OK;
    }
    if (want_eval && p->B > 0) {   // counters and the compaction's counting pass share one kernel
        if ((rc = eval_and_compact(ctx, p->d_hard, p->d_label_bits, p->d_fail, p->B, p->d_nms_counts, p->d_index,
                                   p->d_count, s))) return rc;
    } else if ((rc = ldpc_compact(ctx, p->d_fail, p->B, p->d_index, p->d_count, stream))) return rc;
    if (F == 0) return LDPC_OK;
    const OsdFrames fr{p->d_llr, p->d_index, p->d_count, F};
    LDPC_EV(2);
    if ((rc = fam->front(ctx, fr, p->d_perm, p->d_parity, s))) return rc;
    LDPC_EV(3);
    if ((rc = fam->scan(ctx, fr, p->d_perm, p->d_parity, &p->osd, {p->d_cw, p->d_metric, p->d_best, p->d_ntep},
                        osd_counting(p->d_label_bits, p->d_osd_counts), s))) return rc;
    LDPC_EV(4);
#undef LDPC_EV
    if (p->merge) return ldpc_osd_merge(ctx, p->d_cw, p->d_index, p->d_count, F, p->d_hard, p->d_label_bits, p->d_final_counts, stream);
    return LDPC_OK;
}

int ldpc_dlosd_pipeline_run(ldpc_ctx *ctx, const ldpc_dlosd_pipeline *p, void *stream)
{
    int family, rc;
    int64_t F;                          // the rows the list buffers hold
    if ((rc = dlosd_pipeline_check(ctx, p, kDlosdWho, &family, &F))) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t *ev = nullptr;
    unsigned *rec = nullptr;            // which of the slot's events THIS run records (ldpc_pipeline_timing reads only those)
    if (p->timing_slot >= 0) {
        ev = ctx->timing + p->timing_slot * 6;
        rec = &ctx->timing_recorded[p->timing_slot];
        *rec = 0;
    }
#define LDPC_EV(i) do { if (ev) { LDPC_HIP(hipEventRecord(ev[i], s)); *rec |= 1u << (i); } } while (0)
    LDPC_EV(0);
    if ((rc = ldpc_nms_decode(ctx, p->d_llr, p->B, p->T, p->alpha, p->w_in, p->w_out, p->d_soft, nullptr, p->d_hard,
                              p->d_fail, p->nms_kernel, stream))) return rc;
    LDPC_EV(1);
    const bool want_eval = p->d_label_bits && p->d_nms_counts;
    if (!p->osd_enable) {
        if (want_eval && (rc = ldpc_eval_counts(ctx, p->d_hard, p->d_label_bits, p->d_fail, p->B, p->d_nms_counts, stream))) return rc;
        return LDPC_OK;
    }
    if (want_eval && p->B > 0) {   // counters and the compaction's counting pass share one kernel
        if ((rc = eval_and_compact(ctx, p->d_hard, p->d_label_bits, p->d_fail, p->B, p->d_nms_counts, p->d_index,
                                   p->d_count, s))) return rc;
    } else if ((rc = ldpc_compact(ctx, p->d_fail, p->B, p->d_index, p->d_count, stream))) return rc;
    if (F == 0) return LDPC_OK;
    const HosdStage &fam = family == LDPC_HOSD_FAMILY_L ? hosdl_stage() : hosd_stage(family);
    LDPC_EV(2);
    // without a CNN the ordering values are the channel values: the gather fills d_order_llr with them where the caller gave it,
    // else front end and scan read d_metric_llr for both inputs
    const float *xo = p->d_order_llr ? p->d_order_llr : p->d_metric_llr;
    if (p->cnn_weights) {
        if ((rc = ldpc_nms_traj_rows(ctx, p->d_llr, p->d_index, p->d_count, F, p->T, p->alpha, p->w_in, p->w_out, p->d_rows, p->nms_kernel,
                                     stream))) return rc;
        if ((rc = dia_cnn_counted(ctx, p->d_rows, p->d_count, F, p->T + 1, p->cnn_weights, p->d_order_llr, s))) return rc;
        xo = p->d_order_llr;
    }
    if ((rc = dlosd_gather(ctx, p->d_llr, p->d_label_bits, p->d_index, p->d_count, F, p->d_metric_llr, p->cnn_weights ? nullptr : p->d_order_llr,
                           p->d_list_labels, s))) return rc;
    if ((rc = fam.front(ctx, xo, p->d_count, F, p->d_lri, p->d_uidx, p->d_M, p->d_nswaps, s))) return rc;
    LDPC_EV(3);
    if ((rc = fam.sliding(ctx, xo, p->d_metric_llr, p->d_count, F, p, p->d_label_bits ? p->d_list_labels : nullptr, s))) return rc;
    LDPC_EV(4);
#undef LDPC_EV
    if (p->d_dl_counts &&
        (rc = dlosd_counts(p->d_deep_limit, p->d_label_bits ? p->d_success : nullptr, p->d_label_bits ? p->d_global_min : nullptr,
                           p->d_label_bits ? p->d_truth : nullptr, p->d_teps_evaluated, p->d_block_off, p->nblk, p->win,
                           p->d_count, F, p->d_dl_counts, s))) return rc;
    if (p->merge) return ldpc_osd_merge(ctx, p->d_cw, p->d_index, p->d_count, F, p->d_hard, p->d_label_bits, p->d_final_counts, stream);
    return LDPC_OK;
}

int ldpc_pipeline_timing(ldpc_ctx *ctx, int32_t slot, float *ms)
{
    if (!ctx || !ms || slot < 0 || slot >= LDPC_TIMING_SLOTS || !ctx->timing)
        return fail(LDPC_E_ARG, "ldpc_pipeline_timing: no timed run in slot %d", slot);
    hipEvent_t *ev = ctx->timing + slot * 6;
    const unsigned rec = ctx->timing_recorded[slot];     // events of the LAST run that used the slot (all were recorded once at creation)
    ms[0] = ms[1] = ms[2] = 0.0f;
    if ((rec & 3u) != 3u) return fail(LDPC_E_ARG, "ldpc_pipeline_timing: no timed run in slot %d", slot);
    LDPC_HIP(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
    if ((rec & 0xCu) == 0xCu && hipEventElapsedTime(&ms[1], ev[2], ev[3]) != hipSuccess) { ms[1] = 0.0f; (void)hipGetLastError(); }
    if ((rec & 0x18u) == 0x18u && hipEventElapsedTime(&ms[2], ev[3], ev[4]) != hipSuccess) { ms[2] = 0.0f; (void)hipGetLastError(); }
    return LDPC_OK;
}

}  // extern "C"
