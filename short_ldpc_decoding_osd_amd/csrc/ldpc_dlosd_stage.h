// The launches behind ldpc_dlosd_pipeline_run (ldpc_api.hip), each beside the kernels it launches: every one runs on
// min(*d_count, F) frames, F the capacity that sizes the grid, on arguments that dlosd_pipeline_check (ldpc_dlosd_check.h)
// has validated.
#pragma once

#include "ldpc_internal.h"

namespace ldpc {

constexpr const char *kDlosdWho = "ldpc_dlosd_pipeline_run";   // the name in the texts of whatever these launches still refuse

// A family's counted front end and sliding scan behind one signature; d_lri / d_uidx travel as void *: their element is the
// family's (u8, or u16 for the long family).  xo / xm: the ordering and the metric values, [F][n].  The rest of the scan's
// arguments are the pipeline's members.
struct HosdStage {
    int (*front)(ldpc_ctx *, const float *xo, const int32_t *d_count, int64_t F, void *d_lri, void *d_uidx, uint64_t *d_M, int32_t *d_nswaps,
                 hipStream_t);
    int (*sliding)(ldpc_ctx *, const float *xo, const float *xm, const int32_t *d_count, int64_t F, const ldpc_dlosd_pipeline *p,
                   const uint64_t *d_label, hipStream_t);
};
const HosdStage &hosd_stage(int family);     // LDPC_HOSD_FAMILY_128 / _X / _W: ldpc_hosd.hip
const HosdStage &hosdl_stage();              // LDPC_HOSD_FAMILY_L: ldpc_hosdl.hip

// ldpc_dia_cnn (ldpc_dia.hip)
int dia_cnn_counted(const ldpc_ctx *ctx, const float *d_rows, const int32_t *d_count, int64_t F, int L, const float *weights, float *d_out,
                    hipStream_t st);
// d_metric_llr[j] = d_llr[d_index[j]] (and d_order_llr[j], where given: the ordering values of DIA = False) and, with labels,
// d_list_labels[j] = d_label_bits[d_index[j]] (ldpc_util.hip)
int dlosd_gather(const ldpc_ctx *ctx, const float *d_llr, const uint64_t *d_label_bits, const int32_t *d_index, const int32_t *d_count, int64_t F,
                 float *d_metric_llr, float *d_order_llr, uint64_t *d_list_labels, hipStream_t st);
// d_dl_counts of ldpc_dlosd_pipeline (ldpc_util.hip); d_success, d_global_min, d_truth and d_teps_evaluated nullable: success is
// d_success or, without it, d_global_min == d_truth
int dlosd_counts(const int32_t *d_deep_limit, const uint8_t *d_success, const float *d_global_min, const float *d_truth, const int32_t *d_teps_evaluated, const int32_t *d_block_off, int nblk,
                 int win, const int32_t *d_count, int64_t F, int64_t *d_dl_counts, hipStream_t st);

}  // namespace ldpc
