// Sanitizer build only (python -m short_ldpc_decoding_osd_amd.build --asan --run): a stand-alone program that drives the
// host-side validation of ldpc_osd_merge, ldpc_family_pipeline_run and ldpc_dlosd_pipeline_run (ldpc_sanitizer_checks.cpp over
// ldpc_family_check.h and ldpc_dlosd_check.h) under -fsanitize=address,undefined.  No device: the contexts are made by hand, with the shape of a code and the k of each family's
// tables as ldpc_ctx_create would leave them, and every pointer is a host address that nothing dereferences.  A call that
// passes validation ends in the stub's "exists only in the HIP build".  Exit status 0 when every expectation holds.
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "ldpc_internal.h"

static int failures = 0;

static void expect(int rc, int want, const char *text, const char *what)
{
    const char *err = ldpc_last_error();
    if (rc != want || (text && !strstr(err, text))) {
        printf("FAIL %s: rc %d (want %d), message '%s' (want '%s')\n", what, rc, want, err, text ? text : "");
        ++failures;
    }
}

static ldpc_ctx *make_ctx(int n, int k)
{
    ldpc_ctx *ctx = new ldpc_ctx();
    ctx->code.n = n; ctx->code.k = k; ctx->code.m = n - k;
    const int m = n - k;
    ctx->osd_tables.k = k <= 64 && m <= 64 ? k : 0;
    ctx->osdw_tables.k = n <= 128 && m <= 64 ? k : 0;
    ctx->osdl_tables.k = n <= 384 && k <= 192 && m <= 192 ? k : 0;
    // the H-form families, as hosd_ctx_init / hosdl_ctx_init decide for an H of exactly n - k rows
    ctx->hosdw_ok = n <= 128 && m >= 1 && m <= 64 && k >= 1 && k <= 127;
    ctx->hosdx_ok = ctx->hosdw_ok && k <= 64;
    ctx->hosd_ok = n == 128 && k == 64;
    ctx->hosdl_ok = n <= 384 && m >= 1 && m <= 192 && k >= 1 && k <= 192;
    return ctx;
}

int main()
{
    static uint64_t words[8];
    static int32_t ints[8];
    static int64_t counts[8];
    static float floats[8];
    static uint8_t bytes[8];
    const float alpha[4] = {0.7f, 0.7f, 0.7f, 0.7f};
    const char *stub = "exists only in the HIP build";

    ldpc_ctx *c121 = make_ctx(121, 80), *c96 = make_ctx(96, 48), *c384 = make_ctx(384, 192), *c1056 = make_ctx(1056, 880);

    // ---- ldpc_osd_merge
    expect(ldpc_osd_merge(nullptr, words, ints, ints, 4, words, words, counts, nullptr), LDPC_E_ARG, "ldpc_osd_merge: bad arguments", "merge ctx");
    expect(ldpc_osd_merge(c96, words, ints, ints, -1, words, words, counts, nullptr), LDPC_E_ARG, "ldpc_osd_merge: bad arguments", "merge F < 0");
    expect(ldpc_osd_merge(c96, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr), LDPC_OK, nullptr, "merge F == 0");
    expect(ldpc_osd_merge(c96, nullptr, ints, ints, 4, words, words, counts, nullptr), LDPC_E_ARG, "ldpc_osd_merge: d_cw is NULL", "merge d_cw");
    expect(ldpc_osd_merge(c96, words, nullptr, ints, 4, words, words, counts, nullptr), LDPC_E_ARG, "ldpc_osd_merge: d_index is NULL", "merge d_index");
    expect(ldpc_osd_merge(c96, words, ints, nullptr, 4, words, words, counts, nullptr), LDPC_E_ARG, "ldpc_osd_merge: d_count is NULL", "merge d_count");
    expect(ldpc_osd_merge(c96, words, ints, ints, 4, nullptr, nullptr, nullptr, nullptr), LDPC_OK, nullptr, "merge nothing to do");
    expect(ldpc_osd_merge(c96, words, ints, ints, 4, nullptr, words, nullptr, nullptr), LDPC_OK, nullptr, "merge labels without counters");
    expect(ldpc_osd_merge(c1056, words, ints, ints, 4, words, nullptr, nullptr, nullptr), LDPC_E_UNSUPPORTED, stub, "merge on a code no family serves");

    // ---- ldpc_family_pipeline_run
    ldpc_family_pipeline good;
    memset(&good, 0, sizeof(good));
    good.d_llr = floats; good.B = 4; good.T = 4; good.alpha = alpha; good.w_in = good.w_out = 1.0f;
    good.d_hard = words; good.d_fail = bytes; good.osd_enable = 1; good.timing_slot = -1;
    good.osd.order = 2; good.osd.algo = LDPC_OSD_CONVENTIONAL;
    good.family = LDPC_OSD_FAMILY_AUTO; good.merge = 1;
    good.d_index = ints; good.d_count = ints; good.d_perm = bytes; good.d_parity = words; good.d_cw = words;
    expect(ldpc_family_pipeline_run(nullptr, &good, nullptr), LDPC_E_ARG, "null argument", "pipeline ctx");
    expect(ldpc_family_pipeline_run(c96, nullptr, nullptr), LDPC_E_ARG, "null argument", "pipeline p");
    expect(ldpc_family_pipeline_run(c96, &good, nullptr), LDPC_E_UNSUPPORTED, "validated: family 1, 4 OSD frames", "AUTO on (96,48)");
    expect(ldpc_family_pipeline_run(c121, &good, nullptr), LDPC_E_UNSUPPORTED, "validated: family 2, 4 OSD frames", "AUTO on (121,80)");
    expect(ldpc_family_pipeline_run(c384, &good, nullptr), LDPC_E_UNSUPPORTED, "validated: family 3, 4 OSD frames", "AUTO on (384,192)");
    expect(ldpc_family_pipeline_run(c1056, &good, nullptr), LDPC_E_UNSUPPORTED, "n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192; this code is (1056,880)", "AUTO on wimax");
    ldpc_family_pipeline p = good;
    p.osd_enable = 0;
    expect(ldpc_family_pipeline_run(c1056, &p, nullptr), LDPC_E_UNSUPPORTED, "validated: family 0, 0 OSD frames", "NMS only on wimax");
    p = good; p.family = LDPC_OSD_FAMILY_X;
    expect(ldpc_family_pipeline_run(c121, &p, nullptr), LDPC_E_UNSUPPORTED, "1 <= k <= 64 and 1 <= n-k <= 64; this code is (121,80)", "X forced on (121,80)");
    p.family = LDPC_OSD_FAMILY_W;
    expect(ldpc_family_pipeline_run(c384, &p, nullptr), LDPC_E_UNSUPPORTED, "1 <= n-k <= 64 and n <= 128; this code is (384,192)", "W forced on (384,192)");
    p.family = LDPC_OSD_FAMILY_L;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_UNSUPPORTED, "validated: family 3", "L forced on (96,48)");
    p.family = 4;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "family 4 is no LDPC_OSD_FAMILY_* value", "family 4");
    p = good; p.osd_capacity = 3;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_UNSUPPORTED, "validated: family 1, 3 OSD frames", "capacity 3");
    p.osd_capacity = 9;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_UNSUPPORTED, "validated: family 1, 4 OSD frames", "capacity above B");
    p.osd_capacity = -1;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "osd_capacity -1 is negative", "capacity -1");
    p = good; p.osd.order = 4;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "ldpc_family_pipeline_run: order 4 outside 0..3", "order 4");
    p.osd.algo = LDPC_OSD_FS;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "ldpc_family_pipeline_run: order 4 outside 0..3", "FS order 4");
    p = good; p.osd.algo = LDPC_OSD_FS; p.osd.d_aux = ints;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "d_aux is not served here", "FS with d_aux");
    p.osd.algo = LDPC_OSD_CONVENTIONAL;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "d_aux is not served here", "conventional with d_aux");
    p.osd.algo = LDPC_OSD_PB;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_UNSUPPORTED, stub, "PB with d_aux");
    p = good; p.osd.flags = 1;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "flags 0x1 are not served here", "flags");
    p = good; p.osd.y_frames = 9;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "y_frames 9 is not served here", "y_frames");
    p = good; p.osd.algo = 7;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "algo 7 is none of", "algo 7");
    p = good; p.d_perm = nullptr;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "ldpc_family_pipeline_run: d_perm is NULL", "d_perm");
    p = good; p.d_parity = nullptr;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "ldpc_family_pipeline_run: d_parity is NULL", "d_parity");
    p = good; p.d_cw = nullptr;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "ldpc_family_pipeline_run: d_cw is NULL", "d_cw");
    p = good; p.d_hard = nullptr;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "d_hard and d_fail are required", "d_hard");
    p = good; p.d_llr = nullptr;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "d_llr is NULL or B outside", "d_llr");
    p = good; p.alpha = nullptr;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "alpha is NULL", "alpha");
    p = good; p.T = 65;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "T=65 outside 0..64", "T");
    p = good; p.timing_slot = LDPC_TIMING_SLOTS;
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "timing_slot 64", "timing_slot 64");
    p.timing_slot = 0;                                   // (a context made by hand has no event pool)
    expect(ldpc_family_pipeline_run(c96, &p, nullptr), LDPC_E_ARG, "timing_slot 0", "timing_slot without a pool");

    // ---- ldpc_dlosd_pipeline_run
    const char *dl = "ldpc_dlosd_pipeline_run: ";
    ldpc_ctx *c128 = make_ctx(128, 64);
    static float fcn[24], cnn[147];
    ldpc_dlosd_pipeline dgood;
    memset(&dgood, 0, sizeof(dgood));
    dgood.d_llr = floats; dgood.B = 4; dgood.T = 6; dgood.alpha = alpha; dgood.w_in = dgood.w_out = 1.0f;   // (alpha is not read)
    dgood.d_hard = words; dgood.d_fail = bytes; dgood.d_label_bits = words; dgood.osd_enable = 1; dgood.timing_slot = -1;
    dgood.family = LDPC_HOSD_FAMILY_AUTO; dgood.merge = 1;
    dgood.d_index = ints; dgood.d_count = ints;
    dgood.cnn_weights = cnn; dgood.n_cnn_weights = 147; dgood.fcn_weights = fcn; dgood.n_fcn_weights = 24;
    dgood.d_teps = bytes; dgood.d_block_off = ints; dgood.nblk = 10; dgood.win = 3; dgood.soft_margin = 0.5;
    dgood.d_rows = floats; dgood.d_order_llr = floats; dgood.d_metric_llr = floats; dgood.d_list_labels = words;
    dgood.d_lri = bytes; dgood.d_uidx = bytes; dgood.d_M = words; dgood.d_deep_limit = ints; dgood.d_cw = words; dgood.d_dl_counts = counts;
    expect(ldpc_dlosd_pipeline_run(nullptr, &dgood, nullptr), LDPC_E_ARG, "ldpc_dlosd_pipeline_run: null argument", "dl ctx");
    expect(ldpc_dlosd_pipeline_run(c96, nullptr, nullptr), LDPC_E_ARG, "ldpc_dlosd_pipeline_run: null argument", "dl p");
    expect(ldpc_dlosd_pipeline_run(c128, &dgood, nullptr), LDPC_E_UNSUPPORTED, "validated: family 1, 4 list rows", "dl AUTO on (128,64)");
    expect(ldpc_dlosd_pipeline_run(c96, &dgood, nullptr), LDPC_E_UNSUPPORTED, "validated: family 2, 4 list rows", "dl AUTO on (96,48)");
    expect(ldpc_dlosd_pipeline_run(c121, &dgood, nullptr), LDPC_E_UNSUPPORTED, "validated: family 3, 4 list rows", "dl AUTO on (121,80)");
    expect(ldpc_dlosd_pipeline_run(c384, &dgood, nullptr), LDPC_E_UNSUPPORTED, "validated: family 4, 4 list rows", "dl AUTO on (384,192)");
    expect(ldpc_dlosd_pipeline_run(c1056, &dgood, nullptr), LDPC_E_UNSUPPORTED,
           "ldpc_dlosd_pipeline_run: long H-form OSD kernels need n <= 384, an H of 1 <= R <= 192 rows, 1 <= n-k <= 192 and 1 <= k <= 192; "
           "this H has 176 rows, n-k = 176, code (1056,880)", "dl AUTO on wimax");
    ldpc_dlosd_pipeline d = dgood;
    d.osd_enable = 0;
    expect(ldpc_dlosd_pipeline_run(c1056, &d, nullptr), LDPC_E_UNSUPPORTED, "validated: family 0, 0 list rows", "dl NMS only on wimax");
    d = dgood; d.family = LDPC_HOSD_FAMILY_128;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_UNSUPPORTED, "H-form OSD kernels need n=128, m=k=64; this code is n=96 m=48 k=48", "dl 128 forced on (96,48)");
    d.family = LDPC_HOSD_FAMILY_X;
    expect(ldpc_dlosd_pipeline_run(c121, &d, nullptr), LDPC_E_UNSUPPORTED,
           "ldpc_dlosd_pipeline_run: H-form OSD kernels need 1 <= k <= 64 and an H of exactly n-k <= 64 rows; this H has 41 rows", "dl X forced on (121,80)");
    d.family = LDPC_HOSD_FAMILY_W;
    expect(ldpc_dlosd_pipeline_run(c384, &d, nullptr), LDPC_E_UNSUPPORTED, "ldpc_dlosd_pipeline_run: wide H-form OSD kernels need n <= 128", "dl W forced on (384,192)");
    d.family = LDPC_HOSD_FAMILY_L;
    expect(ldpc_dlosd_pipeline_run(c128, &d, nullptr), LDPC_E_UNSUPPORTED, "validated: family 4", "dl L forced on (128,64)");
    d.family = 5;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_ARG, "family 5 is no LDPC_HOSD_FAMILY_* value", "dl family 5");
    d = dgood; d.osd_capacity = 3;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_UNSUPPORTED, "validated: family 2, 3 list rows", "dl capacity 3");
    d.osd_capacity = -1;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_ARG, "osd_capacity -1 is negative", "dl capacity -1");
    d = dgood; d.win = 0;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_ARG, "win 0 outside 1..15", "dl win 0");
    d.win = 16;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_ARG, "win 16 outside 1..15", "dl win 16");
    d = dgood; d.nblk = 2;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_ARG, "nblk 2 is below win 3", "dl nblk < win");
    d.nblk = 1025;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_UNSUPPORTED, "nblk 1025 TEP blocks, at most 1024", "dl nblk 1025");
    d = dgood; d.group = -1;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_ARG, "group -1 is negative", "dl group");
    d = dgood; d.n_fcn_weights = 23;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_ARG, "n_fcn_weights 23, a window of 3 takes 24", "dl n_fcn_weights");
    d = dgood; d.n_cnn_weights = 149;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_ARG, "n_cnn_weights 149, T + 1 = 7 rows take 147", "dl n_cnn_weights");
    d = dgood; d.T = 4;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_ARG, "cnn_weights with T 4", "dl T + 1 < 7 with a CNN");
    d.cnn_weights = nullptr; d.d_rows = nullptr; d.d_order_llr = nullptr;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_UNSUPPORTED, "validated: family 2", "dl no CNN: any T, no rows");
    const struct { const char *name; size_t off; } required[] = {
        {"fcn_weights", offsetof(ldpc_dlosd_pipeline, fcn_weights)}, {"d_rows", offsetof(ldpc_dlosd_pipeline, d_rows)},
        {"d_order_llr", offsetof(ldpc_dlosd_pipeline, d_order_llr)}, {"d_index", offsetof(ldpc_dlosd_pipeline, d_index)},
        {"d_count", offsetof(ldpc_dlosd_pipeline, d_count)}, {"d_teps", offsetof(ldpc_dlosd_pipeline, d_teps)},
        {"d_block_off", offsetof(ldpc_dlosd_pipeline, d_block_off)}, {"d_metric_llr", offsetof(ldpc_dlosd_pipeline, d_metric_llr)},
        {"d_lri", offsetof(ldpc_dlosd_pipeline, d_lri)}, {"d_uidx", offsetof(ldpc_dlosd_pipeline, d_uidx)},
        {"d_M", offsetof(ldpc_dlosd_pipeline, d_M)}, {"d_cw", offsetof(ldpc_dlosd_pipeline, d_cw)},
        {"d_list_labels", offsetof(ldpc_dlosd_pipeline, d_list_labels)}, {"d_deep_limit", offsetof(ldpc_dlosd_pipeline, d_deep_limit)}};
    for (const auto &r : required) {
        d = dgood;
        memset((char *)&d + r.off, 0, sizeof(void *));
        char want[96];
        snprintf(want, sizeof(want), "%s%s is NULL", dl, r.name);
        expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_ARG, want, r.name);
    }
    d = dgood; d.d_label_bits = nullptr; d.d_list_labels = nullptr;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_UNSUPPORTED, "validated: family 2", "dl no labels, no list labels");
    d = dgood; d.d_dl_counts = nullptr; d.d_deep_limit = nullptr;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_UNSUPPORTED, "validated: family 2", "dl no stage counters, no deep_limit");
    d = dgood; d.d_hard = nullptr;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_ARG, "ldpc_dlosd_pipeline_run: d_hard and d_fail are required", "dl d_hard");
    d = dgood; d.timing_slot = LDPC_TIMING_SLOTS;
    expect(ldpc_dlosd_pipeline_run(c96, &d, nullptr), LDPC_E_ARG, "ldpc_dlosd_pipeline_run: timing_slot 64", "dl timing_slot 64");
    delete c128;
    delete c121; delete c96; delete c384; delete c1056;
    printf("%s: %d failure(s)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
