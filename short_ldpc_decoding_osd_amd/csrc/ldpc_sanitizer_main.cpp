// Sanitizer build only (python -m short_ldpc_decoding_osd_amd.build --asan --run): a stand-alone program that drives the
// host-side validation of ldpc_osd_merge and ldpc_family_pipeline_run (ldpc_sanitizer_checks.cpp over ldpc_family_check.h) under
// -fsanitize=address,undefined.  No device: the contexts are made by hand, with the shape of a code and the k of each family's
// tables as ldpc_ctx_create would leave them, and every pointer is a host address that nothing dereferences.  A call that
// passes validation ends in the stub's "exists only in the HIP build".  Exit status 0 when every expectation holds.
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
    delete c121; delete c96; delete c384; delete c1056;
    printf("%s: %d failure(s)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
