// Sanitizer build only (python -m short_ldpc_decoding_osd_amd.build --asan), beside ldpc_sanitizer_stubs.cpp: the three entry
// points whose whole host side is validation that needs no kernel (ldpc_family_check.h and ldpc_dlosd_check.h, the text the HIP
// build compiles too).
// They run it and then fail like the other stubs, so the refusals -- texts, order, what is checked before a launch -- are
// exercised under -fsanitize=address,undefined: by ldpc_sanitizer_main.cpp, a stand-alone program on contexts made by hand.
#include "ldpc_family_check.h"
#include "ldpc_dlosd_check.h"

extern "C" int ldpc_dlosd_pipeline_run(ldpc_ctx *ctx, const ldpc_dlosd_pipeline *p, void *)
{
    int family;
    int64_t F;
    if (int rc = ldpc::dlosd_pipeline_check(ctx, p, "ldpc_dlosd_pipeline_run", &family, &F)) return rc;
    return ldpc::fail(LDPC_E_UNSUPPORTED, "sanitizer build: ldpc_dlosd_pipeline_run exists only in the HIP build (validated: family %d, %lld list rows)",
                      family, (long long)F);
}

extern "C" int ldpc_osd_merge(ldpc_ctx *ctx, const uint64_t *d_cw, const int32_t *d_index, const int32_t *d_count, int64_t F, uint64_t *d_hard,
                              const uint64_t *d_label_bits, int64_t *d_counts, void *)
{
    bool launch;
    if (int rc = ldpc::osd_merge_check(ctx, d_cw, d_index, d_count, F, d_hard, d_label_bits, d_counts, &launch)) return rc;
    return launch ? ldpc::fail(LDPC_E_UNSUPPORTED, "sanitizer build: ldpc_osd_merge exists only in the HIP build") : LDPC_OK;
}

extern "C" int ldpc_family_pipeline_run(ldpc_ctx *ctx, const ldpc_family_pipeline *p, void *)
{
    int family;
    int64_t F;
    if (int rc = ldpc::family_pipeline_check(ctx, p, "ldpc_family_pipeline_run", &family, &F)) return rc;
    return ldpc::fail(LDPC_E_UNSUPPORTED, "sanitizer build: ldpc_family_pipeline_run exists only in the HIP build (validated: family %d, %lld OSD frames)",
                      family, (long long)F);
}
