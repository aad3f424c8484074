// Device code of the generic NMS iteration (any Tanner graph, one frame per wavefront, messages in LDS), shared by
// nms_generic_kernel (ldpc_nms.hip) and nms_train_kernel (ldpc_nms_train.hip).  The float order is the one of
// ldpc_nms.hip's header comment; both kernels reach it only through these functions, so a training forward pass is the
// decoder's, bit for bit.
#pragma once

#include "ldpc_internal.h"

namespace ldpc {

// magnitude of `mag` with the sign bit of `s`: copysign lowers to one v_bfi_b32
__device__ __forceinline__ unsigned sign_insert(unsigned mag, unsigned s)
{
    return __float_as_uint(__builtin_copysignf(__uint_as_float(mag), __uint_as_float(s)));
}

__device__ __forceinline__ void wave_lds_fence()
{
    // one wavefront = one frame: LDS operations of a wave execute in program order, so only
    // the compiler has to be kept from reordering across the phase boundary.
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// sum of the check->variable messages of variable v over its checks, ascending check index
__device__ __forceinline__ float nms_gen_var_sum(const float *cv, const int *var_ptr, const int *var_edge, int v)
{
    float acc = 0.0f;
    for (int q = var_ptr[v]; q < var_ptr[v + 1]; ++q) acc = acc + cv[var_edge[q]];
    return acc;
}

// tot[v] = (sum of cv over the checks of v) + y[v] * w_in (compute_vc, ms_test.py:124-132); lanes sweep variables
__device__ __forceinline__ void nms_gen_totals(const float *cv, float *tot, const float *yb, float w_in, const int *var_ptr,
                                               const int *var_edge, int n, int lane)
{
    for (int v = lane; v < n; v += 64) tot[v] = nms_gen_var_sum(cv, var_ptr, var_edge, v) + yb[v] * w_in;
}

// the posterior of variable v after the check update (marginalize, ms_test.py:220-228)
__device__ __forceinline__ float nms_gen_marginal(const float *cv, const float *yb, float w_out, const int *var_ptr,
                                                  const int *var_edge, int v)
{
    return nms_gen_var_sum(cv, var_ptr, var_edge, v) + w_out * yb[v];
}

// What the backward pass of nms_train_kernel keeps of one check update (the slices of one iteration; ldpc_nms_train.hip):
//   m1[c], m2[c]  |vc| (unclipped) of the edges top_k(k=2) picks on the clipped magnitudes
//   idx[c]        their positions in the check row: bits 0-7 the m1 edge, 8-15 the m2 edge (0xFF: none)
//   sgn[w*m + c]  sign bit of vc of row position 32*w + j at bit j, w < sw
//   tie[w*m + c]  bit j set where |vc| <= m1: the edges that receive m2 (the m1 edge and any edge tied with it)
struct CheckTape {
    float *m1, *m2;
    unsigned *idx, *sgn, *tie;
};

// One check-node update over all checks (compute_cv2, ms_test.py:180-210); lanes sweep checks.  cv holds the previous
// messages on entry and the new ones on return.  TAPE = true also records the check's CheckTape entry.
template <bool TAPE>
__device__ __forceinline__ void nms_gen_checks(float *cv, const float *tot, float a_it, const int *chk_ptr, const int *chk_var,
                                               int m, int lane, CheckTape tp = {})
{
    for (int c = lane; c < m; c += 64) {
        const int e0 = chk_ptr[c], e1 = chk_ptr[c + 1];
        float m1 = __builtin_inff(), m2 = __builtin_inff();
        unsigned sx = 0;
        // tape: the TF tie rule of top_k -- the lower row position first -- on the clipped magnitudes
        float c1 = __builtin_inff(), c2 = __builtin_inff(), r1 = __builtin_inff(), r2 = __builtin_inff();
        int j1 = 0xFF, j2 = 0xFF;
        unsigned s0 = 0, s1 = 0;
        for (int e = e0; e < e1; ++e) {
            float vc = tot[chk_var[e]] - cv[e];
            cv[e] = vc;
            float a = __builtin_fabsf(vc);
            m2 = __builtin_fminf(m2, __builtin_fmaxf(m1, a));
            m1 = __builtin_fminf(m1, a);
            sx ^= __float_as_uint(vc);
            if constexpr (TAPE) {
                const int j = e - e0;
                const float cl = __builtin_fminf(a, 1e30f);
                if (cl < c1) { c2 = c1; r2 = r1; j2 = j1; c1 = cl; r1 = a; j1 = j; }
                else if (cl < c2) { c2 = cl; r2 = a; j2 = j; }
                const unsigned bit = (__float_as_uint(vc) >> 31) << (j & 31);
                if (j < 32) s0 |= bit; else s1 |= bit;
            }
        }
        if constexpr (TAPE) {
            tp.m1[c] = r1;
            tp.m2[c] = r2;
            tp.idx[c] = (unsigned)j1 | ((unsigned)j2 << 8);
            tp.sgn[c] = s0;
            if (e1 - e0 > 32) tp.sgn[m + c] = s1;
        }
        // clamping the order statistics == clamping every |vc| (monotone); a zero
        // minimum means sign(0) = 0 wipes the whole check row (ms_test.py:187-191)
        const float m1s = a_it * __builtin_fminf(m1, 1e30f);
        const float m2s = (m1 == 0.0f) ? 0.0f : a_it * __builtin_fminf(m2, 1e30f);
        unsigned t0 = 0, t1 = 0;
        for (int e = e0; e < e1; ++e) {
            float vc = cv[e];
            const bool gets_m1 = __builtin_fabsf(vc) > m1;
            float mag = gets_m1 ? m1s : m2s;
            cv[e] = __uint_as_float(sign_insert(__float_as_uint(mag), sx ^ __float_as_uint(vc)));
            if constexpr (TAPE) {
                const int j = e - e0;
                const unsigned bit = (unsigned)!gets_m1 << (j & 31);
                if (j < 32) t0 |= bit; else t1 |= bit;
            }
        }
        if constexpr (TAPE) {
            tp.tie[c] = t0;
            if (e1 - e0 > 32) tp.tie[m + c] = t1;
        }
    }
}

}  // namespace ldpc
