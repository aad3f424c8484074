// NMS training: the loss of Decoding_model and its gradient with respect to the effective normalisation factors, forward
// and backward in one launch (ldpc_nms_train_grad, include/ldpc_osd.h).
//
// Reference math (paths relative to LDPC_128/ of the reference): Ldpc_128_training/ms_decoder_dense.py
//   Decoder_Layer.build :74-91, compute_vc :121-134, compute_cv2 :177-208, marginalize :217-226,
//   calculation_loss :210-215, the unrolled loop :102-119 and :232-241.
//   L = sum_{t=1..T} sum_{frame, v} sigmoid_cross_entropy(logits = -soft_t[v], labels = bit[v])
//
// Forward: nms_gen_totals / nms_gen_checks / nms_gen_marginal of ldpc_nms_generic.h, the device code of
// nms_generic_kernel, in the same order -- every posterior is the decoder's, bit for bit.  Each iteration t also writes a
// tape to LDS:
//   per check  CheckTape: |vc| of the m1 and m2 edges, their row positions, the sign bits of vc, the edges that
//              received m2                                                                       (12 + 8 sw B)
//   per variable  dL/dsoft_t[v] = bit[v] - sigmoid(-soft_t[v]), from the forward's own soft_t    (4 B)
// and the backward pass sweeps t = T..1 over the tape, the gradient of cv in the message array, without leaving LDS.
//
// Gradient rules: those of TensorFlow for the ops the reference uses (parity unpinned: TensorFlow is not available to
// check them).
//   signs      result_sign_matrix is under tf.stop_gradient: nothing flows through signs.  S = 0 (a zero vc in the
//              check, equivalently m1 = 0) makes every message of the check 0: nothing flows into its magnitudes or
//              into alpha_t.
//   |vc|       derivative sign(vc), 0 at 0; clip_by_value(., 0, 1e30) passes where 0 <= x <= 1e30.
//   top_k      the gradient of m1 goes to the first edge top_k(k=2) picks on -clip(|vc|), that of m2 to the second;
//              ties go to the lower row position (= lower variable index) first.  An edge with |vc| > m1 receives m1,
//              so its gradient goes to the m1 edge; the m1 edge itself (and any edge tied with it) receives m2, so its
//              gradient goes to the m2 edge.  The tape keeps that split as a bit mask (ties do not change a forward
//              value, but they do route the gradient).
//   vc         vc = tot[var] - cv_prev, tot = sum cv_prev + w_in y:
//              dL/dcv_prev[e] = dL/dtot[var(e)] - dL/dvc[e],  dL/dtot[v] = sum_{e in v} dL/dvc[e].
//   loss       dL/dsoft_t[v] = bit[v] - sigmoid(-soft_t[v]); the value is TF's stable
//              max(x, 0) - x z + log1p(exp(-|x|)), x = -soft_t[v].
// No gradient with respect to the channel values.
//
// Per-frame outputs loss[f] and grad[f][T+2] = {dL/dalpha_0..T-1, dL/dw_in, dL/dw_out}: every lane sums its own
// variables / checks in a fixed order, then a fixed xor-butterfly over the wave; a frame's values do not depend on the
// batch, the grid or the stream.  nms_colsum_kernel reduces them over frames into f64 with a tree whose shape depends on
// B alone (no atomics).
#include <algorithm>

#include "ldpc_nms_generic.h"

namespace ldpc {

constexpr size_t kTrainLdsBudget = LDPC_NMS_TRAIN_LDS_BUDGET;   // per frame (= per wavefront), bytes

__device__ __forceinline__ float wave_sum_lane0(float x)
{
    for (int o = 32; o > 0; o >>= 1) x = x + __shfl_xor(x, o);
    return x;   // every lane holds a sum; lane 0's is the one used
}

// words of LDS one frame needs: messages + totals + channel values, then T tape slices
__host__ __device__ inline size_t train_slice_words(int n, int m, int sw) { return (size_t)n + (size_t)m * (3 + 2 * sw); }
__host__ __device__ inline size_t train_frame_words(int n, int m, int E, int sw, int T)
{
    return (size_t)E + 2 * (size_t)n + (size_t)T * train_slice_words(n, m, sw);
}

__global__ __launch_bounds__(256) void nms_train_kernel(
    const float *__restrict__ llr, const unsigned long long *__restrict__ label, long long B, int T, AlphaArg alpha,
    float w_in, float w_out, float *__restrict__ loss, float *__restrict__ grad, float *__restrict__ traj,
    unsigned long long *__restrict__ hard, unsigned char *__restrict__ fail, const int *__restrict__ chk_ptr,
    const int *__restrict__ chk_var, const int *__restrict__ var_ptr, const int *__restrict__ var_edge, int n, int m,
    int E, int sw)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    float *cv = smem + (size_t)wave * train_frame_words(n, m, E, sw, T);
    float *tot = cv + E;
    float *yb = tot + n;
    float *tape = yb + n;                  // slice t: gsoft[n], m1[m], m2[m], idx[m], sgn[sw*m], tie[sw*m]
    const size_t slice = train_slice_words(n, m, sw);
    const int words = (n + 63) >> 6;

    for (long long f = (long long)blockIdx.x * waves + wave; f < B; f += (long long)gridDim.x * waves) {
        const unsigned long long *lab = label + f * words;
        for (int v = lane; v < n; v += 64) {
            float y = llr[f * n + v];
            yb[v] = y;
            tot[v] = y;  // T == 0: the posterior is the channel value
        }
        for (int e = lane; e < E; e += 64) cv[e] = 0.0f;
        wave_lds_fence();
        // ---------------------------------------------------------------- forward + tape
        float lsum = 0.0f;
        for (int it = 0; it < T; ++it) {
            float *sl = tape + (size_t)it * slice;
            CheckTape tp{sl + n, sl + n + m, reinterpret_cast<unsigned *>(sl + n + 2 * m), reinterpret_cast<unsigned *>(sl + n + 3 * m),
                         reinterpret_cast<unsigned *>(sl + n + (3 + sw) * m)};
            nms_gen_totals(cv, tot, yb, w_in, var_ptr, var_edge, n, lane);
            wave_lds_fence();
            nms_gen_checks<true>(cv, tot, alpha.a[it], chk_ptr, chk_var, m, lane, tp);
            wave_lds_fence();
            for (int v = lane; v < n; v += 64) {
                const float o = nms_gen_marginal(cv, yb, w_out, var_ptr, var_edge, v);
                if (traj) traj[((long long)it * B + f) * n + v] = o;
                if (it == T - 1) tot[v] = o;
                const float z = (float)((lab[v >> 6] >> (v & 63)) & 1ull);
                const float x = -o;
                lsum = lsum + ((__builtin_fmaxf(x, 0.0f) - x * z) + log1pf(expf(-__builtin_fabsf(x))));
                // dL/dsoft = z - sigmoid(x) = (z ? sigmoid(o) : -sigmoid(x)): no cancellation when z = 1 and x << 0.
                // sigmoid(q) = 1 / (1 + exp(-q)) for q >= 0, exp(q) / (1 + exp(q)) below: no overflow either way
                const float q = (z != 0.0f) ? o : x;
                const float ex = expf(-__builtin_fabsf(q));
                const float sig = (q >= 0.0f) ? 1.0f / (1.0f + ex) : ex / (1.0f + ex);
                sl[v] = (z != 0.0f) ? sig : -sig;
            }
            wave_lds_fence();
        }
        // outputs of the decoder: packed hard decision (soft > 0 ? 0 : 1), syndrome flag
        if (hard)
            for (int w = 0; w < words; ++w) {
                int v = w * 64 + lane;
                unsigned long long bits = __ballot(v < n && !(tot[v] > 0.0f));
                if (lane == 0) hard[f * words + w] = bits;
            }
        if (fail) {
            int bad = 0;
            for (int c = lane; c < m; c += 64) {
                int par = 0;
                for (int e = chk_ptr[c]; e < chk_ptr[c + 1]; ++e) par ^= !(tot[chk_var[e]] > 0.0f);
                bad |= par;
            }
            unsigned long long anybad = __ballot(bad);
            if (lane == 0) fail[f] = anybad != 0;
        }
        lsum = wave_sum_lane0(lsum);
        if (loss && lane == 0) loss[f] = lsum;
        if (!grad) { wave_lds_fence(); continue; }
        // ---------------------------------------------------------------- backward, t = T .. 1
        // cv becomes g = dL/dcv_t, tot becomes dL/dtot_t
        wave_lds_fence();
        for (int e = lane; e < E; e += 64) cv[e] = 0.0f;
        wave_lds_fence();
        float gwin = 0.0f, gwout = 0.0f;
        for (int it = T - 1; it >= 0; --it) {
            const float *sl = tape + (size_t)it * slice;
            const float *t_m1 = sl + n, *t_m2 = sl + n + m;
            const unsigned *t_idx = reinterpret_cast<const unsigned *>(sl + n + 2 * m);
            const unsigned *t_sgn = reinterpret_cast<const unsigned *>(sl + n + 3 * m);
            const unsigned *t_tie = reinterpret_cast<const unsigned *>(sl + n + (3 + sw) * m);
            const float a_it = alpha.a[it];
            // marginalize: soft_t[v] = sum cv_t + w_out y
            for (int v = lane; v < n; v += 64) {
                const float gs = sl[v];
                for (int q = var_ptr[v]; q < var_ptr[v + 1]; ++q) cv[var_edge[q]] = cv[var_edge[q]] + gs;
                gwout = gwout + gs * yb[v];
            }
            wave_lds_fence();
            // compute_cv2: cv_t[e] = alpha_t * mag[e] * S * sign(vc_e); the gradient of vc is left in cv (0 off the two
            // argmin edges)
            float galpha = 0.0f;
            for (int c = lane; c < m; c += 64) {
                const int e0 = chk_ptr[c], e1 = chk_ptr[c + 1];
                const float r1 = t_m1[c], r2 = t_m2[c];
                const unsigned ix = t_idx[c];
                const int j1 = ix & 0xFF, j2 = (ix >> 8) & 0xFF;
                const unsigned s0 = t_sgn[c], s1 = (e1 - e0 > 32) ? t_sgn[m + c] : 0u;
                const unsigned q0 = t_tie[c], q1 = (e1 - e0 > 32) ? t_tie[m + c] : 0u;
                if (!(r1 != 0.0f) || j1 == 0xFF) {          // S = 0: the row's messages are constants
                    for (int e = e0; e < e1; ++e) cv[e] = 0.0f;
                    continue;
                }
                const unsigned par = (__builtin_popcount(s0) ^ __builtin_popcount(s1)) & 1u;
                float g1 = 0.0f, g2 = 0.0f;     // sum of g * S * sign(vc) over the edges that received m1 / m2
                for (int e = e0; e < e1; ++e) {
                    const int j = e - e0;
                    const unsigned sb = ((j < 32 ? s0 >> j : s1 >> (j - 32)) & 1u) ^ par;
                    const float g = sb ? -cv[e] : cv[e];
                    if ((j < 32 ? q0 >> j : q1 >> (j - 32)) & 1u) g2 = g2 + g;
                    else g1 = g1 + g;
                    cv[e] = 0.0f;
                }
                const float m1c = __builtin_fminf(r1, 1e30f), m2c = __builtin_fminf(r2, 1e30f);
                galpha = galpha + (m1c * g1 + m2c * g2);
                const float gm1 = a_it * g1, gm2 = a_it * g2;
                // d|vc|/dvc = sign(vc) (vc != 0 here: |vc| >= m1 > 0); the clip passes where |vc| <= 1e30
                const unsigned b1 = (j1 < 32 ? s0 >> j1 : s1 >> (j1 - 32)) & 1u;
                if (r1 <= 1e30f) cv[e0 + j1] = b1 ? -gm1 : gm1;
                if (j2 != 0xFF && r2 <= 1e30f) {
                    const unsigned b2 = (j2 < 32 ? s0 >> j2 : s1 >> (j2 - 32)) & 1u;
                    cv[e0 + j2] = b2 ? -gm2 : gm2;
                }
            }
            galpha = wave_sum_lane0(galpha);
            if (lane == 0) grad[f * (T + 2) + it] = galpha;
            wave_lds_fence();
            // compute_vc: tot = sum cv_prev + w_in y, vc = tot[var] - cv_prev
            for (int v = lane; v < n; v += 64) {
                const float gt = nms_gen_var_sum(cv, var_ptr, var_edge, v);
                tot[v] = gt;
                gwin = gwin + gt * yb[v];
            }
            wave_lds_fence();
            if (it > 0) {
                for (int e = lane; e < E; e += 64) cv[e] = tot[chk_var[e]] - cv[e];
                wave_lds_fence();
            }
        }
        gwin = wave_sum_lane0(gwin);
        gwout = wave_sum_lane0(gwout);
        if (lane == 0) {
            grad[f * (T + 2) + T] = gwin;
            grad[f * (T + 2) + T + 1] = gwout;
        }
        wave_lds_fence();
    }
}

// out[blockIdx.x * K + k] = sum of src[r * K + k] over the rows r of block blockIdx.x (rows_per_block of them), in f64.
// Thread i sums rows i, i + 256, ... of the block in order; then a fixed binary tree over the 256 partial sums.  The
// shape depends on (rows, rows_per_block) alone.
template <typename TIn>
__global__ __launch_bounds__(256) void nms_colsum_kernel(const TIn *__restrict__ src, long long rows, int K,
                                                         long long rows_per_block, double *__restrict__ out)
{
    __shared__ double part[256];
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    for (int k = 0; k < K; ++k) {
        double acc = 0.0;
        for (long long r = r0 + threadIdx.x; r < r1; r += 256) acc += (double)src[r * K + k];
        part[threadIdx.x] = acc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[(long long)blockIdx.x * K + k] = part[0];
        __syncthreads();
    }
}

// columns of a [rows][K] matrix -> d_sum[K] (f64): blocks of kRowsPerBlock rows, then one block over their sums
static int column_sums(const float *src, long long rows, int K, double *d_sum, hipStream_t st)
{
    constexpr long long kRowsPerBlock = 4096;
    const long long nb = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
    double *part = nullptr;
    LDPC_HIP(hipMallocAsync((void **)&part, sizeof(double) * (size_t)(nb * K), st));
    hipLaunchKernelGGL(nms_colsum_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st, src, rows, K, kRowsPerBlock, part);
    hipLaunchKernelGGL(nms_colsum_kernel<double>, dim3(1), dim3(256), 0, st, (const double *)part, nb, K, nb, d_sum);
    const hipError_t e = hipGetLastError();
    (void)hipFreeAsync(part, st);
    if (e != hipSuccess) return hip_fail(e, "nms column sums");
    return LDPC_OK;
}

int train_lds_bytes(const ldpc_code &c, int T)
{
    const int sw = (c.max_chk_degree + 31) / 32;
    return (int)(sizeof(float) * train_frame_words(c.n, c.m, c.E, sw < 1 ? 1 : sw, T));
}

int launch_nms_train(ldpc_ctx *ctx, const float *d_llr, const uint64_t *d_label, int64_t B, int T, const float *alpha,
                     float w_in, float w_out, float *d_loss, float *d_grad, double *d_loss_sum, double *d_grad_sum,
                     float *d_traj, uint64_t *d_hard, uint8_t *d_fail, hipStream_t st)
{
    const ldpc_code &c = ctx->code;
    int maxdeg = 0;
    for (int r = 0; r < c.m; ++r) maxdeg = std::max(maxdeg, c.chk_ptr[r + 1] - c.chk_ptr[r]);
    if (maxdeg > 64) return fail(LDPC_E_UNSUPPORTED, "ldpc_nms_train_grad: check degree %d above 64", maxdeg);
    const int sw = maxdeg > 32 ? 2 : 1;
    const size_t per_frame = sizeof(float) * train_frame_words(c.n, c.m, c.E, sw, T);
    if (per_frame > kTrainLdsBudget)
        return fail(LDPC_E_UNSUPPORTED, "ldpc_nms_train_grad: the tape of one frame needs %zu B of LDS at T=%d (budget %zu B)",
                    per_frame, T, kTrainLdsBudget);
    AlphaArg a;
    for (int i = 0; i < kMaxIters; ++i) a.a[i] = i < T ? alpha[i] : 0.0f;
    // wavefronts (= frames) per workgroup: as many as fit 64 KiB, so that several workgroups share a CU; a frame beyond
    // 64 KiB runs alone in its workgroup, opted in to the CU's 160 KiB
    int waves = (int)((64 * 1024) / per_frame);
    waves = waves < 1 ? 1 : (waves > 4 ? 4 : waves);
    const size_t lds = per_frame * waves;
    if (lds > 64 * 1024) {
        static thread_local size_t granted = 0;
        if (lds > granted) {
            LDPC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(nms_train_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)lds));
            granted = lds;
        }
    }
    // per-frame loss / gradient are the input of the batch sums: scratch when the caller does not keep them
    float *loss = d_loss, *grad = d_grad;
    if (!loss && d_loss_sum) LDPC_HIP(hipMallocAsync((void **)&loss, sizeof(float) * (size_t)B, st));
    if (!grad && d_grad_sum) LDPC_HIP(hipMallocAsync((void **)&grad, sizeof(float) * (size_t)B * (T + 2), st));
    const long long want = (B + waves - 1) / waves;
    const long long cap = 32768 / waves;
    hipLaunchKernelGGL(nms_train_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(64 * waves), lds, st, d_llr,
                       reinterpret_cast<const unsigned long long *>(d_label), (long long)B, T, a, w_in, w_out, loss, grad, d_traj,
                       reinterpret_cast<unsigned long long *>(d_hard), d_fail, ctx->d_chk_ptr, ctx->d_chk_var, ctx->d_var_ptr,
                       ctx->d_var_edge, c.n, c.m, c.E, sw);
    const hipError_t e = hipGetLastError();
    int rc = e == hipSuccess ? LDPC_OK : hip_fail(e, "nms_train_kernel");
    if (rc == LDPC_OK && d_loss_sum) rc = column_sums(loss, B, 1, d_loss_sum, st);
    if (rc == LDPC_OK && d_grad_sum) rc = column_sums(grad, B, T + 2, d_grad_sum, st);
    if (loss != d_loss) (void)hipFreeAsync(loss, st);
    if (grad != d_grad) (void)hipFreeAsync(grad, st);
    return rc;
}

}  // namespace ldpc
