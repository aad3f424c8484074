// The DL-OSD stage's bit-wise CNN (conv_bitwise) on gfx950 (MI355X): the forward pass of the test stage (ldpc_dia_cnn)
// and the training step -- loss and gradient with respect to every weight -- of the training stage (ldpc_dia_cnn_grad).
//
// Reference (paths relative to LDPC_128/DL_OSD_Testing_serial/ of the reference):
//   conv_bitwise.build / call          nn_net.py:174-197
//   conv_bitwise.preprocessing_inputs  nn_net.py:198-211
// and, relative to LDPC_128/DL_Training_serial/: calculate_loss nn_training.py:293-297, the tape of :390-398.
//
// The network refines the LLR of every bit from that bit's (T+1)-long NMS trajectory: Conv1D 1->8, 8->4, 4->2 (kernel 3,
// valid, no bias), Flatten, Dense(2(L-6) -> 1) with bias.  The PReLU the model constructs is never applied in `call`.
// One thread per (frame, bit); thread v of a frame reads rows[f][l][v], so a wavefront reads 256 consecutive bytes per
// row.  The three convolutions are streamed along the trajectory with rolling buffers of their last three positions, and
// the dense sum follows them, so nothing is indexed at run time but the weights (kernel arguments, uniform).
//
// Float order (part of the contract; the build passes -ffp-contract=off): every conv output is a sequential f32 sum over
// its flattened (tap, in-channel) index, tap-major, starting from the first product; the dense output is the sequential
// sum over the flattened (position, channel) index, position-major, starting from the first product, then + bias.
//
// The training step.  The network is linear (no activation), out = bias + sum_r E[r] x[r] with an effective filter E of
// the weights alone, so with g = dloss/dout = y - sigmoid(-out) the gradient of the batch loss is the back-propagation
// of the network at the single pseudo-input m[r] = sum_{f,v} g x[r] with upstream gradient 1, and dloss/dbias = sum g.
//   dia_grad_kernel         per (frame, bit): the forward pass above (same device function, same bits), the loss term,
//                           g = y ? sigmoid(out) : -sigmoid(-out), then the row is read again (it is in the cache from the
//                           forward pass; the streamed forward keeps three positions, and L is a run-time value up to 64,
//                           so the row cannot wait in registers) for the L products g x[r] (f32, one rounding each).
//                           A thread adds its products, g and the loss term to its own f64 accumulators in LDS
//                           ([L+2][threads]); a fixed tree over the threads ends the workgroup.  No atomics.
//   dia_grad_finish_kernel  one workgroup: the workgroups' partial sums through a fixed tree (lane b sums workgroups b,
//                           b+64, ... in order, then an xor butterfly), then the network's forward and backward pass at m
//                           in f64, written in the packed order of the weights.
// The shape of both trees depends on (F, n, L) alone: repeated calls give the same bits on any stream.
#include "ldpc_internal.h"
#include "ldpc_wave.h"          // the counted form of dia_cnn_kernel
#include "ldpc_dlosd_check.h"   // kDiaMaxL
#include "ldpc_dlosd_stage.h"   // dia_cnn_counted

namespace ldpc {

constexpr int kDiaMaxWeights = 24 + 96 + 24 + 2 * (kDiaMaxL - 6) + 1;
constexpr int kDiaGradMaxBlocks = 4096;          // grid cap of dia_grad_kernel: a few workgroups per CU, 2 MiB of partials at most
constexpr size_t kDiaGradLdsBudget = 48 * 1024;  // accumulators of one workgroup; the workgroup shrinks until they fit

struct DiaCnnArg {             // Keras layouts: Conv1D kernel [3][in][out], Dense kernel [in][1] + bias [1]
    float w1[3 * 1 * 8];
    float w2[3 * 8 * 4];
    float w3[3 * 4 * 2];
    float wd[2 * (kDiaMaxL - 6)];
    float bias;
};

struct DiaPackedArg {          // the same weights in the packed order of the C ABI (dense kernel of 2(L-6), then the bias)
    float v[kDiaMaxWeights];
};

// out of one (frame, bit): x points at rows[f][0][v], consecutive positions n floats apart
__device__ __forceinline__ float dia_forward(const float *__restrict__ x, int L, int n, const DiaCnnArg &w)
{
    float xa = x[0], xb = x[n];
    float c1[3][8] = {};       // conv1 at positions r-2, r-1, r
    float c2[3][4] = {};       // conv2 at positions q-2, q-1, q (q = r-2)
    float acc = 0.0f;
    for (int r = 0; r + 2 < L; ++r) {
        const float xc = x[(long long)(r + 2) * n];
#pragma unroll
        for (int o = 0; o < 8; ++o) { c1[0][o] = c1[1][o]; c1[1][o] = c1[2][o]; }
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            float s = xa * w.w1[o];
            s = s + xb * w.w1[8 + o];
            s = s + xc * w.w1[16 + o];
            c1[2][o] = s;
        }
        xa = xb; xb = xc;
        if (r < 2) continue;
#pragma unroll
        for (int o = 0; o < 4; ++o) { c2[0][o] = c2[1][o]; c2[1][o] = c2[2][o]; }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float s = c1[0][0] * w.w2[o];
#pragma unroll
            for (int j = 1; j < 24; ++j) s = s + c1[j / 8][j % 8] * w.w2[j * 4 + o];
            c2[2][o] = s;
        }
        if (r < 4) continue;
        const int p = r - 4;   // conv3 position
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            float s = c2[0][0] * w.w3[o];
#pragma unroll
            for (int j = 1; j < 12; ++j) s = s + c2[j / 4][j % 4] * w.w3[j * 2 + o];
            const float t = s * w.wd[2 * p + o];
            acc = (p == 0 && o == 0) ? t : acc + t;
        }
    }
    return acc + w.bias;
}

template <class... COUNT>   // (the counted form: ldpc_wave.h)
__global__ __launch_bounds__(256) void dia_cnn_kernel(const float *__restrict__ rows, long long F, int L, int n,
                                                      DiaCnnArg w, float *__restrict__ out, COUNT... count)
{
    if constexpr (kCounted<COUNT...>) {
        F = counted_frames(F, count...);
        if ((long long)blockIdx.x * 256 >= F * n) return;   // (the grid is sized by the capacity, not by the count)
    }
    const long long total = F * n;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long f = i / n;
        const int v = (int)(i - f * n);
        out[i] = dia_forward(rows + f * L * n + v, L, n, w);
    }
}

// part[blockIdx.x][k], k < L: sum of g x[k]; k = L: sum of g; k = L + 1: sum of the loss terms, over the workgroup's
// elements.  Dynamic LDS: (L + 2) * blockDim.x doubles.
__global__ __launch_bounds__(256) void dia_grad_kernel(const float *__restrict__ rows,
                                                       const unsigned long long *__restrict__ label, long long F, int L,
                                                       int n, DiaCnnArg w, float *__restrict__ out, double *__restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) double acc[];   // [L+2][threads]; a thread owns column tid until the tree
    const int threads = blockDim.x, tid = threadIdx.x, K = L + 2, words = (n + 63) >> 6;
    for (int k = 0; k < K; ++k) acc[k * threads + tid] = 0.0;
    const long long total = F * n;
    for (long long i = (long long)blockIdx.x * threads + tid; i < total; i += (long long)gridDim.x * threads) {
        const long long f = i / n;
        const int v = (int)(i - f * n);
        const float *x = rows + f * L * n + v;
        const float o = dia_forward(x, L, n, w);
        if (out) out[i] = o;
        const bool y = (label[f * words + (v >> 6)] >> (v & 63)) & 1ull;
        // TF's stable sigmoid_cross_entropy_with_logits at logits z = -out
        const float z = -o, yf = y ? 1.0f : 0.0f;
        const float term = (__builtin_fmaxf(z, 0.0f) - z * yf) + log1pf(expf(-__builtin_fabsf(z)));
        // dloss/dout = y - sigmoid(z) = y ? sigmoid(out) : -sigmoid(-out): no cancellation; exp(-q) = inf gives 0
        const float q = y ? o : z;
        const float s = 1.0f / (1.0f + expf(-q));
        const float g = y ? s : -s;
        for (int r = 0; r < L; ++r) acc[r * threads + tid] += (double)(g * x[(long long)r * n]);
        acc[L * threads + tid] += (double)g;
        acc[(L + 1) * threads + tid] += (double)term;
    }
    __syncthreads();
    for (int s = threads >> 1; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < K; ++k) acc[k * threads + tid] += acc[k * threads + tid + s];
        __syncthreads();
    }
    for (int k = tid; k < K; k += threads) part[(long long)blockIdx.x * K + k] = acc[k * threads];
}

// One workgroup of 256.  part [nb][L+2] -> loss_sum[1] (nullable), grad_sum[145 + 2(L-6)] (nullable) in packed order.
__global__ __launch_bounds__(256) void dia_grad_finish_kernel(const double *__restrict__ part, int nb, int L, DiaPackedArg w,
                                                              double *__restrict__ loss_sum, double *__restrict__ grad_sum)
{
    __shared__ double S[kDiaMaxL + 2];                 // m[0..L-1], sum g, sum loss
    __shared__ double W[kDiaMaxWeights];
    __shared__ double c1[(kDiaMaxL - 2) * 8], d1[(kDiaMaxL - 2) * 8];   // conv1 at m, dout/dconv1
    __shared__ double c2[(kDiaMaxL - 4) * 4], d2[(kDiaMaxL - 4) * 4];   // conv2 at m, dout/dconv2
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = L + 2;
    for (int k = wave; k < K; k += 4) {
        double a = 0.0;
        for (int b = lane; b < nb; b += 64) a += part[(long long)b * K + k];
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) S[k] = a;
    }
    const int P1 = L - 2, P2 = L - 4, P3 = L - 6, nw = 145 + 2 * P3;
    for (int i = tid; i < nw; i += 256) W[i] = (double)w.v[i];
    __syncthreads();
    if (tid == 0 && loss_sum) loss_sum[0] = S[L + 1];
    if (!grad_sum) return;
    const double *m = S, *w1 = W, *w2 = W + 24, *w3 = W + 120, *wd = W + 144;
    // conv1 at m; dout/dconv2[q][i] = sum over taps t and channels o of w3[t][i][o] wd[2(q-t)+o]
    for (int idx = tid; idx < P1 * 8; idx += 256) {
        const int p = idx >> 3, o = idx & 7;
        c1[idx] = (m[p] * w1[o] + m[p + 1] * w1[8 + o]) + m[p + 2] * w1[16 + o];
    }
    for (int idx = tid; idx < P2 * 4; idx += 256) {
        const int q = idx >> 2, i = idx & 3;
        double a = 0.0;
        for (int t = 0; t < 3; ++t) {
            const int s = q - t;
            if (s < 0 || s >= P3) continue;
            for (int o = 0; o < 2; ++o) a += w3[(t * 4 + i) * 2 + o] * wd[2 * s + o];
        }
        d2[idx] = a;
    }
    __syncthreads();
    // conv2 at m; dout/dconv1[p][i] = sum over t, o of w2[t][i][o] dconv2[p-t][o]
    for (int idx = tid; idx < P2 * 4; idx += 256) {
        const int q = idx >> 2, o = idx & 3;
        double a = 0.0;
        for (int j = 0; j < 24; ++j) a += c1[(q + j / 8) * 8 + j % 8] * w2[j * 4 + o];
        c2[idx] = a;
    }
    for (int idx = tid; idx < P1 * 8; idx += 256) {
        const int p = idx >> 3, i = idx & 7;
        double a = 0.0;
        for (int t = 0; t < 3; ++t) {
            const int q = p - t;
            if (q < 0 || q >= P2) continue;
            for (int o = 0; o < 4; ++o) a += w2[(t * 8 + i) * 4 + o] * d2[q * 4 + o];
        }
        d1[idx] = a;
    }
    __syncthreads();
    // one packed weight per thread
    for (int idx = tid; idx < nw; idx += 256) {
        double a = 0.0;
        if (idx < 24) {                      // conv1 [t][0][o]
            const int t = idx >> 3, o = idx & 7;
            for (int p = 0; p < P1; ++p) a += m[p + t] * d1[p * 8 + o];
        } else if (idx < 120) {              // conv2 [t][i][o]
            const int j = (idx - 24) >> 2, o = (idx - 24) & 3, t = j >> 3, i = j & 7;
            for (int q = 0; q < P2; ++q) a += c1[(q + t) * 8 + i] * d2[q * 4 + o];
        } else if (idx < 144) {              // conv3 [t][i][o]
            const int j = (idx - 120) >> 1, o = (idx - 120) & 1, t = j >> 2, i = j & 3;
            for (int s = 0; s < P3; ++s) a += c2[(s + t) * 4 + i] * wd[2 * s + o];
        } else if (idx < nw - 1) {           // dense [2s+o]: conv3 at m
            const int s = (idx - 144) >> 1, o = (idx - 144) & 1;
            for (int j = 0; j < 12; ++j) a += c2[(s + j / 4) * 4 + j % 4] * w3[j * 2 + o];
        } else {
            a = S[L];                        // bias
        }
        grad_sum[idx] = a;
    }
}

static DiaCnnArg dia_unpack(const float *weights, int L)
{
    DiaCnnArg w = {};
    const float *p = weights;
    for (int i = 0; i < 24; ++i) w.w1[i] = *p++;
    for (int i = 0; i < 96; ++i) w.w2[i] = *p++;
    for (int i = 0; i < 24; ++i) w.w3[i] = *p++;
    for (int i = 0; i < 2 * (L - 6); ++i) w.wd[i] = *p++;
    w.bias = *p;
    return w;
}

static int launch_dia_cnn(const ldpc_ctx *ctx, const float *d_rows, int64_t F, int L, const DiaCnnArg &w, float *d_out,
                          hipStream_t st)
{
    const int n = ctx->code.n;
    const long long total = F * n, want_blocks = (total + 255) / 256;
    const unsigned grid = (unsigned)(want_blocks < 65536 ? want_blocks : 65536);
    hipLaunchKernelGGL(dia_cnn_kernel<>, dim3(grid), dim3(256), 0, st, d_rows, (long long)F, L, n, w, d_out);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

// ldpc_dia_cnn on min(*d_count, F) trajectories (ldpc_dlosd_pipeline_run, which validated L and the weights); the grid of F
int dia_cnn_counted(const ldpc_ctx *ctx, const float *d_rows, const int32_t *d_count, int64_t F, int L, const float *weights, float *d_out,
                    hipStream_t st)
{
    const int n = ctx->code.n;
    const long long total = F * n, want_blocks = (total + 255) / 256;
    const unsigned grid = (unsigned)(want_blocks < 65536 ? want_blocks : 65536);
    hipLaunchKernelGGL(dia_cnn_kernel<const int *>, dim3(grid), dim3(256), 0, st, d_rows, (long long)F, L, n, dia_unpack(weights, L), d_out,
                       (const int *)d_count);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // namespace ldpc

using namespace ldpc;

extern "C" {

int ldpc_dia_cnn(ldpc_ctx *ctx, const float *d_rows, int64_t F, int32_t L, const float *weights, int32_t n_weights,
                 float *d_out, void *stream)
{
    if (!ctx || F < 0 || L < 7 || L > kDiaMaxL || !weights || (F > 0 && (!d_rows || !d_out)))
        return fail(LDPC_E_ARG, "ldpc_dia_cnn: bad arguments (L = %d: 7 <= L <= %d)", (int)L, kDiaMaxL);
    const int nd = 2 * (L - 6), want = 24 + 96 + 24 + nd + 1;
    if (n_weights != want)
        return fail(LDPC_E_ARG, "ldpc_dia_cnn: %d weights, L = %d takes %d", (int)n_weights, (int)L, want);
    if (F == 0) return LDPC_OK;
    return launch_dia_cnn(ctx, d_rows, F, L, dia_unpack(weights, L), d_out, (hipStream_t)stream);
}

int ldpc_dia_cnn_grad(ldpc_ctx *ctx, const float *d_rows, const uint64_t *d_label_bits, int64_t F, int32_t L,
                      const float *weights, int32_t n_weights, float *d_out, double *d_loss_sum, double *d_grad_sum,
                      void *stream)
{
    static const char who[] = "ldpc_dia_cnn_grad";
    if (!ctx) return fail(LDPC_E_ARG, "%s: ctx is NULL", who);
    if (F < 0) return fail(LDPC_E_ARG, "%s: F = %lld is negative", who, (long long)F);
    if (L < 7 || L > kDiaMaxL) return fail(LDPC_E_ARG, "%s: L = %d outside 7..%d", who, (int)L, kDiaMaxL);
    const int want = 145 + 2 * (L - 6);
    if (n_weights != want) return fail(LDPC_E_ARG, "%s: n_weights = %d, L = %d takes %d", who, (int)n_weights, (int)L, want);
    if (int rc = first_null(who, {{"weights", weights}})) return rc;
    if (F == 0) return LDPC_OK;
    if (int rc = first_null(who, {{"d_rows", d_rows}, {"d_label_bits", d_label_bits}})) return rc;
    if (!d_out && !d_loss_sum && !d_grad_sum) return LDPC_OK;
    const hipStream_t st = (hipStream_t)stream;
    const DiaCnnArg w = dia_unpack(weights, L);
    if (!d_loss_sum && !d_grad_sum) return launch_dia_cnn(ctx, d_rows, F, L, w, d_out, st);
    DiaPackedArg pw = {};
    for (int i = 0; i < want; ++i) pw.v[i] = weights[i];
    // the largest workgroup of 256, 128 or 64 whose f64 accumulators fit the budget (256 up to L = 22, 128 up to L = 46)
    const int K = L + 2, n = ctx->code.n;
    int threads = 256;
    while (threads > 64 && sizeof(double) * (size_t)K * threads > kDiaGradLdsBudget) threads >>= 1;
    const long long total = F * n, want_blocks = (total + threads - 1) / threads;
    const int nb = (int)(want_blocks < kDiaGradMaxBlocks ? want_blocks : kDiaGradMaxBlocks);
    double *part = nullptr;
    LDPC_HIP(hipMallocAsync((void **)&part, sizeof(double) * (size_t)nb * K, st));
    hipLaunchKernelGGL(dia_grad_kernel, dim3((unsigned)nb), dim3(threads), sizeof(double) * (size_t)K * threads, st, d_rows,
                       reinterpret_cast<const unsigned long long *>(d_label_bits), (long long)F, (int)L, n, w, d_out, part);
    hipLaunchKernelGGL(dia_grad_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)part, nb, (int)L, pw, d_loss_sum,
                       d_grad_sum);
    const hipError_t e = hipGetLastError();
    (void)hipFreeAsync(part, st);
    if (e != hipSuccess) return hip_fail(e, "dia_grad_kernel");
    return LDPC_OK;
}

}  // extern "C"
