// The DL-OSD stage's bit-wise CNN (conv_bitwise) on gfx950 (MI355X).
//
// Reference (paths relative to LDPC_128/DL_OSD_Testing_serial/ of the reference):
//   conv_bitwise.build / call          nn_net.py:174-197
//   conv_bitwise.preprocessing_inputs  nn_net.py:198-211
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
#include "ldpc_internal.h"

namespace ldpc {

constexpr int kDiaMaxL = 64;   // longest trajectory (T + 1) the weight block in the kernel arguments holds

struct DiaCnnArg {             // Keras layouts: Conv1D kernel [3][in][out], Dense kernel [in][1] + bias [1]
    float w1[3 * 1 * 8];
    float w2[3 * 8 * 4];
    float w3[3 * 4 * 2];
    float wd[2 * (kDiaMaxL - 6)];
    float bias;
};

__global__ __launch_bounds__(256) void dia_cnn_kernel(const float *__restrict__ rows, long long F, int L, int n,
                                                      DiaCnnArg w, float *__restrict__ out)
{
    const long long total = F * n;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long f = i / n;
        const int v = (int)(i - f * n);
        const float *x = rows + f * L * n + v;
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
        out[i] = acc + w.bias;
    }
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
    DiaCnnArg w = {};
    const float *p = weights;
    for (int i = 0; i < 24; ++i) w.w1[i] = *p++;
    for (int i = 0; i < 96; ++i) w.w2[i] = *p++;
    for (int i = 0; i < 24; ++i) w.w3[i] = *p++;
    for (int i = 0; i < nd; ++i) w.wd[i] = *p++;
    w.bias = *p;
    const int n = ctx->code.n;
    const long long total = F * n, want_blocks = (total + 255) / 256;
    const unsigned grid = (unsigned)(want_blocks < 65536 ? want_blocks : 65536);
    hipLaunchKernelGGL(dia_cnn_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_rows, (long long)F, (int)L, n, w, d_out);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // extern "C"
