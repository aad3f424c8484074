// Training of the sliding-window early-stop classifier (Predict_outlier_light) on gfx950: the window builder
// (ldpc_fcn_windows) and the loss / gradient of one batch of windows (ldpc_fcn_grad).  Included from ldpc_hosd.hip after
// the scan kernels, whose SlideFcnArg, kSlideMaxWin and kHosdMaxBlocks it shares.
//
// Reference (paths relative to LDPC_128/DL_Training_serial/ of the reference):
//   reform_inputs                      interval_boundary.py:224-249
//   shuffle_data / calculation_loss    predict_phase.py:104-135, the tape of :203-212, the validation of :236-260
//
// Windows.  One thread per output row (window position i, record r), row i*R + r: the window is read into registers, put in
// ascending order by a fixed network of compare-exchanges (the width is a template parameter, so nothing is indexed at run
// time), and its label is (min(window) == min(record)) && success.  The record minima come from a first kernel, one thread
// per record, through scratch that is allocated and freed in stream order.  Every operation is exact.
//
// Loss and gradient.  One window per thread (grid-stride), weights by value in the kernel arguments.  The forward pass
// restates slide_p1's float order per thread: h = x.W1 and z = h.W2, each a sequential f32 sum from the first product,
// m = max(z), e_c = expf(z_c - m), p_c = e_c / (e0 + e1).  The network is linear up to the softmax, so a thread keeps only
// the moments m[i][c] = sum x_i g_c (2(win+1) doubles), its loss, the two accuracy sums and three counts; a wave butterfly
// and a fixed sum over the waves end the workgroup, and a one-workgroup finish kernel sums the workgroups' partials by a
// fixed tree (lane b sums workgroups b, b+64, ... in order, then an xor butterfly) and back-propagates in f64:
//   dW1[i][j] = sum_c m[i][c] W2[j][c],   dW2[j][c] = sum_i W1[i][j] m[i][c]   (ascending index).
// No float atomics; the shape of both trees depends on (B, win) alone.
#pragma once

namespace ldpc {

constexpr int kFcnGradMaxBlocks = 256;    // grid cap of fcn_grad_kernel: a workgroup per CU; beyond 65 536 windows a thread takes several

// record minima: rowmin[r] = min over the nblk entries of record r (sequential from the first entry, `<` keeps the first)
__global__ __launch_bounds__(256) void fcn_rowmin_kernel(const float *__restrict__ block_min, const int *__restrict__ index,
                                                         long long R, int nblk, float *__restrict__ rowmin)
{
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < R; r += (long long)gridDim.x * 256) {
        const float *row = block_min + (index ? (long long)index[r] : r) * nblk;
        float m = row[0];
        for (int b = 1; b < nblk; ++b) m = row[b] < m ? row[b] : m;
        rowmin[r] = m;
    }
}

template <int WIN>
__global__ __launch_bounds__(256) void fcn_windows_kernel(const float *__restrict__ block_min,
                                                          const unsigned char *__restrict__ success,
                                                          const int *__restrict__ index, const float *__restrict__ rowmin,
                                                          long long R, int nblk, float *__restrict__ inputs,
                                                          unsigned char *__restrict__ labels,
                                                          unsigned long long *__restrict__ class_count)
{
    __shared__ unsigned long long ones_s, rows_s;
    if (threadIdx.x == 0) ones_s = rows_s = 0;
    __syncthreads();
    const long long total = (long long)(nblk - WIN + 1) * R;
    unsigned my_ones = 0, my_rows = 0;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long long)gridDim.x * 256) {
        const long long i = o / R, r = o - i * R;
        const long long f = index ? (long long)index[r] : r;
        const float *src = block_min + f * nblk + i;
        float a[WIN];
#pragma unroll
        for (int j = 0; j < WIN; ++j) a[j] = src[j];
#pragma unroll
        for (int e = 1; e < WIN; ++e)            // insertion by adjacent compare-exchanges: fixed indices, exact
#pragma unroll
            for (int j = e; j > 0; --j) {
                const float lo = a[j] < a[j - 1] ? a[j] : a[j - 1], hi = a[j] < a[j - 1] ? a[j - 1] : a[j];
                a[j - 1] = lo;
                a[j] = hi;
            }
        float *dst = inputs + o * (WIN + 1);
#pragma unroll
        for (int j = 0; j < WIN; ++j) dst[j] = a[j];
        dst[WIN] = (float)i;
        const unsigned char y = (a[0] == rowmin[r] && success[f]) ? 1 : 0;
        labels[o] = y;
        my_ones += y;
        ++my_rows;
    }
    if (!class_count) return;
    atomicAdd(&ones_s, (unsigned long long)my_ones);
    atomicAdd(&rows_s, (unsigned long long)my_rows);
    __syncthreads();
    if (threadIdx.x == 0 && rows_s) {
        atomicAdd(&class_count[0], rows_s - ones_s);
        atomicAdd(&class_count[1], ones_s);
    }
}

__device__ __forceinline__ double fcn_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ long long fcn_wave_sum(long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// D = win + 1 inputs.  part [gridDim.x][2D + 3]: m[i][c] at 2i + c, then the loss, sum sw [pred == y], sum sw;
// cnt [gridDim.x][3]: #[y == pred], #[y > pred], #[y < pred].  Both NULL: the forward pass alone (p_out).
template <int D>
__global__ __launch_bounds__(256) void fcn_grad_kernel(const float *__restrict__ inputs, const unsigned char *__restrict__ labels,
                                                       const float *__restrict__ weight, const int *__restrict__ index,
                                                       long long B, SlideFcnArg w, float penalty, float *__restrict__ p_out,
                                                       double *__restrict__ part, long long *__restrict__ cnt)
{
    constexpr int K = 2 * D + 3;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    long long n_eq = 0, n_gt = 0, n_lt = 0;
    for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < B; b += (long long)gridDim.x * 256) {
        const long long row = index ? (long long)index[b] : b;
        const float *src = inputs + row * D;
        float x[D], h[D];
#pragma unroll
        for (int i = 0; i < D; ++i) x[i] = src[i];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            float s = x[0] * w.w1[j];
#pragma unroll
            for (int i = 1; i < D; ++i) s = s + x[i] * w.w1[i * D + j];
            h[j] = s;
        }
        float z0 = h[0] * w.w2[0], z1 = h[0] * w.w2[1];
#pragma unroll
        for (int j = 1; j < D; ++j) {
            z0 = z0 + h[j] * w.w2[2 * j];
            z1 = z1 + h[j] * w.w2[2 * j + 1];
        }
        const float m = z1 > z0 ? z1 : z0;
        const float e0 = expf(z0 - m), e1 = expf(z1 - m);
        const float p0 = e0 / (e0 + e1), p1 = e1 / (e0 + e1);
        if (p_out) {
            p_out[2 * b] = p0;
            p_out[2 * b + 1] = p1;
        }
        if (!part) continue;
        const int y = labels[row] ? 1 : 0, pred = p0 < p1 ? 1 : 0;
        const double sw = weight ? (double)weight[row] : 1.0;
        const double s = sw * ((pred && !y) ? (double)penalty : 1.0);
        const float py = y ? p1 : p0;
        const bool live = py >= 1e-30f;
        const double g0 = live ? s * ((double)p0 - (y ? 0.0 : 1.0)) : 0.0;
        const double g1 = live ? s * ((double)p1 - (y ? 1.0 : 0.0)) : 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            acc[2 * i] += (double)x[i] * g0;
            acc[2 * i + 1] += (double)x[i] * g1;
        }
        acc[2 * D] += -s * log((double)__builtin_fmaxf(py, 1e-30f));
        acc[2 * D + 1] += pred == y ? sw : 0.0;
        acc[2 * D + 2] += sw;
        n_eq += y == pred;
        n_gt += y > pred;
        n_lt += y < pred;
    }
    if (!part) return;
    __shared__ double wsum[4][K];
    __shared__ long long wcnt[4][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = fcn_wave_sum(acc[k]);
        if (lane == 0) wsum[wave][k] = v;
    }
    n_eq = fcn_wave_sum(n_eq);
    n_gt = fcn_wave_sum(n_gt);
    n_lt = fcn_wave_sum(n_lt);
    if (lane == 0) {
        wcnt[wave][0] = n_eq;
        wcnt[wave][1] = n_gt;
        wcnt[wave][2] = n_lt;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256)
        part[(long long)blockIdx.x * K + k] = ((wsum[0][k] + wsum[1][k]) + wsum[2][k]) + wsum[3][k];
    if (threadIdx.x < 3)
        cnt[(long long)blockIdx.x * 3 + threadIdx.x] =
            ((wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x]) + wcnt[2][threadIdx.x]) + wcnt[3][threadIdx.x];
}

// One workgroup of 256.  part [nb][2D + 3], cnt [nb][3] -> the nullable outputs of ldpc_fcn_grad.
__global__ __launch_bounds__(256) void fcn_grad_finish_kernel(const double *__restrict__ part, const long long *__restrict__ cnt,
                                                              int nb, int D, SlideFcnArg w, double *__restrict__ loss_sum,
                                                              double *__restrict__ grad_sum, double *__restrict__ acc_out,
                                                              long long *__restrict__ counts)
{
    __shared__ double S[2 * (kSlideMaxWin + 1) + 3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = 2 * D + 3;
    for (int k = wave; k < K; k += 4) {
        double a = 0.0;
        for (int b = lane; b < nb; b += 64) a += part[(long long)b * K + k];
        a = fcn_wave_sum(a);
        if (lane == 0) S[k] = a;
    }
    if (counts && wave == 3) {
        for (int k = 0; k < 3; ++k) {
            long long a = 0;
            for (int b = lane; b < nb; b += 64) a += cnt[(long long)b * 3 + k];
            a = fcn_wave_sum(a);
            if (lane == 0) counts[k] = a;
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (loss_sum) loss_sum[0] = S[2 * D];
        if (acc_out) {
            acc_out[0] = S[2 * D + 1];
            acc_out[1] = S[2 * D + 2];
        }
    }
    if (!grad_sum) return;
    for (int idx = tid; idx < D * D + 2 * D; idx += 256) {
        double a;
        if (idx < D * D) {                           // dW1[i][j]
            const int i = idx / D, j = idx - i * D;
            a = S[2 * i] * (double)w.w2[2 * j] + S[2 * i + 1] * (double)w.w2[2 * j + 1];
        } else {                                     // dW2[j][c]
            const int j = (idx - D * D) >> 1, c = (idx - D * D) & 1;
            a = (double)w.w1[j] * S[c];
            for (int i = 1; i < D; ++i) a += (double)w.w1[i * D + j] * S[2 * i + c];
        }
        grad_sum[idx] = a;
    }
}

template <int WIN>
static void launch_fcn_windows(const float *block_min, const uint8_t *success, const int32_t *index, const float *rowmin,
                               int64_t R, int nblk, float *inputs, uint8_t *labels, int64_t *class_count, hipStream_t st)
{
    const long long total = (long long)(nblk - WIN + 1) * R, want = (total + 255) / 256;
    hipLaunchKernelGGL(fcn_windows_kernel<WIN>, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(256), 0, st, block_min, success,
                       index, rowmin, (long long)R, nblk, inputs, labels, reinterpret_cast<unsigned long long *>(class_count));
}

template <int D>
static void launch_fcn_grad(const float *inputs, const uint8_t *labels, const float *weight, const int32_t *index, int64_t B,
                            const SlideFcnArg &w, float penalty, float *p, double *part, long long *cnt, int nb, hipStream_t st)
{
    hipLaunchKernelGGL(fcn_grad_kernel<D>, dim3((unsigned)nb), dim3(256), 0, st, inputs, labels, weight, index, (long long)B, w,
                       penalty, p, part, cnt);
}

// the instantiation for a run-time window width 1..kSlideMaxWin (validated by the caller)
#define LDPC_FCN_DISPATCH(win, CALL)                                                                                        \
    switch (win) {                                                                                                          \
    case 1: CALL(1); break;   case 2: CALL(2); break;   case 3: CALL(3); break;   case 4: CALL(4); break;                   \
    case 5: CALL(5); break;   case 6: CALL(6); break;   case 7: CALL(7); break;   case 8: CALL(8); break;                   \
    case 9: CALL(9); break;   case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break;                 \
    case 13: CALL(13); break; case 14: CALL(14); break; default: CALL(15); break;                                           \
    }

static int fcn_windows_run(const float *d_block_min, const uint8_t *d_success, const int32_t *d_index, int64_t R, int nblk,
                           int win, float *d_inputs, uint8_t *d_labels, int64_t *d_class_count, hipStream_t st)
{
    float *rowmin = nullptr;
    LDPC_HIP(hipMallocAsync((void **)&rowmin, sizeof(float) * (size_t)R, st));
    hipError_t e = hipSuccess;
    if (d_class_count) e = hipMemsetAsync(d_class_count, 0, 2 * sizeof(int64_t), st);
    if (e == hipSuccess) {
        const long long want = (R + 255) / 256;
        hipLaunchKernelGGL(fcn_rowmin_kernel, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(256), 0, st, d_block_min, d_index,
                           (long long)R, nblk, rowmin);
#define LDPC_FCN_CALL(W) launch_fcn_windows<W>(d_block_min, d_success, d_index, rowmin, R, nblk, d_inputs, d_labels, d_class_count, st)
        LDPC_FCN_DISPATCH(win, LDPC_FCN_CALL)
#undef LDPC_FCN_CALL
        e = hipGetLastError();
    }
    (void)hipFreeAsync(rowmin, st);
    if (e != hipSuccess) return hip_fail(e, "fcn_windows_kernel");
    return LDPC_OK;
}

static int fcn_grad_run(const float *d_inputs, const uint8_t *d_labels, const float *d_weight, const int32_t *d_index, int64_t B,
                        int win, const SlideFcnArg &w, float penalty, float *d_p, double *d_loss_sum, double *d_grad_sum,
                        double *d_acc, int64_t *d_counts, hipStream_t st)
{
    const bool sums = d_loss_sum || d_grad_sum || d_acc || d_counts;
    const int D = win + 1, K = 2 * D + 3;
    const long long want = (B + 255) / 256;
    const int nb = (int)(want < kFcnGradMaxBlocks ? want : kFcnGradMaxBlocks);
    double *part = nullptr;
    long long *cnt = nullptr;
    if (sums) {
        LDPC_HIP(hipMallocAsync((void **)&part, (sizeof(double) * K + sizeof(long long) * 3) * (size_t)nb, st));
        cnt = reinterpret_cast<long long *>(part + (size_t)nb * K);
    }
#define LDPC_FCN_CALL(W) launch_fcn_grad<W + 1>(d_inputs, d_labels, d_weight, d_index, B, w, penalty, d_p, part, cnt, nb, st)
    LDPC_FCN_DISPATCH(win, LDPC_FCN_CALL)
#undef LDPC_FCN_CALL
    if (sums)
        hipLaunchKernelGGL(fcn_grad_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)part, (const long long *)cnt, nb, D, w,
                           d_loss_sum, d_grad_sum, d_acc, reinterpret_cast<long long *>(d_counts));
    const hipError_t e = hipGetLastError();
    if (sums) (void)hipFreeAsync(part, st);
    if (e != hipSuccess) return hip_fail(e, "fcn_grad_kernel");
    return LDPC_OK;
}

}  // namespace ldpc
