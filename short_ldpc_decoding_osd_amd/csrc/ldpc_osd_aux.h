// OSD kernels round the decoders: one given TEP per frame, the success counters, the check of a frame list.
#pragma once

#include "ldpc_search.h"

namespace ldpc {

// One given TEP per frame (one_tep_compare, FS_OSD/fs_testing.py:51-64): re-encode the MRB hard decisions with the
// positions of `mask` flipped, Hamming distance and weighted distance of the candidate -- the SAME LUT evaluation and
// float order as the searches (the Python helper of that name used to restate the order in NumPy).
__global__ __launch_bounds__(256) void osd_tep_eval_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, const unsigned char *__restrict__ perm_in, const u64 *__restrict__ parity_in, const u64 *__restrict__ mask,
        u64 *__restrict__ cw_out, float *__restrict__ metric_out, int *__restrict__ hd_out)
{
    __shared__ SearchLds lds[4];
    const int lane = threadIdx.x & 63;
    SearchLds &L = lds[threadIdx.x >> 6];
    const long long nframes = frame_count(count, F);
    for (long long f = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); f < nframes; f += (long long)gridDim.x * 4) {
        const long long src = index ? index[f] : f;
        const SearchFrame S = search_prepare(L, y, src, perm_in, parity_in, f, lane);
        const u64 E = mask[f];
        const u64 D = S.d0 ^ wave_xor64(((E >> lane) & 1) ? L.P[lane] : 0ull);
        float mrb = 0.0f;                                  // flipped MRB weights, ascending position, sequential
        for (u64 m = E; m; m &= m - 1) mrb = mrb + L.w[__builtin_ctzll(m)];
        const float cost = tep_cost(L, mrb, D);
        search_finish(L, S, E, D, f, lane, cw_out);
        if (lane == 0) {
            if (metric_out) metric_out[f] = cost;
            if (hd_out) hd_out[f] = __popcll(E) + __popcll(D);
        }
    }
}

__global__ __launch_bounds__(256) void osd_counts_kernel(const u64 *__restrict__ cw, const u64 *__restrict__ label, const int *__restrict__ index,
        const int *__restrict__ count, const int *__restrict__ ntep, long long F, u64 *__restrict__ counts)
{
    __shared__ u64 part[4][3];
    const long long nframes = frame_count(count, F);
    u64 n = 0, wrong = 0, teps = 0;
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < nframes; f += (long long)gridDim.x * blockDim.x) {
        const long long src = index ? index[f] : f;
        n += 1;
        wrong += (cw[f * 2] != label[src * 2]) || (cw[f * 2 + 1] != label[src * 2 + 1]);
        teps += ntep ? (u64)ntep[f] : 0ull;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n += __shfl_down(n, off, 64); wrong += __shfl_down(wrong, off, 64); teps += __shfl_down(teps, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[wave][0] = n; part[wave][1] = wrong; part[wave][2] = teps; }
    __syncthreads();
    if (threadIdx.x < 3)
        atomicAdd(&counts[threadIdx.x], part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
}

// ldpc_osd_params.y_frames (debug aid): the frame list the kernels will follow, with every entry outside [0, y_frames)
// replaced by 0 and counted
__global__ __launch_bounds__(256) void index_guard_kernel(const int *__restrict__ index, const int *__restrict__ count, long long F,
        long long y_frames, int *__restrict__ safe, unsigned long long *__restrict__ errors)
{
    const long long nframes = frame_count(count, F);
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < nframes; f += (long long)gridDim.x * blockDim.x) {
        const int v = index[f];
        const bool bad = v < 0 || v >= y_frames;
        safe[f] = bad ? 0 : v;
        if (bad) atomicAdd(errors, 1ull);
    }
}

}  // namespace ldpc
