// OSD kernels, the short ones (one frame per wavefront, no MFMA: bit and compare work): osd_ge_kernel, osd_front_kernel and
//   osd_search_kernel   conventional order-p search over the reference's TEP table: per frame a byte-indexed LUT of partial |y'|
//                       sums in LDS (8 x 256 floats), each lane evaluates one TEP per round: parity word = d0 ^ P'[i] ^ P'[j] ...,
//                       metric = flipped-MRB weights + 8 LUT terms in a FIXED order (the canonical order the oracle uses, see
//                       oracle/np_oracle.py weighted_distance), first minimum.
#pragma once

#include "ldpc_search.h"
#include "ldpc_front.h"

namespace ldpc {

// ---------------------------------------------------------------------------------------
// ldpc_osd_ge: elimination of caller-supplied matrices (row-major in, row-major out)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void osd_ge_kernel(const u64 *__restrict__ rows_in, long long F, u64 *__restrict__ rows_out,
        unsigned char *__restrict__ swaps, int *__restrict__ nswaps)
{
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    for (long long f = wave; f < F; f += (long long)gridDim.x * 4) {
        const u64 *src = rows_in + f * 128;
        u64 C1 = transpose64(src[lane * 2], lane);      // row r, columns 0..63  -> column lane, bit r
        u64 C2 = transpose64(src[lane * 2 + 1], lane);
        int rho = lane, idx1 = lane, idx2 = lane + 64;
        const int ns = ge_columns(C1, C2, rho, idx1, idx2, lane, swaps ? swaps + f * 128 : nullptr);
        // back to row-major, logical row order: lane = physical row after the transpose
        const u64 R1 = transpose64(C1, lane), R2 = transpose64(C2, lane);
        rows_out[f * 128 + lane * 2] = shfl64(R1, rho);
        rows_out[f * 128 + lane * 2 + 1] = shfl64(R2, rho);
        if (nswaps && lane == 0) nswaps[f] = ns;
    }
}

// ---------------------------------------------------------------------------------------
// OSD front end (the per-frame device code: ldpc_front.h)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void osd_front_kernel(const float *__restrict__ y, const int *__restrict__ index, const int *__restrict__ count,
        long long F, const u64 *__restrict__ Gcols, unsigned char *__restrict__ perm_out, u64 *__restrict__ parity_out, int *__restrict__ nswaps)
{
    __shared__ FrontLds L;   // one wavefront per workgroup
    __shared__ u64 Gl[128];  // the columns of G: the same for every frame, so the gather after the sort reads LDS, not L2
    const int lane = threadIdx.x;
    const u64 g1 = Gcols[lane], g2 = Gcols[64 + lane];              // in flight while the count and the first frames are fetched
    const long long nframes = frame_count(count, F);
    // Software pipeline over the frames of this workgroup (the launcher's grid is front_grid(): frames block, block + grid, ...):
    // the frame number is asked for two frames ahead and the y row one frame ahead.  A list entry stays a 32-bit value until
    // the trip that forms the row address with it (widening it is a use, and a use is where the wave waits for the load), and
    // the row's magnitude bits are taken at the end of the trip before, so that nothing is awaited right behind its request.
    const long long G = gridDim.x;
    long long f0 = blockIdx.x, f1 = f0 + G, f2 = f1 + G;
    int ia = 0, ib = 0;
    unsigned a1 = 0, a2 = 0;
    if (index && f0 < nframes) ia = index[f0];
    if (index && f1 < nframes) ib = index[f1];
    if (f0 < nframes) {
        const long long src = index ? (long long)ia : f0;
        a1 = __float_as_uint(y[src * 128 + lane]) & 0x7FFFFFFFu; a2 = __float_as_uint(y[src * 128 + 64 + lane]) & 0x7FFFFFFFu;
    }
    Gl[lane] = g1; Gl[64 + lane] = g2;                              // (read after the first wave_fence of front_device_vals)
    while (f0 < nframes) {
        unsigned yb1 = 0, yb2 = 0;
        if (f1 < nframes) {
            const long long src = index ? (long long)ib : f1;
            yb1 = __float_as_uint(y[src * 128 + lane]); yb2 = __float_as_uint(y[src * 128 + 64 + lane]);
        }
        int ic = 0;
        if (index && f2 < nframes) ic = index[f2];
        // (true: see GE_LANE_OPAQUE, ldpc_front.h)
        const FrontResult res = front_device_vals<true>(L, a1, a2, Gl, lane);
        perm_out[f0 * 128 + lane] = (unsigned char)res.o1;
        perm_out[f0 * 128 + 64 + lane] = (unsigned char)res.o2;
        parity_out[f0 * 64 + lane] = res.Prow;
        if (nswaps && lane == 0) nswaps[f0] = res.ns;
        f0 = f1; f1 = f2; f2 += G;
        asm volatile("" : "+v"(yb1), "+v"(yb2));    // (no instruction: keeps the two ANDs, the row's first use, down here)
        ib = ic; a1 = yb1 & 0x7FFFFFFFu; a2 = yb2 & 0x7FFFFFFFu;
    }
}

// ---------------------------------------------------------------------------------------
// conventional order-p search (convention_osd_main, convention_osd.py:49-76)
// ---------------------------------------------------------------------------------------
// WAVES = 1 for the long scans (one wavefront per workgroup: compile-time LDS base for the LUT reads, frames
// balanced by the dispatcher), 4 for orders 0 and 1, where a frame is too little work to pay for a workgroup
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void osd_search_kernel(const float *__restrict__ y, const int *__restrict__ index,
        const int *__restrict__ count, long long F, const unsigned char *__restrict__ perm_in, const u64 *__restrict__ parity_in,
        const uchar4 *__restrict__ teps, int ntep, u64 *__restrict__ cw_out, float *__restrict__ metric_out, int *__restrict__ best_out,
        int *__restrict__ ntep_out)
{
    __shared__ SearchLds lds[WAVES];
    const int lane = threadIdx.x & 63;
    SearchLds &L = lds[WAVES == 1 ? 0 : threadIdx.x >> 6];
    const long long nframes = frame_count(count, F);
    const long long wave = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);

    for (long long f = wave; f < nframes; f += (long long)gridDim.x * WAVES) {
        const long long src = index ? index[f] : f;
        const SearchFrame S = search_prepare(L, y, src, perm_in, parity_in, f, lane);
        // scan the TEP table, one TEP per lane per round; strict '<' keeps the first minimum
        float best = __builtin_inff();
        int bestt = 0x7FFFFFFF;
        u64 bestD = 0, bestE = 0;
        // (exact early exit on the metric prefix, see tep_cost_bounded; `bound` = the wave's best so far)
        float bound = __builtin_inff();
        int trip = 0;
        for (int t0 = 0; t0 < ntep; t0 += 64, ++trip) {
            const int t = t0 + lane;
            if (t < ntep) {
                u64 D, E;
                float mrb, c;
                tep_apply(L, teps[t], S.d0, D, E, mrb);
                if (tep_cost_bounded(L, mrb, D, bound, c) && c < best) { best = c; bestt = t; bestD = D; bestE = E; }
            }
            if ((trip & 7) == 0) bound = wave_min_f32(best);
        }
        wave_argmin(best, bestt, bestD, bestE, lane);
        search_finish(L, S, bestE, bestD, f, lane, cw_out);
        store_results(f, lane, best, bestt, ntep, metric_out, best_out, ntep_out);
    }
}

}  // namespace ldpc
