// Small streaming kernels around the decoders: error statistics, failed-frame compaction,
// bit (un)packing.  All are HBM-bound byte movers; they read/write every byte once with
// coalesced accesses and reduce in registers / LDS before touching an atomic.
//
// Reference (paths relative to LDPC_128/): Ldpc_128_testing/ms_test.py:36-54 (get_eval),
// :51 (failure index), Ldpc_128_testing/data_generating.py / read_TFdata.py (labels are one
// int64 per bit).
#include "ldpc_internal.h"
#include "ldpc_family_check.h"   // osd_merge_check
#include "ldpc_dlosd_stage.h"    // dlosd_gather, dlosd_counts

namespace ldpc {

// ---------------------------------------------------------------------------------------
// get_eval counters.  One thread per frame; per-wave reduction by shuffles, one atomic set
// per wave.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void eval_counts_kernel(const unsigned long long *__restrict__ hard,
                                                          const unsigned long long *__restrict__ label,
                                                          const unsigned char *__restrict__ fail, long long B,
                                                          int words, unsigned long long *__restrict__ counts)
{
    __shared__ unsigned long long part[4][5];
    unsigned long long ferr = 0, berr = 0, und = 0, sf = 0, cnt = 0;
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < B; f += (long long)gridDim.x * blockDim.x) {
        int e = 0;
        for (int w = 0; w < words; ++w) e += __popcll(hard[f * words + w] ^ label[f * words + w]);
        const int bad = fail ? fail[f] != 0 : 0;
        cnt += 1; berr += e; ferr += e != 0; sf += bad; und += (fail && !bad && e != 0);
    }
    cnt = wave_sum(cnt); ferr = wave_sum(ferr); berr = wave_sum(berr); und = wave_sum(und); sf = wave_sum(sf);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = cnt; part[wave][1] = ferr; part[wave][2] = berr; part[wave][3] = und; part[wave][4] = sf;
    }
    __syncthreads();
    // one atomic per counter per block (a few hundred in all): contended same-line atomics
    // serialise at the memory side, so keep them rare
    if (threadIdx.x < 5)
        atomicAdd(&counts[threadIdx.x], part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
}

// ---------------------------------------------------------------------------------------
// ldpc_osd_merge: the OSD codewords back among the NMS decisions, and the bit errors before and after.  One lane per
// listed frame j < min(*count, F): f = index[j], the `words` words of hard[f] are replaced by cw[j] -- the lane reads
// the old word before it writes the new one, and the entries of index are distinct, so the in-place form has no race --
// and counts[4] += {frames, frames with cw[j] != label[f], bit errors of cw[j], bit errors of the OLD hard[f]}.
// Work proportional to the failures: a listed frame costs 2-3 reads and a write of `words` words.  Per-wave reduction
// by shuffles, one atomic per counter and block.
// ---------------------------------------------------------------------------------------
template <bool HARD, bool COUNT>
__global__ __launch_bounds__(256) void osd_merge_kernel(const unsigned long long *__restrict__ cw, const int *__restrict__ index,
                                                        const int *__restrict__ count, long long F, int words,
                                                        unsigned long long *__restrict__ hard,
                                                        const unsigned long long *__restrict__ label,
                                                        unsigned long long *__restrict__ counts)
{
    __shared__ unsigned long long part[4][4];
    const long long c = *count, nframes = c < F ? c : F;
    if ((long long)blockIdx.x * blockDim.x >= nframes) return;   // (the whole block: the grid is sized by F, not by the count)
    unsigned long long cnt = 0, wrong = 0, after = 0, before = 0;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nframes; j += (long long)gridDim.x * blockDim.x) {
        const long long f = index[j];
        int ea = 0, eb = 0;
        for (int w = 0; w < words; ++w) {
            const unsigned long long v = cw[j * words + w];
            if constexpr (COUNT) {
                const unsigned long long l = label[f * words + w];
                ea += __popcll(v ^ l);
                if constexpr (HARD) eb += __popcll(hard[f * words + w] ^ l);
            }
            if constexpr (HARD) hard[f * words + w] = v;
        }
        cnt += 1; wrong += ea != 0; after += ea; before += eb;
    }
    if constexpr (COUNT) {
        cnt = wave_sum(cnt); wrong = wave_sum(wrong); after = wave_sum(after); before = wave_sum(before);
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { part[wave][0] = cnt; part[wave][1] = wrong; part[wave][2] = after; part[wave][3] = before; }
        __syncthreads();
        if (threadIdx.x < 4)
            atomicAdd(&counts[threadIdx.x], part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
    }
}

// ---------------------------------------------------------------------------------------
// The two small kernels of ldpc_dlosd_pipeline_run, both on the listed frames j < min(*count, F) and with no workspace.
// dlosd_gather_kernel: the H-form calls take dense rows, so xm[j] = llr[index[j]] (n floats) and, with labels,
// list_label[j] = label[index[j]] (`words` words), and xo[j] = xm[j] where the caller wants the ordering values of DIA = False in a
// buffer of their own.  One wavefront per listed frame, consecutive lanes on consecutive
// elements; V4: 16-byte loads and stores, for n a multiple of 4 (then every row of both arrays is 16-byte aligned).
// dlosd_counts_kernel: counts[6] += {frames, frames with success, frames without, sum of deep - win + 1, sum of
// block_off[deep], sum of nteps}; success is the scan's byte or, without it, gmin[j] == truth[j] (the scan's own comparison, on
// the two floats it wrote); with neither, and without nteps, their counters stay.  block_off has nblk + 1 entries and
// the sliding scans write win <= deep <= nblk; the index is clamped all the same, so nothing beyond block_off[nblk] is read
// whatever the buffer holds.  Per-wave reduction by shuffles, one atomic per counter and block.
// ---------------------------------------------------------------------------------------
template <bool V4>
__global__ __launch_bounds__(256) void dlosd_gather_kernel(const float *__restrict__ llr, const unsigned long long *__restrict__ label,
                                                           const int *__restrict__ index, const int *__restrict__ count, long long F,
                                                           int n, int words, float *__restrict__ xm, float *__restrict__ xo,
                                                           unsigned long long *__restrict__ list_label)
{
    const long long c = *count, nframes = c < F ? c : F;
    if ((long long)blockIdx.x * 4 >= nframes) return;   // (the whole block: the grid is sized by F, not by the count)
    const int lane = threadIdx.x & 63;
    for (long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); j < nframes; j += (long long)gridDim.x * 4) {
        const long long f = index[j];
        if constexpr (V4) {
            const float4 *__restrict__ src = reinterpret_cast<const float4 *>(llr + f * n);
            float4 *__restrict__ dst = reinterpret_cast<float4 *>(xm + j * n);
            float4 *__restrict__ dst2 = reinterpret_cast<float4 *>(xo + j * n);
            for (int v = lane; v < (n >> 2); v += 64) { const float4 t = src[v]; dst[v] = t; if (xo) dst2[v] = t; }
        } else {
            for (int v = lane; v < n; v += 64) { const float t = llr[f * n + v]; xm[j * n + v] = t; if (xo) xo[j * n + v] = t; }
        }
        if (label)
            for (int w = lane; w < words; w += 64) list_label[j * words + w] = label[f * words + w];
    }
}

__global__ __launch_bounds__(256) void dlosd_counts_kernel(const int *__restrict__ deep, const unsigned char *__restrict__ success,
                                                           const float *__restrict__ gmin, const float *__restrict__ truth,
                                                           const int *__restrict__ nteps, const int *__restrict__ block_off, int nblk,
                                                           int win, const int *__restrict__ count, long long F,
                                                           unsigned long long *__restrict__ counts)
{
    __shared__ unsigned long long part[4][6];
    const long long c = *count, nframes = c < F ? c : F;
    if ((long long)blockIdx.x * blockDim.x >= nframes) return;   // (the whole block: the grid is sized by F, not by the count)
    unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nframes; j += (long long)gridDim.x * blockDim.x) {
        const int dl = deep[j], at = dl < 0 ? 0 : (dl < nblk ? dl : nblk);
        v[0] += 1;
        if (success || (gmin && truth)) { const bool ok = success ? success[j] != 0 : gmin[j] == truth[j]; v[1] += ok; v[2] += !ok; }
        v[3] += (unsigned long long)(long long)(dl - win + 1);
        v[4] += (unsigned long long)(long long)block_off[at];
        if (nteps) v[5] += (unsigned long long)(long long)nteps[j];
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const unsigned long long s = wave_sum(v[i]);
        if ((threadIdx.x & 63) == 0) part[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < 6)
        atomicAdd(&counts[threadIdx.x], part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
}

// ---------------------------------------------------------------------------------------
// Ordered compaction in ONE launch and with NO scratch memory (so calls on different streams of one
// context cannot disturb each other).  The flags are cut into at most kMaxSeg contiguous segments, one
// per block.  A block first counts the set flags BEFORE its segment itself -- 16 flags per load, the flag
// array is L2-resident (1 B per frame: the last of 64 blocks re-reads 126 KiB at B = 131 072) -- and then
// scans its own segment 2048 or 8192 flags at a time, scattering ascending frame numbers.  The redundant prefix
// reads grow with B / 2 per block, i.e. stay ~1 % of the NMS time of the same batch at any B.
// The block that owns the last segment writes the total.
// ---------------------------------------------------------------------------------------
constexpr int kMaxSeg = 256;   // segments (= blocks) per launch

__device__ __forceinline__ int nonzero_bytes(unsigned long long v)
{
    const unsigned long long k7 = 0x7F7F7F7F7F7F7F7Full;
    return __popcll((((v & k7) + k7) | v) & ~k7);
}

// FPT consecutive flags of one thread as a bit mask
template <int FPT>
__device__ __forceinline__ unsigned flags_of(const unsigned char *flag, long long base, long long B, bool aligned)
{
    unsigned bits = 0;
    if (FPT == 8 && aligned && base + 8 <= B) {
        unsigned long long v = *reinterpret_cast<const unsigned long long *>(flag + base);
#pragma unroll
        for (int i = 0; i < 8; ++i) bits |= (unsigned)(((v >> (8 * i)) & 0xFF) != 0) << i;
    } else {
#pragma unroll
        for (int i = 0; i < FPT; ++i) if (base + i < B) bits |= (unsigned)(flag[base + i] != 0) << i;
    }
    return bits;
}

constexpr int kCompactThreads = 1024, kCompactWaves = kCompactThreads / 64;

__device__ __forceinline__ int block_sum(int v, int *wsum /*[kCompactWaves] shared*/)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();                         // wsum may still be read from an earlier use
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < kCompactWaves; ++w) t += wsum[w];
    return t;
}

// EVAL: the get_eval counters of the same frames ride along (ldpc_pipeline_run: the flags are the
// syndrome flags either way), so the pipeline needs neither eval_counts_kernel nor a second pass.
// 1024 threads per block: the prefix count of the LAST block is a chain of (flags before it) / 16 KiB dependent
// trips of ~0.4 us each (the flags were written by other XCDs: L2 misses) -- 8 trips at B = 131 072.
// FPT flags per thread and step: 2 for batches up to 524 288 frames (2048 flags per block), 8 beyond.
template <bool EVAL, int FPT>
__global__ __launch_bounds__(kCompactThreads) void compact_kernel(const unsigned char *__restrict__ flag, long long B, long long seg,
                                                                  int *__restrict__ index, int *__restrict__ count,
                                                                  const unsigned long long *__restrict__ hard,
                                                                  const unsigned long long *__restrict__ label, int words,
                                                                  unsigned long long *__restrict__ counts)
{
    constexpr int NT = kCompactThreads, kStep = NT * FPT;
    __shared__ int wsum[kCompactWaves];
    __shared__ unsigned long long epart[kCompactWaves][4];
    const long long lo = (long long)blockIdx.x * seg;
    const long long hi = lo + seg < B ? lo + seg : B;
    const bool al16 = (reinterpret_cast<unsigned long long>(flag) & 15) == 0;
    // ---- set flags before this segment (lo is a multiple of 16): independent loads, four in flight per thread
    int acc = 0;
    if (al16) {
        long long i = (long long)threadIdx.x * 16;
        for (; i + 3LL * NT * 16 < lo; i += 4LL * NT * 16) {
            const uint4 v0 = *reinterpret_cast<const uint4 *>(flag + i), v1 = *reinterpret_cast<const uint4 *>(flag + i + NT * 16LL);
            const uint4 v2 = *reinterpret_cast<const uint4 *>(flag + i + 2LL * NT * 16), v3 = *reinterpret_cast<const uint4 *>(flag + i + 3LL * NT * 16);
            acc += nonzero_bytes(((unsigned long long)v0.y << 32) | v0.x) + nonzero_bytes(((unsigned long long)v0.w << 32) | v0.z);
            acc += nonzero_bytes(((unsigned long long)v1.y << 32) | v1.x) + nonzero_bytes(((unsigned long long)v1.w << 32) | v1.z);
            acc += nonzero_bytes(((unsigned long long)v2.y << 32) | v2.x) + nonzero_bytes(((unsigned long long)v2.w << 32) | v2.z);
            acc += nonzero_bytes(((unsigned long long)v3.y << 32) | v3.x) + nonzero_bytes(((unsigned long long)v3.w << 32) | v3.z);
        }
        for (; i < lo; i += NT * 16LL) {
            const uint4 v = *reinterpret_cast<const uint4 *>(flag + i);
            acc += nonzero_bytes(((unsigned long long)v.y << 32) | v.x) + nonzero_bytes(((unsigned long long)v.w << 32) | v.z);
        }
    } else {
        for (long long i = threadIdx.x; i < lo; i += NT) acc += flag[i] != 0;
    }
    int base = block_sum(acc, wsum);
    // ---- own segment
    unsigned long long ferr = 0, berr = 0, und = 0, cnt = 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long c0 = lo; c0 < hi; c0 += kStep) {
        const long long fb = c0 + threadIdx.x * FPT;
        const unsigned bits = fb < hi ? flags_of<FPT>(flag, fb, hi, al16) : 0;
        const int mine = __popc(bits);
        if constexpr (EVAL) {   // frame c0 + q NT + thread: coalesced loads of the hard words and labels
            if (words == 2) {   // n = 128: every load of the step is issued before the first is used (one memory latency)
                ulonglong2 hv[FPT], lv[FPT];
                unsigned char fv[FPT];
#pragma unroll
                for (int q = 0; q < FPT; ++q) {
                    const long long f = c0 + q * NT + threadIdx.x, fc = f < hi ? f : lo;
                    hv[q] = *reinterpret_cast<const ulonglong2 *>(hard + fc * 2);
                    lv[q] = *reinterpret_cast<const ulonglong2 *>(label + fc * 2);
                    fv[q] = flag[fc];
                }
#pragma unroll
                for (int q = 0; q < FPT; ++q) {
                    if (c0 + q * NT + threadIdx.x < hi) {
                        const int e = __popcll(hv[q].x ^ lv[q].x) + __popcll(hv[q].y ^ lv[q].y);
                        cnt += 1; berr += e; ferr += e != 0; und += (fv[q] == 0 && e != 0);
                    }
                }
            } else {
#pragma unroll
                for (int q = 0; q < FPT; ++q) {
                    const long long f = c0 + q * NT + threadIdx.x;
                    if (f < hi) {
                        int e = 0;
                        for (int w = 0; w < words; ++w) e += __popcll(hard[f * words + w] ^ label[f * words + w]);
                        cnt += 1; berr += e; ferr += e != 0; und += (flag[f] == 0 && e != 0);
                    }
                }
            }
        }
        int incl = mine;   // exclusive scan over the threads: in-wave inclusive scan, then wave offsets
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        __syncthreads();
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kCompactWaves; ++w) { woff += w < wave ? wsum[w] : 0; tot += wsum[w]; }
        int pos = base + woff + incl - mine;
#pragma unroll
        for (int i = 0; i < FPT; ++i)
            if ((bits >> i) & 1) index[pos++] = (int)(fb + i);
        base += tot;
    }
    if (hi == B && threadIdx.x == 0) *count = base;
    if constexpr (EVAL) {   // counts[] = {frames, frame_err, bit_err, undetected, synd_fail}
        cnt = wave_sum(cnt); ferr = wave_sum(ferr); berr = wave_sum(berr); und = wave_sum(und);
        if (lane == 0) { epart[wave][0] = cnt; epart[wave][1] = ferr; epart[wave][2] = berr; epart[wave][3] = und; }
        const int before = block_sum(acc, wsum);   // (also the barrier that publishes epart)
        if (threadIdx.x < 4) {
            unsigned long long t = 0;
#pragma unroll
            for (int w = 0; w < kCompactWaves; ++w) t += epart[w][threadIdx.x];
            atomicAdd(&counts[threadIdx.x], t);
        }
        if (threadIdx.x == 4) atomicAdd(&counts[4], (unsigned long long)(base - before));
    }
}

static void compact_geometry(int64_t B, int fpt, unsigned *blocks, long long *seg)
{
    const int64_t step = (int64_t)kCompactThreads * fpt;
    const int64_t chunks = (B + step - 1) / step;
    const int64_t per = (chunks + kMaxSeg - 1) / kMaxSeg;   // steps per segment
    *seg = (long long)per * step;
    *blocks = (unsigned)((B + *seg - 1) / *seg);
}

template <bool EVAL>
static void launch_compact(const uint8_t *d_flag, int64_t B, int32_t *d_index, int32_t *d_count, const unsigned long long *hard,
                           const unsigned long long *label, int words, unsigned long long *counts, hipStream_t st)
{
    unsigned blocks; long long seg;
    if (B <= (int64_t)kMaxSeg * kCompactThreads * 2) {
        compact_geometry(B, 2, &blocks, &seg);
        hipLaunchKernelGGL((compact_kernel<EVAL, 2>), dim3(blocks), dim3(kCompactThreads), 0, st, d_flag, (long long)B, seg, d_index, d_count, hard, label, words, counts);
    } else {
        compact_geometry(B, 8, &blocks, &seg);
        hipLaunchKernelGGL((compact_kernel<EVAL, 8>), dim3(blocks), dim3(kCompactThreads), 0, st, d_flag, (long long)B, seg, d_index, d_count, hard, label, words, counts);
    }
}

// ---------------------------------------------------------------------------------------
// bit packing: one wavefront packs 64 bits per step with a ballot
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pack_bits_kernel(const T *__restrict__ bits, long long B, int n, int words,
                                                        unsigned long long *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long total = B * words;
    for (long long t = wave; t < total; t += (long long)gridDim.x * 4) {
        const long long f = t / words;
        const int v = (int)(t % words) * 64 + lane;
        const unsigned long long m = __ballot(v < n && (bits[f * n + v] & 1));
        if (lane == 0) out[t] = m;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void unpack_bits_kernel(const unsigned long long *__restrict__ in, long long B,
                                                          int n, int words, T *__restrict__ bits)
{
    const long long total = B * n;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long f = t / n;
        const int v = (int)(t % n);
        bits[t] = (T)((in[f * words + (v >> 6)] >> (v & 63)) & 1);
    }
}

static unsigned grid_for(long long items, int per_block, unsigned cap = 4096)
{
    long long g = (items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return (unsigned)(g < cap ? g : cap);
}

}  // namespace ldpc

using namespace ldpc;

extern "C" {

int ldpc_eval_counts(ldpc_ctx *ctx, const uint64_t *d_hard, const uint64_t *d_label, const uint8_t *d_fail,
                     int64_t B, int64_t *d_counts, void *stream)
{
    if (!ctx || !d_hard || !d_label || !d_counts || B < 0) return fail(LDPC_E_ARG, "ldpc_eval_counts: bad arguments");
    if (B == 0) return LDPC_OK;
    const int words = (ctx->code.n + 63) / 64;
    hipLaunchKernelGGL(eval_counts_kernel, dim3(grid_for(B, 1024, 128)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned long long *>(d_hard),
                       reinterpret_cast<const unsigned long long *>(d_label), d_fail, (long long)B, words,
                       reinterpret_cast<unsigned long long *>(d_counts));
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_osd_merge(ldpc_ctx *ctx, const uint64_t *d_cw, const int32_t *d_index, const int32_t *d_count, int64_t F, uint64_t *d_hard,
                   const uint64_t *d_label_bits, int64_t *d_counts, void *stream)
{
    bool launch;
    if (int rc = osd_merge_check(ctx, d_cw, d_index, d_count, F, d_hard, d_label_bits, d_counts, &launch)) return rc;
    if (!launch) return LDPC_OK;
    const bool counting = d_label_bits && d_counts;   // a pair or neither, as in the family decode calls
    const int words = (ctx->code.n + 63) / 64;
    const auto kern = d_hard ? (counting ? osd_merge_kernel<true, true> : osd_merge_kernel<true, false>) : osd_merge_kernel<false, true>;
    hipLaunchKernelGGL(kern, dim3(grid_for(F, 256, 1024)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned long long *>(d_cw), d_index, d_count, (long long)F, words,
                       reinterpret_cast<unsigned long long *>(d_hard), reinterpret_cast<const unsigned long long *>(d_label_bits),
                       reinterpret_cast<unsigned long long *>(d_counts));
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // extern "C"

namespace ldpc {
// (a kernel, not hipMemsetAsync: a memset node captured into a hipGraph did not run on later replays, ROCm 7.2)
__global__ void zero_word_kernel(int32_t *p) { *p = 0; }
}  // namespace ldpc

extern "C" {

int ldpc_compact(ldpc_ctx *ctx, const uint8_t *d_flag, int64_t B, int32_t *d_index, int32_t *d_count, void *stream)
{
    if (!ctx || !d_count || B < 0 || B > 0x7FFFFFFFLL || (B > 0 && (!d_flag || !d_index)))
        return fail(LDPC_E_ARG, "ldpc_compact: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) { hipLaunchKernelGGL(ldpc::zero_word_kernel, dim3(1), dim3(1), 0, st, d_count); LDPC_HIP(hipGetLastError()); return LDPC_OK; }
    launch_compact<false>(d_flag, B, d_index, d_count, nullptr, nullptr, 0, nullptr, st);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // extern "C"

namespace ldpc {

// ldpc_eval_counts + ldpc_compact on the same flags in one launch (ldpc_pipeline_run)
int eval_and_compact(ldpc_ctx *ctx, const uint64_t *d_hard, const uint64_t *d_label, const uint8_t *d_fail, int64_t B,
                     int64_t *d_counts, int32_t *d_index, int32_t *d_count, hipStream_t st)
{
    if (!ctx || !d_hard || !d_label || !d_fail || !d_counts || !d_index || !d_count || B <= 0 || B > 0x7FFFFFFFLL)
        return fail(LDPC_E_ARG, "eval_and_compact: bad arguments");
    launch_compact<true>(d_fail, B, d_index, d_count, reinterpret_cast<const unsigned long long *>(d_hard),
                         reinterpret_cast<const unsigned long long *>(d_label), (ctx->code.n + 63) / 64,
                         reinterpret_cast<unsigned long long *>(d_counts), st);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

// the gather and the stage counters of ldpc_dlosd_pipeline_run (ldpc_dlosd_stage.h), F > 0
int dlosd_gather(const ldpc_ctx *ctx, const float *d_llr, const uint64_t *d_label_bits, const int32_t *d_index, const int32_t *d_count, int64_t F,
                 float *d_metric_llr, float *d_order_llr, uint64_t *d_list_labels, hipStream_t st)
{
    const int n = ctx->code.n, words = (n + 63) / 64;
    const bool v4 = n % 4 == 0 && ((uintptr_t)d_llr | (uintptr_t)d_metric_llr | (uintptr_t)d_order_llr) % 16 == 0;
    hipLaunchKernelGGL(v4 ? dlosd_gather_kernel<true> : dlosd_gather_kernel<false>, dim3(grid_for(F, 4, 8192)), dim3(256), 0, st, d_llr,
                       reinterpret_cast<const unsigned long long *>(d_label_bits), d_index, d_count, (long long)F, n, words, d_metric_llr,
                       d_order_llr, reinterpret_cast<unsigned long long *>(d_list_labels));
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int dlosd_counts(const int32_t *d_deep_limit, const uint8_t *d_success, const float *d_global_min, const float *d_truth, const int32_t *d_teps_evaluated, const int32_t *d_block_off, int nblk,
                 int win, const int32_t *d_count, int64_t F, int64_t *d_dl_counts, hipStream_t st)
{
    hipLaunchKernelGGL(dlosd_counts_kernel, dim3(grid_for(F, 256, 1024)), dim3(256), 0, st, d_deep_limit, d_success, d_global_min, d_truth, d_teps_evaluated,
                       d_block_off, nblk, win, d_count, (long long)F, reinterpret_cast<unsigned long long *>(d_dl_counts));
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // namespace ldpc

extern "C" {

int ldpc_pack_bits(ldpc_ctx *ctx, const void *d_bits, int32_t elem_size, int64_t B, uint64_t *d_words, void *stream)
{
    if (!ctx || !d_bits || !d_words || B < 0) return fail(LDPC_E_ARG, "ldpc_pack_bits: bad arguments");
    if (B == 0) return LDPC_OK;
    const int n = ctx->code.n, words = (n + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    auto *out = reinterpret_cast<unsigned long long *>(d_words);
    const dim3 g(grid_for(B * words, 4, 8192)), b(256);
    switch (elem_size) {
    case 1: hipLaunchKernelGGL(pack_bits_kernel<unsigned char>, g, b, 0, st, (const unsigned char *)d_bits, (long long)B, n, words, out); break;
    case 4: hipLaunchKernelGGL(pack_bits_kernel<int>, g, b, 0, st, (const int *)d_bits, (long long)B, n, words, out); break;
    case 8: hipLaunchKernelGGL(pack_bits_kernel<long long>, g, b, 0, st, (const long long *)d_bits, (long long)B, n, words, out); break;
    default: return fail(LDPC_E_ARG, "ldpc_pack_bits: elem_size %d (want 1, 4 or 8)", elem_size);
    }
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

int ldpc_unpack_bits(ldpc_ctx *ctx, const uint64_t *d_words, int64_t B, void *d_bits, int32_t elem_size, void *stream)
{
    if (!ctx || !d_bits || !d_words || B < 0) return fail(LDPC_E_ARG, "ldpc_unpack_bits: bad arguments");
    if (B == 0) return LDPC_OK;
    const int n = ctx->code.n, words = (n + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    auto *in = reinterpret_cast<const unsigned long long *>(d_words);
    const dim3 g(grid_for(B * n, 256, 8192)), b(256);
    switch (elem_size) {
    case 1: hipLaunchKernelGGL(unpack_bits_kernel<unsigned char>, g, b, 0, st, in, (long long)B, n, words, (unsigned char *)d_bits); break;
    case 4: hipLaunchKernelGGL(unpack_bits_kernel<int>, g, b, 0, st, in, (long long)B, n, words, (int *)d_bits); break;
    case 8: hipLaunchKernelGGL(unpack_bits_kernel<long long>, g, b, 0, st, in, (long long)B, n, words, (long long *)d_bits); break;
    default: return fail(LDPC_E_ARG, "ldpc_unpack_bits: elem_size %d (want 1, 4 or 8)", elem_size);
    }
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // extern "C"
