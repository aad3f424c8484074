// Device-side frame generator: counter-based AWGN / Rayleigh frames (ldpc_gen_frames, include/ldpc_osd.h).
// Replaces, on the device, Testing_data_gen_128/data_generating.py:13-51 and Training_data_gen_128/data_generating.py:41-81:
// random message . G, BPSK 0 -> +1, v = mean (. a) + sigma z, y = bit ? -v : v, and the packed labels.
//
// Frame i of a set is a pure function of (seed, frame0 + i, channel parameters): every random word is one output word
// of Philox4x32-10 (Salmon et al., SC'11) under key (seed low, seed high) and counter (idx low, idx high, block, stream)
// -- the stream contract of the header and of DESIGN.md section 3.  Nothing is kept between calls, nothing per stream.
//
// Mapping: one lane per NOISE BLOCK, i.e. four consecutive columns of one frame; a workgroup of 256 lanes owns groups of whole
// frames (up to 2048 blocks a group, see launch_gen) and walks a group's blocks 256 at a time.  Per group of frames:
//   1. the message words of the group's frames go to LDS (one Philox call per 128 message bits),
//   2. every lane forms its four code bits as the parity of message & column of G (columns packed over k, transposed so
//      that consecutive lanes read consecutive words: in LDS where they fit, from global memory otherwise), draws its four
//      normals, fades, signs and stores them -- one 16-byte store when n is a multiple of 4 and y is 16-byte aligned --,
//   3. one lane per label word collects sixteen 4-bit groups from LDS.
// No atomics, no scratch memory, one launch: capturable.
#include <math.h>

#include "ldpc_internal.h"

namespace ldpc {

constexpr int kGenThreads = 256;
constexpr int kGenItems = 2048;            // lane items (noise blocks) of a group of frames at most, where one frame has fewer
constexpr size_t kGenLdsG = 48u * 1024u;   // packed G stays in LDS up to this many bytes (CCSDS (128,64): 1 KiB; wimax (1056,880): 116 KiB, global)
constexpr size_t kGenLdsMax = 64u * 1024u;

struct Philox4 {
    uint32_t x, y, z, w;
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return {c0, c1, c2, c3};
}

// (0, 1]: x = 0xFFFFFFFF converts to 2^32 and gives 1 (radius 0), x = 0 gives 2^-33
__device__ __forceinline__ float gen_ua(uint32_t x) { return (float)x * 2.3283064365386963e-10f + 1.1641532182693481e-10f; }
// [0, 1), exact
__device__ __forceinline__ float gen_tb(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-08f; }

__device__ __forceinline__ void gen_pair(uint32_t xa, uint32_t xb, float *za, float *zb)
{
    const float r = sqrtf(-2.0f * logf(gen_ua(xa)));
    float s, c;
    sincospif(2.0f * gen_tb(xb), &s, &c);
    *za = r * c;
    *zb = r * s;
}

struct GenArgs {
    uint32_t k0, k1;            // Philox key
    unsigned long long frame0;
    long long B;
    int n, k, nb, kw, kb, fpw, words;   // nb = ceil(n/4) noise blocks, kw = ceil(k/32) message words, kb = ceil(k/128)
    float sigma, mean;
    int all_zeros, rayleigh, vec4;
    unsigned long long fade_len;
    long long groups;
};

// Gt: [kw][4][nb] u32 -- word w of column 4 b + j of G (bit i = G[32 w + i][4 b + j]), zero for columns >= n and rows >= k
template <bool G_LDS>
__global__ __launch_bounds__(kGenThreads) void gen_frames_kernel(GenArgs a, const uint32_t *__restrict__ Gt, float *__restrict__ y,
                                                                 unsigned long long *__restrict__ label)
{
    extern __shared__ uint32_t lds[];
    const int tid = threadIdx.x;
    const int gwords = a.kw * 4 * a.nb, mw = a.kb * 4;
    uint32_t *sG = lds;                                        // [gwords] with G_LDS
    uint32_t *sMsg = lds + (G_LDS ? gwords : 0);               // [fpw][mw]
    unsigned char *sNib = reinterpret_cast<unsigned char *>(sMsg + a.fpw * mw);   // [fpw][nb] four code bits of a block
    const bool coded = !a.all_zeros;
    if (G_LDS && coded)
        for (int i = tid; i < gwords; i += kGenThreads) sG[i] = Gt[i];
    const uint32_t *G = G_LDS ? sG : Gt;
    const int items = a.fpw * a.nb;

    for (long long g = blockIdx.x; g < a.groups; g += gridDim.x) {
        const long long f0 = g * a.fpw;
        __syncthreads();   // sG is filled; sMsg / sNib of the previous group are read
        if (coded) {       // stream 0: block j of frame f = message bits 128 j ..
            for (int t = tid; t < a.fpw * a.kb; t += kGenThreads) {
                const int fl = t / a.kb, j = t - fl * a.kb;
                const unsigned long long idx = a.frame0 + (unsigned long long)(f0 + fl);
                const Philox4 m = philox4x32_10((uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)j, 0u, a.k0, a.k1);
                const uint32_t w[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int bit0 = 128 * j + 32 * q, left = a.k - bit0;   // bits at or beyond k are discarded
                    sMsg[fl * mw + 4 * j + q] = left >= 32 ? w[q] : (left > 0 ? w[q] & ((1u << left) - 1u) : 0u);
                }
            }
            __syncthreads();
        }
        for (int it = tid; it < items; it += kGenThreads) {
            const int fl = it / a.nb, b = it - fl * a.nb;
            const long long f = f0 + fl;
            if (f >= a.B) continue;
            uint32_t bits = 0;
            if (coded) {
                uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0;
                const uint32_t *msg = sMsg + fl * mw;
                for (int w = 0; w < a.kw; ++w) {
                    const uint32_t m = msg[w];
                    const uint32_t *col = G + (size_t)w * 4 * a.nb + b;
                    p0 ^= m & col[0]; p1 ^= m & col[a.nb]; p2 ^= m & col[2 * a.nb]; p3 ^= m & col[3 * a.nb];
                }
                bits = (__popc(p0) & 1) | ((__popc(p1) & 1) << 1) | ((__popc(p2) & 1) << 2) | ((__popc(p3) & 1) << 3);
                if (label) sNib[it] = (unsigned char)bits;
            }
            if (!y) continue;
            const unsigned long long idx = a.frame0 + (unsigned long long)f;
            const Philox4 x = philox4x32_10((uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)b, 1u, a.k0, a.k1);   // stream 1
            float z[4], v[4];
            gen_pair(x.x, x.y, &z[0], &z[1]);
            gen_pair(x.z, x.w, &z[2], &z[3]);
            if (a.rayleigh) {   // stream 2: one amplitude per fading block of fade_len samples of the global sample sequence
                const unsigned long long s0 = idx * (unsigned long long)a.n + 4ull * b;
                unsigned long long qprev = ~0ull;
                float amp = 0.0f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned long long q = (s0 + j) / a.fade_len;
                    if (j == 0 || q != qprev) {
                        const Philox4 h = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), 0u, 2u, a.k0, a.k1);
                        amp = sqrtf(-logf(gen_ua(h.x)));
                        qprev = q;
                    }
                    v[j] = a.mean * amp + a.sigma * z[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = a.mean + a.sigma * z[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (bits >> j) & 1 ? -v[j] : v[j];
            float *row = y + (size_t)f * a.n + 4 * b;
            if (a.vec4) {
                *reinterpret_cast<float4 *>(row) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * b + j < a.n) row[j] = v[j];
            }
        }
        if (label) {
            if (coded) __syncthreads();
            for (int t = tid; t < a.fpw * a.words; t += kGenThreads) {
                const int fl = t / a.words, w = t - fl * a.words;
                const long long f = f0 + fl;
                if (f >= a.B) continue;
                unsigned long long word = 0;
                if (coded) {
                    const unsigned char *nib = sNib + fl * a.nb;
                    for (int i = 0; i < 16; ++i) {
                        const int blk = 16 * w + i;
                        if (blk < a.nb) word |= (unsigned long long)nib[blk] << (4 * i);
                    }
                }
                label[(size_t)f * a.words + w] = word;
            }
        }
    }
}

// The transposed packed G of the context (see gen_frames_kernel); uploaded once by ldpc_ctx_create.
int gen_ctx_init(ldpc_ctx *ctx)
{
    const ldpc_code &c = ctx->code;
    const int nb = (c.n + 3) / 4, kw = (c.k + 31) / 32;
    std::vector<uint32_t> t((size_t)kw * 4 * nb, 0u);
    for (int r = 0; r < c.k; ++r)
        for (int v = 0; v < c.n; ++v)
            if (c.G[(size_t)r * c.n + v] & 1) t[((size_t)(r >> 5) * 4 + (v & 3)) * nb + (v >> 2)] |= 1u << (r & 31);
    LDPC_HIP(hipMalloc((void **)&ctx->d_gen_G, sizeof(uint32_t) * (t.size() ? t.size() : 1)));
    if (!t.empty()) LDPC_HIP(hipMemcpy(ctx->d_gen_G, t.data(), sizeof(uint32_t) * t.size(), hipMemcpyHostToDevice));
    return LDPC_OK;
}

void gen_ctx_release(ldpc_ctx *ctx)
{
    (void)hipFree(ctx->d_gen_G);
    ctx->d_gen_G = nullptr;
}

int launch_gen(ldpc_ctx *ctx, const ldpc_gen_params *p, int64_t B, float *d_y, uint64_t *d_label_bits, hipStream_t st)
{
    const ldpc_code &c = ctx->code;
    GenArgs a;
    a.k0 = (uint32_t)p->seed; a.k1 = (uint32_t)(p->seed >> 32);
    a.frame0 = (unsigned long long)p->frame0;
    a.B = B;
    a.n = c.n; a.k = c.k;
    a.nb = (c.n + 3) / 4; a.kw = (c.k + 31) / 32; a.kb = (c.k + 127) / 128;
    // Frames per group: up to kGenItems lane items, so that a pass between two barriers keeps every lane busy for several
    // independent blocks (and the message draws fill more than a handful of lanes); fewer, down to one pass of the
    // workgroup, when the batch is too small to give every CU four groups that way.  The frames do not depend on it.
    const long long fpw_lo = a.nb >= kGenThreads ? 1 : kGenThreads / a.nb, fpw_hi = a.nb >= kGenItems ? 1 : kGenItems / a.nb;
    const long long fpw_want = (B + (long long)ctx->cu_count * 4 - 1) / ((long long)ctx->cu_count * 4);
    a.fpw = (int)(fpw_want < fpw_lo ? fpw_lo : fpw_want > fpw_hi ? fpw_hi : fpw_want);
    a.words = (c.n + 63) / 64;
    a.sigma = p->sigma; a.mean = p->mean;
    a.all_zeros = (p->flags & LDPC_GEN_F_ALL_ZEROS) != 0;
    a.rayleigh = (p->flags & LDPC_GEN_F_RAYLEIGH) != 0;
    a.vec4 = c.n % 4 == 0 && (reinterpret_cast<uintptr_t>(d_y) & 15) == 0;
    a.fade_len = a.rayleigh ? (unsigned long long)p->fade_len : 1ull;
    a.groups = (B + a.fpw - 1) / a.fpw;
    const size_t gbytes = sizeof(uint32_t) * (size_t)a.kw * 4 * a.nb;
    const size_t own = sizeof(uint32_t) * (size_t)a.fpw * a.kb * 4 + (((size_t)a.fpw * a.nb + 3) & ~(size_t)3);
    const bool g_lds = gbytes <= kGenLdsG && gbytes + own <= kGenLdsMax;
    const size_t lds = own + (g_lds ? gbytes : 0);
    if (lds > kGenLdsMax)
        return fail(LDPC_E_UNSUPPORTED, "ldpc_gen_frames: a frame of this code needs %zu bytes of LDS (limit %zu)", lds, kGenLdsMax);
    const long long cap = (long long)ctx->cu_count * 8;   // resident workgroups walk the groups: G is staged once per workgroup
    const dim3 grid((unsigned)(a.groups < cap ? a.groups : cap)), block(kGenThreads);
    auto *lab = reinterpret_cast<unsigned long long *>(d_label_bits);
    if (g_lds) hipLaunchKernelGGL(gen_frames_kernel<true>, grid, block, lds, st, a, ctx->d_gen_G, d_y, lab);
    else hipLaunchKernelGGL(gen_frames_kernel<false>, grid, block, lds, st, a, ctx->d_gen_G, d_y, lab);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // namespace ldpc
