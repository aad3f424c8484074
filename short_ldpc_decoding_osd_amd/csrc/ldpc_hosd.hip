// H-form ordered-statistics primitives for the DL-OSD stage on gfx950 (MI355X), in three families: (128,64) (ldpc_hosd_*)
// here, any shape with k, n - k <= 64 (ldpc_hosdx_*) in ldpc_hosdx.h, high-rate codes and an H with redundant rows
// (ldpc_hosdw_*) in ldpc_hosdw.h.  A family owns what differs: its front end, its LDS plan and columns, its metric and its
// per-frame set-up.  The block scans themselves -- the two forms of the search, the sliding-window scan -- are written once
// in ldpc_hosd_scan.h over a family's traits, and the host side of all nine entry points once at the end of this file.
//
// Reference (paths relative to LDPC_128/DL_OSD_Testing_serial/ of the reference):
//   mag_input_gen / check_matrix_reorder   ordered_statistics_decoding.py:25-41
//   identify_mrb / full_gf2elim            ordered_statistics_decoding.py:43-80, 222-257
//   acquire_min / sliding_osd              ordered_statistics_decoding.py:153-186
//
// The dual of ldpc_osd.hip: positions are sorted by ASCENDING reliability, the elimination runs
// on the permuted H (-> [I | M], the identity part on the least reliable independent positions),
// a candidate is [M . mrb, mrb], and the scan is organised in caller-defined TEP blocks whose
// minima feed the reference's sliding-window network on the host.  Two separate LLR inputs: one
// orders the positions and supplies the starting MRB hard decisions (the CNN-refined values in
// the reference), the other (trajectory row 0) supplies the metric.  One frame per wavefront.
#include <tuple>

#include "ldpc_internal.h"
#include "ldpc_wave.h"
#include "ldpc_hosd_scan.h"
#include "ldpc_dlosd_check.h"   // hosd_family_refusal: the sentence of each family
#include "ldpc_dlosd_stage.h"   // HosdStage: the counted launches of ldpc_dlosd_pipeline_run

namespace ldpc {

struct __attribute__((aligned(16))) HFrontLds {
    RankLds rank;              // reliability sort (bucket_ranks, ldpc_wave.h)
    u64 colbuf[64];            // M columns in updated MRB order, bit = physical row
    unsigned mask[4];          // which sorted positions ended up in the MRB
    unsigned char lri[128];    // sorted position -> original bit
};

template <class... COUNT>   // (the counted form: ldpc_wave.h)
__global__ __launch_bounds__(256) void hosd_front_kernel(const float *__restrict__ x, long long F,
                                                         const u64 *__restrict__ Hcols,
                                                         unsigned char *__restrict__ lri_out,
                                                         unsigned char *__restrict__ uidx_out, u64 *__restrict__ M_out,
                                                         int *__restrict__ nswaps, COUNT... count)
{
    if constexpr (kCounted<COUNT...>) {
        F = counted_frames(F, count...);
        if ((long long)blockIdx.x * 4 >= F) return;   // (the grid is sized by the capacity, not by the count)
    }
    __shared__ HFrontLds lds[4];
    const int lane = threadIdx.x & 63;
    HFrontLds &L = lds[threadIdx.x >> 6];
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);

    for (long long f = wave; f < F; f += (long long)gridDim.x * 4) {
        // ---- mag_input_gen (:25-28): rank in ascending |x|, ties -> lower index ------------
        // ascending order of (|x| bits, index) = descending order of the complemented key, buckets mirrored
        // (hosd_sort_ascending with n = 128 compiles to other code for this kernel, so the sort stays spelt out here)
        const unsigned a1 = __float_as_uint(x[f * 128 + lane]) & 0x7FFFFFFFu, a2 = __float_as_uint(x[f * 128 + 64 + lane]) & 0x7FFFFFFFu;
        const float bs = bucket_scale(a1, a2);
        int r1, r2;
        bucket_ranks(L.rank, ~(((u64)a1 << 32) | (unsigned)lane), ~(((u64)a2 << 32) | (unsigned)(lane + 64)), 63 - bucket_of(a1, bs),
                     63 - bucket_of(a2, bs), lane, r1, r2);
        L.lri[r1] = (unsigned char)lane;
        L.lri[r2] = (unsigned char)(lane + 64);
        if (lane < 4) L.mask[lane] = 0;
        wave_fence();
        // ---- H with columns in sorted order (:38-40), column-major, then full_gf2elim (:222-257)
        const int s1 = L.lri[lane], s2 = L.lri[lane + 64];
        u64 C1 = Hcols[s1];
        u64 C2 = Hcols[s2];
        int rho = lane, idx1 = lane, idx2 = lane + 64;
        const int ns = ge_columns(C1, C2, rho, idx1, idx2, lane, nullptr);
        // ---- identify_mrb (:58-69): LRB = index_order[:64] as left by the elimination, MRB sorted
        atomicOr(&L.mask[idx2 >> 5], 1u << (idx2 & 31));
        wave_fence();
        const unsigned m[4] = {L.mask[0], L.mask[1], L.mask[2], L.mask[3]};
        const int rankM = below_mask(m, idx2);          // updated MRB position of column 64 + lane
        L.colbuf[rankM] = C2;
        wave_fence();
        // rows of updated_M: transpose to (lane = physical row, bit = MRB position), then logical row
        // r = the row whose pivot sits in column r = physical row rho[r]
        const u64 R = transpose64(L.colbuf[lane], lane);
        M_out[f * 64 + lane] = shfl64(R, rho);
        lri_out[f * 128 + lane] = (unsigned char)s1;
        lri_out[f * 128 + 64 + lane] = (unsigned char)s2;
        uidx_out[f * 128 + lane] = (unsigned char)idx1;
        uidx_out[f * 128 + 64 + rankM] = (unsigned char)idx2;
        if (nswaps && lane == 0) nswaps[f] = ns;
        wave_fence();
    }
}

// RUNS: the per-thread-run form (a small table: 23 KiB of LDS, 6 workgroups per CU -- the kernel answers to occupancy: 0.34 ms at
// 4 workgroups per CU with 4-byte TEPs and 1024 block keys, 0.31 at 5); otherwise rounds 1-2's work items (25.7 KiB).
template <bool RUNS>
struct __attribute__((aligned(16))) HSearchLds {
    float lut[16][256];   // lut[b][v]: partial metric of discrepancy byte b (updated positions 8b..8b+7)
    u64 Mcol[64];         // column j of updated_M (bit r = M[r][j])
    float w[128];         // |metric_llr| in updated order
    u64 keys[RUNS ? kHosdRunBlocks : kHosdMaxBlocks];   // per block: (metric bits << 32) | TEP index, minimum = first minimum
    u64 hgL, hgM, mrb0, DL0, best, cw[2];
    int ticket, heavy;
    float truth;          // the label's metric (hosd_frame_setup with labels)
    unsigned char o[128]; // original bit index of updated position p
    int boff[RUNS ? kHosdRunBlocks + 1 : 1];            // block_off, once per workgroup
    unsigned short tl[RUNS ? kHosdLdsTeps : 2];         // the TEP table, once per workgroup: x | y << 6 | weight << 12
};

template <class LDS>
__device__ __forceinline__ float hosd_cost(const LDS &L, u64 DL, u64 DM)
{
    float acc = lut_byte<0>(L.lut, DL);
    acc = acc + lut_byte<1>(L.lut, DL); acc = acc + lut_byte<2>(L.lut, DL); acc = acc + lut_byte<3>(L.lut, DL);
    acc = acc + lut_byte<4>(L.lut, DL); acc = acc + lut_byte<5>(L.lut, DL); acc = acc + lut_byte<6>(L.lut, DL);
    acc = acc + lut_byte<7>(L.lut, DL);
    acc = acc + lut_byte<0>(&L.lut[8], DM); acc = acc + lut_byte<1>(&L.lut[8], DM); acc = acc + lut_byte<2>(&L.lut[8], DM);
    acc = acc + lut_byte<3>(&L.lut[8], DM); acc = acc + lut_byte<4>(&L.lut[8], DM); acc = acc + lut_byte<5>(&L.lut[8], DM);
    acc = acc + lut_byte<6>(&L.lut[8], DM); acc = acc + lut_byte<7>(&L.lut[8], DM);
    return acc;
}

template <class LDS>
__device__ __forceinline__ void hosd_apply(const LDS &L, uchar4 s, u64 &DL, u64 &DM)
{
    if (s.w > 0) { DL ^= L.Mcol[s.x]; DM ^= 1ull << s.x; }
    if (s.w > 1) { DL ^= L.Mcol[s.y]; DM ^= 1ull << s.y; }
    if (s.w > 2) { DL ^= L.Mcol[s.z]; DM ^= 1ull << s.z; }
}

// Per-frame set-up shared by the block scans (hosd_search_kernel, hosd_sliding_kernel): values in updated order, hard
// decisions, M columns, block keys reset, byte LUTs, the order-0 discrepancies DL0 / DM0 and (with labels) the label's metric
// (L.truth, and truth[f] where truth is given).
// On return every thread sees the LUTs, the M columns and the keys of blocks 0..nblk-1 reset to ~0.
template <class LDS>
__device__ __forceinline__ void hosd_frame_setup(LDS &L, const HScanIn &in, long long f, float *__restrict__ truth, u64 &DL0, u64 &DM0)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *__restrict__ xo = in.xo, *__restrict__ xm = in.xm;
    const unsigned char *__restrict__ lri = in.lri, *__restrict__ uidx = in.uidx;
    const u64 *__restrict__ Mrows = in.Mrows, *__restrict__ label = in.label;
    const int nblk = in.nblk;
    // ---- phase 0: values in updated order (:172-176), hard decisions, M columns, key reset --------
    if (tid < 128) {
        const int o = lri[f * 128 + uidx[f * 128 + tid]];
        const float m = xm[f * 128 + o];
        L.o[tid] = (unsigned char)o;
        L.w[tid] = __builtin_fabsf(m);
        const u64 hg = __ballot(!(m > 0.0f));                       // order_hard_original (:180)
        if (wave == 0) { if (lane == 0) L.hgL = hg; }
        else {
            const u64 h0 = __ballot(!(xo[f * 128 + o] > 0.0f));      // initial_mrb (:186-187)
            if (lane == 0) { L.hgM = hg; L.mrb0 = h0; }
        }
    } else if (wave == 2) {
        L.Mcol[lane] = transpose64(Mrows[f * 64 + lane], lane);
    } else {
        if (lane == 0) { L.ticket = 0; L.best = ~0ull; L.cw[0] = 0; L.cw[1] = 0; }
    }
    for (int b = tid; b < nblk; b += 256) L.keys[b] = ~0ull;
    __syncthreads();
    // ---- phase 1: byte LUTs (four per wavefront), order-0 discrepancy of the LRB part (:155,:159) --
    build_byte_luts<4>(&L.lut[4 * wave], &L.w[32 * wave], lane);
    if (wave == 0) {
        const u64 d = wave_xor64(((L.mrb0 >> lane) & 1) ? L.Mcol[lane] : 0ull) ^ L.hgL;
        if (lane == 0) L.DL0 = d;
    }
    __syncthreads();
    DL0 = L.DL0; DM0 = L.mrb0 ^ L.hgM;
    if (label && wave == 1) {
        const u64 l0 = label[f * 2], l1 = label[f * 2 + 1];
        const int o1 = L.o[lane], o2 = L.o[64 + lane];
        const u64 labL = __ballot(((o1 < 64 ? l0 : l1) >> (o1 & 63)) & 1);
        const u64 labM = __ballot(((o2 < 64 ? l0 : l1) >> (o2 & 63)) & 1);
        const float t = hosd_cost(L, labL ^ L.hgL, labM ^ L.hgM);     // (:181-183)
        if (lane == 0) { if (truth) truth[f] = t; L.truth = t; }
    }
}

// The (128,64) family for the scans of ldpc_hosd_scan.h: one-word columns, a constant shape, TEP positions of 6 bits.  The
// packed table takes a position modulo 64, so a position beyond 63 (the caller's error) cannot reach the weight field.
struct Hosd128 {
    template <bool RUNS> using Lds = HSearchLds<RUNS>;
    static constexpr int kPosBits = 6;
    static __device__ __forceinline__ unsigned pos(unsigned char v) { return v & 63; }
    template <class LDS> static __device__ __forceinline__ float cost(const LDS &L, u64 DL, u64 DM, HShape128) { return hosd_cost(L, DL, DM); }
    template <class LDS>
    static __device__ __forceinline__ void setup(LDS &L, HShape128, const HScanIn &in, long long f, float *__restrict__ truth, u64 &DL0, u64 &DM0)
    {
        hosd_frame_setup(L, in, f, truth, DL0, DM0);
    }
};

template <bool RUNS>
__global__ __launch_bounds__(256) void hosd_search_kernel(const float *__restrict__ xo, const float *__restrict__ xm,
                                                          long long F, const unsigned char *__restrict__ lri,
                                                          const unsigned char *__restrict__ uidx,
                                                          const u64 *__restrict__ Mrows, const uchar4 *__restrict__ teps,
                                                          const int *__restrict__ block_off, int nblk,
                                                          const u64 *__restrict__ label, float *__restrict__ block_min,
                                                          int *__restrict__ block_arg, float *__restrict__ truth,
                                                          u64 *__restrict__ cw_out, float *__restrict__ metric_out,
                                                          int *__restrict__ best_out)
{
    __shared__ Hosd128::Lds<RUNS> L;
    hosd_search_body<Hosd128, RUNS>(L, HShape128(), {xo, xm, F, lri, uidx, Mrows, teps, block_off, nblk, label}, block_min, block_arg,
                                    {truth, cw_out, metric_out, best_out});
}

HOSD_SLIDING_KERNEL(hosd_sliding_kernel, Hosd128, HOSD_NO_SHAPE_PARAMS, HShape128 sh)

}  // namespace ldpc

#include "ldpc_hosdx.h"   // the any-shape family (k, n - k <= 64): its front end, columns and set-up
#include "ldpc_hosdw.h"   // the wide family (k up to 127, an H of up to 127 rows of rank <= 64): the same
#include "ldpc_fcn.h"     // training of the sliding-window classifier: window builder, loss and gradient

namespace ldpc {

// The H columns for every shape the H-form kernels serve.  ldpc_hosdw_* take n <= 128, an H of 1 <= R <= 127 rows as given
// and rank 1 <= n - k <= 64 (two-word R-bit columns); of these ldpc_hosdx_* take 1 <= k <= 64 and an H of exactly n - k
// rows (m-bit words), and ldpc_hosd_* (128,64) alone.
int hosd_ctx_init(ldpc_ctx *ctx)
{
    const ldpc_code &c = ctx->code;
    ctx->hosd_ok = ctx->hosdx_ok = ctx->hosdw_ok = false;
    const int rank = c.n - c.k;
    if (c.n > 128 || c.m < 1 || c.m > 127 || rank < 1 || rank > 64 || rank > c.m || c.k < 1 || c.k > 127)
        return LDPC_OK;                                                                     // entry points will report UNSUPPORTED
    std::vector<u64> wide(256, 0);
    for (int r = 0; r < c.m; ++r)
        for (int v = 0; v < c.n; ++v)
            if (c.H[(size_t)r * c.n + v]) wide[2 * v + (r >> 6)] |= 1ull << (r & 63);
    LDPC_HIP(hipMalloc((void **)&ctx->d_HcolsW, sizeof(u64) * 256));
    LDPC_HIP(hipMemcpy(ctx->d_HcolsW, wide.data(), sizeof(u64) * 256, hipMemcpyHostToDevice));
    ctx->hosdw_ok = true;
    if (c.k > 64 || c.m != rank) return LDPC_OK;
    std::vector<u64> cols(128, 0);
    for (int v = 0; v < c.n; ++v) cols[v] = wide[2 * v];
    LDPC_HIP(hipMalloc((void **)&ctx->d_Hcols, sizeof(u64) * 128));
    LDPC_HIP(hipMemcpy(ctx->d_Hcols, cols.data(), sizeof(u64) * 128, hipMemcpyHostToDevice));
    ctx->hosdx_ok = true;
    ctx->hosd_ok = c.n == 128 && c.m == 64 && c.k == 64;
    return LDPC_OK;
}

void hosd_ctx_release(ldpc_ctx *ctx)
{
    (void)hipFree(ctx->d_Hcols);
    (void)hipFree(ctx->d_HcolsW);
    ctx->d_Hcols = ctx->d_HcolsW = nullptr;
}

static unsigned grid_for(int64_t F, int waves_per_block)
{
    const int64_t want = (F + waves_per_block - 1) / waves_per_block;
    return (unsigned)(want < 1 ? 1 : (want < 8192 ? want : 8192));
}

// ---- the host side of the nine entry points, once.  A family supplies: whether the context serves the code and the text
// of its refusal (check), its H-column table (hcols), its kernels, and the shape arguments they take after F (front_shape /
// scan_shape).  `who` is the name of the extern "C" entry point, for the error texts.
struct HostHosd128 {
    static int check(const ldpc_ctx *ctx, const char *)
    {
        if (ctx->hosd_ok) return LDPC_OK;
        return hosd_family_refusal(ctx, LDPC_HOSD_FAMILY_128, nullptr);
    }
    static const uint64_t *hcols(const ldpc_ctx *ctx) { return ctx->d_Hcols; }
    static constexpr auto front = hosd_front_kernel<>;
    static constexpr auto front_counted = hosd_front_kernel<const int *>;
    static constexpr auto sliding = hosd_sliding_kernel<>;
    static constexpr auto sliding_counted = hosd_sliding_kernel<const int *>;
    template <bool RUNS> static constexpr auto search = hosd_search_kernel<RUNS>;
    static std::tuple<> front_shape(const ldpc_code &) { return {}; }
    static std::tuple<> scan_shape(const ldpc_code &) { return {}; }
};

struct HostHosdX {
    static int check(const ldpc_ctx *ctx, const char *who)
    {
        if (ctx->hosdx_ok) return LDPC_OK;
        return hosd_family_refusal(ctx, LDPC_HOSD_FAMILY_X, who);
    }
    static const uint64_t *hcols(const ldpc_ctx *ctx) { return ctx->d_Hcols; }
    static constexpr auto front = hosdx_front_kernel<>;
    static constexpr auto front_counted = hosdx_front_kernel<const int *>;
    static constexpr auto sliding = hosdx_sliding_kernel<>;
    static constexpr auto sliding_counted = hosdx_sliding_kernel<const int *>;
    template <bool RUNS> static constexpr auto search = hosdx_search_kernel<RUNS>;
    static std::tuple<int, int> front_shape(const ldpc_code &c) { return {c.n, c.m}; }
    static std::tuple<int, int> scan_shape(const ldpc_code &c) { return {c.n, c.n - c.k}; }   // (n - k == c.m wherever hosdx_ok holds)
};

struct HostHosdW {
    static int check(const ldpc_ctx *ctx, const char *who)
    {
        if (ctx->hosdw_ok) return LDPC_OK;
        return hosd_family_refusal(ctx, LDPC_HOSD_FAMILY_W, who);
    }
    static const uint64_t *hcols(const ldpc_ctx *ctx) { return ctx->d_HcolsW; }
    static constexpr auto front = hosdw_front_kernel<>;
    static constexpr auto front_counted = hosdw_front_kernel<const int *>;
    static constexpr auto sliding = hosdw_sliding_kernel<>;
    static constexpr auto sliding_counted = hosdw_sliding_kernel<const int *>;
    template <bool RUNS> static constexpr auto search = hosdw_search_kernel<RUNS>;
    static std::tuple<int, int, int> front_shape(const ldpc_code &c) { return {c.n, c.m, c.n - c.k}; }
    static std::tuple<int, int> scan_shape(const ldpc_code &c) { return {c.n, c.n - c.k}; }
};

// kernel(head..., shape..., tail...) on `blocks` workgroups of 256 threads
template <class K, class... H, class... S, class... T>
static void hosd_launch(K kernel, unsigned blocks, void *stream, const std::tuple<H...> &head, const std::tuple<S...> &shape,
                        const std::tuple<T...> &tail)
{
    std::apply([&](const auto &...a) { hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a...); },
               std::tuple_cat(head, shape, tail));
}

static const u64 *w64(const uint64_t *p) { return reinterpret_cast<const u64 *>(p); }
static u64 *w64(uint64_t *p) { return reinterpret_cast<u64 *>(p); }

// the classifier of the sliding scans and of ldpc_fcn_grad: the kernel argument (its weight count: ldpc_hosd_limits.h)
static SlideFcnArg slide_fcn_arg(const float *fcn_weights, int win)
{
    const int d = win + 1;
    SlideFcnArg w = {};
    for (int i = 0; i < d * d; ++i) w.w1[i] = fcn_weights[i];
    for (int i = 0; i < 2 * d; ++i) w.w2[i] = fcn_weights[d * d + i];
    return w;
}

template <class FAM>
static int hosd_front(const char *who, ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint8_t *d_lri, uint8_t *d_uidx, uint64_t *d_M,
                      int32_t *d_nswaps, void *stream, const int32_t *d_count = nullptr)
{
    if (!ctx || F < 0) return fail(LDPC_E_ARG, "%s: bad arguments (ctx %p, F %lld)", who, (void *)ctx, (long long)F);
    if (F > 0)
        if (int rc = first_null(who, {{"d_order_llr", d_order_llr}, {"d_lri", d_lri}, {"d_uidx", d_uidx}, {"d_M", d_M}})) return rc;
    if (int rc = FAM::check(ctx, who)) return rc;
    if (F == 0) return LDPC_OK;
    const auto head = std::make_tuple(d_order_llr, (long long)F);
    const auto tail = std::make_tuple(w64(FAM::hcols(ctx)), d_lri, d_uidx, w64(d_M), d_nswaps);
    // (d_count: the counted form, on min(*d_count, F) frames -- ldpc_dlosd_pipeline_run alone)
    if (d_count)
        hosd_launch(FAM::front_counted, grid_for(F, 4), stream, head, FAM::front_shape(ctx->code), std::tuple_cat(tail, std::make_tuple((const int *)d_count)));
    else
        hosd_launch(FAM::front, grid_for(F, 4), stream, head, FAM::front_shape(ctx->code), tail);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

template <class FAM>
static int hosd_search(const char *who, ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                       const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off, int32_t nblk,
                       const uint64_t *d_label_bits, float *d_block_min, int32_t *d_block_arg, float *d_truth, uint64_t *d_cw,
                       float *d_metric, int32_t *d_best, void *stream)
{
    if (!ctx || F < 0 || nblk < 0)
        return fail(LDPC_E_ARG, "%s: bad arguments (ctx %p, F %lld, nblk %d)", who, (void *)ctx, (long long)F, (int)nblk);
    if (F > 0) {
        if (int rc = first_null(who, {{"d_order_llr", d_order_llr}, {"d_metric_llr", d_metric_llr}, {"d_lri", d_lri},
                                      {"d_uidx", d_uidx}, {"d_M", d_M}, {"d_block_off", d_block_off}})) return rc;
        if (nblk > 0)     // (the kernels read d_teps[0 .. d_block_off[nblk]), device data)
            if (int rc = first_null(who, {{"d_teps", d_teps}, {"d_block_min", d_block_min}})) return rc;
    }
    if (d_truth && !d_label_bits) return fail(LDPC_E_ARG, "%s: d_truth needs d_label_bits", who);
    if (int rc = FAM::check(ctx, who)) return rc;
    if (nblk > kHosdMaxBlocks) return fail(LDPC_E_UNSUPPORTED, "%s: %d TEP blocks, at most %d", who, nblk, kHosdMaxBlocks);
    if (F == 0) return LDPC_OK;
    // (the TEP table's size is device data: both forms are launched and one of them returns at once)
    const auto head = std::make_tuple(d_order_llr, d_metric_llr, (long long)F);
    const auto tail = std::make_tuple(d_lri, d_uidx, w64(d_M), reinterpret_cast<const uchar4 *>(d_teps), d_block_off, (int)nblk,
                                      w64(d_label_bits), d_block_min, d_block_arg, d_truth, w64(d_cw), d_metric, d_best);
    hosd_launch(FAM::template search<true>, grid_for(F, 1), stream, head, FAM::scan_shape(ctx->code), tail);
    hosd_launch(FAM::template search<false>, grid_for(F, 1), stream, head, FAM::scan_shape(ctx->code), tail);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

template <class FAM>
static int hosd_sliding(const char *who, ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                        const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off, int32_t nblk,
                        int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights, int32_t group,
                        const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min, float *d_truth, uint8_t *d_success,
                        uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_teps_evaluated, void *stream,
                        const int32_t *d_count = nullptr)
{
    if (!ctx || F < 0 || win < 1 || win > kSlideMaxWin || nblk < win || group < 0)
        return fail(LDPC_E_ARG, "%s: bad arguments (ctx %p, F %lld, win %d, nblk %d, group %d)", who, (void *)ctx, (long long)F,
                    (int)win, (int)nblk, (int)group);
    if (int rc = first_null(who, {{"fcn_weights", fcn_weights}})) return rc;
    if (F > 0)
        if (int rc = first_null(who, {{"d_order_llr", d_order_llr}, {"d_metric_llr", d_metric_llr}, {"d_lri", d_lri},
                                      {"d_uidx", d_uidx}, {"d_M", d_M}, {"d_teps", d_teps}, {"d_block_off", d_block_off}})) return rc;
    if (n_weights != fcn_weight_count(win))
        return fail(LDPC_E_ARG, "%s: %d classifier weights, a window of %d takes %d", who, (int)n_weights, (int)win, fcn_weight_count(win));
    if ((d_truth || d_success) && !d_label_bits) return fail(LDPC_E_ARG, "%s: d_truth / d_success need d_label_bits", who);
    if (int rc = FAM::check(ctx, who)) return rc;
    if (nblk > kHosdMaxBlocks) return fail(LDPC_E_UNSUPPORTED, "%s: %d TEP blocks, at most %d", who, nblk, kHosdMaxBlocks);
    if (F == 0) return LDPC_OK;
    const auto head = std::make_tuple(d_order_llr, d_metric_llr, (long long)F);
    const auto tail = std::make_tuple(d_lri, d_uidx, w64(d_M), reinterpret_cast<const uchar4 *>(d_teps), d_block_off, (int)nblk, (int)win,
                                      soft_margin, slide_fcn_arg(fcn_weights, win), (int)group, w64(d_label_bits), d_deep_limit, d_global_min,
                                      d_truth, d_success, w64(d_cw), d_metric, d_best, d_teps_evaluated);
    // (d_count: the counted form, on min(*d_count, F) frames -- ldpc_dlosd_pipeline_run alone)
    if (d_count)
        hosd_launch(FAM::sliding_counted, grid_for(F, 1), stream, head, FAM::scan_shape(ctx->code),
                    std::tuple_cat(tail, std::make_tuple((const int *)d_count)));
    else
        hosd_launch(FAM::sliding, grid_for(F, 1), stream, head, FAM::scan_shape(ctx->code), tail);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

// The three families of this unit as ldpc_dlosd_pipeline_run sees them: the host side above with the device-side count.
template <class FAM>
struct HosdStageOf {
    static int front(ldpc_ctx *ctx, const float *xo, const int32_t *d_count, int64_t F, void *d_lri, void *d_uidx, uint64_t *d_M,
                     int32_t *d_nswaps, hipStream_t s)
    {
        return hosd_front<FAM>(kDlosdWho, ctx, xo, F, static_cast<uint8_t *>(d_lri), static_cast<uint8_t *>(d_uidx), d_M, d_nswaps, s, d_count);
    }
    static int sliding(ldpc_ctx *ctx, const float *xo, const float *xm, const int32_t *d_count, int64_t F, const ldpc_dlosd_pipeline *p,
                       const uint64_t *d_label, hipStream_t s)
    {
        return hosd_sliding<FAM>(kDlosdWho, ctx, xo, xm, F, static_cast<const uint8_t *>(p->d_lri), static_cast<const uint8_t *>(p->d_uidx),
                                 p->d_M, p->d_teps, p->d_block_off, p->nblk, p->win, p->soft_margin, p->fcn_weights, p->n_fcn_weights,
                                 p->group, d_label, p->d_deep_limit, p->d_global_min, d_label ? p->d_truth : nullptr,
                                 d_label ? p->d_success : nullptr, p->d_cw, p->d_metric, p->d_best, p->d_teps_evaluated, s, d_count);
    }
};
const HosdStage &hosd_stage(int family)
{
    static const HosdStage st128{HosdStageOf<HostHosd128>::front, HosdStageOf<HostHosd128>::sliding},
        stx{HosdStageOf<HostHosdX>::front, HosdStageOf<HostHosdX>::sliding}, stw{HosdStageOf<HostHosdW>::front, HosdStageOf<HostHosdW>::sliding};
    return family == LDPC_HOSD_FAMILY_128 ? st128 : family == LDPC_HOSD_FAMILY_X ? stx : stw;
}

}  // namespace ldpc

using namespace ldpc;

extern "C" {

int ldpc_hosd_front(ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint8_t *d_lri, uint8_t *d_uidx,
                    uint64_t *d_M, int32_t *d_nswaps, void *stream)
{
    return hosd_front<HostHosd128>("ldpc_hosd_front", ctx, d_order_llr, F, d_lri, d_uidx, d_M, d_nswaps, stream);
}

int ldpc_hosd_search(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F,
                     const uint8_t *d_lri, const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps,
                     const int32_t *d_block_off, int32_t nblk, const uint64_t *d_label_bits, float *d_block_min,
                     int32_t *d_block_arg, float *d_truth, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                     void *stream)
{
    return hosd_search<HostHosd128>("ldpc_hosd_search", ctx, d_order_llr, d_metric_llr, F, d_lri, d_uidx, d_M, d_teps, d_block_off, nblk,
                                    d_label_bits, d_block_min, d_block_arg, d_truth, d_cw, d_metric, d_best, stream);
}

int ldpc_hosd_sliding(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                      const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                      int32_t nblk, int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights,
                      int32_t group, const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min,
                      float *d_truth, uint8_t *d_success, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                      int32_t *d_teps_evaluated, void *stream)
{
    return hosd_sliding<HostHosd128>("ldpc_hosd_sliding", ctx, d_order_llr, d_metric_llr, F, d_lri, d_uidx, d_M, d_teps, d_block_off, nblk,
                                     win, soft_margin, fcn_weights, n_weights, group, d_label_bits, d_deep_limit, d_global_min, d_truth,
                                     d_success, d_cw, d_metric, d_best, d_teps_evaluated, stream);
}

int ldpc_hosdx_supported(const ldpc_ctx *ctx) { return ctx && ctx->hosdx_ok ? 1 : 0; }

int ldpc_hosdx_front(ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint8_t *d_lri, uint8_t *d_uidx, uint64_t *d_M,
                     int32_t *d_nswaps, void *stream)
{
    return hosd_front<HostHosdX>("ldpc_hosdx_front", ctx, d_order_llr, F, d_lri, d_uidx, d_M, d_nswaps, stream);
}

int ldpc_hosdx_search(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                      const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                      int32_t nblk, const uint64_t *d_label_bits, float *d_block_min, int32_t *d_block_arg, float *d_truth,
                      uint64_t *d_cw, float *d_metric, int32_t *d_best, void *stream)
{
    return hosd_search<HostHosdX>("ldpc_hosdx_search", ctx, d_order_llr, d_metric_llr, F, d_lri, d_uidx, d_M, d_teps, d_block_off, nblk,
                                  d_label_bits, d_block_min, d_block_arg, d_truth, d_cw, d_metric, d_best, stream);
}

int ldpc_hosdx_sliding(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                       const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                       int32_t nblk, int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights,
                       int32_t group, const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min,
                       float *d_truth, uint8_t *d_success, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                       int32_t *d_teps_evaluated, void *stream)
{
    return hosd_sliding<HostHosdX>("ldpc_hosdx_sliding", ctx, d_order_llr, d_metric_llr, F, d_lri, d_uidx, d_M, d_teps, d_block_off, nblk,
                                   win, soft_margin, fcn_weights, n_weights, group, d_label_bits, d_deep_limit, d_global_min, d_truth,
                                   d_success, d_cw, d_metric, d_best, d_teps_evaluated, stream);
}

int ldpc_hosdw_supported(const ldpc_ctx *ctx) { return ctx && ctx->hosdw_ok ? 1 : 0; }

int ldpc_hosdw_front(ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint8_t *d_lri, uint8_t *d_uidx, uint64_t *d_M,
                     int32_t *d_nswaps, void *stream)
{
    return hosd_front<HostHosdW>("ldpc_hosdw_front", ctx, d_order_llr, F, d_lri, d_uidx, d_M, d_nswaps, stream);
}

int ldpc_hosdw_search(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                      const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                      int32_t nblk, const uint64_t *d_label_bits, float *d_block_min, int32_t *d_block_arg, float *d_truth,
                      uint64_t *d_cw, float *d_metric, int32_t *d_best, void *stream)
{
    return hosd_search<HostHosdW>("ldpc_hosdw_search", ctx, d_order_llr, d_metric_llr, F, d_lri, d_uidx, d_M, d_teps, d_block_off, nblk,
                                  d_label_bits, d_block_min, d_block_arg, d_truth, d_cw, d_metric, d_best, stream);
}

int ldpc_hosdw_sliding(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                       const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                       int32_t nblk, int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights,
                       int32_t group, const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min,
                       float *d_truth, uint8_t *d_success, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                       int32_t *d_teps_evaluated, void *stream)
{
    return hosd_sliding<HostHosdW>("ldpc_hosdw_sliding", ctx, d_order_llr, d_metric_llr, F, d_lri, d_uidx, d_M, d_teps, d_block_off, nblk,
                                   win, soft_margin, fcn_weights, n_weights, group, d_label_bits, d_deep_limit, d_global_min, d_truth,
                                   d_success, d_cw, d_metric, d_best, d_teps_evaluated, stream);
}

int ldpc_fcn_windows(ldpc_ctx *ctx, const float *d_block_min, const uint8_t *d_success, const int32_t *d_index, int64_t R,
                     int32_t nblk, int32_t win, float *d_inputs, uint8_t *d_labels, int64_t *d_class_count, void *stream)
{
    static const char who[] = "ldpc_fcn_windows";
    if (!ctx) return fail(LDPC_E_ARG, "%s: ctx is NULL", who);
    if (R < 0) return fail(LDPC_E_ARG, "%s: R = %lld is negative", who, (long long)R);
    if (win < 1 || win > kSlideMaxWin) return fail(LDPC_E_ARG, "%s: win = %d outside 1..%d", who, (int)win, kSlideMaxWin);
    if (nblk < win || nblk > kHosdMaxBlocks)
        return fail(LDPC_E_ARG, "%s: nblk = %d outside win = %d .. %d", who, (int)nblk, (int)win, kHosdMaxBlocks);
    if (R == 0) return LDPC_OK;
    if (int rc = first_null(who, {{"d_block_min", d_block_min}, {"d_success", d_success}, {"d_inputs", d_inputs},
                                  {"d_labels", d_labels}})) return rc;
    return fcn_windows_run(d_block_min, d_success, d_index, R, nblk, win, d_inputs, d_labels, d_class_count, (hipStream_t)stream);
}

int ldpc_fcn_grad(ldpc_ctx *ctx, const float *d_inputs, const uint8_t *d_labels, const float *d_weight, const int32_t *d_index,
                  int64_t B, int32_t win, const float *fcn_weights, int32_t n_weights, float penalty, float *d_p,
                  double *d_loss_sum, double *d_grad_sum, double *d_acc, int64_t *d_counts, void *stream)
{
    static const char who[] = "ldpc_fcn_grad";
    if (!ctx) return fail(LDPC_E_ARG, "%s: ctx is NULL", who);
    if (B < 0) return fail(LDPC_E_ARG, "%s: B = %lld is negative", who, (long long)B);
    if (win < 1 || win > kSlideMaxWin) return fail(LDPC_E_ARG, "%s: win = %d outside 1..%d", who, (int)win, kSlideMaxWin);
    const int want = fcn_weight_count(win);
    if (n_weights != want) return fail(LDPC_E_ARG, "%s: n_weights = %d, win = %d takes %d", who, (int)n_weights, (int)win, want);
    if (int rc = first_null(who, {{"fcn_weights", fcn_weights}})) return rc;
    if (B == 0) return LDPC_OK;
    if (int rc = first_null(who, {{"d_inputs", d_inputs}})) return rc;
    const bool sums = d_loss_sum || d_grad_sum || d_acc || d_counts;
    if (sums)
        if (int rc = first_null(who, {{"d_labels", d_labels}})) return rc;
    if (!sums && !d_p) return LDPC_OK;
    return fcn_grad_run(d_inputs, d_labels, d_weight, d_index, B, win, slide_fcn_arg(fcn_weights, win), penalty, d_p, d_loss_sum, d_grad_sum, d_acc, d_counts,
                        (hipStream_t)stream);
}

}  // extern "C"
