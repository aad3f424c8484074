// PB-OSD kernels for (128,64) codes on gfx950 (MI355X): the translation unit.  Here: the host side (workspace, tuning, launch_pb).
// The device code lies in eight headers, included in the order of the stages (ONE translation unit on purpose: the kernels share
// inlined device code, and the order of the definitions is the order of the code object):
//   ldpc_pb_common.h   the algorithm; float conventions, per-frame quantities, the two rules, TEP algebra, records
//   ldpc_pb_singles.h  pb_singles_kernel
//   ldpc_pb_wave.h     pb_wave_kernel and the two functions of its rare paths; it includes, in this order,
//     ldpc_pb_walk.h     a frame's LDS, the items and cursors, the walk that produces a chunk and the choice of its bound
//     ldpc_pb_rules.h    what the three sort-free scans share, and where they differ on purpose
//     ldpc_pb_pass.h     the cost of a candidate, the two wavefront scans, the sorted path
//   ldpc_pb_coop.h     pb_coop_kernel (the workgroup scan)    ldpc_pb_seq.h  pb_seq_kernel
#include <math.h>

#include "ldpc_pb_common.h"
#include "ldpc_pb_singles.h"
#include "ldpc_pb_wave.h"
#include "ldpc_pb_coop.h"
#include "ldpc_pb_seq.h"

namespace ldpc {

// the control words of a call start at zero (a one-wavefront kernel, not hipMemsetAsync: captured into a hipGraph the
// memset node did not clear the words on the second and later replays -- ROCm 7.2 -- and the tickets ran on)
__global__ __launch_bounds__(64) void pb_ctl_clear_kernel(int *__restrict__ ctl)
{
    for (int i = threadIdx.x; i < kPbCtlInts; i += 64) ctl[i] = 0;
}

// chunk targets: the first chunk's count is only guessed (+-40 %), the others follow the growth of the counts
ldpc_pb_tuning pb_default_tuning()
{
    ldpc_pb_tuning t;
    t.budget = 4096; t.budget_s = t.budget / 8; t.budget_m = t.budget / 4; t.budget_l = 2 * t.budget; t.budget_xl = 6 * t.budget;
    t.t1 = 320; t.t2 = 600; t.t3 = 3072;        // (t2 measured at 1.0 / 2.5 dB: 512: 4.16 / 0.548 ms, 600: 4.08 / 0.532, 676: 4.11 / 0.554, 760: 4.37 / 0.561)
    // The tail rule.  One search call at a time (means over four batches x 12 launches, ms at 2.5 / 2.0 / 1.0 dB): off 0.484 / 1.020 / 4.159,
    // 10 %: 0.451 / 0.967 / 3.852, 20 %: 0.431 / 0.948 / 3.790, 30 %: 0.424 / 0.929 / 3.775, 40 %: 0.436 / 0.926 / 3.753 (budget / 16; / 8 and / 4
    // within 1 %).  Four batches in flight (bench.py's graph, 10^8 frames/s at 2.5 / 2.0 dB, 10^7 at 1.0 dB), where the tails hide behind
    // the other batches and the total work counts: off 2.715 / 1.335 / 3.30, 15 %: 2.708 / 1.324 / 3.357, 25 %: 2.670 / 1.311 / 3.343,
    // 40 %: 2.626 / - / 3.31.  20 %: a tenth off a lone call, one per cent off the throughput at 2.5 dB, one per cent on it at 1.0 dB.
    t.late_min = 4608; t.late_maxlen = 1 << 30; t.late_pct = 20; t.late_div = 16;
    t.handoff_maxlen = 1 << 30;
    return t;
}

int pb_ctx_init(ldpc_ctx *ctx)
{
    OsdState *st = state(ctx);
    st->pb_tuning = pb_default_tuning();
    static_assert(sizeof(PbCoopLds<kPbCoopW>) * (16 / kPbCoopW) <= 160 * 1024, "16 wavefronts of this kernel per CU");
    LDPC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pb_coop_kernel<kPbCoopW>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)sizeof(PbCoopLds<kPbCoopW>)));
    return LDPC_OK;
}

// list replay: the list is append-only, at most 1 + 2 (N_max - 1) slots; spilled slots first, spilled chunk minima after
static int pb_spill_layout(ldpc_ctx *ctx, int order, int64_t *spill_slots, int64_t *stride)
{
    const int64_t nmax = ctx->osd_tables.ntep[order];
    const int64_t slots = 2 * nmax + 2;
    if (slots > (int64_t)kPbSuper * 4096) return fail(LDPC_E_UNSUPPORTED, "ldpc_osd_decode: PB-OSD list of %lld slots exceeds the kernel's limit", (long long)slots);
    *spill_slots = slots > kPbLdsSlots ? slots - kPbLdsSlots : 0;
    *stride = *spill_slots + (slots / 64 + 2) + 2;
    return LDPC_OK;
}

// PB-OSD part of a stream's workspace: control words, the two frame lists, the list replay's spill areas
static int stream_ws_pb(ldpc_ctx *ctx, hipStream_t s, int64_t frames, int64_t spill_stride, StreamWs **out)
{
    OsdState *st = state(ctx);
    std::lock_guard<std::mutex> lock(st->mu);
    StreamWs &w = st->ws[s];
    const bool grow_list = frames > w.pb_cap || !w.d_pb_ctl, grow_spill = spill_stride > w.pb_spill_stride;
    const bool capturing = stream_capturing(s);
    if ((grow_list || grow_spill) && capturing)
        return fail(LDPC_E_NOMEM, "PB-OSD workspace of this stream must be sized before capturing (ldpc_osd_reserve_stream with the "
                    "PB-OSD parameters, or one eager call on the stream)");
    if ((grow_list || grow_spill) && w.captured)
        return fail(LDPC_E_NOMEM, "PB-OSD workspace of this stream is referenced by a captured graph and cannot grow: destroy the graph and "
                    "call ldpc_osd_release_stream, or reserve the larger size before capturing");
    if (capturing) w.captured = true;
    if (grow_list) {
        (void)hipFree(w.d_pb_list); w.d_pb_list = nullptr; w.pb_cap = 0;
        if (!w.d_pb_ctl && hipMalloc((void **)&w.d_pb_ctl, sizeof(int) * kPbCtlInts) != hipSuccess)
            return fail(LDPC_E_NOMEM, "PB-OSD control words could not be allocated");
        (void)hipFree(w.d_pb_prep); w.d_pb_prep = nullptr;
        (void)hipFree(w.d_pb_carry); w.d_pb_carry = nullptr;
        const int64_t sub_cap = (frames + kPbSub - 1) / kPbSub;
        if (hipMalloc((void **)&w.d_pb_list, sizeof(int) * (2 * (size_t)kPbSub * (size_t)sub_cap)) != hipSuccess ||
            hipMalloc(&w.d_pb_carry, sizeof(unsigned) * kPbRecWords * (size_t)kPbHeavyCap) != hipSuccess ||
            hipMalloc(&w.d_pb_prep, sizeof(unsigned) * kPbR1Words * (size_t)frames) != hipSuccess)
            return fail(LDPC_E_NOMEM, "PB-OSD frame lists for %lld frames could not be allocated", (long long)frames);
        w.pb_cap = frames; w.pb_sub_cap = sub_cap;
    }
    if (grow_spill) {
        (void)hipFree(w.d_pb_spill); w.d_pb_spill = nullptr; w.pb_spill_stride = 0;
        if (hipMalloc(&w.d_pb_spill, sizeof(PbEntry) * (size_t)spill_stride * kPbSeqBlocks * 4) != hipSuccess)
            return fail(LDPC_E_NOMEM, "PB-OSD frontier workspace (%lld entries per wave) could not be allocated", (long long)spill_stride);
        w.pb_spill_stride = spill_stride;
    }
    *out = &w;
    return LDPC_OK;
}

// ldpc_osd_reserve_stream for algo = PB: everything launch_pb would allocate for `frames` frames of this order
int pb_reserve(ldpc_ctx *ctx, hipStream_t s, int64_t frames, int order)
{
    int64_t spill_slots, stride;
    if (int rc = pb_spill_layout(ctx, order, &spill_slots, &stride)) return rc;
    StreamWs *w;
    return stream_ws_pb(ctx, s, frames, stride, &w);
}

// One straight sequence of launches on the stream: clear, singles, chunk kernel, workgroup kernel, list replay.  Everything that
// can fail -- the list replay's spill layout, the stream's workspace and, inside it, the refusals during a stream capture --
// is done before the first of them is enqueued: a call that one of these refuses has put nothing on the stream.  (The
// hipGetLastError at the end reports a failed launch after all five were issued.)
int launch_pb(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
              const unsigned char *d_perm, const u64 *d_parity, const ldpc_osd_params *p, int pb_mode, bool front_inside,
              uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep, hipStream_t s)
{
    OsdState *st = state(ctx);
    const int64_t nmax = ctx->osd_tables.ntep[p->order];
    int64_t spill_slots, stride;
    if (int rc = pb_spill_layout(ctx, p->order, &spill_slots, &stride)) return rc;
    StreamWs *w;
    if (int rc = stream_ws_pb(ctx, s, F, stride, &w)) return rc;
    // ---- nothing below this line fails before the launches
    PbParams pp;
    pp.order = p->order; pp.nmax = (int)nmax; pp.cmin_off = spill_slots;
    // When a search leaves the chunk kernel for the workgroup kernel: after `budget` TEPs, the budget chosen ON THE DEVICE from the
    // length of the frame's sub-list of list A (a sixteenth of the frames that search beyond the weight-1 head), so that the
    // workgroup kernel gets the tails, 1000-3500 frames a call, and never the bulk (its list holds 2 x kPbCoopHalf frames).
    // Measured per 131 072-frame step (round 3), PB kernels with the budget of the schedule / the neighbouring ones / no hand-over:
    //   3.5 dB (length 42)    512: 0.20 ms              2.0 dB  (1750)   8192: 1.50 | 4096: 1.52 | 16384: 1.61 | none 1.80
    //   3.0 dB (177)         1024: 0.34                 1.75 dB (2560)   8192: 2.20 | 16384: 2.26 | 4096: 2.91 | none 2.50
    //   2.5 dB (626)         4096: 0.70 | 2048: 0.70    1.5 dB  (3475)  16384: 3.22 | 8192: 3.78 | none 3.41
    //   2.25 dB (1090)       4096: 1.02 | none 1.45     1.0 dB  (5300)  16384: 6.26 | 8192: 6.85 | none 6.44
    // (serial kernel sums; with four batches in flight -- bench.py's graph -- 24576 beats 16384 and none at 1.0 dB: 2.15 / 2.12 / 2.14 x 10^7
    //  frames/s, and ties with 16384 at 1.5 dB: 4.25 x 10^7 against 4.18 without)
    // The schedule is a property of the CONTEXT (ldpc_ctx_set_pb_tuning, validated there; defaults: pb_default_tuning) and is
    // copied here under the state's lock: no environment variable is read on the decode path (rounds 1-3 read thirteen).
    ldpc_pb_tuning tn;
    {
        std::lock_guard<std::mutex> lock(st->mu);
        tn = st->pb_tuning;
    }
    pp.budget = tn.budget; pp.budget_s = tn.budget_s; pp.budget_m = tn.budget_m; pp.budget_l = tn.budget_l; pp.budget_xl = tn.budget_xl;
    pp.t1 = tn.t1; pp.t2 = tn.t2; pp.t3 = tn.t3;
    pp.late_min = tn.late_min; pp.late_maxlen = tn.late_maxlen; pp.late_pct = tn.late_pct; pp.late_div = tn.late_div;
    pp.handoff_maxlen = tn.handoff_maxlen;
    pp.c4 = (float)(-4.0 * (1.0 / pow(10.0, (double)p->snr_db / 10.0)));    // -4 * noise_variance, pb_testing.py:50-52
    PbOut O{reinterpret_cast<u64 *>(d_cw), d_metric, d_best, d_ntep, reinterpret_cast<int *>(p->d_aux)};
    const int64_t list_len = (int64_t)kPbSub * w->pb_sub_cap;   // >= pb_cap
    int *listA = w->d_pb_list, *listB = w->d_pb_list + list_len;
    unsigned *carry = reinterpret_cast<unsigned *>(w->d_pb_carry);      // [kPbHeavyCap] records of kPbRecWords words
    const int sub_cap = (int)w->pb_sub_cap;
    unsigned *recs = reinterpret_cast<unsigned *>(w->d_pb_prep);      // [pb_cap] records of kPbR1Words words (singles -> chunk kernel)
    hipLaunchKernelGGL(pb_ctl_clear_kernel, dim3(1), dim3(64), 0, s, w->d_pb_ctl);
    const int64_t want = (F + 3) / 4;
    const unsigned g1 = (unsigned)(F < 1 ? 1 : (F < 32768 ? F : 32768));
    // front_inside (ldpc_osd_decode's option): the front end runs inside the singles kernel, nothing goes through a workspace --
    // the frames of list B are then set up from the singles records (mode 2, every frame to the list replay, writes none)
    const u64 *const Gcols = ctx->osd_tables.d_Gcols;
    if (front_inside)
        hipLaunchKernelGGL((pb_singles_kernel<true>), dim3(g1), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, d_perm, d_parity, Gcols, pp,
                           pb_mode, st->d_cdf_half, w->d_pb_ctl, listA, listB, sub_cap, recs, O);
    else
        hipLaunchKernelGGL((pb_singles_kernel<false>), dim3(g1), dim3(64), 0, s, d_y, d_index, d_count, (long long)F, d_perm, d_parity, Gcols, pp,
                           pb_mode, st->d_cdf_half, w->d_pb_ctl, listA, listB, sub_cap, recs, O);
    // (three instantiations by what the context's probe of the wave_rol:1 DPP control found -- the walk rotates a copy of the
    //  weights through the wavefront: -1 = a lane receives its upper neighbour's value, +1 = its lower neighbour's, 0 = not a
    //  rotation: LDS reads instead)
    const int rot = ctx->dpp_wave_rol_dir;
    // chunk kernel: one workgroup (= one wavefront) per (sub-list, entry); a multiple of 16 workgroups, at most 65 536 (a
    // workgroup then takes every 4096th entry of its sub-list).  Workgroups beyond their sub-list's length leave at once.
    const int64_t g2w = ((F + kPbSub - 1) / kPbSub) * kPbSub;
    const unsigned g2 = (unsigned)(g2w < 65536 ? g2w : 65536);
    if (rot < 0) hipLaunchKernelGGL((pb_wave_kernel<kPbWaveCap, -1>), dim3(g2), dim3(64), 0, s, pp, st->d_cdf_half, w->d_pb_ctl,
                                    listA, listB, sub_cap, carry, recs, O);
    else if (rot > 0) hipLaunchKernelGGL((pb_wave_kernel<kPbWaveCap, 1>), dim3(g2), dim3(64), 0, s, pp, st->d_cdf_half, w->d_pb_ctl,
                                         listA, listB, sub_cap, carry, recs, O);
    else hipLaunchKernelGGL((pb_wave_kernel<kPbWaveCap, 0>), dim3(g2), dim3(64), 0, s, pp, st->d_cdf_half, w->d_pb_ctl,
                            listA, listB, sub_cap, carry, recs, O);
    // the long searches the chunk kernel handed on (at most kPbHeavyCap, in two halves; the workgroups find an empty list otherwise)
    const unsigned g4 = (unsigned)(F < kPbCoopGrid ? F : kPbCoopGrid);
    hipLaunchKernelGGL((pb_coop_kernel<kPbCoopW>), dim3(g4), dim3(64 * kPbCoopW), sizeof(PbCoopLds<kPbCoopW>), s,
                       pp, st->d_cdf_half, w->d_pb_ctl, listB, carry, O);
    const unsigned g3 = (unsigned)(want < kPbSeqBlocks ? (want < 1 ? 1 : want) : kPbSeqBlocks);
    hipLaunchKernelGGL(pb_seq_kernel, dim3(g3), dim3(256), 0, s, d_y, d_index, d_perm, d_parity, front_inside ? recs : (const unsigned *)nullptr, pp, st->d_cdf_half,
                       reinterpret_cast<PbEntry *>(w->d_pb_spill), (long long)w->pb_spill_stride, w->d_pb_ctl, listB, O);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}

}  // namespace ldpc

extern "C" {

int ldpc_ctx_get_pb_tuning(ldpc_ctx *ctx, ldpc_pb_tuning *out)
{
    using namespace ldpc;
    if (!ctx || !out || !ctx->osd_state) return fail(LDPC_E_ARG, "ldpc_ctx_get_pb_tuning: null argument");
    OsdState *st = state(ctx);
    std::lock_guard<std::mutex> lock(st->mu);
    *out = st->pb_tuning;
    return LDPC_OK;
}

int ldpc_ctx_set_pb_tuning(ldpc_ctx *ctx, const ldpc_pb_tuning *t)
{
    using namespace ldpc;
    if (!ctx || !ctx->osd_state) return fail(LDPC_E_ARG, "ldpc_ctx_set_pb_tuning: null context");
    ldpc_pb_tuning v = t ? *t : pb_default_tuning();
    const int budgets[5] = {v.budget_s, v.budget_m, v.budget, v.budget_l, v.budget_xl};
    for (int b : budgets)
        if (b < 1) return fail(LDPC_E_ARG, "ldpc_ctx_set_pb_tuning: hand-over budgets must be >= 1 TEP (got %d)", b);
    constexpr int kcap = PbwCaps<kPbWaveCap, true>::KCAP;
    if (v.t1 < 32 || v.t1 > kcap || v.t2 < 32 || v.t2 > kcap)
        return fail(LDPC_E_ARG, "ldpc_ctx_set_pb_tuning: chunk targets t1 / t2 must lie in [32, %d] (got %d, %d)", kcap, v.t1, v.t2);
    if (v.t3 < 256 || v.t3 > kCoopCap) return fail(LDPC_E_ARG, "ldpc_ctx_set_pb_tuning: t3 must lie in [256, %d] (got %d)", kCoopCap, v.t3);
    if (v.late_div < 1 || v.late_pct < 0 || v.late_min < 0 || v.late_maxlen < 0 || v.handoff_maxlen < 0)
        return fail(LDPC_E_ARG, "ldpc_ctx_set_pb_tuning: late_div must be >= 1 and the other fields >= 0");
    OsdState *st = state(ctx);
    std::lock_guard<std::mutex> lock(st->mu);
    st->pb_tuning = v;
    return LDPC_OK;
}

}  // extern "C"
