// OSD front end of one frame on one wavefront: reliability sort, column gather, GF(2) elimination, MRB bookkeeping
// (swapped_info / identify_mrb, PB_OSD/pb_testing.py:268-320).  Shared by osd_front_kernel, the fused order-2 kernel
// (ldpc_osd.hip) and the fused PB-OSD head (pb_singles_kernel, ldpc_pb_singles.h).
#pragma once
#include "ldpc_internal.h"
#include "ldpc_bits.h"
#include "ldpc_wave.h"

namespace ldpc {

struct __attribute__((aligned(16))) FrontLds {
    RankLds rank;            // reliability sort (bucket_ranks, ldpc_wave.h); afterwards its first 1 KiB: the transposition's scratch
    unsigned mask[4];        // 128-bit membership mask of the MRB indices
    unsigned char pi1[128];  // sorted position -> original bit
    unsigned char rowsrc[64];
    unsigned char perm[128]; // primed position -> original bit
};

struct FrontResult {
    int o1, o2;   // original bit index of primed positions lane and 64 + lane
    u64 Prow;     // row `lane` of P'
    int ns;       // recorded column exchanges (-1: rank-deficient)
};


// sort + column gather + elimination + bookkeeping of one frame (one wavefront); results in registers
// (a1 / a2: the magnitude bits of y[lane] / y[64 + lane]; Gcols: the 128 columns of G, in global memory or -- osd_front_kernel,
//  which copies them once per workgroup -- in LDS: the function is inlined, so the gather below is then a ds_read_b64)
template <bool GE_LANE_OPAQUE = false>
__device__ __forceinline__ FrontResult front_device_vals(FrontLds &L, unsigned a1, unsigned a2, const u64 *__restrict__ Gcols, int lane)
{
    // ---- reliability sort: rank of each |y| in descending order, ties -> lower index ------
    // sort key = (|y| bits, 127 - index) as one 64-bit integer: "u before v" <=> key_u > key_v (bucket_ranks)
    const float bs = bucket_scale(a1, a2);
    int r1, r2;
    bucket_ranks(L.rank, ((u64)a1 << 32) | (unsigned)(127 - lane), ((u64)a2 << 32) | (unsigned)(63 - lane), bucket_of(a1, bs),
                 bucket_of(a2, bs), lane, r1, r2);
    L.pi1[r1] = (unsigned char)lane;
    L.pi1[r2] = (unsigned char)(lane + 64);
    if (lane < 4) L.mask[lane] = 0;
    wave_fence();
    // ---- G with columns in sorted order, column-major ------------------------------------
    u64 C1 = Gcols[L.pi1[lane]];
    u64 C2 = Gcols[L.pi1[lane + 64]];
    int rho = lane, idx1 = lane, idx2 = lane + 64;
    // The elimination compares the lane number with each of its 64 step numbers, in the exchange path only (a step in thirty).
    // Given the kernel's own `lane`, the compiler computes all 64 compares ahead of osd_front_kernel's frame loop and parks 37
    // of the 64 SGPR pairs in lanes of two VGPRs: 64 v_cmp + 74 v_writelane per workgroup, two VGPRs that the kernel does not
    // have to spare at 8 waves per SIMD, and a v_readlane pair wherever one is used.  GE_LANE_OPAQUE hands the elimination a copy of the
    // lane number that the compiler cannot see through (an empty asm, no instruction), so each compare stays in the block
    // that uses it.  For osd_front_kernel only: in osd_fused2r_kernel, at 128 VGPRs, the same copy moves eight VGPRs to scratch.
    int ge_lane = lane;
    if constexpr (GE_LANE_OPAQUE) asm volatile("" : "+v"(ge_lane));
    const int ns = ge_columns(C1, C2, rho, idx1, idx2, ge_lane, nullptr);
    // ---- identify_mrb bookkeeping (pb_testing.py:276-304) --------------------------------
    // (no column exchange -- the 64 most reliable columns were independent: a quarter of the frames -- leaves every index
    //  where the sort put it: the ranks are the lane numbers and the membership mask is not needed)
    int rankM = lane, rankL = lane;
    if (ns != 0) {
        atomicOr(&L.mask[idx1 >> 5], 1u << (idx1 & 31));
        wave_fence();
        const unsigned m[4] = {L.mask[0], L.mask[1], L.mask[2], L.mask[3]};
        rankM = below_mask(m, idx1);         // new MRB position of slot `lane`
        rankL = idx2 - below_mask(m, idx2);  // new parity column of slot `lane`
    }
    L.perm[rankM] = L.pi1[idx1];
    L.perm[64 + rankL] = L.pi1[idx2];
    L.rowsrc[rankM] = (unsigned char)rho;          // pivot of MRB slot `lane` is physical row rho
    // ---- rows of P': the 64x64 bit transposition of the parity columns, with rankL and rowsrc folded into LDS addresses ----
    // The lane's column (bit = physical row) goes to LDS a byte at a time: byte g of column c at ta[64 g + c], so the eight
    // bytes at ta[8 (8 g + cb)] are the 8x8 block of rows 8 g .. 8 g + 7 and columns 8 cb .. 8 cb + 7, one column per byte.
    // Lane 8 g + cb transposes that block in registers (transpose8x8: one row per byte) and scatters it row-major, byte cb of
    // row 8 g + i at tb[8 (8 g + i) + cb]; row rowsrc[lane] is then one 64-bit read.  Where the cross-lane form (transpose64
    // and a shfl64 by rowsrc) took 14 ds_bpermute and six butterfly stages, this takes 16 byte stores, two 64-bit reads and the
    // block transpose.  The scratch is the sort's key array, dead since the ranks were formed (the fence behind pi1); the
    // next frame's sort writes it again behind the last fence below.
    unsigned char *const ta = reinterpret_cast<unsigned char *>(L.rank.bk), *const tb = ta + 512;
    {
        const unsigned lo = (unsigned)C2, hi = (unsigned)(C2 >> 32);
        unsigned char *const a = ta + rankL;
        a[0] = (unsigned char)lo; a[64] = (unsigned char)(lo >> 8); a[128] = (unsigned char)(lo >> 16); a[192] = (unsigned char)(lo >> 24);
        a[256] = (unsigned char)hi; a[320] = (unsigned char)(hi >> 8); a[384] = (unsigned char)(hi >> 16); a[448] = (unsigned char)(hi >> 24);
    }
    wave_fence();
    {
        const u64 blk = transpose8x8(*reinterpret_cast<const u64 *>(ta + 8 * lane));
        const unsigned lo = (unsigned)blk, hi = (unsigned)(blk >> 32);
        unsigned char *const b = tb + (((lane >> 3) << 6) | (lane & 7));
        b[0] = (unsigned char)lo; b[8] = (unsigned char)(lo >> 8); b[16] = (unsigned char)(lo >> 16); b[24] = (unsigned char)(lo >> 24);
        b[32] = (unsigned char)hi; b[40] = (unsigned char)(hi >> 8); b[48] = (unsigned char)(hi >> 16); b[56] = (unsigned char)(hi >> 24);
    }
    wave_fence();
    FrontResult res;
    res.Prow = *reinterpret_cast<const u64 *>(tb + 8 * L.rowsrc[lane]);
    res.o1 = L.perm[lane];
    res.o2 = L.perm[64 + lane];
    res.ns = ns;
    wave_fence();
    return res;
}

}  // namespace ldpc
