// PB-OSD with the code's n and k as kernel arguments: what osdx_pb_kernel (ldpc_osdx_pb.h, k <= 64) and osdw_pb_kernel
// (ldpc_osdw_pb.h, k <= 127) share -- the kernel argument, the layout of the context's PB table, the encoding of a frontier
// slot and the wave arg-min of a pop.  Declarations only: no kernel is defined here.
#pragma once

#include "ldpc_wave.h"

namespace ldpc {

struct PbxParams {
    int order, nmax;         // nmax = sum_{w <= order} C(k, w)
    float c4;                // (float)(-4 / 10^(snr_db / 10))
};

// the context's PB table (OsdTables::d_pb / OsdwTables::d_pb, float64): cdfH[65] = P[Bin(m, 1/2) <= b] (zero beyond m), then the
// ratios of consecutive binomial coefficients (m - i) / (i + 1) and (k - i) / (i + 1), 64 entries each (zero beyond m - 1 / k - 1;
// of the second only the entries i < order <= 3 are read, so 64 of them serve k up to 127 as well)
constexpr int kPbxCdfH = 0, kPbxCoefM = 65, kPbxCoefK = 129, kPbxTabSize = 193;

// meta of an empty slot (its sum is +inf); a live one holds seq << 8 | cursor, seq < 2 N_max <= 683 008 (k = 127, order 3)
constexpr int kPbxEmpty = 0x7FFFFFFF;

__device__ __forceinline__ double readlane_f64(double v, int lane)
{
    return __longlong_as_double((long long)readlane64((u64)__double_as_longlong(v), lane));
}

// wave arg-min on (sum, meta): the lane of the first minimum, sum and meta of it in every lane
__device__ __forceinline__ int pbx_argmin(float &s, int &meta)
{
    const int wl = wave_argmin_lane(s, meta);
    s = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), wl));
    meta = __builtin_amdgcn_readlane(meta, wl);
    return wl;
}

}  // namespace ldpc
