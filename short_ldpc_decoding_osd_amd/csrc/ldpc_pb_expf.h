// PB-OSD: the deterministic exp of oracle/ldpc_oracle.c det_expf (IEEE + - * / only, so host and device agree bit for bit),
// shared by the (128,64) kernels (ldpc_pb_common.h) and the any-shape kernel (ldpc_osdx_pb.h).
#pragma once

namespace ldpc {

__device__ __forceinline__ float det_expf(float x)
{
    if (x > 88.0f) x = 88.0f;
    if (x < -87.0f) return 0.0f;
    const float kf = __builtin_floorf(x * 1.44269504f + 0.5f);
    const float r = (x - kf * 0.693359375f) - kf * -2.12194440e-4f;
    float p = 1.9875691500e-4f;
    p = p * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    const float e = (p * (r * r) + r) + 1.0f;
    return e * __int_as_float(((int)kf + 127) << 23);
}

}  // namespace ldpc
