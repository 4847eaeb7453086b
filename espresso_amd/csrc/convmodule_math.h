// Rounding rules of the Conformer convolution module's middle, shared by the offline kernels (convmodule.hip) and the streamed
// one (stream_convmodule.hip): one copy of the GLU gate and of the BatchNorm scale / shift, so both passes round alike.
#pragma once
#include "common.h"

__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }  // (v_rcp_f32, see silu_f)

// U = bf16(a * sigmoid(g)) for 8 adjacent channels (16 bytes of a, 16 bytes of g)
__device__ __forceinline__ void glu_gate8(const uint4& a, const uint4& g, uint32_t (&pk)[4]) {
  const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, gw[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    pk[e] = pack_bf2(__uint_as_float(aw[e] << 16) * sigmoid_f(__uint_as_float(gw[e] << 16)),
                     __uint_as_float(aw[e] & 0xffff0000u) * sigmoid_f(__uint_as_float(gw[e] & 0xffff0000u)));
}
__device__ __forceinline__ uint4 glu_gate8(const uint4& a, const uint4& g) {
  uint32_t pk[4];
  glu_gate8(a, g, pk);
  return make_uint4(pk[0], pk[1], pk[2], pk[3]);
}

// BatchNorm as one multiply-add per element: y = z * sc + sh
__device__ __forceinline__ void bn_scale_shift(float mean, float rstd, float gamma, float beta, float& sc, float& sh) {
  sc = rstd * gamma;
  sh = beta - mean * sc;
}
// H = bf16(act(z * sc + sh)) for 8 adjacent channels of a 16-byte row of Z; act = SiLU (2), ReLU (1) or identity
__device__ __forceinline__ void bn_act8(const uint4& z8, const float (&sc)[8], const float (&sh)[8], int act, float (&o)[8]) {
  const uint32_t wv[4] = {z8.x, z8.y, z8.z, z8.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float z = (e & 1) ? __uint_as_float(wv[e >> 1] & 0xffff0000u) : __uint_as_float(wv[e >> 1] << 16);
    const float y = z * sc[e] + sh[e];
    o[e] = act == 2 ? silu_f(y) : (act == 1 ? fmaxf(y, 0.f) : y);
  }
}
__device__ __forceinline__ uint4 bn_act8(const uint4& z8, const float (&sc)[8], const float (&sh)[8], int act) {
  float o[8];
  bn_act8(z8, sc, sh, act, o);
  return make_uint4(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7]));
}
