// The fp32 operations the per-token posterior kernels share (prefix_posterior.hip, prefix_posterior_long.hip): both include
// this header so that the one-workgroup kernel and the tiled one do the same operations in the same order.
#pragma once
#include "common.h"

// log(exp(a) + exp(b)), -inf safe, on the hardware exp2 / log2 (v_exp_f32, v_log_f32): a frame of the CTC kernel is 32 of these
// per thread in series, and common.h's log_add (log1pf: ~40 instructions) made it 12x the aligner's frame.  The argument of the
// log is in [1, 2], where the instruction's error (1 ulp of a result <= 1) is below half an ulp of any |score| >= 1.
__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  const float r = m + __logf(1.f + __expf(-fabsf(a - b)));
  return m == -INFINITY ? -INFINITY : r;
}

__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }

// one factor: Psi_i - Psi_{i-1}, clamped to <= 0; -inf (never NaN) from the first Psi = -inf on
__device__ __forceinline__ float factor(float hi, float lo) { return hi == -INFINITY ? -INFINITY : fminf(hi - lo, 0.f); }
