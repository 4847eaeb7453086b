// The fp32 log-softmax of one row, for a 256-thread workgroup: the row routine of ea_log_softmax_* (loss.hip) and of the
// long-form kernels (long_form.hip), written once so that a stitched row has the bits of a plain one.
//
// What fixes the bits is the sum: thread t adds exp(x[c] - max) for c = t, t + 256, ... in that order, the 64 lanes of a wave
// combine by the xor butterfly and the four waves are added in wave order (block_sum).  So the sum pass keeps its lane-strided
// 4- / 2-byte loads (a wave still reads 256 / 128 contiguous bytes per request).  The maximum does not depend on the order and
// the output pass is element-wise: with kVec16 they use 16-byte loads and stores where the row's addresses allow them, the
// elements before the first aligned address and after the last whole vector going through clamped scalar loads that every lane
// issues (no load in a divergent branch).  kVec16 = false is the code ea_log_softmax_* always had.
#pragma once
#include "common.h"

template <typename TIn>
__device__ __forceinline__ float lsm_ld(const TIn* __restrict__ x, int c) {
  if constexpr (sizeof(TIn) == 2) return bf2f(x[c]); else return x[c];
}

// Elements per 16-byte load of the input, and the loaded vector as floats.
template <typename TIn> struct LsmVec { static constexpr int kE = 16 / (int)sizeof(TIn); };

template <typename TIn>
__device__ __forceinline__ void lsm_ld16(const TIn* __restrict__ p, float (&v)[LsmVec<TIn>::kE]) {
  if constexpr (sizeof(TIn) == 2) {
    const bf16x8_t r = *reinterpret_cast<const bf16x8_t*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = bf2f((bf16_t)r[i]);
  } else {
    const f32x4_t r = *reinterpret_cast<const f32x4_t*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = r[i];
  }
}

// The split of a row of V elements at x into [0, head) scalar, nvec 16-byte vectors from `head`, and the rest scalar.
template <typename TIn>
__device__ __forceinline__ void lsm_split(const TIn* x, int V, int& head, int& nvec) {
  constexpr int kE = LsmVec<TIn>::kE;
  const int mis = (int)((uintptr_t)x & 15);
  head = ((16 - mis) & 15) / (int)sizeof(TIn);
  if (head > V) head = V;
  nvec = (V - head) / kE;
}

// Scalar element i of the row's `ns` scalar elements (the head, then the tail), clamped into the row: every lane loads.
__device__ __forceinline__ int lsm_scalar_col(int i, int head, int vec_end, int V) {
  const int c = i < head ? i : vec_end + (i - head);
  return c < V ? c : V - 1;
}

// The row's log-sum-exp (to every thread).  V >= 1; sm: 16 floats of LDS.
template <typename TIn, bool kVec16>
__device__ __forceinline__ float log_softmax_row_lse(const TIn* __restrict__ x, int V, float* sm) {
  float mx = -INFINITY;
  if constexpr (kVec16) {
    constexpr int kE = LsmVec<TIn>::kE;
    int head, nvec;
    lsm_split(x, V, head, nvec);
    const int vec_end = head + nvec * kE, ns = V - nvec * kE;  // ns < 2 * kE <= 16 scalar elements
    for (int i = threadIdx.x; i < nvec; i += 256) {
      float v[kE];
      lsm_ld16(x + head + i * kE, v);
#pragma unroll
      for (int e = 0; e < kE; ++e) mx = fmaxf(mx, v[e]);
    }
    const float v = lsm_ld(x, lsm_scalar_col(threadIdx.x, head, vec_end, V));
    if ((int)threadIdx.x < ns) mx = fmaxf(mx, v);
  } else {
    for (int c = threadIdx.x; c < V; c += 256) mx = fmaxf(mx, lsm_ld(x, c));
  }
  mx = block_max(mx, sm);
  float s = 0.f;
  for (int c = threadIdx.x; c < V; c += 256) s += expf(lsm_ld(x, c) - mx);
  s = block_sum(s, sm);
  return mx + logf(s);
}

// o[c] = x[c] - lse for c < V.
template <typename TIn, bool kVec16>
__device__ __forceinline__ void log_softmax_row_write(const TIn* __restrict__ x, int V, float lse, float* __restrict__ o) {
  if constexpr (kVec16) {
    constexpr int kE = LsmVec<TIn>::kE;
    int head, nvec;
    lsm_split(x, V, head, nvec);
    if (((uintptr_t)(o + head) & 15) == 0) {  // (uniform over the workgroup) the output is aligned where the input is
      const int vec_end = head + nvec * kE, ns = V - nvec * kE;
      for (int i = threadIdx.x; i < nvec; i += 256) {
        float v[kE];
        lsm_ld16(x + head + i * kE, v);
        f32x4_t* dst = reinterpret_cast<f32x4_t*>(o + head + i * kE);
#pragma unroll
        for (int q = 0; q < kE / 4; ++q) {
          const f32x4_t w = {v[4 * q] - lse, v[4 * q + 1] - lse, v[4 * q + 2] - lse, v[4 * q + 3] - lse};
          dst[q] = w;
        }
      }
      const int c = lsm_scalar_col(threadIdx.x, head, vec_end, V);
      const float v = lsm_ld(x, c);
      if ((int)threadIdx.x < ns) o[c] = v - lse;
      return;
    }
  }
  for (int c = threadIdx.x; c < V; c += 256) o[c] = lsm_ld(x, c) - lse;
}
