// Device helpers shared by the CTC prefix beam searches (ctc_beam.hip, ctc_lexicon_beam.hip): 48-bit ordering keys,
// the workgroup-wide radix select over them, log-add-exp, the prefix hash and L2 loads of the workgroup's own writes.
#pragma once
#include "common.h"

namespace {

// L1-bypassing loads of what this workgroup's own atomics and stores wrote earlier
__device__ __forceinline__ unsigned long long ld_l2(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_l2(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t tab_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  return (uint32_t)k;
}

__device__ __forceinline__ float lae(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + log1pf(expf(-fabsf(a - b)));
}

// order-preserving map of a float to 32 unsigned bits (-0 folded into +0)
__device__ __forceinline__ uint64_t ord32(float f) {
  const uint32_t u = __float_as_uint(f + 0.f);
  return (uint64_t)(u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u));
}
// unique 48-bit key: larger value first, then lower index (0 = absent)
__device__ __forceinline__ uint64_t mk_key(float v, int idx) { return (ord32(v) << 16) | (uint64_t)(0xFFFF - idx); }

struct SelectScratch {
  unsigned hist[256];
  uint64_t prefix;
  int need, done;
};

// The n-th largest of the nonzero keys key(0..N) (blockDim 256, all threads call).  Returns 1 when there are n or fewer
// nonzero keys (then every nonzero key is selected).  MSB-first radix select, 8 bits per pass over 48-bit keys.
template <class KeyFn>
__device__ uint64_t select_nth(KeyFn key, int N, int n, SelectScratch& s) {
  const int tid = threadIdx.x;
  if (tid == 0) { s.prefix = 0; s.need = n; s.done = 0; }
  for (int shift = 40; shift >= 0; shift -= 8) {
    s.hist[tid] = 0u;
    __syncthreads();
    const uint64_t prefix = s.prefix;
    const uint64_t hi = ~0ull << (shift + 8);
    for (int i = tid; i < N; i += 256) {
      const uint64_t k = key(i);
      if (k && (k & hi) == prefix) atomicAdd(&s.hist[(k >> shift) & 255], 1u);
    }
    __syncthreads();
    if (tid < 64) {  // wave 0: lane L holds digits 255-4L .. 252-4L, scanned from the top
      unsigned c[4], tot = 0;
#pragma unroll
      for (int m = 0; m < 4; ++m) { c[m] = s.hist[255 - 4 * tid - m]; tot += c[m]; }
      unsigned incl = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o, 64);
        if (tid >= o) incl += v;
      }
      const unsigned all = __shfl(incl, 63, 64);
      const unsigned need = (unsigned)s.need;
      if (shift == 40 && all <= need) {
        if (tid == 0) s.done = 1;
      } else {
        unsigned run = incl - tot;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          if (run < need && run + c[m] >= need) {
            s.prefix = prefix | ((uint64_t)(255 - 4 * tid - m) << shift);
            s.need = (int)(need - run);
          }
          run += c[m];
        }
      }
    }
    __syncthreads();
    if (s.done) return 1;
  }
  return s.prefix;
}

template <typename TX>
__device__ __forceinline__ float ldx(const TX* p, int i) {
  if constexpr (sizeof(TX) == 2) return bf2f(p[i]); else return p[i];
}

}  // namespace
