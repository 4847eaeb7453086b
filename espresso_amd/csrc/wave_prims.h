// Wave-level primitives shared by the MFMA kernels: MFMA wrappers, the transposing LDS reads (ds_read_b64_tr_b16) issued from inline
// asm, the counted waits behind global_load_lds, the direct-to-LDS load, the XCD-aware grid remap and the swizzles of the LDS images
// that more than one kernel uses.
//
// The rule these helpers exist to keep (CDNA HIP programming guide, "Inline asm in a HIP kernel: what hipcc does not do for an `asm`
// statement", item 1): hipcc does not count a load issued from inline asm.  It emits no s_waitcnt for it and takes the destination
// registers as written when the statement ends, so it may copy, spill or consume them before the data has landed.  Hence
//   * a read and its `s_waitcnt lgkmcnt(0)` sit in ONE statement with early-clobber outputs (trr16 / trr8 / trr8x1 / trr20), or
//   * the reads are issued un-waited (read8) and EVERY destination is tied "+v" to the wait statement that completes them
//     (wait8 / wait16), so that no consumer can be scheduled above the wait;
//   * global_load_lds has no register destination, but its data is only in LDS after the caller's own counted `vmcnt` wait
//     (wait_vmcnt<N>) followed by a barrier: __syncthreads() does not wait for it.
// Why asm at all: through the builtin, hipcc puts `s_waitcnt vmcnt(0)` in front of the first transposing read of every tile (it cannot
// tell the read from the global_load_lds writes in flight), which drains the operand prefetch in the middle of the tile it should
// overlap with.
#pragma once
#include "common.h"

namespace {

typedef short bf16x4_t __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// ---- MFMA ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4_t mfma32(bf16x8_t a, bf16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(__attribute__((ext_vector_type(8))) __bf16, a),
                                                 __builtin_bit_cast(__attribute__((ext_vector_type(8))) __bf16, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4_t mfma16(bf16x4_t a, bf16x4_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x4_t pack4(float a, float b, float c, float d) {
  uint2 pk;
  pk.x = pack_bf2(a, b);
  pk.y = pack_bf2(c, d);
  return __builtin_bit_cast(bf16x4_t, pk);
}

// ---- transposing reads --------------------------------------------------------------------------------------------------------
// ds_read_b64_tr_b16: lane (g = lane>>4, i = lane&15) passes the address of element [k0(g) + (i>>2)][m0 + 4*(i&3)] of a row-major
// image and receives the four elements [k0(g) + e][m0 + i], e = 0..3 (probed on hardware: tools/probes/tr_read_probe.hip).
__device__ __forceinline__ uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)p; }
// 4 addresses x 4 immediate offsets -> o[a*4 + q] = image at ad[a] + OFFq
template <int O0, int O1, int O2, int O3>
__device__ __forceinline__ void trr16(const uint32_t (&ad)[4], uint2 (&o)[16]) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %16 offset:%20\n\tds_read_b64_tr_b16 %1, %16 offset:%21\n\t"
      "ds_read_b64_tr_b16 %2, %16 offset:%22\n\tds_read_b64_tr_b16 %3, %16 offset:%23\n\t"
      "ds_read_b64_tr_b16 %4, %17 offset:%20\n\tds_read_b64_tr_b16 %5, %17 offset:%21\n\t"
      "ds_read_b64_tr_b16 %6, %17 offset:%22\n\tds_read_b64_tr_b16 %7, %17 offset:%23\n\t"
      "ds_read_b64_tr_b16 %8, %18 offset:%20\n\tds_read_b64_tr_b16 %9, %18 offset:%21\n\t"
      "ds_read_b64_tr_b16 %10, %18 offset:%22\n\tds_read_b64_tr_b16 %11, %18 offset:%23\n\t"
      "ds_read_b64_tr_b16 %12, %19 offset:%20\n\tds_read_b64_tr_b16 %13, %19 offset:%21\n\t"
      "ds_read_b64_tr_b16 %14, %19 offset:%22\n\tds_read_b64_tr_b16 %15, %19 offset:%23\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7]), "=&v"(o[8]),
        "=&v"(o[9]), "=&v"(o[10]), "=&v"(o[11]), "=&v"(o[12]), "=&v"(o[13]), "=&v"(o[14]), "=&v"(o[15])
      : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3]), "i"(O0), "i"(O1), "i"(O2), "i"(O3)
      : "memory");
}
// 2 addresses x 4 immediate offsets
template <int O0, int O1, int O2, int O3>
__device__ __forceinline__ void trr8(const uint32_t (&ad)[2], uint2 (&o)[8]) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8 offset:%10\n\tds_read_b64_tr_b16 %1, %8 offset:%11\n\t"
      "ds_read_b64_tr_b16 %2, %8 offset:%12\n\tds_read_b64_tr_b16 %3, %8 offset:%13\n\t"
      "ds_read_b64_tr_b16 %4, %9 offset:%10\n\tds_read_b64_tr_b16 %5, %9 offset:%11\n\t"
      "ds_read_b64_tr_b16 %6, %9 offset:%12\n\tds_read_b64_tr_b16 %7, %9 offset:%13\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7])
      : "v"(ad[0]), "v"(ad[1]), "i"(O0), "i"(O1), "i"(O2), "i"(O3)
      : "memory");
}
// 8 addresses, no offsets
__device__ __forceinline__ void trr8x1(const uint32_t (&ad)[8], uint2 (&o)[8]) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8\n\tds_read_b64_tr_b16 %1, %9\n\tds_read_b64_tr_b16 %2, %10\n\tds_read_b64_tr_b16 %3, %11\n\t"
      "ds_read_b64_tr_b16 %4, %12\n\tds_read_b64_tr_b16 %5, %13\n\tds_read_b64_tr_b16 %6, %14\n\tds_read_b64_tr_b16 %7, %15\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7])
      : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3]), "v"(ad[4]), "v"(ad[5]), "v"(ad[6]), "v"(ad[7])
      : "memory");
}
// 20 addresses, no offsets (the five 16-row blocks of a wave's positional window x four 16-column tiles)
__device__ __forceinline__ void trr20(const uint32_t (&ad)[20], uint2 (&o)[20]) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %20\n\tds_read_b64_tr_b16 %1, %21\n\tds_read_b64_tr_b16 %2, %22\n\tds_read_b64_tr_b16 %3, %23\n\t"
      "ds_read_b64_tr_b16 %4, %24\n\tds_read_b64_tr_b16 %5, %25\n\tds_read_b64_tr_b16 %6, %26\n\tds_read_b64_tr_b16 %7, %27\n\t"
      "ds_read_b64_tr_b16 %8, %28\n\tds_read_b64_tr_b16 %9, %29\n\tds_read_b64_tr_b16 %10, %30\n\tds_read_b64_tr_b16 %11, %31\n\t"
      "ds_read_b64_tr_b16 %12, %32\n\tds_read_b64_tr_b16 %13, %33\n\tds_read_b64_tr_b16 %14, %34\n\tds_read_b64_tr_b16 %15, %35\n\t"
      "ds_read_b64_tr_b16 %16, %36\n\tds_read_b64_tr_b16 %17, %37\n\tds_read_b64_tr_b16 %18, %38\n\tds_read_b64_tr_b16 %19, %39\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7]), "=&v"(o[8]),
        "=&v"(o[9]), "=&v"(o[10]), "=&v"(o[11]), "=&v"(o[12]), "=&v"(o[13]), "=&v"(o[14]), "=&v"(o[15]), "=&v"(o[16]),
        "=&v"(o[17]), "=&v"(o[18]), "=&v"(o[19])
      : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3]), "v"(ad[4]), "v"(ad[5]), "v"(ad[6]), "v"(ad[7]), "v"(ad[8]), "v"(ad[9]),
        "v"(ad[10]), "v"(ad[11]), "v"(ad[12]), "v"(ad[13]), "v"(ad[14]), "v"(ad[15]), "v"(ad[16]), "v"(ad[17]), "v"(ad[18]),
        "v"(ad[19])
      : "memory");
}
// eight transposing reads (4 addresses x 2 row offsets), NOT waited for: o[2 a + h] = address a at offset h
template <int O0, int O1>
__device__ __forceinline__ void read8(const uint32_t (&ad)[4], uint2 (&o)[8]) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8 offset:%12\n\tds_read_b64_tr_b16 %1, %8 offset:%13\n\t"
      "ds_read_b64_tr_b16 %2, %9 offset:%12\n\tds_read_b64_tr_b16 %3, %9 offset:%13\n\t"
      "ds_read_b64_tr_b16 %4, %10 offset:%12\n\tds_read_b64_tr_b16 %5, %10 offset:%13\n\t"
      "ds_read_b64_tr_b16 %6, %11 offset:%12\n\tds_read_b64_tr_b16 %7, %11 offset:%13"
      : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7])
      : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3]), "i"(O0), "i"(O1)
      : "memory");
}
// the wait for every outstanding LDS read; the registers of the reads it completes are tied to it so that no consumer is
// scheduled above it
__device__ __forceinline__ void wait8(uint2 (&o)[8]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]), "+v"(o[4]), "+v"(o[5]), "+v"(o[6]), "+v"(o[7])
               :
               : "memory");
}
__device__ __forceinline__ void wait16(uint2 (&o)[8], uint2 (&q)[8]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]), "+v"(o[4]), "+v"(o[5]), "+v"(o[6]), "+v"(o[7]), "+v"(q[0]), "+v"(q[1]),
                 "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7])
               :
               : "memory");
}
// two 4-element results (rows k .. k+3 and k+4 .. k+7 of one column) -> one 16x16x32 MFMA operand
__device__ __forceinline__ bf16x8_t cat2(uint2 lo, uint2 hi) {
  return __builtin_bit_cast(bf16x8_t, make_uint4(lo.x, lo.y, hi.x, hi.y));
}

// ---- waits --------------------------------------------------------------------------------------------------------------------
// tile kt of a global_load_lds ring has landed once at most N younger load instructions of this wavefront are outstanding
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N == 0 || N == 2 || N == 3 || N == 4 || N == 6 || N == 8 || N == 9 || N == 12 || N == 16 || N == 18, "vmcnt value not listed");
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 9) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
  else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
}
// LDS traffic only (not __syncthreads(): that also waits for a prefetch in flight)
__device__ __forceinline__ void wait_lgkmcnt0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// ---- small helpers ------------------------------------------------------------------------------------------------------------
// 16 bytes per lane, global -> LDS: the wave instruction fills 1 KB from `ldst` (wave-uniform) on, lane l at byte 16 l
__device__ __forceinline__ void glds16(const void* gsrc, void* ldst) {
  __builtin_amdgcn_global_load_lds((gptr_t)gsrc, (lptr_t)ldst, 16, 0, 0);
}
// bijective XCD-aware remap of a 1-D grid (8 XCDs, round-robin dispatch): consecutive virtual ids stay on one XCD and so share
// ONE L2
__device__ __forceinline__ int xcd_remap(int id, int total) {
  const int xcd = id & 7, q = total >> 3, r = total & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
}
// LDS written by some lanes of this wave, read by others (no other wave touches the wave's slab)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- swizzles of the images that more than one kernel reads with transposing reads ---------------------------------------------
// [k rows][64 columns] bf16 image, 128-byte rows: 32-byte chunk c of row r is stored at chunk c ^ tr_sw_rows128(r), which makes the
// 8 rows x 32 bytes one 32-lane read cycle touches hit 64 distinct banks
__device__ __forceinline__ int tr_sw_rows128(int r) { return (r & 3) ^ ((r >> 3) & 1); }
// [64 k rows][128 or 256 columns] bf16 image, 256- or 512-byte rows: the 16-byte slot s of row r holds source slot
// s ^ tr_sw_rows256(r).  A half-wave of a transposing read touches rows {8g + e : g in a pair, e < 4} x 32 bytes: the term gives those
// 8 rows 8 different 32-byte positions of a 256-byte bank window, and does not change under the +4-row / +32-row immediates
__device__ __forceinline__ int tr_sw_rows256(int r) { return ((r & 3) | ((r >> 1) & 4)) << 1; }

}  // namespace
