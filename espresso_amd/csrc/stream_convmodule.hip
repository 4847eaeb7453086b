// Streamed middle of a CAUSAL Conformer convolution module (GLU -> depthwise Conv1d with KW-1 frames of left context ->
// BatchNorm1d with running statistics -> SiLU), one chunk at a time for many streams.
//
// State of one layer: carry bf16 [max_streams][KW-1][C], the last KW-1 rows of U = a*sigmoid(g) of every stream, oldest first.
// A zeroed slab is the utterance's left zero padding.  With X = [carry ; U of the chunk's n rows],
//   Z[j] = bf16(sum_k w[k] * X[j + k]),  k ascending, fp32          (the rows glu_dwconv_fwd_kernel<KW, KW-1> sees)
//   H[j] = bf16(silu(Z[j] * sc + sh))                                (bn_act_fwd_kernel's arithmetic)
// and the slab becomes the last KW-1 rows of X.
//
// One workgroup per (batch entry, 64-channel tile).  Every 16-byte load of the tile (carry rows, a and g of the new rows) is
// requested before the first use; X is kept in LDS as the bf16 values the convolution consumes, Z goes through a second LDS
// tile so that H, Z and the new carry leave as 16-byte rows.  The workgroup is the only reader and the only writer of its
// slab columns and has read all of them before the barrier, so the slab is updated in place.
#include "common.h"
#include "convmodule_math.h"
#include "espresso_amd.h"

namespace {

constexpr int SC_CT = 64;       // channels per workgroup
constexpr int SC_MAXCS = 128;   // rows per chunk
constexpr int SC_NCH = SC_MAXCS * (SC_CT / 8) / 256;  // 16-byte chunks of the new rows per thread (each of a and g)

template <int KW>
__global__ __launch_bounds__(256) void stream_glu_dwconv_bn_act_kernel(
    const bf16_t* __restrict__ Y, const float* __restrict__ w, const float* __restrict__ mean_rstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, bf16_t* __restrict__ carry, const int* __restrict__ slot_idx, const int* __restrict__ n_new,
    const int* __restrict__ row_off, bf16_t* __restrict__ H, bf16_t* __restrict__ Z, int C, int cs, int max_streams, int total_rows) {
  constexpr int HALO = KW - 1;
  static_assert(HALO * (SC_CT / 8) <= 256, "one carry chunk per thread");
  extern __shared__ __attribute__((aligned(16))) char sc_smem[];
  const int b = blockIdx.x, c0 = blockIdx.y * SC_CT;
  const int n = n_new[b], slot = slot_idx[b], r0 = row_off[b];
  if (n <= 0 || n > cs || slot < 0 || slot >= max_streams || r0 < 0 || r0 + n > total_rows) return;  // (uniform per workgroup)
  bf16_t (*sx)[SC_CT] = reinterpret_cast<bf16_t (*)[SC_CT]>(sc_smem);           // [HALO + n][CT]: X
  bf16_t (*sz)[SC_CT] = reinterpret_cast<bf16_t (*)[SC_CT]>(sc_smem) + HALO + cs;  // [n][CT]: Z
  bf16_t* slab = carry + (long)slot * HALO * C;
  const int c8 = (threadIdx.x & 7) * 8, rr = threadIdx.x >> 3;  // this thread's 8-channel chunk (the same on every trip) and row
  const bool c_ok = c0 + c8 < C;                                // C % 8 == 0: a chunk is inside or outside as a whole
  const int cc = c_ok ? c0 + c8 : 0;                            // (clamped address, the value is dropped)
  // ---- every load first ----
  uint4 vc, va[SC_NCH], vg[SC_NCH];
  vc = *reinterpret_cast<const uint4*>(slab + (long)min(rr, HALO - 1) * C + cc);
#pragma unroll
  for (int k = 0; k < SC_NCH; ++k) {
    va[k] = vg[k] = make_uint4(0, 0, 0, 0);
    if (32 * k < n) {  // (uniform)
      const bf16_t* yr = Y + (long)(r0 + min(rr + 32 * k, n - 1)) * (2L * C) + cc;
      va[k] = *reinterpret_cast<const uint4*>(yr);
      vg[k] = *reinterpret_cast<const uint4*>(yr + C);
    }
  }
  const int cl = threadIdx.x & (SC_CT - 1), grp = threadIdx.x >> 6;
  float wk[KW];
#pragma unroll
  for (int k = 0; k < KW; ++k) wk[k] = c0 + cl < C ? w[(long)(c0 + cl) * KW + k] : 0.f;
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bn_scale_shift(mean_rstd[cc + e], mean_rstd[C + cc + e], gamma[cc + e], beta[cc + e], sc[e], sh[e]);
  // ---- X = [carry ; gated new rows] ----
  if (!c_ok) vc = make_uint4(0, 0, 0, 0);  // (channels past C of a ragged last tile)
  if (rr < HALO) *reinterpret_cast<uint4*>(&sx[rr][c8]) = vc;
#pragma unroll
  for (int k = 0; k < SC_NCH; ++k) {
    const int row = rr + 32 * k;
    uint4 u4 = glu_gate8(va[k], vg[k]);
    if (!c_ok) u4 = make_uint4(0, 0, 0, 0);
    if (row < n) *reinterpret_cast<uint4*>(&sx[HALO + row][c8]) = u4;
  }
  __syncthreads();
  // ---- Z rows grp, grp + 4, ... of channel cl, taps ascending ----
  for (int j = grp; j < n; j += 4) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < KW; ++k) acc += wk[k] * bf2f(sx[j + k][cl]);
    sz[j][cl] = f2bf(acc);
  }
  __syncthreads();
  // ---- H, Z and the new carry leave as 16-byte rows ----
  if (!c_ok) return;
#pragma unroll
  for (int k = 0; k < SC_NCH; ++k) {
    const int row = rr + 32 * k;
    if (row >= n) break;
    const uint4 z8 = *reinterpret_cast<const uint4*>(&sz[row][c8]);
    if (Z) *reinterpret_cast<uint4*>(Z + (long)(r0 + row) * C + cc) = z8;
    *reinterpret_cast<uint4*>(H + (long)(r0 + row) * C + cc) = bn_act8(z8, sc, sh, 2);
  }
  if (rr < HALO) *reinterpret_cast<uint4*>(slab + (long)rr * C + cc) = *reinterpret_cast<const uint4*>(&sx[n + rr][c8]);
}

}  // namespace

extern "C" int ea_stream_convmodule_supported(int C, int KW, int chunk_size) {
  if (KW != 3 && KW != 7 && KW != 15 && KW != 31) return 0;
  return C > 0 && C % 8 == 0 && chunk_size >= 1 && chunk_size <= SC_MAXCS;
}

extern "C" int ea_stream_glu_dwconv_bn_act(const void* Y, const float* w, const float* mean_rstd, const float* gamma, const float* beta,
                                           void* carry, const int* slot_idx, const int* n_new, const int* row_off, void* H, void* Z,
                                           int B, int C, int KW, int chunk_size, int max_streams, int total_rows, hipStream_t stream) {
  if (B <= 0) return 0;
  if (!ea_stream_convmodule_supported(C, KW, chunk_size) || max_streams < 1) return -2;
  const dim3 grid(B, (C + SC_CT - 1) / SC_CT);
  const size_t lds = (size_t)(KW - 1 + 2 * chunk_size) * SC_CT * sizeof(bf16_t);
#define EA_SC_LAUNCH(K)                                                                                                            \
  hipLaunchKernelGGL(stream_glu_dwconv_bn_act_kernel<K>, grid, dim3(256), lds, stream, (const bf16_t*)Y, w, mean_rstd, gamma, beta, \
                     (bf16_t*)carry, slot_idx, n_new, row_off, (bf16_t*)H, (bf16_t*)Z, C, chunk_size, max_streams, total_rows)
  switch (KW) {
    case 3: EA_SC_LAUNCH(3); break;
    case 7: EA_SC_LAUNCH(7); break;
    case 15: EA_SC_LAUNCH(15); break;
    default: EA_SC_LAUNCH(31); break;
  }
#undef EA_SC_LAUNCH
  return EA_CHECK_LAUNCH();
}
