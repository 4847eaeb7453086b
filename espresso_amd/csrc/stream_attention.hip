// Chunk-streaming self-attention over a per-stream ring K/V cache (incremental inference of encoders trained with
// `encoder.chunk_size > 0`, `chunk_right_window == 0`; espresso/tools/utils.py chunk_streaming_mask with
// always_partial_in_last=True is the function reproduced).
//
// Cache of one layer: bf16 [max_streams][W][2C], W = (L+1)*cs ring slots per stream, K in columns [0, C), V in [C, 2C).
// Chunk c of a stream lives in slots (c % (L+1))*cs .. +cs.  frames[slot] (device) counts the frames appended BEFORE the
// chunk being processed; it is a multiple of cs while the stream is running (only the last chunk is short), so the current
// chunk is c = frames / cs and ring block g holds chunk c' = c - ((c - g) mod (L+1)), valid when c' >= 0 (and, for c' == c,
// for the first n_new entries).  Absolute frame positions follow from c' — nothing is read back by the host per chunk.
//
// ea_stream_attention: one workgroup (4 waves) per (batch entry, head).  A wave takes QB query rows at a time; its lanes own
// the ring slots (lane, lane+64, ...), so one 16-byte-vector pass over a K row serves QB scores; softmax in fp32 over the
// wave; P is rounded to bf16 AFTER normalisation (as ea_relpos_softmax_fwd does on the offline masked path) and staged in
// LDS; P.V runs with lanes over the head dim (64/dh slot groups, reduced by shuffles).  The work per (stream, head) is
// n*W*dh*3 FMAs on <= 24 KiB of cache: bound by the cache bytes and the launch, not by the VALU (DESIGN.md kernel table).
#include "common.h"
#include "espresso_amd.h"
#include "wave_prims.h"

namespace {

constexpr int SA_WAVES = 4;
constexpr int SA_QB = 4;      // query rows per wave pass
constexpr int SA_MAXK = 8;    // ring slots per lane -> W <= 512
constexpr int SA_MAXW = 64 * SA_MAXK;
constexpr int SA_MAXCS = 128;

__device__ __forceinline__ void unpack8(const uint4 u, float (&f)[8]) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = __uint_as_float(w[e] << 16);
    f[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
  }
}

struct RingGeom {
  int c;      // current chunk index
  int nblk;   // L + 1
  int cs;
  int n;      // new rows of the current chunk
  // position of ring slot s (absolute frame index), or -1 when the slot holds nothing this chunk may see
  __device__ __forceinline__ int pos(int s) const {
    const int g = s / cs, off = s - g * cs;
    int back = (c - g) % nblk;
    if (back < 0) back += nblk;
    const int cp = c - back;
    if (cp < 0) return -1;
    if (cp == c && off >= n) return -1;
    return cp * cs + off;
  }
};

template <int DH>
__global__ __launch_bounds__(SA_WAVES * 64) void stream_attention_kernel(
    const bf16_t* __restrict__ qu, const bf16_t* __restrict__ qv, long ldq, const bf16_t* __restrict__ cache,
    const bf16_t* __restrict__ pp, long ldpp, int pp_center, int pp_rows, const int* __restrict__ slot_idx,
    const int* __restrict__ n_new, const int* __restrict__ row_off, const int* __restrict__ frames,
    bf16_t* __restrict__ out, long ldo, int H, int C, int cs, int L, int max_streams, int total_rows) {
  constexpr int G = 64 / DH;  // slot groups of the P.V pass
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int n = n_new[b];
  const int slot = slot_idx[b];
  const int r0 = row_off[b];
  if (n <= 0 || n > cs || slot < 0 || slot >= max_streams || r0 < 0 || r0 + n > total_rows) return;
  const int W = (L + 1) * cs;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  RingGeom rg;
  rg.c = frames[slot] / cs;
  rg.nblk = L + 1;
  rg.cs = cs;
  rg.n = n;
  const bf16_t* kc = cache + (long)slot * W * 2 * C + h * DH;
  const bf16_t* vc = kc + C;

  __shared__ __attribute__((aligned(16))) float s_q[SA_WAVES][2][SA_QB][DH];
  __shared__ __attribute__((aligned(16))) float s_p[SA_WAVES][SA_QB][SA_MAXW];

  int jpos[SA_MAXK];
#pragma unroll
  for (int kk = 0; kk < SA_MAXK; ++kk) {
    const int s = kk * 64 + lane;
    jpos[kk] = s < W ? rg.pos(s) : -1;
  }

  for (int i0 = wv * SA_QB; i0 < n; i0 += SA_WAVES * SA_QB) {
    // stage this pass's query rows as fp32 (rows past n: zeros, never stored)
    for (int e = lane; e < SA_QB * DH; e += 64) {
      const int q = e / DH, d = e - q * DH;
      const int i = i0 + q;
      float a = 0.f, c2 = 0.f;
      if (i < n) {
        a = bf2f(qu[(long)(r0 + i) * ldq + h * DH + d]);
        if (qv) c2 = bf2f(qv[(long)(r0 + i) * ldq + h * DH + d]);
      }
      s_q[wv][0][q][d] = a;
      s_q[wv][1][q][d] = c2;
    }
    wave_lds_sync();

    float sc[SA_QB][SA_MAXK];
#pragma unroll
    for (int kk = 0; kk < SA_MAXK; ++kk) {
#pragma unroll
      for (int q = 0; q < SA_QB; ++q) sc[q][kk] = -INFINITY;
      if (kk * 64 >= W) continue;
      const int s = kk * 64 + lane;
      const int pj = jpos[kk];
      if (pj < 0) continue;
      float acc[SA_QB];
#pragma unroll
      for (int q = 0; q < SA_QB; ++q) acc[q] = 0.f;
      const bf16_t* krow = kc + (long)s * 2 * C;
#pragma unroll
      for (int d0 = 0; d0 < DH; d0 += 8) {
        float kf[8];
        unpack8(*reinterpret_cast<const uint4*>(krow + d0), kf);
#pragma unroll
        for (int q = 0; q < SA_QB; ++q)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[q] = fmaf(s_q[wv][0][q][d0 + e], kf[e], acc[q]);
      }
      if (pp) {
#pragma unroll
        for (int q = 0; q < SA_QB; ++q) {
          // table row of relative position (key - query), "positive when the key is to the right of the query"
          const int r = pp_center + pj - (rg.c * cs + i0 + q);
          if (r < 0 || r >= pp_rows) continue;  // only rows of queries past n can fall outside
          const bf16_t* prow = pp + (long)r * ldpp + h * DH;
          float bd = 0.f;
#pragma unroll
          for (int d0 = 0; d0 < DH; d0 += 8) {
            float pf[8];
            unpack8(*reinterpret_cast<const uint4*>(prow + d0), pf);
#pragma unroll
            for (int e = 0; e < 8; ++e) bd = fmaf(s_q[wv][1][q][d0 + e], pf[e], bd);
          }
          acc[q] += bd;
        }
      }
#pragma unroll
      for (int q = 0; q < SA_QB; ++q) sc[q][kk] = acc[q];
    }

    // fp32 softmax per query row over the wave; probabilities rounded to bf16 after normalisation
#pragma unroll
    for (int q = 0; q < SA_QB; ++q) {
      float m = -INFINITY;
#pragma unroll
      for (int kk = 0; kk < SA_MAXK; ++kk) m = fmaxf(m, sc[q][kk]);
      m = wave_max(m);
      float sum = 0.f;
#pragma unroll
      for (int kk = 0; kk < SA_MAXK; ++kk) {
        const float e = sc[q][kk] == -INFINITY ? 0.f : __expf(sc[q][kk] - m);
        sc[q][kk] = e;
        sum += e;
      }
      sum = wave_sum(sum);
      const float inv = sum > 0.f ? 1.f / sum : 0.f;
#pragma unroll
      for (int kk = 0; kk < SA_MAXK; ++kk)
        if (kk * 64 < W && kk * 64 + lane < W) s_p[wv][q][kk * 64 + lane] = bf2f(f2bf(sc[q][kk] * inv));
    }
    wave_lds_sync();

    // P.V: lane = (slot group, d); group gi walks slots gi, gi+G, ...
    const int d = lane % DH, gi = lane / DH;
    float o[SA_QB];
#pragma unroll
    for (int q = 0; q < SA_QB; ++q) o[q] = 0.f;
    for (int s = gi; s < W; s += G) {
      if (rg.pos(s) < 0) continue;
      const float vv = bf2f(vc[(long)s * 2 * C + d]);
#pragma unroll
      for (int q = 0; q < SA_QB; ++q) o[q] = fmaf(s_p[wv][q][s], vv, o[q]);
    }
#pragma unroll
    for (int q = 0; q < SA_QB; ++q) {
      float v = o[q];
#pragma unroll
      for (int off = DH; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
      if (gi == 0 && i0 + q < n) out[(long)(r0 + i0 + q) * ldo + h * DH + d] = f2bf(v);
    }
    wave_lds_sync();  // s_q / s_p are rewritten by the next pass
  }
}

// ring append: rows of the current chunk -> slots (c % (L+1))*cs + i, K and V together (2C contiguous bf16 of the fused QKV row)
__global__ __launch_bounds__(256) void stream_kv_append_kernel(const bf16_t* __restrict__ kv, long ldkv, bf16_t* __restrict__ cache,
                                                               const int* __restrict__ slot_idx, const int* __restrict__ n_new,
                                                               const int* __restrict__ row_off, const int* __restrict__ frames,
                                                               int C, int cs, int L, int max_streams, int total_rows) {
  const int b = blockIdx.x;
  const int n = n_new[b], slot = slot_idx[b], r0 = row_off[b];
  if (n <= 0 || n > cs || slot < 0 || slot >= max_streams || r0 < 0 || r0 + n > total_rows) return;
  const int W = (L + 1) * cs;
  const int c = frames[slot] / cs;
  const int base = (c % (L + 1)) * cs;
  const int nch = (2 * C) >> 3;
  bf16_t* dst = cache + ((long)slot * W + base) * 2 * C;
  for (int e = threadIdx.x; e < n * nch; e += blockDim.x) {
    const int i = e / nch, ch = e - i * nch;
    *reinterpret_cast<uint4*>(dst + (long)i * 2 * C + ch * 8) = *reinterpret_cast<const uint4*>(kv + (long)(r0 + i) * ldkv + ch * 8);
  }
}

__global__ void stream_advance_kernel(int* __restrict__ frames, const int* __restrict__ slot_idx, const int* __restrict__ n_new,
                                      int B, int cs, int max_streams) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = n_new[b], slot = slot_idx[b];
  if (n <= 0 || n > cs || slot < 0 || slot >= max_streams) return;
  frames[slot] += n;
}

}  // namespace

extern "C" int ea_stream_attention_supported(int dh, int chunk_size, int left_chunks, int C) {
  if (dh != 16 && dh != 32 && dh != 64) return 0;
  if (chunk_size < 1 || chunk_size > SA_MAXCS || left_chunks < 0) return 0;
  if ((long)(left_chunks + 1) * chunk_size > SA_MAXW) return 0;
  return C > 0 && C % dh == 0 && C % 8 == 0;
}

extern "C" int ea_stream_kv_append(const void* kv, long ldkv, void* cache, const int* slot_idx, const int* n_new,
                                   const int* row_off, const int* frames, int B, int C, int chunk_size, int left_chunks,
                                   int max_streams, int total_rows, hipStream_t stream) {
  if (B <= 0) return 0;
  if (C <= 0 || C % 8 || ldkv % 8 || chunk_size < 1 || left_chunks < 0 || max_streams < 1) return -2;
  hipLaunchKernelGGL(stream_kv_append_kernel, dim3(B), dim3(256), 0, stream, (const bf16_t*)kv, ldkv, (bf16_t*)cache, slot_idx,
                     n_new, row_off, frames, C, chunk_size, left_chunks, max_streams, total_rows);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_stream_attention(const void* qu, const void* qv, long ldq, const void* cache, const void* pp, long ldpp,
                                   int pp_center, int pp_rows, const int* slot_idx, const int* n_new, const int* row_off,
                                   const int* frames, void* out, long ldo, int B, int H, int dh, int chunk_size, int left_chunks,
                                   int max_streams, int total_rows, hipStream_t stream) {
  if (B <= 0) return 0;
  const int C = H * dh;
  if (!ea_stream_attention_supported(dh, chunk_size, left_chunks, C) || max_streams < 1) return -2;
  if (ldq % 8 || (pp && (ldpp % 8 || !qv))) return -2;
  if (pp) {  // every (query, key) distance of a chunk must have a table row
    const int W = (left_chunks + 1) * chunk_size;
    if (pp_center - (W - 1) < 0 || pp_center + chunk_size - 1 >= pp_rows) return -2;
  }
#define EA_SA_LAUNCH(DH)                                                                                                       \
  hipLaunchKernelGGL(stream_attention_kernel<DH>, dim3(B * H), dim3(SA_WAVES * 64), 0, stream, (const bf16_t*)qu,             \
                     (const bf16_t*)(pp ? qv : nullptr), ldq, (const bf16_t*)cache, (const bf16_t*)pp, ldpp, pp_center, pp_rows, \
                     slot_idx, n_new, row_off, frames, (bf16_t*)out, ldo, H, C, chunk_size, left_chunks, max_streams, total_rows)
  if (dh == 16) EA_SA_LAUNCH(16);
  else if (dh == 32) EA_SA_LAUNCH(32);
  else EA_SA_LAUNCH(64);
#undef EA_SA_LAUNCH
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_stream_advance(int* frames, const int* slot_idx, const int* n_new, int B, int chunk_size, int max_streams,
                                 hipStream_t stream) {
  if (B <= 0) return 0;
  hipLaunchKernelGGL(stream_advance_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, frames, slot_idx, n_new, B, chunk_size,
                     max_streams);
  return EA_CHECK_LAUNCH();
}
