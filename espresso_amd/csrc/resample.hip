// Band-limited rational resampler (polyphase Hann-windowed sinc, Kaldi's LinearResample with num_zeros = 6, roll-off 0.99) for
// ragged batches and for stream pieces, so that audio of any sample rate reaches the fbank front-end at the front-end's rate.
//
// The filter lives on the host (espresso_amd/data/resample.py builds taps[phases][K] and first[phases] in fp64 and rounds
// them once to fp32); this file only evaluates
//   y[j] = sum_k taps[p][k] * x[first[p] + u * in_unit + k],   p = j mod phases, u = j div phases,  x = 0 outside what is held,
// on ABSOLUTE sample indices j (64-bit): an offline utterance has bases 0, a stream piece carries the index of its first held
// input sample and of its first output, and both evaluate the same expression on the same operands.
//
// THE ARITHMETIC OF ONE OUTPUT IS FIXED: acc = +0; for k ascending: acc = fmaf(taps[p][k], x_k, acc), in fp32.  A sample
// that is not held enters as fmaf(w, 0, acc), which leaves acc's bits alone (acc is never -0: it starts at +0).  Streamed
// output equals offline output bit for bit because of this and of nothing else here: tiling, staging and where the table is
// read from change which memory an operand comes from, never the operand or the order.
//
// Memory-bound streaming op: one workgroup per 1024 outputs of one utterance stages the contiguous input span its outputs read
// (1024 outputs at 96 kHz -> 16 kHz: 6144 + 73 floats) in LDS once, converted to fp32, so every input sample is fetched from
// HBM once per tile and the K-fold reuse is served by LDS.  The tap table sits beside it when it fits (row stride made odd:
// consecutive threads are consecutive phases, and an odd stride spreads them over all banks); a larger table (16001 -> 16000:
// 16 000 rows) is read through L2.  A span that does not fit, or a `first` table that is not the monotone one of the
// definition, takes the direct path: the same loop with bounds-checked global reads.
#include "common.h"
#include "espresso_amd.h"

namespace {

constexpr int TILE = 1024, THREADS = 256, PER_THREAD = TILE / THREADS;
constexpr int LDS_FLOATS = 16000;  // 62.5 KB of the 64 KB a workgroup may claim here; 8 floats below are static

__device__ __forceinline__ long wave_min_l(long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}
__device__ __forceinline__ long wave_max_l(long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// span_cap: floats of dynamic LDS set aside for the input span (0: read the input from global memory); taps_lds: the table
// follows it there with row stride `tstride`.
template <typename TS>
__global__ __launch_bounds__(THREADS) void resample_kernel(
    const TS* __restrict__ in, const long* __restrict__ in_off, const long* __restrict__ in_base, float* __restrict__ out,
    const long* __restrict__ out_off, const long* __restrict__ out_base, const float* __restrict__ taps,
    const int* __restrict__ first, int phases, int K, int in_unit, int span_cap, int taps_lds, int tstride) {
  extern __shared__ float lds[];
  __shared__ long s_red[2][THREADS / 64];
  const int b = blockIdx.y, t = threadIdx.x;
  const long o0 = out_off[b];
  const long n_out = out_off[b + 1] - o0;
  const long d0 = (long)blockIdx.x * TILE;  // first output of this tile, relative to the utterance's slot
  if (d0 >= n_out) return;
  const int cnt = (int)(n_out - d0 < TILE ? n_out - d0 : TILE);
  const long i0 = in_off[b];
  const long n_in = in_off[b + 1] - i0;
  const long ib = in_base ? in_base[b] : 0;
  const long J0 = (out_base ? out_base[b] : 0) + d0;  // absolute index of the tile's first output
  const long u0 = J0 / phases;
  const int p0 = (int)(J0 - u0 * phases);
  const long x0 = u0 * in_unit;  // absolute input index of unit u0's origin

  // first input index of each of this thread's outputs, relative to x0 (fits 32 bits: TILE outputs from one origin)
  int ph[PER_THREAD];
  long st[PER_THREAD];
  long smin = INT64_MAX, smax = INT64_MIN;
#pragma unroll
  for (int i = 0; i < PER_THREAD; ++i) {
    const int d = t + THREADS * i;
    const int q = p0 + d;  // < phases + TILE
    const int du = q / phases;
    ph[i] = q - du * phases;
    st[i] = (long)first[ph[i]] + (long)du * in_unit;
    if (d < cnt) {
      smin = st[i] < smin ? st[i] : smin;
      smax = st[i] > smax ? st[i] : smax;
    }
  }
  smin = wave_min_l(smin);
  smax = wave_max_l(smax);
  if ((t & 63) == 0) {
    s_red[0][t >> 6] = smin;
    s_red[1][t >> 6] = smax;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    smin = s_red[0][w] < smin ? s_red[0][w] : smin;
    smax = s_red[1][w] > smax ? s_red[1][w] : smax;
  }
  const long span = smax - smin + K;  // inputs [x0 + smin, x0 + smin + span) cover every read of the tile
  const bool staged = span <= (long)span_cap;  // uniform over the workgroup
  const long rel0 = x0 + smin - ib;            // position of the span's first sample in what is held for the utterance

  if (staged) {
    const TS* src = in + i0;
    for (int i = t; i < (int)span; i += THREADS) {
      const long r = rel0 + i;
      lds[i] = (r >= 0 && r < n_in) ? (float)src[r] : 0.f;
    }
  }
  float* tl = lds + span_cap;
  if (taps_lds) {
    for (int i = t; i < phases * K; i += THREADS) {
      const int p = i / K;
      tl[p * tstride + (i - p * K)] = taps[i];
    }
  }
  __syncthreads();

#pragma unroll
  for (int i = 0; i < PER_THREAD; ++i) {
    const int d = t + THREADS * i;
    if (d >= cnt) break;
    const float* w = taps_lds ? tl + ph[i] * tstride : taps + (long)ph[i] * K;
    float acc = 0.f;
    if (staged) {
      const float* x = lds + (int)(st[i] - smin);
      for (int k = 0; k < K; ++k) acc = __builtin_fmaf(w[k], x[k], acc);
    } else {
      const TS* src = in + i0;
      const long r0 = x0 + st[i] - ib;
      for (int k = 0; k < K; ++k) {
        const long r = r0 + k;
        const float xv = (r >= 0 && r < n_in) ? (float)src[r] : 0.f;
        acc = __builtin_fmaf(w[k], xv, acc);
      }
    }
    out[o0 + d0 + d] = acc;
  }
}

template <typename TS>
int resample_launch(const TS* in, const long* in_offsets, const long* in_base, float* out, const long* out_offsets,
                    const long* out_base, int B, const float* taps, const int* first, int phases, int K, int in_unit,
                    long max_out, hipStream_t stream) {
  if (B <= 0 || max_out <= 0) return 0;
  if (K <= 0 || K > 4096 || phases <= 0 || in_unit <= 0 || B > 65535) return -2;
  const long tiles = (max_out + TILE - 1) / TILE;
  if (tiles > 0x7fffffffL) return -2;
  // the monotone table of the definition: TILE consecutive outputs start within (TILE - 1) * in_unit / phases + 1 inputs
  long span_cap = ((long)(TILE - 1) * in_unit + phases - 1) / phases + 2 + K;
  span_cap = (span_cap + 3) & ~3L;
  if (span_cap > LDS_FLOATS) span_cap = 0;
  const int tstride = K | 1;
  const int taps_lds = (long)phases * tstride <= LDS_FLOATS - span_cap ? 1 : 0;
  const size_t shmem = ((size_t)span_cap + (taps_lds ? (size_t)phases * tstride : 0)) * sizeof(float);
  hipLaunchKernelGGL(resample_kernel<TS>, dim3((unsigned)tiles, B), dim3(THREADS), shmem, stream, in, in_offsets, in_base, out,
                     out_offsets, out_base, taps, first, phases, K, in_unit, (int)span_cap, taps_lds, tstride);
  return EA_CHECK_LAUNCH();
}

}  // namespace

extern "C" int ea_resample_batch(const float* in, const long* in_offsets, const long* in_base, float* out,
                                 const long* out_offsets, const long* out_base, int B, const float* taps, const int* first,
                                 int phases, int K, int in_unit, long max_out, hipStream_t stream) {
  return resample_launch<float>(in, in_offsets, in_base, out, out_offsets, out_base, B, taps, first, phases, K, in_unit, max_out,
                                stream);
}
extern "C" int ea_resample_batch_i16(const int16_t* in, const long* in_offsets, const long* in_base, float* out,
                                     const long* out_offsets, const long* out_base, int B, const float* taps, const int* first,
                                     int phases, int K, int in_unit, long max_out, hipStream_t stream) {
  return resample_launch<int16_t>(in, in_offsets, in_base, out, out_offsets, out_base, B, taps, first, phases, K, in_unit, max_out,
                                  stream);
}
