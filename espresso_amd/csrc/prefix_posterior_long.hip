// Per-token posteriors of ONE label sequence of any length for gfx950: the sum-product twin of the tiled aligner in
// align_long.hip, as ctc_prefix_kernel (prefix_posterior.hip) is the twin of the one-workgroup aligner; DESIGN.md section 3.10.
// The reference has nothing comparable.  Lattice, move rules and conventions are ctc_prefix_kernel's (Psi_i = log-sum over frames
// of the mass ENTERING token i's state times the frame's emission, the self-loop left out; the t == 0 case; factors clamped to
// <= 0; -inf, never NaN, from the first Psi = -inf on; NaN for a bad target id), the fp32 operations are the same ones in the same
// order (prefix_math.h).  Tiling and ordering are ctc_long_tile_kernel's:
//   ctc_prefix_long_fill_kernel: alpha[] = psi[] = -inf; block b leaves in bad[b] whether it saw a target id outside [0, V) or
//     equal to blank.
//   ctc_prefix_long_tile_kernel: one launch per anti-diagonal i + j = d of tiles of kTB frames x kTS states, one wave per tile,
//     16 states per thread.  A tile takes the scores of its states in the frame before its block from alpha[S] and leaves its last
//     frame there, takes the two states left of it in every frame from edge[j - 1][t][2] and leaves its own two last states in
//     edge[j][t][2], and each thread loads the 8 accumulators of its odd states from psi[U] at the start and stores them at the
//     end: a token's accumulation stays in frame order.  Tiles of one launch touch disjoint parts of the three buffers; ORDER
//     BETWEEN WORKGROUPS COMES FROM LAUNCH BOUNDARIES ONLY: no grid barrier, no cooperative launch, no flag a workgroup waits on.
//     Inside a tile the frame loop is ctc_prefix_kernel's: double-buffered LDS score vector (entries 0, 1: the two states left of
//     the tile), one raw barrier per frame, blank + the thread's 8 label columns requested four frames ahead from a clamped row,
//     no load in a divergent branch.  A tile wholly above the reachable cone (its first state > 2 t + 1 for its last frame t)
//     computes nothing and leaves -inf.  There is no upper cone: Psi counts prefixes whether or not they can still reach the end.
//   ctc_prefix_long_finish_kernel: grid-strided over U + 1: the target check (NaN everywhere), total = lse2(alpha[S-1],
//     alpha[S-2]), logc[u] and, when asked for, psi_out[u].
// There are no backpointers: the workspace is alpha + edge + psi (+ the fill kernel's flags).
#include <algorithm>

#include "common.h"
#include "espresso_amd.h"
#include "prefix_math.h"

namespace {

constexpr int kTB = 128;        // frames per tile and
constexpr int kTS = 1024;       // states per tile: align_long.hip's, which ea_ctc_viterbi_long_tile reports (tests/test_long_posteriors.py)
constexpr int kNT = kTS / 16;   // threads per tile: one wave
constexpr int kMaxFill = 2048;  // blocks of the fill kernel (one flag each)
static_assert(kTB % 4 == 0 && kTS % 32 == 0 && kNT % 64 == 0, "tile shape");

// where the buffers sit in the workspace; every count is a multiple of 64 elements
struct Layout {
  long nI, nJ;  // frame blocks, state tiles
  long Tp, Sp;  // padded frames, padded states
  long edge_off, psi_off, bad_off, bytes;
};

__host__ inline Layout layout(long T, long U) {
  Layout l;
  const long S = 2 * U + 1;
  l.nI = (T + kTB - 1) / kTB;
  l.nJ = (S + kTS - 1) / kTS;
  l.Tp = l.nI * kTB;
  l.Sp = l.nJ * kTS;
  l.edge_off = 4 * l.Sp;
  l.psi_off = l.edge_off + 8 * l.nJ * l.Tp;
  l.bad_off = l.psi_off + 4 * (l.Sp / 2);
  l.bytes = l.bad_off + 4 * kMaxFill;
  return l;
}

template <typename TX>
__device__ __forceinline__ float ldx(const TX* p, long i) {
  if constexpr (sizeof(TX) == 2) return bf2f(p[i]); else return p[i];
}

struct Emis {  // the columns one thread needs in one frame: blank and the labels of its 8 odd states
  float b, y[8];
};

__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the LDS hand-off only: prefetched global loads stay in flight
  __builtin_amdgcn_s_barrier();
}

__global__ __launch_bounds__(256) void ctc_prefix_long_fill_kernel(const int* __restrict__ targets, float* __restrict__ alpha,
                                                                   float* __restrict__ psi, int* __restrict__ bad_out, long Sp, long U,
                                                                   int V, int blank) {
  int bad = 0;
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < Sp; k += (long)gridDim.x * blockDim.x) {  // (U <= Sp / 2)
    alpha[k] = -INFINITY;
    if (k < Sp / 2) psi[k] = -INFINITY;
    if (k < U) {
      const int y = targets[k];
      bad |= y < 0 || y >= V || y == blank;
    }
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) bad_out[blockIdx.x] = bad;
}

template <typename TX>
__global__ __launch_bounds__(kNT) void ctc_prefix_long_tile_kernel(const TX* __restrict__ x, long ld, const int* __restrict__ targets,
                                                                   float* __restrict__ alpha, float* __restrict__ edge,
                                                                   float* __restrict__ psi_g, int T, int V, int U, int blank, int d,
                                                                   int i_lo, long Tp) {
  __shared__ __attribute__((aligned(16))) float s_a[2][kTS + 2];  // [buffer][2 + local state]: entries 0, 1 are the two states left of the tile
  __shared__ __attribute__((aligned(16))) float s_in[2 * (kTB + 1)];  // those two states in the frames t0 - 1 .. t0 + kTB - 1
  __shared__ __attribute__((aligned(16))) float s_out[2 * kTB];  // the tile's own two last states in its frames
  const int i = threadIdx.x;
  const int bi = i_lo + blockIdx.x, bj = d - bi;
  const int t0 = bi * kTB;
  const int S = 2 * U + 1;
  const int g = bj * kNT + i;  // the thread's index over the whole state axis: states 16g .. 16g + 15, tokens 8g .. 8g + 7
  float* eout = edge + ((long)bj * Tp + t0) * 2;
  if ((long)bj * kTS > 2L * (t0 + kTB - 1) + 1) {  // (uniform) above the cone in every frame of the block: alpha and psi stay -inf
    for (int k = i; k < 2 * kTB / 4; k += kNT) reinterpret_cast<float4*>(eout)[k] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    return;
  }

  // labels of this thread's odd states 16g + 2k + 1 (token u = 8g + k), clamped to a valid column; bit k of `skip`: the +2 move
  // into that state is allowed.  A bad id is read as blank here and reported by the fill and finish kernels.
  int col[8];
  unsigned skip = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int u = 8 * g + k;
    const int uc = min(u, max(U - 1, 0));
    const int y = U > 0 ? targets[uc] : blank, yp = U > 0 ? targets[max(uc - 1, 0)] : blank;
    const bool real = u < U;
    col[k] = (real && y >= 0 && y < V) ? y : blank;
    if (real && u > 0 && y != yp) skip |= 1u << k;
  }

  auto fetch = [&](int t, Emis& e) {
    const TX* r = x + (long)min(t, T - 1) * ld;
    e.b = ldx(r, blank);
#pragma unroll
    for (int k = 0; k < 8; ++k) e.y[k] = ldx(r, col[k]);
  };
  Emis q0, q1, q2, q3;
  fetch(t0, q0);
  fetch(t0 + 1, q1);
  fetch(t0 + 2, q2);
  fetch(t0 + 3, q3);

  float* prev = s_a[0];
  float* cur = s_a[1];
  const int s0 = 16 * i;
  float psi[8];
  float* pg = psi_g + (long)bj * (kTS / 2) + 8 * i;
  {  // the frame before the block: the tile's states from alpha, the two states left of it (and their later frames) from edge
    const float* ain = alpha + (long)bj * kTS + s0;
#pragma unroll
    for (int k = 0; k < 16; k += 4) {
      const float4 v = *reinterpret_cast<const float4*>(ain + k);
      *reinterpret_cast<float2*>(prev + 2 + s0 + k) = make_float2(v.x, v.y);
      *reinterpret_cast<float2*>(prev + 4 + s0 + k) = make_float2(v.z, v.w);
    }
    const float4 pa = *reinterpret_cast<const float4*>(pg), pb = *reinterpret_cast<const float4*>(pg + 4);
    psi[0] = pa.x; psi[1] = pa.y; psi[2] = pa.z; psi[3] = pa.w;
    psi[4] = pb.x; psi[5] = pb.y; psi[6] = pb.z; psi[7] = pb.w;
    const float* ein = edge + (long)max(bj - 1, 0) * Tp * 2;
    for (int k = i; k < 2 * (kTB + 1); k += kNT) {
      const int t = t0 - 1 + (k >> 1);
      const float v = ein[(long)max(t, 0) * 2 + (k & 1)];
      const float w = (bj == 0 || t < 0) ? -INFINITY : v;
      s_in[k] = w;
      if (k < 2) prev[k] = w;
    }
  }
  __syncthreads();

  // one frame, as in ctc_prefix_kernel: new[s] = lse(stay, +1, +2) + x[t][label(s)], and for an odd state psi += (+1, +2 mass) *
  // x[t][label].  No branch around the loads; frames from T on keep the scores and add nothing.
  auto step = [&](int tt, Emis& q) {
    const int t = t0 + tt;
    const bool live = t < T;
    const Emis& e = q;
    float p[18];
#pragma unroll
    for (int j = 0; j < 18; j += 2) {
      const float2 v = *reinterpret_cast<const float2*>(prev + s0 + j);
      p[j] = v.x; p[j + 1] = v.y;
    }
    float o[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int s = 16 * g + j;
      const float st = p[j + 2], m1 = p[j + 1];
      float v;
      if (j & 1) {
        const int k = j >> 1;
        const float m2 = ((skip >> k) & 1u) ? p[j] : -INFINITY;
        float enter = lse2(m1, m2) + e.y[k];
        v = lse2(st + e.y[k], enter);
        if (t == 0) { enter = (s == 1 && S > 1) ? e.y[0] : -INFINITY; v = enter; }
        if (live && s < S) psi[k] = lse2(psi[k], enter);
      } else {
        v = lse2(st, m1) + e.b;
        if (t == 0) v = s == 0 ? e.b : -INFINITY;
      }
      o[j] = live ? (s < S ? v : -INFINITY) : st;
    }
    fetch(t + 4, q);  // (after the last use of the set: the load can then take the same registers)
#pragma unroll
    for (int j = 0; j < 16; j += 2) *reinterpret_cast<float2*>(cur + s0 + 2 + j) = make_float2(o[j], o[j + 1]);
    if (i == 0) *reinterpret_cast<float2*>(cur) = *reinterpret_cast<const float2*>(s_in + 2 * (tt + 1));
    if (i == kNT - 1) *reinterpret_cast<float2*>(s_out + 2 * tt) = make_float2(o[14], o[15]);
    lds_barrier();
    float* tmp = prev; prev = cur; cur = tmp;
  };
  for (int tt = 0; tt < kTB; tt += 4) {
    step(tt, q0);
    step(tt + 1, q1);
    step(tt + 2, q2);
    step(tt + 3, q3);
  }
  {
    float* aout = alpha + (long)bj * kTS + s0;
#pragma unroll
    for (int k = 0; k < 16; k += 4) {
      const float2 a = *reinterpret_cast<const float2*>(prev + 2 + s0 + k), b = *reinterpret_cast<const float2*>(prev + 4 + s0 + k);
      *reinterpret_cast<float4*>(aout + k) = make_float4(a.x, a.y, b.x, b.y);
    }
    *reinterpret_cast<float4*>(pg) = make_float4(psi[0], psi[1], psi[2], psi[3]);
    *reinterpret_cast<float4*>(pg + 4) = make_float4(psi[4], psi[5], psi[6], psi[7]);
    for (int k = i; k < 2 * kTB / 4; k += kNT) reinterpret_cast<float4*>(eout)[k] = reinterpret_cast<const float4*>(s_out)[k];
  }
}

// logc[u] = Psi_{u+1} - Psi_u for u < U, logc[U] = total - Psi_U (Psi_0 = 0); psi_out[u] = Psi_{u+1}
__global__ __launch_bounds__(256) void ctc_prefix_long_finish_kernel(const float* __restrict__ alpha, const float* __restrict__ psi,
                                                                     const int* __restrict__ bad_in, int n_bad,
                                                                     float* __restrict__ logc, float* __restrict__ total,
                                                                     float* __restrict__ psi_out, long T, long U) {
  int bad = 0;
  for (int k = threadIdx.x; k < n_bad; k += blockDim.x) bad |= bad_in[k];
  bad = __syncthreads_or(bad);  // a target id outside [0, V) or equal to blank: every output NaN
  const long S = 2 * U + 1;
  float tot;
  if (bad) tot = quiet_nan();
  else if (T == 0) tot = U == 0 ? 0.f : -INFINITY;  // no frame: only the empty sequence is possible
  else tot = lse2(alpha[S - 1], S >= 2 ? alpha[S - 2] : -INFINITY);
  for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u <= U; u += (long)gridDim.x * blockDim.x) {
    float c, po = -INFINITY;
    if (bad) {
      c = po = quiet_nan();
    } else if (T == 0) {
      c = tot;
    } else {
      const float lo = u > 0 ? psi[u - 1] : 0.f;
      if (u < U) { po = psi[u]; c = factor(po, lo); }
      else c = factor(tot, lo);
    }
    logc[u] = c;
    if (psi_out && u < U) psi_out[u] = po;
    if (u == 0) total[0] = tot;
  }
}

template <typename TX>
int launch_prefix_long(const TX* x, long ld, const int* targets, void* workspace, float* logc, float* total, float* psi_out, int T,
                       int V, int U, int blank, hipStream_t stream) {
  const Layout l = layout(T, U);
  float* alpha = (float*)workspace;
  float* edge = (float*)((char*)workspace + l.edge_off);
  float* psi = (float*)((char*)workspace + l.psi_off);
  int* bad = (int*)((char*)workspace + l.bad_off);
  const int nfill = (int)std::min((l.Sp + 255) / 256, (long)kMaxFill);
  hipLaunchKernelGGL(ctc_prefix_long_fill_kernel, dim3(nfill), dim3(256), 0, stream, targets, alpha, psi, bad, l.Sp, (long)U, V, blank);
  for (long d = 0; l.nI > 0 && d < l.nI + l.nJ - 1; ++d) {  // anti-diagonal d: tiles (i, d - i), i_lo <= i <= i_hi
    const long i_lo = std::max(0L, d - (l.nJ - 1)), i_hi = std::min(d, l.nI - 1);
    hipLaunchKernelGGL(ctc_prefix_long_tile_kernel<TX>, dim3((unsigned)(i_hi - i_lo + 1)), dim3(kNT), 0, stream, x, ld,
                       targets, alpha, edge, psi, T, V, U, blank, (int)d, (int)i_lo, l.Tp);
  }
  hipLaunchKernelGGL(ctc_prefix_long_finish_kernel, dim3((unsigned)std::min(((long)U + 256) / 256, 1024L)), dim3(256), 0, stream, alpha,
                     psi, bad, nfill, logc, total, psi_out, (long)T, (long)U);
  return EA_CHECK_LAUNCH();
}

constexpr long kMaxT = 1L << 30, kMaxU = 1L << 28;  // frame and state indices stay in 32 bits (ea_ctc_viterbi_long_align's limits)

}  // namespace

extern "C" long ea_ctc_prefix_long_workspace_bytes(long T, long U) {
  if (T < 0 || U < 0 || T > kMaxT || U > kMaxU) return 0;
  return layout(T, U).bytes;
}

extern "C" int ea_ctc_prefix_long_posteriors(const void* x, long ld, int x_bf16, const int* targets, void* workspace, float* logc,
                                             float* total, float* psi, long T, int V, long U, int blank, hipStream_t stream) {
  if (T < 0 || U < 0 || T > kMaxT || U > kMaxU || V < 1 || ld < V || blank < 0 || blank >= V) return -2;
  if (x_bf16)
    return launch_prefix_long((const bf16_t*)x, ld, targets, workspace, logc, total, psi, (int)T, V, (int)U, blank, stream);
  return launch_prefix_long((const float*)x, ld, targets, workspace, logc, total, psi, (int)T, V, (int)U, blank, stream);
}
