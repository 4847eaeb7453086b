// Per-token posteriors of ONE label sequence of any length for gfx950: the sum-product twin of the tiled aligner in
// align_long.hip, as ctc_prefix_kernel (prefix_posterior.hip) is the twin of the one-workgroup aligner; DESIGN.md section 3.10.
// The reference has nothing comparable.  The frame update is ctc_prefix_kernel's by construction (prefix_frame in ctc_lattice.h, so
// also its conventions: the t == 0 case, the self-loop left out of Psi); tiles, the alpha and edge buffers, the launch order and the
// frame loop are ctc_long_tile_kernel's, from the same header.  This file's own:
//   ctc_prefix_long_fill_kernel: alpha[] = psi[] = -inf; block b leaves in bad[b] whether it saw a target id outside [0, V) or
//     equal to blank.
//   ctc_prefix_long_tile_kernel: each thread loads the 8 accumulators of its odd states from psi[U] at the start of a tile and
//     stores them at the end: a token's accumulation stays in frame order.  A tile above the reachable cone leaves psi at -inf.
//     There is no upper cone: Psi counts prefixes whether or not they can still reach the end.
//   ctc_prefix_long_finish_kernel: grid-strided over U + 1: the target check (NaN everywhere), total = lse2(alpha[S-1],
//     alpha[S-2]), logc[u] (factors clamped to <= 0; -inf, never NaN, from the first Psi = -inf on) and, when asked for, psi_out[u].
// There are no backpointers: the workspace is alpha + edge + psi (+ the fill kernel's flags).
#include <algorithm>

#include "common.h"
#include "ctc_lattice.h"
#include "espresso_amd.h"

namespace {

constexpr int kMaxFill = 2048;  // blocks of the fill kernel (one flag each)

// the workspace: alpha, edge (ctc_lattice.h), then psi and the fill kernel's flags
struct Layout : TileLayout {
  long psi_off, bad_off, bytes;
};

__host__ inline Layout prefix_workspace(long T, long U) {
  Layout l{tile_layout(T, U)};
  l.psi_off = l.tail;
  l.bad_off = l.psi_off + 4 * (l.Sp / 2);
  l.bytes = l.bad_off + 4 * kMaxFill;
  return l;
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
  __shared__ __attribute__((aligned(16))) float s_a[2][kTS + 2];
  __shared__ __attribute__((aligned(16))) float s_in[2 * (kTB + 1)];
  __shared__ __attribute__((aligned(16))) float s_out[2 * kTB];  // (what the three hold: ctc_lattice.h)
  const int i = threadIdx.x;
  const int bi = i_lo + blockIdx.x, bj = d - bi;
  const int t0 = bi * kTB;
  const int S = 2 * U + 1;
  const int g = bj * kNT + i;  // the thread's index over the whole state axis: states 16g .. 16g + 15, tokens 8g .. 8g + 7
  float* eout = edge + ((long)bj * Tp + t0) * 2;
  if (tile_above_cone(eout, bj, t0, i)) return;  // (alpha and psi stay -inf)

  int col[8];
  unsigned skip;
  ctc_labels(targets, g, U, V, blank, col, skip);  // (a bad id is read as blank here and reported by the fill and finish kernels)
  auto fetch = [&](int t, Emis& e) { ctc_fetch(x + (long)min(t, T - 1) * ld, blank, col, e); };
  Emis q0, q1, q2, q3;
  ctc_prefetch(fetch, t0, q0, q1, q2, q3);

  float* prev = s_a[0];
  float* cur = s_a[1];
  const int s0 = 16 * i;
  float psi[8];
  float* pg = psi_g + (long)bj * (kTS / 2) + 8 * i;
  // (before the prologue, whose LDS stores wait for its own loads and with them for these: asked for last, psi would be waited
  // for inside the frame loop, with a count that drains the prefetch)
  const float4 pa = *reinterpret_cast<const float4*>(pg), pb = *reinterpret_cast<const float4*>(pg + 4);
  psi[0] = pa.x; psi[1] = pa.y; psi[2] = pa.z; psi[3] = pa.w;
  psi[4] = pb.x; psi[5] = pb.y; psi[6] = pb.z; psi[7] = pb.w;
  __builtin_amdgcn_sched_barrier(0);
  tile_prologue(prev, s_in, alpha, edge, Tp, bj, t0, i);
  __syncthreads();

  // one frame; frames from T on keep the scores and add nothing
  auto step = [&](int tt, Emis& q) {
    const int t = t0 + tt;
    float o[16];
    prefix_frame(prev + s0, q, skip, 16 * g, S, t, t < T, psi, o);
    fetch(t + 4, q);
    ctc_store(cur + s0 + 2, o);
    tile_handover(cur, s_in, s_out, o, tt, i);
    lds_barrier();
    float* tmp = prev; prev = cur; cur = tmp;
  };
  for (int tt = 0; tt < kTB; tt += 4) {
    step(tt, q0);
    step(tt + 1, q1);
    step(tt + 2, q2);
    step(tt + 3, q3);
  }
  *reinterpret_cast<float4*>(pg) = make_float4(psi[0], psi[1], psi[2], psi[3]);
  *reinterpret_cast<float4*>(pg + 4) = make_float4(psi[4], psi[5], psi[6], psi[7]);
  tile_epilogue(prev, s_out, alpha, eout, bj, i);
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
  const Layout l = prefix_workspace(T, U);
  float* alpha = (float*)workspace;
  float* edge = (float*)((char*)workspace + l.edge_off);
  float* psi = (float*)((char*)workspace + l.psi_off);
  int* bad = (int*)((char*)workspace + l.bad_off);
  const int nfill = (int)std::min((l.Sp + 255) / 256, (long)kMaxFill);
  hipLaunchKernelGGL(ctc_prefix_long_fill_kernel, dim3(nfill), dim3(256), 0, stream, targets, alpha, psi, bad, l.Sp, (long)U, V, blank);
  for_each_antidiagonal(l, [&](int d, int i_lo, unsigned count) {
    hipLaunchKernelGGL(ctc_prefix_long_tile_kernel<TX>, dim3(count), dim3(kNT), 0, stream, x, ld, targets, alpha, edge, psi, T, V, U,
                       blank, d, i_lo, l.Tp);
  });
  hipLaunchKernelGGL(ctc_prefix_long_finish_kernel, dim3((unsigned)std::min(((long)U + 256) / 256, 1024L)), dim3(256), 0, stream, alpha,
                     psi, bad, nfill, logc, total, psi_out, (long)T, (long)U);
  return EA_CHECK_LAUNCH();
}

}  // namespace

extern "C" long ea_ctc_prefix_long_workspace_bytes(long T, long U) {
  if (T < 0 || U < 0 || T > kMaxT || U > kMaxU) return 0;
  return prefix_workspace(T, U).bytes;
}

extern "C" int ea_ctc_prefix_long_posteriors(const void* x, long ld, int x_bf16, const int* targets, void* workspace, float* logc,
                                             float* total, float* psi, long T, int V, long U, int blank, hipStream_t stream) {
  if (T < 0 || U < 0 || T > kMaxT || U > kMaxU || V < 1 || ld < V || blank < 0 || blank >= V) return -2;
  if (x_bf16)
    return launch_prefix_long((const bf16_t*)x, ld, targets, workspace, logc, total, psi, (int)T, V, (int)U, blank, stream);
  return launch_prefix_long((const float*)x, ld, targets, workspace, logc, total, psi, (int)T, V, (int)U, blank, stream);
}
