// Long-form forced alignment for gfx950: the CTC Viterbi search of csrc/align.hip for ONE sequence whose lattice does not fit a
// workgroup (a recording's stitched log-probs against its whole transcript: ~90 000 frames x 20 000 - 120 000 states), DESIGN.md
// section 3.9.  The reference has no forced aligner of its own (it aligns through Kaldi), so these kernels replace nothing of it.
// Lattice, move rules and tie rules are those of ctc_viterbi_kernel, and because max-plus in fp32 does not reassociate, scores and
// path equal that kernel's bit for bit wherever it accepts the problem.
//
// The lattice is cut into tiles of kTB frames x kTS states; tile (i, j) = frame block i, state tile j.
//   ctc_long_init_kernel: alpha[] = -inf, token spans -1, frame labels -2, frame log-probs 0.
//   ctc_long_tile_kernel: one launch per anti-diagonal i + j = d, one workgroup (kTS / 16 threads = one wave) per tile of it.
//     A tile takes the scores of its states in the frame before its block from alpha[S] (left there by tile (i - 1, j), one launch
//     earlier) and leaves its own last frame there; it takes the scores of the two states left of its block, for every frame of
//     the block and the frame before it, from edge[j - 1][t][2] (tile (i, j - 1), one launch earlier, and tile (i - 1, j - 1), two
//     earlier) and leaves those of its own two last states in edge[j][t][2].  Tiles of one launch touch disjoint parts of all
//     three buffers; ORDER BETWEEN WORKGROUPS COMES FROM LAUNCH BOUNDARIES ONLY: no grid barrier, no cooperative launch, no flag
//     one workgroup waits on.  Inside a tile the frame loop is ctc_viterbi_kernel's: thread i owns 16 consecutive states, the
//     scores sit in LDS (double-buffered, one raw barrier per frame), blank + the thread's 8 label columns are requested four
//     frames ahead into four register sets from a clamped row (no load in a divergent branch), one 32-bit word of 2-bit
//     backpointers per thread and frame goes to the workspace with a vector store.  The edge columns pass through LDS: read once
//     per tile, written once per tile.  A tile wholly above the reachable cone (its first state > 2 t + 1 for its last frame t)
//     computes nothing: alpha stays -inf and its edge column is written as -inf.
//   ctc_long_backtrace_kernel: one workgroup.  Checks the targets (a bad id: score NaN, nothing aligned), picks the end state,
//     then walks blocks of kBtBlk frames from the end.  The state falls by at most 2 per frame, so of a block's backpointer rows
//     (S / 16 words each, far more than LDS holds) only the <= kBtW words between the lowest state the walk can reach in the
//     block and the state it enters with are staged; one lane walks them and leaves the block's states in LDS, from which all
//     threads write frame_label, frame_lp = x[t][label] and the token spans.
// Every index into the backpointer workspace and the edge buffer is 64-bit: at T = 10^6, U = 10^5 the rows hold 5 * 10^10 bytes.
#include <algorithm>

#include "common.h"
#include "espresso_amd.h"

namespace {

constexpr int kTB = 128;          // frames per tile (a multiple of 4: the prefetch depth)
constexpr int kTS = 1024;         // states per tile (even; 16 per thread)
constexpr int kNT = kTS / 16;     // threads per tile: one wave
constexpr int kBtBlk = 128;       // frames per backtrace block
constexpr int kBtW = (2 * kBtBlk - 2) / 16 + 2;  // backpointer words a block's walk can reach in one row
constexpr int kBtThreads = 256;
static_assert(kTB % 4 == 0 && kTS % 32 == 0 && kNT % 64 == 0, "tile shape");

// where the three buffers sit in the workspace; every count is a multiple of 64 elements
struct Layout {
  long nI, nJ;  // frame blocks, state tiles
  long Tp, Sp, Wp;  // padded frames, padded states, backpointer words per frame row
  long edge_off, bp_off, bytes;
};

__host__ inline Layout layout(long T, long U) {
  Layout l;
  const long S = 2 * U + 1;
  l.nI = (T + kTB - 1) / kTB;
  l.nJ = (S + kTS - 1) / kTS;
  l.Tp = l.nI * kTB;
  l.Sp = l.nJ * kTS;
  l.Wp = l.Sp / 16;
  l.edge_off = 4 * l.Sp;
  l.bp_off = l.edge_off + 8 * l.nJ * l.Tp;
  l.bytes = l.bp_off + 4 * l.Tp * l.Wp;
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

__global__ __launch_bounds__(256) void ctc_long_init_kernel(float* __restrict__ alpha, int* __restrict__ tok_start,
                                                            int* __restrict__ tok_end, int* __restrict__ frame_label,
                                                            float* __restrict__ frame_lp, long Sp, long U, long T) {
  const long m = U > T ? U : T, n = Sp > m ? Sp : m;
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long)gridDim.x * blockDim.x) {
    if (k < Sp) alpha[k] = -INFINITY;
    if (k < U) { tok_start[k] = -1; tok_end[k] = -1; }
    if (k < T) { frame_label[k] = -2; frame_lp[k] = 0.f; }
  }
}

template <typename TX>
__global__ __launch_bounds__(kNT) void ctc_long_tile_kernel(const TX* __restrict__ x, long ld, const int* __restrict__ targets,
                                                            float* __restrict__ alpha, float* __restrict__ edge,
                                                            uint32_t* __restrict__ bp, int T, int V, int U, int blank, int d,
                                                            int i_lo, long Tp, long Wp) {
  __shared__ __attribute__((aligned(16))) float s_a[2][kTS + 2];  // [buffer][2 + local state]: entries 0, 1 are the two states left of the tile
  __shared__ __attribute__((aligned(16))) float s_in[2 * (kTB + 1)];  // those two states in the frames t0 - 1 .. t0 + kTB - 1
  __shared__ __attribute__((aligned(16))) float s_out[2 * kTB];  // the tile's own two last states in its frames
  const int i = threadIdx.x;
  const int bi = i_lo + blockIdx.x, bj = d - bi;
  const int t0 = bi * kTB;
  const int S = 2 * U + 1;
  const int g = bj * kNT + i;  // the thread's index over the whole state axis: states 16g .. 16g + 15
  float* eout = edge + ((long)bj * Tp + t0) * 2;
  if ((long)bj * kTS > 2L * (t0 + kTB - 1) + 1) {  // (uniform) above the cone in every frame of the block
    for (int k = i; k < 2 * kTB / 4; k += kNT) reinterpret_cast<float4*>(eout)[k] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    return;
  }

  // labels of this thread's odd states 16g + 2k + 1 (token u = 8g + k), clamped to a valid column; bit k of `skip`: the +2 move
  // into that state is allowed.  A bad id is read as blank here and reported by the backtrace kernel.
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
  {  // the frame before the block: the tile's states from alpha, the two states left of it (and their later frames) from edge
    const float* ain = alpha + (long)bj * kTS + s0;
#pragma unroll
    for (int k = 0; k < 16; k += 4) {
      const float4 v = *reinterpret_cast<const float4*>(ain + k);
      *reinterpret_cast<float2*>(prev + 2 + s0 + k) = make_float2(v.x, v.y);
      *reinterpret_cast<float2*>(prev + 4 + s0 + k) = make_float2(v.z, v.w);
    }
    const float* ein = edge + (long)max(bj - 1, 0) * Tp * 2;
    for (int k = i; k < 2 * (kTB + 1); k += kNT) {
      const int t = t0 - 1 + (k >> 1);
      const float v = ein[(long)max(t, 0) * 2 + (k & 1)];
      const float w = (bj == 0 || t < 0) ? -INFINITY : v;
      s_in[k] = w;
      if (k < 2) prev[k] = w;
    }
  }
  uint32_t* bprow = bp + (long)t0 * Wp + g;
  __syncthreads();

  // one frame, as in ctc_viterbi_kernel: new[s] = max(stay, +1, +2) + x[t][label(s)]; ties prefer stay, then +1.  No branch
  // around the loads; frames from T on keep the scores (their backpointer rows are the padding rows T .. Tp - 1).
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
    uint32_t word = 0u;
    float o[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int s = 16 * g + j;
      const float st = p[j + 2], m1 = p[j + 1];
      const float m2 = ((j & 1) && ((skip >> (j >> 1)) & 1u)) ? p[j] : -INFINITY;
      float best = st;
      uint32_t c = 0u;
      if (m1 > best) { best = m1; c = 1u; }
      if (m2 > best) { best = m2; c = 2u; }
      float v;
      if (t == 0) v = s == 0 ? e.b : (s == 1 && S > 1 ? e.y[0] : -INFINITY);
      else v = best + ((j & 1) ? e.y[j >> 1] : e.b);
      o[j] = live ? (s < S ? v : -INFINITY) : st;
      word |= c << (2 * j);
    }
    fetch(t + 4, q);  // (after the last use of the set: the load can then take the same registers)
#pragma unroll
    for (int j = 0; j < 16; j += 2) *reinterpret_cast<float2*>(cur + s0 + 2 + j) = make_float2(o[j], o[j + 1]);
    if (i == 0) *reinterpret_cast<float2*>(cur) = *reinterpret_cast<const float2*>(s_in + 2 * (tt + 1));
    if (i == kNT - 1) *reinterpret_cast<float2*>(s_out + 2 * tt) = make_float2(o[14], o[15]);
    bprow[(long)tt * Wp] = word;
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
    for (int k = i; k < 2 * kTB / 4; k += kNT) reinterpret_cast<float4*>(eout)[k] = reinterpret_cast<const float4*>(s_out)[k];
  }
}

template <typename TX>
__global__ __launch_bounds__(kBtThreads) void ctc_long_backtrace_kernel(const TX* __restrict__ x, long ld,
                                                                        const int* __restrict__ targets,
                                                                        const float* __restrict__ alpha,
                                                                        const uint32_t* __restrict__ bp, int* __restrict__ tok_start,
                                                                        int* __restrict__ tok_end, int* __restrict__ frame_label,
                                                                        float* __restrict__ frame_lp, float* __restrict__ score,
                                                                        int T, int V, int U, int blank, long Wp) {
  __shared__ uint32_t s_bp[kBtBlk * kBtW];
  __shared__ int s_state[kBtBlk + 2];  // [1 + f]: the state in frame t0 + f; [0]: in frame t0 - 1; [n + 1]: in frame t1
  __shared__ int s_end;
  const int i = threadIdx.x, nt = blockDim.x;
  const int S = 2 * U + 1;
  int bad = 0;
  for (int u = i; u < U; u += nt) {
    const int y = targets[u];
    bad |= y < 0 || y >= V || y == blank;
  }
  if (__syncthreads_or(bad)) {  // a target id outside [0, V) or equal to blank: reported (score NaN), not aligned
    if (i == 0) score[0] = __int_as_float(0x7fc00000);
    return;
  }
  if (T == 0) {
    if (i == 0) score[0] = U == 0 ? 0.f : -INFINITY;
    return;
  }
  if (i == 0) {  // end state: S-1 over S-2 on a tie
    const float a1 = alpha[S - 1], a2 = S >= 2 ? alpha[S - 2] : -INFINITY;
    const bool last = a1 >= a2;
    const float sc = last ? a1 : a2;
    score[0] = sc;
    s_end = sc == -INFINITY ? -1 : (last ? S - 1 : S - 2);
  }
  __syncthreads();
  int s = s_end;  // the state in frame t1 - 1
  if (s < 0) return;  // infeasible: score -inf, the fill of the init kernel stays

  int nxt = -1;  // the state in frame t1 (no such frame at the end)
  for (int t1 = T; t1 > 0; t1 -= kBtBlk) {
    const int t0 = max(0, t1 - kBtBlk), n = t1 - t0;
    const int w_lo = max(0, s - 2 * (n - 1)) >> 4, nw = (s >> 4) - w_lo + 1;  // nw <= kBtW
    for (int k = i; k < n * nw; k += nt) {
      const int f = k / nw, w = k - f * nw;
      s_bp[k] = bp[(long)(t0 + f) * Wp + w_lo + w];
    }
    __syncthreads();
    if (i == 0) {
      int ss = s;
      for (int t = t1 - 1; t >= t0; --t) {
        s_state[t - t0 + 1] = ss;
        if (t > 0) ss -= (s_bp[(t - t0) * nw + (ss >> 4) - w_lo] >> (2 * (ss & 15))) & 3u;
      }
      s_state[0] = ss;
      s_state[n + 1] = nxt;
    }
    __syncthreads();
    // labels, log-probs and token spans of the block (the frames of a token are one run of its state)
    for (int k = i; k < n; k += nt) {
      const int t = t0 + k, st = s_state[k + 1];
      const int u = (st & 1) ? (st >> 1) : -1;
      const int lab = u >= 0 ? targets[u] : blank;
      frame_label[t] = u;
      frame_lp[t] = ldx(x + (long)t * ld, lab);
      if (u >= 0) {
        if (t == 0 || s_state[k] != st) tok_start[u] = t;
        if (t == T - 1 || s_state[k + 2] != st) tok_end[u] = t + 1;
      }
    }
    nxt = s_state[1];
    s = s_state[0];
    __syncthreads();
  }
}

template <typename TX>
int launch_long(const TX* x, long ld, const int* targets, void* workspace, int* tok_start, int* tok_end, int* frame_label,
                float* frame_lp, float* score, int T, int V, int U, int blank, hipStream_t stream) {
  const Layout l = layout(T, U);
  float* alpha = (float*)workspace;
  float* edge = (float*)((char*)workspace + l.edge_off);
  uint32_t* bp = (uint32_t*)((char*)workspace + l.bp_off);
  const long n = std::max(l.Sp, (long)std::max(T, U));
  hipLaunchKernelGGL(ctc_long_init_kernel, dim3((unsigned)std::min((n + 255) / 256, 2048L)), dim3(256), 0, stream, alpha, tok_start,
                     tok_end, frame_label, frame_lp, l.Sp, (long)U, (long)T);
  for (long d = 0; l.nI > 0 && d < l.nI + l.nJ - 1; ++d) {  // anti-diagonal d: tiles (i, d - i), i_lo <= i <= i_hi
    const long i_lo = std::max(0L, d - (l.nJ - 1)), i_hi = std::min(d, l.nI - 1);
    hipLaunchKernelGGL(ctc_long_tile_kernel<TX>, dim3((unsigned)(i_hi - i_lo + 1)), dim3(kNT), 0, stream, x, ld, targets, alpha, edge,
                       bp, T, V, U, blank, (int)d, (int)i_lo, l.Tp, l.Wp);
  }
  hipLaunchKernelGGL(ctc_long_backtrace_kernel<TX>, dim3(1), dim3(kBtThreads), 0, stream, x, ld, targets, alpha, bp, tok_start,
                     tok_end, frame_label, frame_lp, score, T, V, U, blank, l.Wp);
  return EA_CHECK_LAUNCH();
}

constexpr long kMaxT = 1L << 30, kMaxU = 1L << 28;  // frame and state indices stay in 32 bits

}  // namespace

extern "C" int ea_ctc_viterbi_long_tile(int* frames, int* states) {
  if (frames) *frames = kTB;
  if (states) *states = kTS;
  return 0;
}

extern "C" long ea_ctc_viterbi_long_workspace_bytes(long T, long U) {
  if (T < 0 || U < 0 || T > kMaxT || U > kMaxU) return 0;
  return layout(T, U).bytes;
}

extern "C" int ea_ctc_viterbi_long_align(const void* x, long ld, int x_bf16, const int* targets, void* workspace, int* tok_start,
                                         int* tok_end, int* frame_label, float* frame_lp, float* score, long T, int V, long U,
                                         int blank, hipStream_t stream) {
  if (T < 0 || U < 0 || T > kMaxT || U > kMaxU || V < 1 || ld < V || blank < 0 || blank >= V) return -2;
  if (x_bf16)
    return launch_long((const bf16_t*)x, ld, targets, workspace, tok_start, tok_end, frame_label, frame_lp, score, (int)T, V, (int)U,
                       blank, stream);
  return launch_long((const float*)x, ld, targets, workspace, tok_start, tok_end, frame_label, frame_lp, score, (int)T, V, (int)U,
                     blank, stream);
}
