// Long-form forced alignment for gfx950: the CTC Viterbi search of csrc/align.hip for ONE sequence whose lattice does not fit a
// workgroup (a recording's stitched log-probs against its whole transcript: ~90 000 frames x 20 000 - 120 000 states), DESIGN.md
// section 3.9.  The reference has no forced aligner of its own (it aligns through Kaldi), so these kernels replace nothing of it.
// Lattice, move rules and tie rules are those of ctc_viterbi_kernel, and because max-plus in fp32 does not reassociate, scores and
// path equal that kernel's bit for bit wherever it accepts the problem.
//
// The lattice is cut into tiles of kTB frames x kTS states; tile (i, j) = frame block i, state tile j.  Tile shape, the alpha and
// edge buffers that carry scores from tile to tile, the launch order and the frame loop are ctc_lattice.h's.  This file's own:
//   ctc_long_init_kernel: alpha[] = -inf, token spans -1, frame labels -2, frame log-probs 0.
//   ctc_long_tile_kernel: one launch per anti-diagonal i + j = d, one workgroup (one wave) per tile of it; per thread and frame one
//     32-bit word of 2-bit backpointers goes to the workspace with a vector store.
//   ctc_long_backtrace_kernel: one workgroup.  Checks the targets (a bad id: score NaN, nothing aligned), picks the end state,
//     then walks blocks of kBtBlk frames from the end.  The state falls by at most 2 per frame, so of a block's backpointer rows
//     (S / 16 words each, far more than LDS holds) only the <= kBtW words between the lowest state the walk can reach in the
//     block and the state it enters with are staged; one lane walks them and leaves the block's states in LDS, from which all
//     threads write frame_label, frame_lp = x[t][label] and the token spans.
// Every index into the backpointer workspace is 64-bit: at T = 10^6, U = 10^5 the rows hold 5 * 10^10 bytes.
#include <algorithm>

#include "common.h"
#include "ctc_lattice.h"
#include "espresso_amd.h"

namespace {

constexpr int kBtBlk = 128;       // frames per backtrace block
constexpr int kBtW = (2 * kBtBlk - 2) / 16 + 2;  // backpointer words a block's walk can reach in one row
constexpr int kBtThreads = 256;

// the workspace: alpha, edge (ctc_lattice.h), then the backpointer rows
struct Layout : TileLayout {
  long Wp, bp_off, bytes;  // backpointer words per frame row
};

__host__ inline Layout align_workspace(long T, long U) {
  Layout l{tile_layout(T, U)};
  l.Wp = l.Sp / 16;
  l.bp_off = l.tail;
  l.bytes = l.bp_off + 4 * l.Tp * l.Wp;
  return l;
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
  __shared__ __attribute__((aligned(16))) float s_a[2][kTS + 2];
  __shared__ __attribute__((aligned(16))) float s_in[2 * (kTB + 1)];
  __shared__ __attribute__((aligned(16))) float s_out[2 * kTB];  // (what the three hold: ctc_lattice.h)
  const int i = threadIdx.x;
  const int bi = i_lo + blockIdx.x, bj = d - bi;
  const int t0 = bi * kTB;
  const int S = 2 * U + 1;
  const int g = bj * kNT + i;  // the thread's index over the whole state axis: states 16g .. 16g + 15
  float* eout = edge + ((long)bj * Tp + t0) * 2;
  if (tile_above_cone(eout, bj, t0, i)) return;

  int col[8];
  unsigned skip;
  ctc_labels(targets, g, U, V, blank, col, skip);  // (a bad id is read as blank here and reported by the backtrace kernel)
  auto fetch = [&](int t, Emis& e) { ctc_fetch(x + (long)min(t, T - 1) * ld, blank, col, e); };
  Emis q0, q1, q2, q3;
  ctc_prefetch(fetch, t0, q0, q1, q2, q3);

  float* prev = s_a[0];
  float* cur = s_a[1];
  const int s0 = 16 * i;
  tile_prologue(prev, s_in, alpha, edge, Tp, bj, t0, i);
  uint32_t* bprow = bp + (long)t0 * Wp + g;
  __syncthreads();

  // one frame; frames from T on keep the scores (their backpointer rows are the padding rows T .. Tp - 1)
  auto step = [&](int tt, Emis& q) {
    const int t = t0 + tt;
    float o[16];
    const uint32_t word = viterbi_frame(prev + s0, q, skip, 16 * g, S, t, t < T, o);
    fetch(t + 4, q);
    ctc_store(cur + s0 + 2, o);
    tile_handover(cur, s_in, s_out, o, tt, i);
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
  tile_epilogue(prev, s_out, alpha, eout, bj, i);
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
  const Layout l = align_workspace(T, U);
  float* alpha = (float*)workspace;
  float* edge = (float*)((char*)workspace + l.edge_off);
  uint32_t* bp = (uint32_t*)((char*)workspace + l.bp_off);
  const long n = std::max(l.Sp, (long)std::max(T, U));
  hipLaunchKernelGGL(ctc_long_init_kernel, dim3((unsigned)std::min((n + 255) / 256, 2048L)), dim3(256), 0, stream, alpha, tok_start,
                     tok_end, frame_label, frame_lp, l.Sp, (long)U, (long)T);
  for_each_antidiagonal(l, [&](int d, int i_lo, unsigned count) {
    hipLaunchKernelGGL(ctc_long_tile_kernel<TX>, dim3(count), dim3(kNT), 0, stream, x, ld, targets, alpha, edge, bp, T, V, U, blank, d,
                       i_lo, l.Tp, l.Wp);
  });
  hipLaunchKernelGGL(ctc_long_backtrace_kernel<TX>, dim3(1), dim3(kBtThreads), 0, stream, x, ld, targets, alpha, bp, tok_start,
                     tok_end, frame_label, frame_lp, score, T, V, U, blank, l.Wp);
  return EA_CHECK_LAUNCH();
}

}  // namespace

extern "C" int ea_ctc_viterbi_long_tile(int* frames, int* states) {
  if (frames) *frames = kTB;
  if (states) *states = kTS;
  return 0;
}

extern "C" long ea_ctc_viterbi_long_workspace_bytes(long T, long U) {
  if (T < 0 || U < 0 || T > kMaxT || U > kMaxU) return 0;
  return align_workspace(T, U).bytes;
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
