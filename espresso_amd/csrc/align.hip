// Forced alignment (Viterbi) of a known transcript for gfx950: the max-plus twins of the CTC and RNN-T scans plus a backtrace.
// The reference gets alignments from Kaldi only (estimate_initial_state_prior_from_alignments.py); its greedy CTC timesteps
// (espresso/tools/ctc_decoder.py:171-186) align the hypothesis, not the transcript.  Both kernels are latency chains: one
// workgroup per utterance, workgroups never talk to each other.
//
// ctc_viterbi_kernel: the lattice of ea_ctc_loss (blank y1 blank ... yU blank, S = 2U + 1 states), max instead of logsumexp.
//   Thread layout, prefetch and the max-plus frame update (viterbi_frame) are ctc_lattice.h's.  This kernel's own: the
//   backpointers, 2 bits per state (0 stay, 1 from s-1, 2 from s-2), 16 states per 32-bit word, one vector store per thread and
//   frame into the workspace, and the backtrace, which streams blocks of frames' backpointer rows into LDS with coalesced loads
//   while one lane walks them there.
// rnnt_viterbi_kernel: the (t,u) lattice of ea_rnnt_scan, swept backwards (best score FROM each node) along anti-diagonals, one
//   lane per u, so that the decision at a node is about its successor: 1 bit per node (1 = emit, 0 = blank), ballot-packed per
//   wave, one row per diagonal.  The walk then goes forwards from (0,0) through blocks of rows staged in LDS the same way.
#include "common.h"
#include "ctc_lattice.h"
#include "espresso_amd.h"

namespace {

constexpr int kCtcMaxW = kCtcMaxS / 16;
constexpr int kCtcBlk = 32;       // backpointer rows staged per backtrace block
constexpr int kRnntMaxU1 = 1024;  // lanes (one per u)
constexpr int kRnntBlk = 64;      // diagonals staged per walk block

template <typename TX>
__global__ __launch_bounds__(128) void ctc_viterbi_kernel(const TX* __restrict__ x, long ld, const int* __restrict__ targets,
                                                          const int* __restrict__ in_len, const int* __restrict__ tgt_len,
                                                          uint32_t* __restrict__ bp, int* __restrict__ tok_start,
                                                          int* __restrict__ tok_end, int* __restrict__ frame_label,
                                                          float* __restrict__ score, int T, int V, int Lmax, int blank, int Wp) {
  __shared__ float s_a[2][kCtcMaxS + 2];         // [buffer][2 + state]: entries 0, 1 stand for the states -2, -1 (-inf)
  __shared__ uint32_t s_bp[kCtcBlk * kCtcMaxW];  // backtrace block
  __shared__ int s_end;
  const int b = blockIdx.x, i = threadIdx.x, nt = blockDim.x;
  const int L = max(0, min(in_len[b], T));
  const int U = max(0, min(tgt_len[b], Lmax));
  const int S = 2 * U + 1;
  const int Wb = (S + 15) / 16;  // backpointer words of this utterance's rows
  const int* tg = targets + (long)b * Lmax;
  int* fl = frame_label + (long)b * T;
  int* ts = tok_start + (long)b * Lmax;
  int* te = tok_end + (long)b * Lmax;

  int col[8];
  unsigned skip;
  const int bad = ctc_labels(tg, i, U, V, blank, col, skip);
  for (int u = i; u < Lmax; u += nt) { ts[u] = -1; te[u] = -1; }
  for (int t = i; t < T; t += nt) fl[t] = -2;
  if (__syncthreads_or(bad)) {  // a target id outside [0, V) or equal to blank: reported (score NaN), not aligned
    if (i == 0) score[b] = __int_as_float(0x7fc00000);
    return;
  }
  if (L == 0) {
    if (i == 0) score[b] = U == 0 ? 0.f : -INFINITY;
    return;
  }

  const TX* xb = x + (long)b * T * ld;
  auto fetch = [&](int t, Emis& e) { ctc_fetch(xb + (long)min(t, L - 1) * ld, blank, col, e); };
  float* prev = s_a[0];
  float* cur = s_a[1];
  const int s0 = 16 * i;
  uint32_t* bprow = bp + (long)b * (T + 3) * Wp + i;

  // one frame.  The loop runs L rounded up to 4 frames; frames from L on keep the scores (their backpointer rows L .. L+2 are
  // padding rows of the workspace)
  auto step = [&](int t, Emis& q) {
    float o[16];
    const uint32_t word = viterbi_frame(prev + s0, q, skip, s0, S, t, t < L, o);
    fetch(t + 4, q);
    ctc_store(cur + s0 + 2, o);
    bprow[(long)t * Wp] = word;
    lds_barrier();
    float* tmp = prev; prev = cur; cur = tmp;
  };

  // frame -1: every state -inf (frame 0 does not use it, but reads it)
  for (int s = i; s < kCtcMaxS + 2; s += nt) { s_a[0][s] = -INFINITY; s_a[1][s] = -INFINITY; }
  Emis q0, q1, q2, q3;
  ctc_prefetch(fetch, 0, q0, q1, q2, q3);
  __syncthreads();
  for (int t = 0; t < L; t += 4) {
    step(t, q0);
    step(t + 1, q1);
    step(t + 2, q2);
    step(t + 3, q3);
  }
  // end state: S-1 over S-2 on a tie
  if (i == 0) {
    const float a1 = prev[2 + S - 1], a2 = S >= 2 ? prev[2 + S - 2] : -INFINITY;
    const bool last = a1 >= a2;
    const float sc = last ? a1 : a2;
    score[b] = sc;
    s_end = sc == -INFINITY ? -1 : (last ? S - 1 : S - 2);
  }
  __threadfence_block();
  __syncthreads();
  int s = s_end;
  if (s < 0) return;  // infeasible: score -inf, no labels

  // backtrace: blocks of kCtcBlk frames, the last block first
  for (int t1 = L; t1 > 0; t1 -= kCtcBlk) {
    const int t0 = max(0, t1 - kCtcBlk), n = (t1 - t0) * Wb;
    for (int k = i; k < n; k += nt) {
      const int f = k / Wb, w = k - f * Wb;
      s_bp[k] = bp[((long)b * (T + 3) + t0 + f) * Wp + w];
    }
    __syncthreads();
    if (i == 0) {
      for (int t = t1 - 1; t >= t0; --t) {
        fl[t] = (s & 1) ? (s >> 1) : -1;
        if (t > 0) s -= (s_bp[(t - t0) * Wb + (s >> 4)] >> (2 * (s & 15))) & 3u;
      }
    }
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();
  // token spans from the frame labels (the frames of a token are one run)
  for (int t = i; t < L; t += nt) {
    const int u = fl[t];
    if (u < 0) continue;
    if (t == 0 || fl[t - 1] != u) ts[u] = t;
    if (t == L - 1 || fl[t + 1] != u) te[u] = t + 1;
  }
}

// blockDim = UP (U1 rounded up to 64): lane u; beta(t,u) = best log-prob from node (t,u) to the end (final blank included)
__global__ __launch_bounds__(1024) void rnnt_viterbi_kernel(const float* __restrict__ lpb, const float* __restrict__ lpy,
                                                            const int* __restrict__ T_len, const int* __restrict__ U_len,
                                                            uint32_t* __restrict__ bp, int* __restrict__ emit_frame,
                                                            float* __restrict__ score, int T, int U1, int UP) {
  __shared__ float s_b[2][kRnntMaxU1 + 1];
  __shared__ uint32_t s_bp[kRnntBlk * (kRnntMaxU1 / 32)];
  __shared__ float s_score;
  const int b = blockIdx.x, u = threadIdx.x, lane = u & 63, wave = u >> 6;
  const int Tb = min(T_len[b], T), Ub = max(0, min(U_len[b], U1 - 1));
  const int Umax = U1 - 1, Wd = UP / 32;
  int* ef = emit_frame + (long)b * Umax;
  for (int k = u; k < Umax; k += UP) ef[k] = -1;
  if (Tb <= 0) {
    if (u == 0) score[b] = -INFINITY;
    return;
  }
  const long base = (long)b * T * U1;
  const int ndiag = Tb + Ub;
  uint32_t* bprow = bp + (long)b * (T + U1 + 3) * Wd + wave * 2 + (lane & 1);
  float* prevbuf = s_b[0];
  float* curbuf = s_b[1];
  s_b[0][u] = -INFINITY;
  s_b[1][u] = -INFINITY;
  if (u == 0) { s_b[0][UP] = -INFINITY; s_b[1][UP] = -INFINITY; }
  // the two log-probs of a node, requested four diagonals ahead from a clamped cell (every lane loads)
  const int uc = u <= Ub ? u : Ub;
  auto fetch = [&](int k, float& pb, float& py) {
    const int kk = k < ndiag ? k : ndiag - 1;
    int t = (ndiag - 1 - kk) - uc;
    t = t < 0 ? 0 : (t > Tb - 1 ? Tb - 1 : t);
    const long idx = base + (long)t * U1 + uc;
    pb = lpb[idx];
    py = lpy[idx];
  };
  float own_prev = -INFINITY;  // beta(t+1, u): this lane's value on the diagonal before
  // one diagonal; as in the CTC kernel the loop has no branch (steps past the last diagonal change nothing that is read: their
  // rows are the workspace's padding rows) and the set of a diagonal is refilled after its last use
  auto step = [&](int k, float& qb, float& qy) {
    const float pb = qb, py = qy;
    const int t = (ndiag - 1 - k) - u;
    const bool in = u <= Ub && t >= 0 && t < Tb;
    const float blk = t == Tb - 1 ? (u == Ub ? pb : -INFINITY) : own_prev + pb;
    const float emt = u < Ub ? prevbuf[u + 1] + py : -INFINITY;
    // ties: emit (the earlier emission); the last frame can only emit, the last token row only take blanks
    const bool e = u < Ub && (t == Tb - 1 || emt >= blk);
    const float val = in ? (e ? emt : blk) : -INFINITY;
    if (in) own_prev = val;
    curbuf[u] = val;
    fetch(k + 4, qb, qy);
    const uint64_t m = __ballot(in && e);
    bprow[(long)k * Wd] = (lane & 1) ? (uint32_t)(m >> 32) : (uint32_t)m;  // (every lane stores: lanes 2 .. 63 repeat 0 and 1)
    lds_barrier();
    float* tmp = prevbuf; prevbuf = curbuf; curbuf = tmp;
  };
  float b0, y0, b1, y1, b2, y2, b3, y3;
  fetch(0, b0, y0);
  fetch(1, b1, y1);
  fetch(2, b2, y2);
  fetch(3, b3, y3);
  __syncthreads();
  for (int k = 0; k < ndiag; k += 4) {
    step(k, b0, y0);
    step(k + 1, b1, y1);
    step(k + 2, b2, y2);
    step(k + 3, b3, y3);
  }
  if (u == 0) { score[b] = own_prev; s_score = own_prev; }  // beta(0, 0): lane 0's value on the last diagonal
  __threadfence_block();
  __syncthreads();
  if (s_score == -INFINITY) return;

  // forward walk from (0,0); row k of the sweep holds diagonal d = ndiag - 1 - k
  int t = 0, uu = 0;
  for (int d0 = 0; d0 < ndiag - 1; d0 += kRnntBlk) {
    const int d1 = min(ndiag - 1, d0 + kRnntBlk), n = (d1 - d0) * Wd;
    for (int k = u; k < n; k += UP) {
      const int f = k / Wd, w = k - f * Wd;
      s_bp[k] = bp[((long)b * (T + U1 + 3) + (ndiag - 1 - (d0 + f))) * Wd + w];
    }
    __syncthreads();
    if (u == 0) {
      for (int d = d0; d < d1; ++d) {
        if ((s_bp[(d - d0) * Wd + (uu >> 5)] >> (uu & 31)) & 1u) { ef[uu] = t; ++uu; }
        else ++t;
      }
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" long ea_ctc_viterbi_workspace_bytes(int B, int T, int Lmax) {
  if (B <= 0 || T < 0 || Lmax < 1 || 2 * Lmax + 1 > kCtcMaxS) return 0;
  return 4L * B * (T + 3) * ctc_threads(Lmax);  // (3 padding rows per utterance, see step)
}

extern "C" int ea_ctc_viterbi_align(const void* x, long ld, int x_bf16, const int* targets, const int* in_len, const int* tgt_len,
                                    void* workspace, int* tok_start, int* tok_end, int* frame_label, float* score, int B, int T,
                                    int V, int Lmax, int blank, hipStream_t stream) {
  if (B <= 0) return 0;
  if (T < 0 || V < 1 || ld < V || Lmax < 1 || 2 * Lmax + 1 > kCtcMaxS || blank < 0 || blank >= V) return -2;
  const int Wp = ctc_threads(Lmax);  // backpointer words per frame row = threads per workgroup
  if (x_bf16)
    hipLaunchKernelGGL(ctc_viterbi_kernel<bf16_t>, dim3(B), dim3(Wp), 0, stream, (const bf16_t*)x, ld, targets, in_len, tgt_len,
                       (uint32_t*)workspace, tok_start, tok_end, frame_label, score, T, V, Lmax, blank, Wp);
  else
    hipLaunchKernelGGL(ctc_viterbi_kernel<float>, dim3(B), dim3(Wp), 0, stream, (const float*)x, ld, targets, in_len, tgt_len,
                       (uint32_t*)workspace, tok_start, tok_end, frame_label, score, T, V, Lmax, blank, Wp);
  return EA_CHECK_LAUNCH();
}

extern "C" long ea_rnnt_viterbi_workspace_bytes(int B, int T, int U1) {
  if (B <= 0 || T < 1 || U1 < 1 || U1 > kRnntMaxU1) return 0;
  return 4L * B * (T + U1 + 3) * (((U1 + 63) & ~63) / 32);  // (3 padding rows per utterance, see step)
}

extern "C" int ea_rnnt_viterbi_align(const float* lpb, const float* lpy, const int* logit_lengths, const int* target_lengths,
                                     void* workspace, int* emit_frame, float* score, int B, int T, int U1, hipStream_t stream) {
  if (B <= 0) return 0;
  if (T < 1 || U1 < 1 || U1 > kRnntMaxU1) return -2;
  const int UP = (U1 + 63) & ~63;
  hipLaunchKernelGGL(rnnt_viterbi_kernel, dim3(B), dim3(UP), 0, stream, lpb, lpy, logit_lengths, target_lengths,
                     (uint32_t*)workspace, emit_frame, score, T, U1, UP);
  return EA_CHECK_LAUNCH();
}
