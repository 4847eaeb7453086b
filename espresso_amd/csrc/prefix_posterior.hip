// Per-token posteriors of a given label sequence for gfx950: the sum-product twins of the Viterbi kernels in align.hip.
// The reference has nothing comparable for CTC / transducer hypotheses (its attention decoder's positional_scores,
// espresso/tools/simple_greedy_decoder.py, are the same quantity for the third model family).
//
// Psi_i = log of the probability that the model's output STARTS WITH y1 .. yi, summed over all continuations and alignments;
// log c_i = Psi_i - Psi_{i-1} (Psi_0 = 0) is the posterior of token i given the audio and the tokens before it, log c_end =
// total - Psi_U that of stopping, and the factors add up to total = log P(y | x) = -(CTC / RNN-T loss).  Both kernels are
// latency chains: one workgroup per hypothesis, workgroups never talk to each other, no workspace (alpha is not stored).
//
// ctc_prefix_kernel: the lattice, thread layout and prefetch of ctc_viterbi_kernel (ctc_lattice.h), log-add-exp where the aligner
//   takes the max: the sum-product frame update is prefix_frame there.  Every odd state (token u) keeps one more accumulator in a
//   register: the log-sum over frames of the mass ENTERING the state times the frame's emission, the self-loop left out.  This
//   kernel's own: the early exits and the factors from Psi.  Hypothesis n reads the log-probs of utterance utt[n]: an n-best list
//   shares its utterance's rows.
// rnnt_prefix_kernel: the forward half of rnnt_scan_kernel along anti-diagonals, one lane per u.  Lane u holds alpha(t,u), hands
//   alpha(t,u) + lpy(t,u) to lane u + 1 through LDS and adds the same value to its accumulator: Psi_{u+1} = lse_t of it.
#include "common.h"
#include "ctc_lattice.h"
#include "espresso_amd.h"

namespace {

constexpr int kRnntMaxU1 = 1024;  // lanes (one per u)

template <typename TX>
__global__ __launch_bounds__(128) void ctc_prefix_kernel(const TX* __restrict__ x, long ld, const int* __restrict__ targets,
                                                         const int* __restrict__ utt, const int* __restrict__ in_len,
                                                         const int* __restrict__ tgt_len, float* __restrict__ logc,
                                                         float* __restrict__ total, float* __restrict__ psi_out, int B, int T, int V,
                                                         int Lmax, int blank) {
  __shared__ float s_a[2][kCtcMaxS + 2];  // [buffer][2 + state]: entries 0, 1 stand for the states -2, -1 (-inf)
  const int n = blockIdx.x, i = threadIdx.x, nt = blockDim.x;
  const int b = utt[n];
  const bool bad_utt = b < 0 || b >= B;
  const int L = bad_utt ? 0 : max(0, min(in_len[b], T));
  const int U = max(0, min(tgt_len[n], Lmax));
  const int S = 2 * U + 1;
  const int* tg = targets + (long)n * Lmax;
  float* lc = logc + (long)n * (Lmax + 1);
  float* po = psi_out ? psi_out + (long)n * Lmax : nullptr;

  int col[8];
  unsigned skip;
  const int bad = ctc_labels(tg, i, U, V, blank, col, skip) || bad_utt;
  if (__syncthreads_or(bad)) {  // an id outside [0, V) or equal to blank, or a row outside [0, B): reported as NaN
    for (int u = i; u <= Lmax; u += nt) lc[u] = quiet_nan();
    if (po) for (int u = i; u < Lmax; u += nt) po[u] = quiet_nan();
    if (i == 0) total[n] = quiet_nan();
    return;
  }
  if (L == 0) {  // no frame: only the empty hypothesis is possible
    const float v = U == 0 ? 0.f : -INFINITY;
    for (int u = i; u <= Lmax; u += nt) lc[u] = u <= U ? v : 0.f;
    if (po) for (int u = i; u < Lmax; u += nt) po[u] = u < U ? -INFINITY : 0.f;
    if (i == 0) total[n] = v;
    return;
  }

  const TX* xb = x + (long)b * T * ld;
  auto fetch = [&](int t, Emis& e) { ctc_fetch(xb + (long)min(t, L - 1) * ld, blank, col, e); };
  float* prev = s_a[0];
  float* cur = s_a[1];
  const int s0 = 16 * i;
  float psi[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) psi[k] = -INFINITY;

  // one frame.  The loop runs L rounded up to 4 frames; frames from L on keep the scores and add nothing
  auto step = [&](int t, Emis& q) {
    float o[16];
    prefix_frame(prev + s0, q, skip, s0, S, t, t < L, psi, o);
    fetch(t + 4, q);
    ctc_store(cur + s0 + 2, o);
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
  // `prev` holds the last frame; `cur` (read for the last time before the last barrier) takes Psi: cur[u] = Psi_u, Psi_0 = 0
  const float tot = lse2(prev[2 + S - 1], S >= 2 ? prev[2 + S - 2] : -INFINITY);
  if (i == 0) cur[0] = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) cur[1 + 8 * i + k] = psi[k];
  __syncthreads();
  for (int u = i; u <= Lmax; u += nt) {
    float c = 0.f;
    if (u < U) c = factor(cur[u + 1], cur[u]);
    else if (u == U) c = factor(tot, cur[u]);
    lc[u] = c;
    if (po && u < Lmax) po[u] = u < U ? cur[u + 1] : 0.f;
  }
  if (i == 0) total[n] = tot;
}

// blockDim = UP (U1 rounded up to 64): lane u; alpha(t,u) = log-prob of reaching node (t,u) from (0,0)
__global__ __launch_bounds__(1024) void rnnt_prefix_kernel(const float* __restrict__ lpb, const float* __restrict__ lpy,
                                                           const int* __restrict__ T_len, const int* __restrict__ U_len,
                                                           float* __restrict__ logc, float* __restrict__ total,
                                                           float* __restrict__ psi_out, int T, int U1, int UP) {
  __shared__ float s_y[2][kRnntMaxU1 + 1];  // [buffer][1 + u] = alpha(t,u) + lpy(t,u) of a diagonal; entry 0: -inf (no row -1)
  __shared__ float s_total;
  const int b = blockIdx.x, u = threadIdx.x;
  const int Tb = min(T_len[b], T), Ub = max(0, min(U_len[b], U1 - 1));
  float* lc = logc + (long)b * U1;
  float* po = psi_out ? psi_out + (long)b * (U1 - 1) : nullptr;
  if (Tb <= 0) {  // no frame: nothing can be emitted, the final blank included
    if (u < U1) lc[u] = u <= Ub ? -INFINITY : 0.f;
    if (po && u < U1 - 1) po[u] = u < Ub ? -INFINITY : 0.f;
    if (u == 0) total[b] = -INFINITY;
    return;
  }
  const long base = (long)b * T * U1;
  const int ndiag = Tb + Ub;
  float* prevbuf = s_y[0];
  float* curbuf = s_y[1];
  s_y[0][u + 1] = -INFINITY;
  s_y[1][u + 1] = -INFINITY;
  if (u == 0) { s_y[0][0] = -INFINITY; s_y[1][0] = -INFINITY; s_total = -INFINITY; }
  // the two log-probs of a node, requested four diagonals ahead from a clamped cell (every lane loads)
  const int uc = u <= Ub ? u : Ub;
  auto fetch = [&](int k, float& pb, float& py) {
    const int kk = k < ndiag ? k : ndiag - 1;
    int t = kk - uc;
    t = t < 0 ? 0 : (t > Tb - 1 ? Tb - 1 : t);
    const long idx = base + (long)t * U1 + uc;
    pb = lpb[idx];
    py = lpy[idx];
  };
  float out_b = -INFINITY;  // alpha(t-1, u) + lpb(t-1, u): this lane's blank move out of the diagonal before
  float psi = -INFINITY;    // Psi_{u+1}
  // one diagonal d = k, t = k - u; as in rnnt_viterbi_kernel the loop has no branch (on the steps past the last diagonal no
  // node is inside) and the set of a diagonal is refilled after its last use
  auto step = [&](int k, float& qb, float& qy) {
    const float pb = qb, py = qy;
    const int t = k - u;
    const bool in = u <= Ub && t >= 0 && t < Tb;
    const float a = t > 0 ? out_b : -INFINITY;
    const float c = prevbuf[u];
    const float val = (t == 0 && u == 0) ? 0.f : lse2(a, c);
    const float oy = (in && u < Ub) ? val + py : -INFINITY;
    if (in) {
      out_b = val + pb;
      psi = lse2(psi, oy);
    }
    curbuf[u + 1] = oy;
    fetch(k + 4, qb, qy);
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
  // lane Ub's last node is (Tb-1, Ub): its blank move is the end of the sequence.  Psi goes through LDS: curbuf[u] = Psi_u
  if (u == Ub) s_total = out_b;
  if (u == 0) curbuf[0] = 0.f;
  curbuf[u + 1] = psi;
  __syncthreads();
  const float tot = s_total;
  if (u < U1) {
    float c = 0.f;
    if (u < Ub) c = factor(curbuf[u + 1], curbuf[u]);
    else if (u == Ub) c = factor(tot, curbuf[u]);
    lc[u] = c;
    if (po && u < U1 - 1) po[u] = u < Ub ? curbuf[u + 1] : 0.f;
  }
  if (u == 0) total[b] = tot;
}

}  // namespace

extern "C" int ea_ctc_prefix_posteriors(const void* x, long ld, int x_bf16, const int* targets, const int* utt, const int* in_len,
                                        const int* tgt_len, float* logc, float* total, float* psi, int N, int B, int T, int V,
                                        int Lmax, int blank, hipStream_t stream) {
  if (N <= 0) return 0;
  if (B < 1 || T < 0 || V < 1 || ld < V || Lmax < 1 || 2 * Lmax + 1 > kCtcMaxS || blank < 0 || blank >= V) return -2;
  const int nt = ctc_threads(Lmax);  // 64 or 128
  if (x_bf16)
    hipLaunchKernelGGL(ctc_prefix_kernel<bf16_t>, dim3(N), dim3(nt), 0, stream, (const bf16_t*)x, ld, targets, utt, in_len,
                       tgt_len, logc, total, psi, B, T, V, Lmax, blank);
  else
    hipLaunchKernelGGL(ctc_prefix_kernel<float>, dim3(N), dim3(nt), 0, stream, (const float*)x, ld, targets, utt, in_len, tgt_len,
                       logc, total, psi, B, T, V, Lmax, blank);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_rnnt_prefix_posteriors(const float* lpb, const float* lpy, const int* logit_lengths, const int* target_lengths,
                                         float* logc, float* total, float* psi, int B, int T, int U1, hipStream_t stream) {
  if (B <= 0) return 0;
  if (T < 1 || U1 < 1 || U1 > kRnntMaxU1) return -2;
  const int UP = (U1 + 63) & ~63;
  hipLaunchKernelGGL(rnnt_prefix_kernel, dim3(B), dim3(UP), 0, stream, lpb, lpy, logit_lengths, target_lengths, logc, total, psi,
                     T, U1, UP);
  return EA_CHECK_LAUNCH();
}
