// Multi-level (sub-word + word) LM shallow fusion kernel for gfx950 (HBM / latency bound, one workgroup per hypothesis).
//
// Reference: espresso/models/external_language_model.py:376-552 (Hori et al. 2017, "Multi-level language modeling and
// decoding for open vocabulary end-to-end speech recognition", adapted to sentences that end with <space> <eos>) over the
// tensorized lexical prefix tree of csrc/lookahead.hip (node 0 = none, children[node][D], prev_subword[node], word_idx[node]).
// The reference walks the hypotheses in a Python loop (one .tolist() per step) and edits the output with ~30 masked tensor
// ops; here everything after the two LMs' GEMM / LSTM-cell calls is one launch:
//   1. word_lp[n] = log_softmax(word_logits[n])      on the first call and where prev == <space>; other rows keep theirs
//   2. tree transition on prev (root on <space>, child if one carries prev, else none) -> nodes[n], is_child
//   3. cum[n]: the running sub-word score of the current word, accumulated from the previous call's output row
//   4. out[n] = subword_weight * log_softmax(sub_logits[n]) (closed vocabulary: logzero once the word left the tree)
//   5. out[n][<space>] = word_lp[n][word] - cum[n]  (no word ends here: word_lp[n][unk] + log(oov_penalty))
//   6. <space> impossible after <space> / <eos>, <eos> only after <space> (and then carries word_lp[n][word <eos>])
#include "common.h"
#include "espresso_amd.h"

namespace {

struct MultiLevelArgs {
  const float* word_logits; long ldw;
  const float* sub_logits; long lds;
  const int* prev_tok; const float* prev_out;
  float* word_lp; float* cum; int* nodes; float* out;
  const int* children; const int* prev_subword; const int* word_idx;
  int Vw, Vs, D;
  float sub_weight, log_oov_penalty, logzero;
  int first, open_vocab, word_eos, word_unk, sub_space, sub_eos, root_id;
};

__global__ __launch_bounds__(256) void multilevel_step_kernel(const MultiLevelArgs a) {
  __shared__ float sm[16];
  __shared__ float s_space_val, s_eos_add;
  __shared__ int s_oov;
  const int n = blockIdx.x;
  const int tk = a.prev_tok[n];
  const bool space = tk == a.sub_space;
  const bool refresh = a.first || space;  // block-uniform

  // 1. word-level distribution of the rows that just closed a word
  const float* zw = a.word_logits + (long)n * a.ldw;
  float* wl = a.word_lp + (long)n * a.Vw;
  float w_lse = 0.f;
  if (refresh) {
    float mx = -INFINITY;
    for (int v = threadIdx.x; v < a.Vw; v += 256) mx = fmaxf(mx, zw[v]);
    mx = block_max(mx, sm);
    float s = 0.f;
    for (int v = threadIdx.x; v < a.Vw; v += 256) s += expf(zw[v] - mx);
    s = block_sum(s, sm);
    w_lse = mx + logf(s);
    for (int v = threadIdx.x; v < a.Vw; v += 256) wl[v] = zw[v] - w_lse;
  }

  // sub-word log-softmax normaliser
  const float* zs = a.sub_logits + (long)n * a.lds;
  float mx = -INFINITY;
  for (int v = threadIdx.x; v < a.Vs; v += 256) mx = fmaxf(mx, zs[v]);
  mx = block_max(mx, sm);
  float s = 0.f;
  for (int v = threadIdx.x; v < a.Vs; v += 256) s += expf(zs[v] - mx);
  s = block_sum(s, sm);
  const float s_lse = mx + logf(s);

  // 2. / 3. / 5. per-row bookkeeping (one thread; the rows just written by the other threads are re-derived from zw, w_lse)
  if (threadIdx.x == 0) {
    const bool tk_ok = tk >= 0 && tk < a.Vs;
    int node = a.root_id;
    bool child = false;
    float c = 0.f;
    if (!a.first) {
      if (!space) {
        const int* ch = a.children + (long)a.nodes[n] * a.D;
        int nxt = 0;  // "none" unless a child carries tk (padded slots are node 0 and add nothing)
        for (int i = 0; i < a.D; ++i) {
          const int cn = ch[i];
          if (a.prev_subword[cn] == tk) nxt += cn;
        }
        node = nxt;
        child = nxt != 0;
      }
      const float pv = tk_ok ? a.prev_out[(long)n * a.Vs + tk] : 0.f;
      if (a.open_vocab) c = space ? 0.f : a.cum[n] + pv;
      else c = child ? a.cum[n] + pv : 0.f;
    }
    a.nodes[n] = node;
    a.cum[n] = c;
    const int w = a.word_idx[node];
    const int wj = w >= 0 ? w : a.word_unk;
    const float lw = refresh ? zw[wj] - w_lse : wl[wj];
    s_space_val = w >= 0 ? lw - c : lw + a.log_oov_penalty;
    s_eos_add = refresh ? zw[a.word_eos] - w_lse : wl[a.word_eos];
    s_oov = !a.first && !a.open_vocab && !space && !child;
  }
  __syncthreads();

  // 4. / 5. / 6. the output row, every column written once
  const bool oov = s_oov;
  const bool no_space = space || tk == a.sub_eos;
  float* o = a.out + (long)n * a.Vs;
  for (int v = threadIdx.x; v < a.Vs; v += 256) {
    float x = oov ? a.logzero : a.sub_weight * (zs[v] - s_lse);
    if (v == a.sub_space) x = no_space ? a.logzero : s_space_val;
    if (v == a.sub_eos) x = space ? x + s_eos_add : a.logzero;
    o[v] = x;
  }
}

}  // namespace

extern "C" int ea_multilevel_lm_step(const float* word_logits, long ldw, const float* sub_logits, long lds, const int* prev_tok,
                                     const float* prev_out, float* word_lp, float* cum, int* nodes, float* out, const int* children,
                                     const int* prev_subword, const int* word_idx, int N, int Vw, int Vs, int D, float subword_weight,
                                     float log_oov_penalty, int first, int open_vocab, int word_eos, int word_unk, int sub_space,
                                     int sub_eos, int root_id, hipStream_t stream) {
  if (N <= 0) return 0;
  if (Vw <= 0 || Vs <= 0 || D <= 0 || word_eos < 0 || word_eos >= Vw || word_unk < 0 || word_unk >= Vw || sub_space < 0 ||
      sub_space >= Vs || sub_eos < 0 || sub_eos >= Vs || ldw < Vw || lds < Vs || (!first && !prev_out))
    return -2;
  MultiLevelArgs a;
  a.word_logits = word_logits; a.ldw = ldw; a.sub_logits = sub_logits; a.lds = lds;
  a.prev_tok = prev_tok; a.prev_out = prev_out;
  a.word_lp = word_lp; a.cum = cum; a.nodes = nodes; a.out = out;
  a.children = children; a.prev_subword = prev_subword; a.word_idx = word_idx;
  a.Vw = Vw; a.Vs = Vs; a.D = D;
  a.sub_weight = subword_weight; a.log_oov_penalty = log_oov_penalty; a.logzero = -10.f;
  a.first = first; a.open_vocab = open_vocab; a.word_eos = word_eos; a.word_unk = word_unk;
  a.sub_space = sub_space; a.sub_eos = sub_eos; a.root_id = root_id;
  hipLaunchKernelGGL(multilevel_step_kernel, dim3(N), dim3(256), 0, stream, a);
  return EA_CHECK_LAUNCH();
}
