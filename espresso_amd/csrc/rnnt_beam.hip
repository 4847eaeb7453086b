// Frame-synchronous transducer beam search ("modified beam search": at most one symbol per encoder frame and hypothesis, equal
// token sequences merged) with optional mass-preserving shallow fusion of one sub-word LM, for gfx950 — the transducer
// counterpart of ctc_beam.hip.  The reference searches transducers with the modified Adaptive Expansion Search only
// (espresso/tools/transducer_beam_search_decoder.py); this search keeps beam, prefix table and selection on the device.
//
// Contract, per utterance: hypotheses = distinct token sequences y with a score s(y) (natural log), at most `beam`, best first,
// start {(), 0}.  ea_rnnt_frame_beam_step takes the joint's fp32 logits of ONE frame t for all B * beam slots (row = b * beam +
// slot; it never sees the encoder), so the state between two calls is exactly the workspace: a streamed search can feed it frame
// by frame.  For every live slot j (dead slots, j >= number of hypotheses, are never read):
//   1. r = log_softmax(logits[:V] / temperature);
//   2. with an LM (row m = log P_lm(. | eos + y_j), weight w): for v != blank f_v = r_v + w * m_v and
//      r_v = f_v + log sum_{v != blank} e^{r_v} - log sum_{v != blank} e^{f_v} (the non-blank mass stays); r_blank untouched.  An LM
//      without a blank entry (lm_no_blank): token v > blank reads column v - 1;
//   3. with eos >= 0 (the model predicts eos): r_blank = logaddexp(r_blank, r_eos), r_eos = -inf;
//   4. candidates: the stay (y_j, s_j + r_blank), key (j, 0, 0), and for the K non-blank tokens with the largest finite r_v
//      (ties: lower id) the extensions (y_j + v, s_j + r_v), key (j, 1, v).
// An extension equal to a hypothesis of the beam merges into that hypothesis' stay (scores: log-add-exp; key and predictor state:
// the stay's).  The `beam` best finite candidates by (-score, key) survive; per surviving slot the step writes parent (row of
// the previous frame), token (the appended token; blank for a stay) and keep (1 = stay): what reorder_state + advance(token,
// state, keep_row) consume for the predictor and the LM.  Frames t >= in_len[b]: parent = identity, keep = 1, nothing changes.
//
// Two kernels per frame.  rnnt_beam_row_kernel, one 256-thread workgroup per live row (B * beam of them: 240 at the recipe's
// batch, about one per CU): the row goes to LDS once (20 KB at V = 5004), max / log-sum-exp / the two non-blank sums / the
// fusion in fp32 there, then the row's top K by radix select; it leaves (K tokens in id order, their r, r_blank) in the
// workspace — no [N][V] log-prob tensor is written.  rnnt_beam_select_kernel, one workgroup per utterance: merge, the `beam`
// best of <= beam * (K + 1) candidates by radix select, the new state and the triples.  One workgroup per utterance doing both
// would run the 7-pass select over V serially for `beam` rows on 24 of 256 CUs.
// Prefix table as ctc_beam.hip: a canonical node per token sequence (hash of (parent node, token)), node ids in creation
// order, cap = 1 + T * beam; sequence equality is node equality: y_j + v == y_i  <=>  node(y_j) == pnode(y_i) && last(y_i) == v.
#include "common.h"
#include "ctc_beam_common.h"
#include "espresso_amd.h"

namespace {

constexpr int kMaxBeam = 64;
constexpr int kMaxK = 64;
constexpr int kMaxCand = kMaxBeam * (kMaxK + 1);
constexpr int kRowLds = 5120;  // row columns staged in LDS (the recipe's V = 5004 fits); columns beyond are recomputed from global

// per-utterance workspace: hash table (parent node, token) -> node, beam state (structure of arrays, `beam` slots), counters,
// prefix table of 1 + T * beam nodes, and what the row phase hands to the select phase
struct RnntWs {
  unsigned long long* tab_key;  // 0 = empty, else (parent + 1) << 32 | token
  int* tab_val;
  float* score;
  int *len, *last, *node, *pnode, *cnt /*[0] = hypotheses, [1] = nodes*/, *node_par, *node_tok;
  float* rblank;  // [beam] r_blank of the slot's row
  int* rnc;       // [beam] candidates of the row (<= K)
  int* ctok;      // [beam][kMaxK] candidate tokens, ascending
  float* cval;    // [beam][kMaxK] their r
  int cap, tsize;
};

__host__ __device__ __forceinline__ long rnnt_ws_cap(int T, int beam) { return 1L + (long)T * beam; }
__host__ __device__ __forceinline__ long rnnt_ws_tsize(int T, int beam) {
  long n = 64;
  while (n < 2 * rnnt_ws_cap(T, beam)) n <<= 1;
  return n;
}
__host__ __device__ __forceinline__ long rnnt_ws_words(int T, int beam) {  // 4-byte words per utterance (even)
  const long w = 3 * rnnt_ws_tsize(T, beam) + 5L * beam + 2 + 2 * rnnt_ws_cap(T, beam) + 2L * beam + 2L * beam * kMaxK;
  return (w + 1) & ~1L;
}

__device__ __forceinline__ RnntWs rnnt_ws(void* ws, int b, int T, int beam) {
  RnntWs w;
  w.cap = (int)rnnt_ws_cap(T, beam);
  w.tsize = (int)rnnt_ws_tsize(T, beam);
  int* base = (int*)ws + (long)b * rnnt_ws_words(T, beam);
  w.tab_key = (unsigned long long*)base;
  w.tab_val = base + 2L * w.tsize;
  w.score = (float*)(w.tab_val + w.tsize);
  w.len = (int*)(w.score + beam);
  w.last = w.len + beam;
  w.node = w.last + beam;
  w.pnode = w.node + beam;
  w.cnt = w.pnode + beam;
  w.node_par = w.cnt + 2;
  w.node_tok = w.node_par + w.cap;
  w.rblank = (float*)(w.node_tok + w.cap);
  w.rnc = (int*)(w.rblank + beam);
  w.ctok = w.rnc + beam;
  w.cval = (float*)(w.ctok + (long)beam * kMaxK);
  return w;
}

struct RowArgs {
  const float* logits; long ld;
  const float* lm_rows; long ld_lm; int lm_no_blank;
  const int* in_len; void* ws;
  int T, V, beam, K, blank, eos;
  float temperature, lm_weight;
  int t;
};

// steps 1 - 3 of the contract and the row's top K, one workgroup per (utterance, slot)
__global__ __launch_bounds__(256) void rnnt_beam_row_kernel(const RowArgs a) {
  __shared__ float s_row[kRowLds];
  __shared__ SelectScratch s_sel;
  __shared__ float s_red[16];
  __shared__ int s_cunsorted[kMaxK];
  __shared__ int s_nc;
  const int n = blockIdx.x, b = n / a.beam, j = n - b * a.beam, tid = threadIdx.x;
  const RnntWs w = rnnt_ws(a.ws, b, a.T, a.beam);
  if (a.t >= min(a.in_len[b], a.T)) return;  // past the end of this utterance
  const int nh = a.t == 0 ? 1 : w.cnt[0];    // (frame 0 starts from the empty hypothesis: the select phase initialises)
  if (j >= nh) return;                       // dead slot: the row is not read
  const float* x = a.logits + (long)n * a.ld;
  const float* m = a.lm_rows ? a.lm_rows + (long)n * a.ld_lm : nullptr;
  const int V = a.V, blank = a.blank, eos = a.eos;
  const float temp = a.temperature, lw = a.lm_weight;
  auto lm_col = [&](int v) { return a.lm_no_blank && v > blank ? v - 1 : v; };

  // 1. z = logits / temperature to LDS; max, log-sum-exp, and the non-blank part of the sum
  float mx = -INFINITY;
  for (int v = tid; v < V; v += 256) {
    const float z = x[v] / temp;
    if (v < kRowLds) s_row[v] = z;
    mx = fmaxf(mx, z);
  }
  mx = block_max(mx, s_red);
  auto z_of = [&](int v) { return v < kRowLds ? s_row[v] : x[v] / temp; };
  float sa = 0.f, snb = 0.f;
  for (int v = tid; v < V; v += 256) {
    const float e = expf(z_of(v) - mx);
    sa += e;
    snb += v == blank ? 0.f : e;
  }
  sa = block_sum(sa, s_red);
  snb = block_sum(snb, s_red);
  const float lse = mx + logf(sa);
  float rb = z_of(blank) - lse;
  float shift = -lse;  // r_v = (what LDS holds for v) + shift

  // 2. fusion: f_v replaces z_v for v != blank; the shift gives the fused row the non-blank mass of the unfused one
  if (m) {
    float fm = -INFINITY;
    for (int v = tid; v < V; v += 256) {
      if (v == blank) continue;
      const float f = z_of(v) - lse + lw * m[lm_col(v)];
      if (v < kRowLds) s_row[v] = f;
      fm = fmaxf(fm, f);
    }
    fm = block_max(fm, s_red);
    auto f_of = [&](int v) { return v < kRowLds ? s_row[v] : x[v] / temp - lse + lw * m[lm_col(v)]; };
    float sf = 0.f;
    for (int v = tid; v < V; v += 256) sf += v == blank ? 0.f : expf(f_of(v) - fm);
    sf = block_sum(sf, s_red);
    shift = logf(snb) - logf(sa) - (fm + logf(sf));
  }
  auto r_of = [&](int v) {
    if (v < kRowLds) return s_row[v] + shift;
    return (m ? x[v] / temp - lse + lw * m[lm_col(v)] : x[v] / temp) + shift;
  };
  // 3. the model's eos counts as blank
  if (eos >= 0) rb = lae(rb, r_of(eos));

  // 4. the K non-blank tokens with the largest finite r, listed in token-id order
  auto tok_key = [&](int v) -> uint64_t {
    if (v == blank || v == eos) return 0ull;
    const float r = r_of(v);
    return isfinite(r) ? mk_key(r, v) : 0ull;
  };
  const uint64_t kth = select_nth(tok_key, V, a.K, s_sel);
  if (tid == 0) s_nc = 0;
  __syncthreads();
  for (int v = tid; v < V; v += 256) {
    const uint64_t k = tok_key(v);
    if (k && k >= kth) s_cunsorted[atomicAdd(&s_nc, 1)] = v;
  }
  __syncthreads();
  const int nc = s_nc;  // <= K: the keys are unique
  if (tid < nc) {
    const int v = s_cunsorted[tid];
    int r = 0;
    for (int i = 0; i < nc; ++i) r += s_cunsorted[i] < v;
    w.ctok[(long)j * kMaxK + r] = v;
    w.cval[(long)j * kMaxK + r] = r_of(v);
  }
  if (tid == 0) { w.rblank[j] = rb; w.rnc[j] = nc; }
}

struct SelArgs {
  const int* in_len; void* ws;
  int* parent; int* token; uint8_t* keep;
  int T, beam, K, blank, t;
};

// merge, selection and the new state of one utterance
__global__ __launch_bounds__(256) void rnnt_beam_select_kernel(const SelArgs a) {
  __shared__ uint64_t s_key[kMaxCand];
  __shared__ SelectScratch s_sel;
  __shared__ int s_ctok[kMaxBeam * kMaxK];   // [slot][K]
  __shared__ float s_cval[kMaxBeam * kMaxK];
  __shared__ float s_score[kMaxBeam], s_rb[kMaxBeam], s_stay[kMaxBeam];
  __shared__ int s_len[kMaxBeam], s_last[kMaxBeam], s_node[kMaxBeam], s_pnode[kMaxBeam], s_nc[kMaxBeam];
  __shared__ unsigned long long s_merged[kMaxBeam];  // bit r of slot j: extension (j, r) merged into a stay
  __shared__ int s_sel_idx[kMaxBeam];
  __shared__ int s_nsel, s_nfresh;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int beam = a.beam, K = a.K, K1 = a.K + 1;
  const RnntWs w = rnnt_ws(a.ws, b, a.T, beam);
  const long row0 = (long)b * beam;

  if (a.t == 0) {  // the empty hypothesis, an empty node table
    for (int i = tid; i < w.tsize; i += 256) w.tab_key[i] = 0ull;
    if (tid == 0) {
      w.score[0] = 0.f; w.len[0] = 0; w.last[0] = -1; w.node[0] = 0; w.pnode[0] = -1;
      w.cnt[0] = 1; w.cnt[1] = 1;
      w.node_par[0] = -1; w.node_tok[0] = -1;
    }
    __threadfence_block();
    __syncthreads();
  }
  if (a.t >= min(a.in_len[b], a.T)) {  // past the end of this utterance: the beam stands still
    if (tid < beam) { a.parent[row0 + tid] = (int)(row0 + tid); a.token[row0 + tid] = a.blank; a.keep[row0 + tid] = 1; }
    return;
  }
  const int nh = a.t == 0 ? 1 : w.cnt[0];
  const int nnodes = a.t == 0 ? 1 : w.cnt[1];
  if (tid < nh) {
    s_score[tid] = w.score[tid]; s_len[tid] = w.len[tid]; s_last[tid] = w.last[tid]; s_node[tid] = w.node[tid];
    s_pnode[tid] = w.pnode[tid]; s_rb[tid] = w.rblank[tid]; s_nc[tid] = w.rnc[tid];
    s_merged[tid] = 0ull;
  }
  for (int i = tid; i < nh * K; i += 256) {  // (entries at or beyond a row's count are never used)
    const int j = i / K, r = i - j * K;
    s_ctok[i] = w.ctok[(long)j * kMaxK + r];
    s_cval[i] = w.cval[(long)j * kMaxK + r];
  }
  __syncthreads();

  // stays; a stay absorbs the extension y' + v == y (y' in the beam, v among its candidates)
  if (tid < nh) {
    float st = s_score[tid] + s_rb[tid];
    if (s_len[tid] > 0) {
      int src = -1;
      for (int j = 0; j < nh; ++j) src = s_node[j] == s_pnode[tid] ? j : src;
      if (src >= 0) {
        const int nc = min(s_nc[src], K);
        for (int r = 0; r < nc; ++r)
          if (s_ctok[src * K + r] == s_last[tid]) {
            atomicOr(&s_merged[src], 1ull << r);
            st = lae(st, s_score[src] + s_cval[src * K + r]);
          }
      }
    }
    s_stay[tid] = st;
  }
  __syncthreads();

  // candidates; index i = slot * (K + 1) + (0: stay, 1 + r: extension by the slot's r-th candidate token)
  const int N = nh * K1;
  for (int i = tid; i < N; i += 256) {
    const int j = i / K1, q = i - j * K1;
    float s = NAN;
    if (q == 0) s = s_stay[j];
    else if (q - 1 < s_nc[j] && !((s_merged[j] >> (q - 1)) & 1ull)) s = s_score[j] + s_cval[j * K + q - 1];
    s_key[i] = isfinite(s) ? mk_key(s, i) : 0ull;
  }
  __syncthreads();
  const uint64_t cth = select_nth([&](int i) { return s_key[i]; }, N, beam, s_sel);
  if (tid == 0) s_nsel = 0;
  __syncthreads();
  for (int i = tid; i < N; i += 256) {
    const uint64_t k = s_key[i];
    if (k && k >= cth) s_sel_idx[atomicAdd(&s_nsel, 1)] = i;
  }
  __syncthreads();
  const int ns = s_nsel;

  // the new state (wave 0: lane = one selected candidate, written to slot = its rank)
  float n_score = 0.f;
  int n_len = 0, n_last = -1, n_node = 0, n_pnode = -1, slot = 0, par = 0, ext = 0, fresh = 0, tslot = -1;
  if (tid < ns) {
    const int i = s_sel_idx[tid];
    const uint64_t k = s_key[i];
    for (int m = 0; m < ns; ++m) slot += s_key[s_sel_idx[m]] > k;
    const int j = i / K1, q = i - j * K1;
    par = j;
    if (q == 0) {
      n_score = s_stay[j]; n_len = s_len[j]; n_last = s_last[j]; n_node = s_node[j]; n_pnode = s_pnode[j];
    } else {
      ext = 1;
      n_score = s_score[j] + s_cval[j * K + q - 1];
      n_len = s_len[j] + 1; n_last = s_ctok[j * K + q - 1]; n_pnode = s_node[j];
      // the node of y_j + v: found in the hash table, or claimed there (distinct keys within one frame)
      const unsigned long long key = ((unsigned long long)(n_pnode + 1) << 32) | (uint32_t)n_last;
      const uint32_t mask = (uint32_t)w.tsize - 1u;
      for (uint32_t h = tab_hash(key) & mask;; h = (h + 1) & mask) {
        const unsigned long long cur = ld_l2(w.tab_key + h);
        if (cur == key) { n_node = ld_l2(w.tab_val + h); break; }
        if (cur == 0ull && atomicCAS(w.tab_key + h, 0ull, key) == 0ull) { fresh = 1; tslot = (int)h; break; }
      }
    }
  }
  if (tid < 64) {  // fresh nodes numbered in lane order (deterministic)
    const unsigned long long fm = __ballot(fresh);
    if (fresh) {
      const int id = nnodes + __popcll(fm & ((1ull << tid) - 1ull));
      n_node = id;
      w.tab_val[tslot] = id;
      if (id < w.cap) { w.node_par[id] = n_pnode; w.node_tok[id] = n_last; }
    }
    if (tid == 0) s_nfresh = __popcll(fm);
  }
  __syncthreads();
  if (tid < ns) {
    w.score[slot] = n_score; w.len[slot] = n_len; w.last[slot] = n_last; w.node[slot] = n_node; w.pnode[slot] = n_pnode;
    a.parent[row0 + slot] = (int)(row0 + par);
    a.token[row0 + slot] = ext ? n_last : a.blank;
    a.keep[row0 + slot] = (uint8_t)!ext;
  } else if (tid < beam) {  // empty slot: any valid row
    a.parent[row0 + tid] = (int)row0; a.token[row0 + tid] = a.blank; a.keep[row0 + tid] = 1;
  }
  if (tid == 0) { w.cnt[0] = ns; w.cnt[1] = nnodes + s_nfresh; }
}

// final score = s, or s / max(1, |y|); the nbest best by (-final, slot), backtracked into tokens [B][nbest][T]
__global__ __launch_bounds__(64) void rnnt_beam_finish_kernel(void* ws, int T, int beam, int nbest, int pad, int normalize,
                                                              int* tokens, int* lengths, float* scores, int* nhyp) {
  __shared__ float s_fin[kMaxBeam];
  const int b = blockIdx.x, j = threadIdx.x;
  const RnntWs w = rnnt_ws(ws, b, T, beam);
  const int nh = T == 0 ? 1 : w.cnt[0];  // (no frame at all: no step ran; the empty hypothesis)
  if (j < nh) {
    const float s = T == 0 ? 0.f : w.score[j];
    const int n = T == 0 ? 0 : w.len[j];
    s_fin[j] = normalize ? s / (float)max(1, n) : s;
  }
  __syncthreads();
  if (j == 0) nhyp[b] = min(nh, nbest);
  if (j < nh) {
    const float s = s_fin[j];
    int rank = 0;
    for (int m = 0; m < nh; ++m) rank += s_fin[m] > s || (s_fin[m] == s && m < j);
    if (rank < nbest) {
      int* out = tokens + ((long)b * nbest + rank) * T;
      const int n = T == 0 ? 0 : w.len[j];
      for (int u = n; u < T; ++u) out[u] = pad;
      int node = T == 0 ? 0 : w.node[j];
      for (int u = n - 1; u >= 0 && node > 0; --u) { out[u] = w.node_tok[node]; node = w.node_par[node]; }
      lengths[b * nbest + rank] = n;
      scores[b * nbest + rank] = s;
    }
  }
  for (int r = nh + j; r < nbest; r += 64) {
    int* out = tokens + ((long)b * nbest + r) * T;
    for (int u = 0; u < T; ++u) out[u] = pad;
    lengths[b * nbest + r] = 0;
    scores[b * nbest + r] = -INFINITY;
  }
}

}  // namespace

extern "C" long ea_rnnt_frame_beam_workspace_bytes(int B, int T, int beam) {
  if (B <= 0 || T < 0 || beam < 1 || beam > kMaxBeam) return 0;
  return (long)B * rnnt_ws_words(T, beam) * 4L;
}

extern "C" int ea_rnnt_frame_beam_step(const float* logits, long ld, const float* lm_rows, long ld_lm, int lm_no_blank,
                                       const int* in_len, void* workspace, int* parent, int* token, void* keep, int B, int T, int V,
                                       int beam, int K, int blank, int eos, float temperature, float lm_weight, int t,
                                       hipStream_t stream) {
  if (B <= 0) return 0;
  if (!logits || !in_len || !workspace || !parent || !token || !keep || T < 1 || t < 0 || t >= T || V < 2 || V > 65535 || ld < V ||
      beam < 1 || beam > kMaxBeam || K < 1 || K > kMaxK || K > V - 1 || blank < 0 || blank >= V || eos < -1 || eos >= V ||
      eos == blank || !(temperature > 0.f) || (lm_rows && ld_lm < (lm_no_blank ? V - 1 : V)))
    return -2;
  RowArgs r;
  // weight 0 is no fusion: the LM rows are not read (an entry of -inf times 0 would be NaN)
  r.logits = logits; r.ld = ld; r.lm_rows = lm_weight != 0.f ? lm_rows : nullptr; r.ld_lm = ld_lm; r.lm_no_blank = lm_no_blank;
  r.in_len = in_len; r.ws = workspace;
  r.T = T; r.V = V; r.beam = beam; r.K = K; r.blank = blank; r.eos = eos;
  r.temperature = temperature; r.lm_weight = lm_rows ? lm_weight : 0.f;
  r.t = t;
  hipLaunchKernelGGL(rnnt_beam_row_kernel, dim3(B * beam), dim3(256), 0, stream, r);
  SelArgs s;
  s.in_len = in_len; s.ws = workspace; s.parent = parent; s.token = token; s.keep = (uint8_t*)keep;
  s.T = T; s.beam = beam; s.K = K; s.blank = blank; s.t = t;
  hipLaunchKernelGGL(rnnt_beam_select_kernel, dim3(B), dim3(256), 0, stream, s);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_rnnt_frame_beam_finish(void* workspace, int B, int T, int beam, int nbest, int pad, int normalize, int* tokens,
                                         int* lengths, float* scores, int* nhyp, hipStream_t stream) {
  if (B <= 0) return 0;
  if (!workspace || !tokens || !lengths || !scores || !nhyp || T < 0 || beam < 1 || beam > kMaxBeam || nbest < 1 || nbest > beam)
    return -2;
  hipLaunchKernelGGL(rnnt_beam_finish_kernel, dim3(B), dim3(64), 0, stream, workspace, T, beam, nbest, pad, normalize, tokens,
                     lengths, scores, nhyp);
  return EA_CHECK_LAUNCH();
}
