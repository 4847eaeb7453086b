// CTC prefix beam search (Hannun et al. 2014, "First-pass large vocabulary continuous speech recognition using
// bi-directional recurrent DNNs") with optional shallow fusion of a sub-word LM, for gfx950.  The reference decodes CTC
// with a beam only through Flashlight's KenLM lexicon decoder (espresso/tools/ctc_decoder.py:55-71); this is its
// neural-LM counterpart.  Latency bound: one 256-thread workgroup per utterance owns that utterance's beam in the
// workspace, and workgroups never talk to each other.
//
// Per frame (ctc_beam_step_kernel, one frame per launch with an LM, the whole utterance in one launch without):
//   1. the K best non-blank tokens of the frame row (ties: lower id), by radix select on unique 48-bit keys;
//   2. the <= beam * (K + 1) candidates in LDS: every hypothesis stays (blank / repeat of its last token) and extends by
//      every candidate token; an extension y' + c that equals a hypothesis y of the beam merges into y's stay;
//   3. the `beam` best by score (ties: parent slot, stay before extension, token id), again by radix select;
//   4. the new state, and with an LM the (gather row, token, keep) triple the host's LM update consumes.
// Prefixes are canonical nodes of a per-utterance prefix table (node 0 = the empty prefix; node_par / node_tok = the
// backpointers, filled as extensions survive).  A hash table keyed by the exact pair (parent node, token) gives every token
// sequence exactly one node, so y' + c == y  <=>  node(y') == pnode(y) && last(y) == c: prefixes merge iff their token
// sequences are equal.
// ctc_beam_finish_kernel adds the LM's end-of-sentence term, sorts and walks the backpointers into token rows.
//
// Hotword biasing (BIAS instantiations, ea_ctc_prefix_beam_bias_*): every hypothesis also carries a state q of the context
// graph (ctc_beam_common.h) and its running bias b, both functions of the token sequence alone, so merging is untouched.  Per
// frame the root's edges of the K candidate tokens go to LDS; every extension (slot, candidate) takes one automaton step on
// its own lane (slots in the root, the usual case, read LDS only), b' joins its ranking key, and (q', b') wait in LDS for the
// selected ones.  The finish takes the pending phi(q) back.  LDS: 92 968 bytes (the unbiased instantiation: 58 664).
#include "common.h"
#include "ctc_beam_common.h"
#include "espresso_amd.h"

namespace {

constexpr int kMaxBeam = 64;
constexpr int kMaxK = 64;
constexpr int kMaxCand = kMaxBeam * (kMaxK + 1);
constexpr int kRowLds = 5120;  // frame-row columns staged in LDS (the recipe's V = 5004 fits); columns beyond: global

// per-utterance workspace: hash table (parent node, token) -> node, beam state (structure of arrays, `beam` slots), counters,
// prefix table of 1 + T * beam nodes
struct BeamWs {
  unsigned long long* tab_key;  // 0 = empty, else (parent + 1) << 32 | token
  int* tab_val;
  float *pb, *pnb, *lm;
  int *len, *last, *node, *pnode, *cnt /*[0] = hypotheses, [1] = nodes*/, *node_par, *node_tok;
  int cap, tsize;
};

__host__ __device__ __forceinline__ long beam_ws_cap(int T, int beam) { return 1L + (long)T * beam; }
__host__ __device__ __forceinline__ long beam_ws_tsize(int T, int beam) {
  long n = 64;
  while (n < 2 * beam_ws_cap(T, beam)) n <<= 1;
  return n;
}
__host__ __device__ __forceinline__ long beam_ws_words(int T, int beam) {  // 4-byte words per utterance (even)
  const long w = 3 * beam_ws_tsize(T, beam) + 7L * beam + 2 + 2 * beam_ws_cap(T, beam);
  return (w + 1) & ~1L;
}

__device__ __forceinline__ BeamWs beam_ws(void* ws, int b, int T, int beam) {
  BeamWs w;
  w.cap = (int)beam_ws_cap(T, beam);
  w.tsize = (int)beam_ws_tsize(T, beam);
  int* base = (int*)ws + (long)b * beam_ws_words(T, beam);
  w.tab_key = (unsigned long long*)base;
  w.tab_val = base + 2L * w.tsize;
  w.pb = (float*)(w.tab_val + w.tsize);
  w.pnb = w.pb + beam;
  w.lm = w.pnb + beam;
  w.len = (int*)(w.lm + beam);
  w.last = w.len + beam;
  w.node = w.last + beam;
  w.pnode = w.node + beam;
  w.cnt = w.pnode + beam;
  w.node_par = w.cnt + 2;
  w.node_tok = w.node_par + w.cap;
  return w;
}

struct StepArgs {
  const void* x; long ld; const int* in_len; void* ws;
  const float* lm_rows; long ld_lm;
  int* lm_parent; int* lm_token; uint8_t* lm_keep;
  int T, V, beam, K, blank;
  float lm_weight, ins_bonus;
  int t0, t1;
};
struct BiasStepArgs : StepArgs { CgTables g; };

// the biased search's own per-slot state (q, b): behind the B unbiased workspaces, whose layout stays what it is
struct BiasWs { int* q; float* b; };
__device__ __forceinline__ BiasWs bias_ws(void* ws, int B, int b, int T, int beam) {
  int* base = (int*)ws + (long)B * beam_ws_words(T, beam) + 2L * b * beam;
  return {base, (float*)(base + beam)};
}

template <bool BIAS> struct BiasLds {};
template <> struct BiasLds<true> {
  int q[kMaxBeam]; float b[kMaxBeam];       // per slot
  int cq[kMaxCand]; float cb[kMaxCand];     // per extension: the state and the running bias after it
  int rchild[kMaxK]; float rboost[kMaxK];   // the root's edge by each candidate token of the frame
};

template <typename TX, bool BIAS>
__global__ __launch_bounds__(256) void ctc_beam_step_kernel(const std::conditional_t<BIAS, BiasStepArgs, StepArgs> a) {
  __shared__ BiasLds<BIAS> s_bias;
  __shared__ uint64_t s_key[kMaxCand];
  __shared__ SelectScratch s_sel;
  __shared__ float s_pb[kMaxBeam], s_pnb[kMaxBeam], s_lm[kMaxBeam];  // beam state of the previous frame, slot-indexed
  __shared__ int s_len[kMaxBeam], s_last[kMaxBeam], s_node[kMaxBeam], s_pnode[kMaxBeam];
  __shared__ int s_lrank[kMaxBeam], s_msrc[kMaxBeam];  // rank of the last token among the candidates; merging extension's slot
  __shared__ unsigned long long s_merged[kMaxBeam];     // bit r of slot j: extension (j, r) merged into a stay
  __shared__ int s_ctok[kMaxK], s_cunsorted[kMaxK];
  __shared__ float s_cx[kMaxK];
  __shared__ int s_sel_idx[kMaxBeam];
  __shared__ float s_row[kRowLds];  // the frame row, read 7 times by the top-K select
  __shared__ int s_nhyp, s_nnodes, s_ncand, s_nsel, s_nfresh;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int beam = a.beam, K = a.K, K1 = a.K + 1;
  const BeamWs w = beam_ws(a.ws, b, a.T, beam);
  const int L = min(a.in_len[b], a.T);
  const float lw = a.lm_rows ? a.lm_weight : 0.f;
  const long row0 = (long)b * beam;

  if (a.t0 == 0) {  // the empty prefix, an empty node table
    for (int i = tid; i < w.tsize; i += 256) w.tab_key[i] = 0ull;
    if (tid == 0) {
      w.pb[0] = 0.f; w.pnb[0] = -INFINITY; w.lm[0] = 0.f;
      w.len[0] = 0; w.last[0] = -1; w.node[0] = 0; w.pnode[0] = -1;
      w.cnt[0] = 1; w.cnt[1] = 1;
      w.node_par[0] = -1; w.node_tok[0] = -1;
      if constexpr (BIAS) {
        const BiasWs bw = bias_ws(a.ws, gridDim.x, b, a.T, beam);
        bw.q[0] = 0; bw.b[0] = 0.f;
      }
    }
    __threadfence_block();
    __syncthreads();
  }
  if (tid == 0) { s_nhyp = ld_l2(w.cnt); s_nnodes = ld_l2(w.cnt + 1); }
  if (tid < beam) {
    s_pb[tid] = w.pb[tid]; s_pnb[tid] = w.pnb[tid]; s_lm[tid] = w.lm[tid];
    s_len[tid] = w.len[tid]; s_last[tid] = w.last[tid]; s_node[tid] = w.node[tid]; s_pnode[tid] = w.pnode[tid];
    if constexpr (BIAS) {
      const BiasWs bw = bias_ws(a.ws, gridDim.x, b, a.T, beam);
      s_bias.q[tid] = bw.q[tid]; s_bias.b[tid] = bw.b[tid];
    }
  }
  __syncthreads();

  for (int t = a.t0; t < a.t1; ++t) {
    if (t >= L) {  // past the end of this utterance: the beam stands still (the LM rows are kept)
      if (a.lm_parent && tid < beam) {
        a.lm_parent[row0 + tid] = (int)(row0 + tid); a.lm_token[row0 + tid] = a.blank; a.lm_keep[row0 + tid] = 1;
      }
      continue;
    }
    const TX* xr = (const TX*)a.x + ((long)b * a.T + t) * a.ld;
    for (int v = tid; v < min(a.V, kRowLds); v += 256) s_row[v] = ldx(xr, v);
    __syncthreads();
    auto xv = [&](int v) { return v < kRowLds ? s_row[v] : ldx(xr, v); };
    const int nh = s_nhyp;

    // 1. top-K non-blank tokens of the frame, listed in token-id order
    const int V = a.V, blank = a.blank;
    auto tok_key = [&](int v) -> uint64_t { return v == blank ? 0ull : mk_key(xv(v), v); };
    const uint64_t kth = select_nth(tok_key, V, K, s_sel);
    if (tid == 0) s_ncand = 0;
    __syncthreads();
    for (int v = tid; v < V; v += 256) {
      const uint64_t k = tok_key(v);
      if (k && k >= kth) s_cunsorted[atomicAdd(&s_ncand, 1)] = v;
    }
    __syncthreads();
    if (tid < K) {
      const int v = s_cunsorted[tid];
      int r = 0;
      for (int i = 0; i < K; ++i) r += s_cunsorted[i] < v;
      s_ctok[r] = v;
      s_cx[r] = xv(v);
      if constexpr (BIAS) {
        const CgRoot rt = cg_root(a.g, v);
        s_bias.rchild[r] = rt.child; s_bias.rboost[r] = rt.boost;
      }
    }
    if (tid < kMaxBeam) s_merged[tid] = 0ull;
    __syncthreads();

    // 2a. stays that absorb an extension: y = y' + c with c a candidate and y' in the beam
    if (tid < nh) {
      const int l = s_last[tid];
      int r = -1;
      if (s_len[tid] > 0)
        for (int i = 0; i < K; ++i) r = s_ctok[i] == l ? i : r;
      int src = -1;
      if (r >= 0)
        for (int j = 0; j < nh; ++j) src = s_node[j] == s_pnode[tid] ? j : src;
      s_lrank[tid] = r;
      s_msrc[tid] = src;
      if (src >= 0) atomicOr(&s_merged[src], 1ull << r);
    }
    __syncthreads();

    // 2b. candidate scores; index i = slot * (K + 1) + (0: stay, 1 + r: extension by the r-th candidate token)
    const float xb = xv(blank);
    auto stay_pnb = [&](int j) {
      const int r = s_lrank[j];
      float pnb = r >= 0 ? s_pnb[j] + s_cx[r] : -INFINITY;
      const int src = s_msrc[j];
      if (src >= 0) pnb = lae(pnb, (s_last[src] == s_last[j] ? s_pb[src] : lae(s_pb[src], s_pnb[src])) + s_cx[r]);
      return pnb;
    };
    auto ext_pnb = [&](int j, int r) { return (s_ctok[r] == s_last[j] ? s_pb[j] : lae(s_pb[j], s_pnb[j])) + s_cx[r]; };
    auto ext_lm = [&](int j, int r) { return a.lm_rows ? s_lm[j] + a.lm_rows[(row0 + j) * a.ld_lm + s_ctok[r]] : 0.f; };
    const int N = nh * K1;
    for (int i = tid; i < N; i += 256) {
      const int j = i / K1, q = i - j * K1;
      uint64_t key = 0ull;
      if (q == 0) {
        float s = lae(lae(s_pb[j], s_pnb[j]) + xb, stay_pnb(j)) + lw * s_lm[j] + a.ins_bonus * (float)s_len[j];
        if constexpr (BIAS) s += s_bias.b[j];
        key = mk_key(s, i);
      } else if (!((s_merged[j] >> (q - 1)) & 1ull)) {
        float s = ext_pnb(j, q - 1) + lw * ext_lm(j, q - 1) + a.ins_bonus * (float)(s_len[j] + 1);
        if constexpr (BIAS) {  // one automaton step per live extension, each on its own lane
          const CgStep st = cg_step(a.g, s_bias.q[j], s_ctok[q - 1], CgRoot{s_bias.rchild[q - 1], s_bias.rboost[q - 1]});
          const float nb = s_bias.b[j] + st.inc;
          s_bias.cq[i] = st.q; s_bias.cb[i] = nb;
          s += nb;
        }
        key = mk_key(s, i);
      }
      s_key[i] = key;
    }
    __syncthreads();

    // 3. the `beam` best candidates
    const uint64_t cth = select_nth([&](int i) { return s_key[i]; }, N, beam, s_sel);
    if (tid == 0) s_nsel = 0;
    __syncthreads();
    for (int i = tid; i < N; i += 256) {
      const uint64_t k = s_key[i];
      if (k && k >= cth) s_sel_idx[atomicAdd(&s_nsel, 1)] = i;
    }
    __syncthreads();
    const int ns = s_nsel;

    // 4. new state (wave 0: lane = one selected candidate, written to slot = its rank)
    float n_pb = 0.f, n_pnb = 0.f, n_lm = 0.f;
    int n_len = 0, n_last = -1, n_node = 0, n_pnode = -1, slot = 0, par = 0, ext = 0, fresh = 0, tslot = -1;
    int n_q = 0;
    float n_b = 0.f;
    if (tid < ns) {
      const int i = s_sel_idx[tid];
      const uint64_t k = s_key[i];
      for (int m = 0; m < ns; ++m) slot += s_key[s_sel_idx[m]] > k;
      const int j = i / K1, q = i - j * K1;
      par = j;
      if (q == 0) {
        n_pb = lae(s_pb[j], s_pnb[j]) + xb; n_pnb = stay_pnb(j); n_lm = s_lm[j];
        n_len = s_len[j]; n_last = s_last[j]; n_node = s_node[j]; n_pnode = s_pnode[j];
        if constexpr (BIAS) { n_q = s_bias.q[j]; n_b = s_bias.b[j]; }
      } else {
        ext = 1;
        if constexpr (BIAS) { n_q = s_bias.cq[i]; n_b = s_bias.cb[i]; }
        const int r = q - 1;
        n_pb = -INFINITY; n_pnb = ext_pnb(j, r); n_lm = ext_lm(j, r);
        n_len = s_len[j] + 1; n_last = s_ctok[r]; n_pnode = s_node[j];
        // the node of prefix(j) + c: found in the hash table, or claimed there (distinct keys within one frame)
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
        const int id = s_nnodes + __popcll(fm & ((1ull << tid) - 1ull));
        n_node = id;
        w.tab_val[tslot] = id;
        if (id < w.cap) { w.node_par[id] = n_pnode; w.node_tok[id] = n_last; }
      }
      if (tid == 0) s_nfresh = __popcll(fm);
    }
    __syncthreads();
    if (tid < ns) {
      s_pb[slot] = n_pb; s_pnb[slot] = n_pnb; s_lm[slot] = n_lm;
      s_len[slot] = n_len; s_last[slot] = n_last; s_node[slot] = n_node; s_pnode[slot] = n_pnode;
      if constexpr (BIAS) { s_bias.q[slot] = n_q; s_bias.b[slot] = n_b; }
      if (a.lm_parent) {
        a.lm_parent[row0 + slot] = (int)(row0 + par);
        a.lm_token[row0 + slot] = ext ? n_last : a.blank;
        a.lm_keep[row0 + slot] = (uint8_t)!ext;
      }
    } else if (a.lm_parent && tid < beam) {  // empty slot: any valid row
      a.lm_parent[row0 + tid] = (int)row0; a.lm_token[row0 + tid] = a.blank; a.lm_keep[row0 + tid] = 1;
    }
    if (tid == 0) { s_nhyp = ns; s_nnodes += s_nfresh; }
    __threadfence();  // this frame's table entries, before the next frame's L2 reads
    __syncthreads();
  }

  if (tid == 0) { w.cnt[0] = s_nhyp; w.cnt[1] = s_nnodes; }
  if (tid < beam) {
    w.pb[tid] = s_pb[tid]; w.pnb[tid] = s_pnb[tid]; w.lm[tid] = s_lm[tid];
    w.len[tid] = s_len[tid]; w.last[tid] = s_last[tid]; w.node[tid] = s_node[tid]; w.pnode[tid] = s_pnode[tid];
    if constexpr (BIAS) {
      const BiasWs bw = bias_ws(a.ws, gridDim.x, b, a.T, beam);
      bw.q[tid] = s_bias.q[tid]; bw.b[tid] = s_bias.b[tid];
    }
  }
}

struct NoBias {};

// final score = s(y) + lm_weight * log P_lm(eos | y) [+ b - phi(q)]; the nbest best, sorted, backtracked into tokens [B][nbest][T]
template <bool BIAS>
__global__ __launch_bounds__(64) void ctc_beam_finish_kernel(void* ws, const float* lm_rows, long ld_lm, float lm_weight,
                                                             float ins_bonus, int eos, int T, int beam, int nbest, int pad,
                                                             int* tokens, int* lengths, float* scores, int* nhyp,
                                                             const std::conditional_t<BIAS, CgTables, NoBias> g) {
  __shared__ float s_fin[kMaxBeam];
  const int b = blockIdx.x, j = threadIdx.x;
  const BeamWs w = beam_ws(ws, b, T, beam);
  const int nh = w.cnt[0];
  const long row0 = (long)b * beam;
  if (j < nh) {
    float s = lae(w.pb[j], w.pnb[j]) + ins_bonus * (float)w.len[j];
    if (lm_rows) s += lm_weight * (w.lm[j] + lm_rows[(row0 + j) * ld_lm + eos]);
    if constexpr (BIAS) {
      const BiasWs bw = bias_ws(ws, gridDim.x, b, T, beam);
      s += bw.b[j] - cg_phi(g, bw.q[j]);
    }
    s_fin[j] = s;
  }
  __syncthreads();
  if (j == 0) nhyp[b] = min(nh, nbest);
  if (j < nh) {
    const float s = s_fin[j];
    int rank = 0;
    for (int m = 0; m < nh; ++m) rank += s_fin[m] > s || (s_fin[m] == s && m < j);
    if (rank < nbest) {
      int* out = tokens + ((long)b * nbest + rank) * T;
      const int n = w.len[j];
      for (int u = n; u < T; ++u) out[u] = pad;
      int node = w.node[j];
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

// replay of token rows through the context graph: one lane per row
__global__ __launch_bounds__(256) void context_graph_score_kernel(const CgTables g, const int* tokens, const int* lens, int N,
                                                                   int L, float* running, float* final_bias, int* q_out) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  cg_replay(g, tokens + (long)n * L, min(max(lens[n], 0), L), running ? running + (long)n * L : nullptr, final_bias + n,
            q_out + n);
}

}  // namespace

extern "C" long ea_ctc_prefix_beam_workspace_bytes(int B, int T, int beam) {
  if (B <= 0 || T < 0 || beam < 1 || beam > kMaxBeam) return 0;
  return (long)B * beam_ws_words(T, beam) * 4L;
}

static int step_args_ok(long ld, const float* lm_rows, long ld_lm, const int* lm_parent, const int* lm_token, const void* lm_keep,
                        int T, int V, int beam, int K, int blank, int t0, int t1) {
  return !(T < 0 || V < 2 || V > 65535 || ld < V || beam < 1 || beam > kMaxBeam || K < 1 || K > kMaxK || K > V - 1 || blank < 0 ||
           blank >= V || t0 < 0 || t1 < t0 || t1 > T || (lm_rows && (ld_lm < V || !lm_parent || !lm_token || !lm_keep)));
}

static void fill_step_args(StepArgs& a, const void* x, long ld, const int* in_len, void* workspace, const float* lm_rows, long ld_lm,
                           int* lm_parent, int* lm_token, void* lm_keep, int T, int V, int beam, int K, int blank, float lm_weight,
                           float ins_bonus, int t0, int t1) {
  a.x = x; a.ld = ld; a.in_len = in_len; a.ws = workspace;
  a.lm_rows = lm_rows; a.ld_lm = ld_lm;
  a.lm_parent = lm_parent; a.lm_token = lm_token; a.lm_keep = (uint8_t*)lm_keep;
  a.T = T; a.V = V; a.beam = beam; a.K = K; a.blank = blank;
  a.lm_weight = lm_weight; a.ins_bonus = ins_bonus;
  a.t0 = t0; a.t1 = t1;
}

extern "C" int ea_ctc_prefix_beam_step(const void* x, long ld, int x_bf16, const int* in_len, void* workspace,
                                       const float* lm_rows, long ld_lm, int* lm_parent, int* lm_token, void* lm_keep, int B,
                                       int T, int V, int beam, int K, int blank, float lm_weight, float ins_bonus, int t0, int t1,
                                       hipStream_t stream) {
  if (B <= 0) return 0;
  if (!step_args_ok(ld, lm_rows, ld_lm, lm_parent, lm_token, lm_keep, T, V, beam, K, blank, t0, t1)) return -2;
  StepArgs a;
  fill_step_args(a, x, ld, in_len, workspace, lm_rows, ld_lm, lm_parent, lm_token, lm_keep, T, V, beam, K, blank, lm_weight,
                 ins_bonus, t0, t1);
  if (x_bf16)
    hipLaunchKernelGGL((ctc_beam_step_kernel<bf16_t, false>), dim3(B), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((ctc_beam_step_kernel<float, false>), dim3(B), dim3(256), 0, stream, a);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_prefix_beam_finish(void* workspace, const float* lm_rows, long ld_lm, float lm_weight, float ins_bonus,
                                         int eos, int B, int T, int beam, int nbest, int pad, int* tokens, int* lengths,
                                         float* scores, int* nhyp, hipStream_t stream) {
  if (B <= 0) return 0;
  if (T < 0 || beam < 1 || beam > kMaxBeam || nbest < 1 || nbest > beam || (lm_rows && eos < 0)) return -2;
  hipLaunchKernelGGL(ctc_beam_finish_kernel<false>, dim3(B), dim3(64), 0, stream, workspace, lm_rows, ld_lm, lm_weight,
                     ins_bonus, eos, T, beam, nbest, pad, tokens, lengths, scores, nhyp, NoBias{});
  return EA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------ hotword biasing
extern "C" long ea_ctc_prefix_beam_bias_workspace_bytes(int B, int T, int beam) {
  const long base = ea_ctc_prefix_beam_workspace_bytes(B, T, beam);
  return base ? base + (long)B * 2L * beam * 4L : 0;
}

extern "C" int ea_ctc_prefix_beam_bias_step(const void* x, long ld, int x_bf16, const int* in_len, void* workspace,
                                            const float* lm_rows, long ld_lm, int* lm_parent, int* lm_token, void* lm_keep,
                                            const int* cg_nodes, const int* cg_edges, const int* cg_root, int cg_n_nodes,
                                            int cg_n_edges, int B, int T, int V, int beam, int K, int blank, float lm_weight,
                                            float ins_bonus, int t0, int t1, hipStream_t stream) {
  if (B <= 0) return 0;
  BiasStepArgs a;
  if (!step_args_ok(ld, lm_rows, ld_lm, lm_parent, lm_token, lm_keep, T, V, beam, K, blank, t0, t1) ||
      !cg_tables(a.g, cg_nodes, cg_edges, cg_root, cg_n_nodes, cg_n_edges, V))
    return -2;
  fill_step_args(a, x, ld, in_len, workspace, lm_rows, ld_lm, lm_parent, lm_token, lm_keep, T, V, beam, K, blank, lm_weight,
                 ins_bonus, t0, t1);
  if (x_bf16)
    hipLaunchKernelGGL((ctc_beam_step_kernel<bf16_t, true>), dim3(B), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((ctc_beam_step_kernel<float, true>), dim3(B), dim3(256), 0, stream, a);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_prefix_beam_bias_finish(void* workspace, const float* lm_rows, long ld_lm, float lm_weight, float ins_bonus,
                                              int eos, const int* cg_nodes, int cg_n_nodes, int B, int T, int beam, int nbest,
                                              int pad, int* tokens, int* lengths, float* scores, int* nhyp, hipStream_t stream) {
  if (B <= 0) return 0;
  if (T < 0 || beam < 1 || beam > kMaxBeam || nbest < 1 || nbest > beam || (lm_rows && eos < 0) || !cg_nodes || cg_n_nodes < 1)
    return -2;
  hipLaunchKernelGGL(ctc_beam_finish_kernel<true>, dim3(B), dim3(64), 0, stream, workspace, lm_rows, ld_lm, lm_weight, ins_bonus,
                     eos, T, beam, nbest, pad, tokens, lengths, scores, nhyp, cg_nodes_only(cg_nodes, cg_n_nodes));
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_context_graph_score_host(const int* nodes_host, const int* edges_host, const int* root_host, int n_nodes,
                                           int n_edges, int V, const int* tokens_host, const int* lens_host, int N, int L,
                                           float* running_host, float* final_host, int* q_host) {
  CgTables g;
  if (N < 0 || L < 0 || !cg_tables(g, nodes_host, edges_host, root_host, n_nodes, n_edges, V)) return -2;
  // host tables are checked in full: every index in range, fail links strictly towards the root in node order
  for (int n = 0; n < n_nodes; ++n) {
    const int* r = nodes_host + 4L * n;
    if (r[0] < 0 || r[1] < r[0] || r[1] > n_edges || r[2] < 0 || r[2] >= n_nodes) return -2;
  }
  for (int e = 0; e < n_edges; ++e)
    if (edges_host[4L * e + 1] < 1 || edges_host[4L * e + 1] >= n_nodes) return -2;
  for (int v = 0; v < V; ++v)
    if (root_host[2L * v] < -1 || root_host[2L * v] >= n_nodes) return -2;
  for (int n = 0; n < N; ++n) {
    const int len = lens_host[n] < 0 ? 0 : (lens_host[n] > L ? L : lens_host[n]);
    cg_replay(g, tokens_host + (long)n * L, len, running_host ? running_host + (long)n * L : nullptr, final_host + n, q_host + n);
  }
  return 0;
}

extern "C" int ea_context_graph_score(const int* nodes, const int* edges, const int* root, int n_nodes, int n_edges, int V,
                                      const int* tokens, const int* lens, int N, int L, float* running, float* final_bias,
                                      int* q_out, hipStream_t stream) {
  CgTables g;
  if (N < 0 || L < 0 || !cg_tables(g, nodes, edges, root, n_nodes, n_edges, V)) return -2;
  if (N == 0) return 0;
  hipLaunchKernelGGL(context_graph_score_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, g, tokens, lens, N, L, running,
                     final_bias, q_out);
  return EA_CHECK_LAUNCH();
}
