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
//
// The streamed search (ea_ctc_prefix_beam_stream_*): the frame (ctc_beam_frame), the beam's load and store and the finish are
// __device__ templates with two wrappers each.  The offline kernels find an utterance's workspace by its batch index and its
// rows in [B][T][ld]; the streamed kernels find a stream's in one of max_streams slots (frame counter, the same workspace for
// max_frames frames, (q, b)) and its rows at row_off[b] of a packed piece.  Both instantiate the same body, so a stream fed in
// any pieces gives the offline results bit for bit; nodes are numbered in lane order and the hash is a lookup only, so
// max_frames, which sizes the table, does not change them.  LDS as above.
//
// Time stamps (kTimes instantiations, ea_ctc_prefix_beam_times_* / ea_ctc_prefix_beam_stream_times_*): every hypothesis also
// carries vb / vnb, which are pb / pnb with max in place of log-add-exp (the score of its best single alignment path; the LM,
// bonus and bias terms are functions of the token sequence and stay out), and eb / enb, pointers into a per-utterance pool of
// time nodes (parent time node, frame); node 0 = no tokens.  Stay: vb' = max(vb, vnb) + x[blank] with the pointer of the larger
// (tie: eb); vnb' = vnb + x[last], enb' = enb.  Extension by c: from (vb, eb) if c == last, else from the larger of (vb, eb),
// (vnb, enb) (tie: the blank one); vnb'' = that + x[c], a NEW time node (its pointer, t); vb'' = -inf.  An extension that merges
// into a stay replaces the stay's (vnb', enb') only if it is strictly larger.  Time nodes are made for selected candidates only,
// numbered in lane order: at most `beam` per frame, so the pool has the prefix table's cap = 1 + T * beam.  Nothing of this
// enters a ranking key: tokens, scores and triples are those of the search without times, bit for bit.  The finish walks the
// chain of the larger pointer (tie: eb) into times[u] = the frame at which token u starts on that path, and returns max(vb, vnb).
// The state lives in a SEPARATE caller-allocated times workspace; the beam workspace / stream state is the twin's, unchanged.
// Per utterance (offline, T frames) or per stream slot (T = max_frames), 4-byte words:
//   times words(T, beam) = 4 * beam + 2 + 2 * cap,  cap = 1 + T * beam
// (vb, vnb fp32 [beam]; eb, enb int32 [beam]; the node counter and a pad word; tpar [cap], tfrm [cap]).  The step kernels write
// tpar / tfrm and only the finish reads them, across a kernel boundary.  LDS: 1 032 bytes more than the twin's.
//
// Endpointing (ea_ctc_prefix_beam_stream_endpoint): a read-only probe of a slot and its times slot after an accept: for the live
// hypothesis the partial kernel reports, its length L and E, the frame of its last token on its best path (tfrm of the pointer of
// the larger of (vb, eb), (vnb, enb), tie eb: what the times finish writes as times[L - 1]), and the first rule that holds of
// silence (F - 1 - E frames without a token), empty and length (endpoint_rule, ctc_beam_common.h).  The caller then reads the
// finish and resets the slot: the stream goes on in a new segment, whose results are those of the offline search over its frames
// alone.  One wave per slot, no LDS.
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

// what a frame needs besides its row and its beam, the same for the offline and the streamed search
struct FrameParams {
  const float* lm_rows; long ld_lm;
  int* lm_parent; int* lm_token; uint8_t* lm_keep;
  int V, beam, K, blank;
  float lm_weight, ins_bonus;
};
struct StepArgs {
  const void* x; long ld; const int* in_len; void* ws;
  FrameParams p;
  int T, t0, t1;
};
struct BiasStepArgs : StepArgs { CgTables g; };
struct TimesStepArgs : BiasStepArgs { void* tws; };
struct NoBias {};
struct NoTimes {};

// the times workspace of one utterance / stream slot (see the header)
struct TimesWs {
  float *vb, *vnb;
  int *eb, *enb, *cnt /*[0] = time nodes*/, *tpar, *tfrm;
  int cap;
};
template <bool kTimes> using TimesOf = std::conditional_t<kTimes, TimesWs, NoTimes>;
__host__ __device__ __forceinline__ long times_ws_words(int T, int beam) { return 4L * beam + 2 + 2 * beam_ws_cap(T, beam); }
__device__ __forceinline__ TimesWs times_ws(void* tws, long idx, int T, int beam) {
  TimesWs w;
  w.cap = (int)beam_ws_cap(T, beam);
  int* base = (int*)tws + idx * times_ws_words(T, beam);
  w.vb = (float*)base;
  w.vnb = w.vb + beam;
  w.eb = base + 2L * beam;
  w.enb = w.eb + beam;
  w.cnt = w.enb + beam;
  w.tpar = w.cnt + 2;
  w.tfrm = w.tpar + w.cap;
  return w;
}
template <bool kTimes>
__device__ __forceinline__ TimesOf<kTimes> times_of(void* tws, long idx, int T, int beam) {
  if constexpr (kTimes) return times_ws(tws, idx, T, beam); else return NoTimes{};
}
template <bool BIAS> using GraphOf = std::conditional_t<BIAS, CgTables, NoBias>;
template <bool BIAS, class A>
__device__ __forceinline__ GraphOf<BIAS> graph_of(const A& a) {  // the graph of a kernel's bias arguments
  if constexpr (BIAS) return a.g; else return NoBias{};
}

// the biased search's own per-slot state (q, b): behind the B unbiased workspaces, whose layout stays what it is
struct BiasWs { int* q; float* b; };
__device__ __forceinline__ BiasWs bias_ws_at(int* base, int beam) { return {base, (float*)(base + beam)}; }
__device__ __forceinline__ BiasWs bias_ws(void* ws, int B, int b, int T, int beam) {
  return bias_ws_at((int*)ws + (long)B * beam_ws_words(T, beam) + 2L * b * beam, beam);
}

template <bool BIAS> struct BiasLds {};
template <> struct BiasLds<true> {
  int q[kMaxBeam]; float b[kMaxBeam];       // per slot
  int cq[kMaxCand]; float cb[kMaxCand];     // per extension: the state and the running bias after it
  int rchild[kMaxK]; float rboost[kMaxK];   // the root's edge by each candidate token of the frame
};

template <bool kTimes> struct TimesLds {};
template <> struct TimesLds<true> {
  float vb[kMaxBeam], vnb[kMaxBeam];  // per slot: the Viterbi scores and their time-node pointers
  int eb[kMaxBeam], enb[kMaxBeam];
  int ntn, ntfresh;
};

// LDS of a step kernel: the beam, which lives here over the frames of one launch, and the scratch of one frame
template <bool BIAS, bool kTimes = false>
struct FrameLds : BiasLds<BIAS>, TimesLds<kTimes> {
  uint64_t key[kMaxCand];
  SelectScratch sel;
  unsigned long long merged[kMaxBeam];                       // bit r of slot j: extension (j, r) merged into a stay
  float pb[kMaxBeam], pnb[kMaxBeam], lm[kMaxBeam];           // beam state of the previous frame, slot-indexed
  int len[kMaxBeam], last[kMaxBeam], node[kMaxBeam], pnode[kMaxBeam];
  int lrank[kMaxBeam], msrc[kMaxBeam];  // rank of the last token among the candidates; merging extension's slot
  int ctok[kMaxK], cunsorted[kMaxK];
  float cx[kMaxK];
  int sel_idx[kMaxBeam];
  float row[kRowLds];  // the frame row, read 7 times by the top-K select
  int nhyp, nnodes, ncand, nsel, nfresh;
};

// the state before frame 0: the empty prefix, an empty node table; the caller synchronises
template <bool kTimes = false>
__device__ __forceinline__ void ctc_beam_init(const BeamWs& w, const BiasWs* bw, const TimesOf<kTimes>& tw = {}) {
  const int tid = threadIdx.x;
  for (int i = tid; i < w.tsize; i += 256) w.tab_key[i] = 0ull;
  if (tid == 0) {
    w.pb[0] = 0.f; w.pnb[0] = -INFINITY; w.lm[0] = 0.f;
    w.len[0] = 0; w.last[0] = -1; w.node[0] = 0; w.pnode[0] = -1;
    w.cnt[0] = 1; w.cnt[1] = 1;
    w.node_par[0] = -1; w.node_tok[0] = -1;
    if (bw) { bw->q[0] = 0; bw->b[0] = 0.f; }
    if constexpr (kTimes) {
      tw.vb[0] = 0.f; tw.vnb[0] = -INFINITY; tw.eb[0] = 0; tw.enb[0] = 0;
      tw.cnt[0] = 1; tw.cnt[1] = 0;
      tw.tpar[0] = -1; tw.tfrm[0] = -1;
    }
  }
}

// beam <-> workspace; the caller synchronises after the load
template <bool BIAS, bool kTimes = false>
__device__ __forceinline__ void ctc_beam_load(FrameLds<BIAS, kTimes>& s, const BeamWs& w, const BiasWs& bw, int beam,
                                              const TimesOf<kTimes>& tw = {}) {
  const int tid = threadIdx.x;
  if (tid == 0) { s.nhyp = ld_l2(w.cnt); s.nnodes = ld_l2(w.cnt + 1); }
  if constexpr (kTimes) {
    if (tid == 0) s.ntn = ld_l2(tw.cnt);
    if (tid < beam) { s.vb[tid] = tw.vb[tid]; s.vnb[tid] = tw.vnb[tid]; s.eb[tid] = tw.eb[tid]; s.enb[tid] = tw.enb[tid]; }
  }
  if (tid < beam) {
    s.pb[tid] = w.pb[tid]; s.pnb[tid] = w.pnb[tid]; s.lm[tid] = w.lm[tid];
    s.len[tid] = w.len[tid]; s.last[tid] = w.last[tid]; s.node[tid] = w.node[tid]; s.pnode[tid] = w.pnode[tid];
    if constexpr (BIAS) { s.q[tid] = bw.q[tid]; s.b[tid] = bw.b[tid]; }
  }
}
template <bool BIAS, bool kTimes = false>
__device__ __forceinline__ void ctc_beam_store(const FrameLds<BIAS, kTimes>& s, const BeamWs& w, const BiasWs& bw, int beam,
                                               const TimesOf<kTimes>& tw = {}) {
  const int tid = threadIdx.x;
  if (tid == 0) { w.cnt[0] = s.nhyp; w.cnt[1] = s.nnodes; }
  if constexpr (kTimes) {
    if (tid == 0) tw.cnt[0] = s.ntn;
    if (tid < beam) { tw.vb[tid] = s.vb[tid]; tw.vnb[tid] = s.vnb[tid]; tw.eb[tid] = s.eb[tid]; tw.enb[tid] = s.enb[tid]; }
  }
  if (tid < beam) {
    w.pb[tid] = s.pb[tid]; w.pnb[tid] = s.pnb[tid]; w.lm[tid] = s.lm[tid];
    w.len[tid] = s.len[tid]; w.last[tid] = s.last[tid]; w.node[tid] = s.node[tid]; w.pnode[tid] = s.pnode[tid];
    if constexpr (BIAS) { bw.q[tid] = s.q[tid]; bw.b[tid] = s.b[tid]; }
  }
}

// the triple of an entry whose beam stands still (the LM rows are kept)
__device__ __forceinline__ void ctc_beam_identity(const FrameParams& a, long row0) {
  const int tid = threadIdx.x;
  if (a.lm_parent && tid < a.beam) {
    a.lm_parent[row0 + tid] = (int)(row0 + tid); a.lm_token[row0 + tid] = a.blank; a.lm_keep[row0 + tid] = 1;
  }
}

// One frame over the beam in LDS: the row xr, the prefix table of w; row0 = the first row of this entry in lm_rows and in the
// triple arrays.  The one body of the offline and the streamed step kernels.  kTimes: t = the frame's number, tw = its pool.
template <typename TX, bool BIAS, bool kTimes = false>
__device__ __forceinline__ void ctc_beam_frame(FrameLds<BIAS, kTimes>& s, const FrameParams& a, const BeamWs& w, const TX* xr,
                                               long row0, const GraphOf<BIAS>& g, [[maybe_unused]] int t = 0,
                                               const TimesOf<kTimes>& tw = {}) {
  const int tid = threadIdx.x;
  const int beam = a.beam, K = a.K, K1 = a.K + 1;
  const float lw = a.lm_rows ? a.lm_weight : 0.f;
  for (int v = tid; v < min(a.V, kRowLds); v += 256) s.row[v] = ldx(xr, v);
  __syncthreads();
  auto xv = [&](int v) { return v < kRowLds ? s.row[v] : ldx(xr, v); };
  const int nh = s.nhyp;

  // 1. top-K non-blank tokens of the frame, listed in token-id order
  const int V = a.V, blank = a.blank;
  auto tok_key = [&](int v) -> uint64_t { return v == blank ? 0ull : mk_key(xv(v), v); };
  const uint64_t kth = select_nth(tok_key, V, K, s.sel);
  if (tid == 0) s.ncand = 0;
  __syncthreads();
  for (int v = tid; v < V; v += 256) {
    const uint64_t k = tok_key(v);
    if (k && k >= kth) s.cunsorted[atomicAdd(&s.ncand, 1)] = v;
  }
  __syncthreads();
  if (tid < K) {
    const int v = s.cunsorted[tid];
    int r = 0;
    for (int i = 0; i < K; ++i) r += s.cunsorted[i] < v;
    s.ctok[r] = v;
    s.cx[r] = xv(v);
    if constexpr (BIAS) {
      const CgRoot rt = cg_root(g, v);
      s.rchild[r] = rt.child; s.rboost[r] = rt.boost;
    }
  }
  if (tid < kMaxBeam) s.merged[tid] = 0ull;
  __syncthreads();

  // 2a. stays that absorb an extension: y = y' + c with c a candidate and y' in the beam
  if (tid < nh) {
    const int l = s.last[tid];
    int r = -1;
    if (s.len[tid] > 0)
      for (int i = 0; i < K; ++i) r = s.ctok[i] == l ? i : r;
    int src = -1;
    if (r >= 0)
      for (int j = 0; j < nh; ++j) src = s.node[j] == s.pnode[tid] ? j : src;
    s.lrank[tid] = r;
    s.msrc[tid] = src;
    if (src >= 0) atomicOr(&s.merged[src], 1ull << r);
  }
  __syncthreads();

  // 2b. candidate scores; index i = slot * (K + 1) + (0: stay, 1 + r: extension by the r-th candidate token)
  const float xb = xv(blank);
  auto stay_pnb = [&](int j) {
    const int r = s.lrank[j];
    float pnb = r >= 0 ? s.pnb[j] + s.cx[r] : -INFINITY;
    const int src = s.msrc[j];
    if (src >= 0) pnb = lae(pnb, (s.last[src] == s.last[j] ? s.pb[src] : lae(s.pb[src], s.pnb[src])) + s.cx[r]);
    return pnb;
  };
  auto ext_pnb = [&](int j, int r) { return (s.ctok[r] == s.last[j] ? s.pb[j] : lae(s.pb[j], s.pnb[j])) + s.cx[r]; };
  auto ext_lm = [&](int j, int r) { return a.lm_rows ? s.lm[j] + a.lm_rows[(row0 + j) * a.ld_lm + s.ctok[r]] : 0.f; };
  // kTimes: the same with max; `e` the time node the path comes from, `fresh` = a new node (e, t) is due if this one survives
  struct Vit { float v; int e; bool fresh; };
  [[maybe_unused]] auto ext_vit = [&](int j, int r) -> Vit {
    if constexpr (kTimes) {
      const bool nb = s.ctok[r] != s.last[j] && s.vnb[j] > s.vb[j];
      return {(nb ? s.vnb[j] : s.vb[j]) + s.cx[r], nb ? s.enb[j] : s.eb[j], true};
    } else {
      return {0.f, 0, false};
    }
  };
  [[maybe_unused]] auto stay_vit = [&](int j) -> Vit {
    if constexpr (kTimes) {
      const int r = s.lrank[j];
      Vit o{r >= 0 ? s.vnb[j] + s.cx[r] : -INFINITY, s.enb[j], false};
      const int src = s.msrc[j];
      if (src >= 0) {
        const Vit x = ext_vit(src, r);
        if (x.v > o.v) o = x;
      }
      return o;
    } else {
      return {0.f, 0, false};
    }
  };
  const int N = nh * K1;
  for (int i = tid; i < N; i += 256) {
    const int j = i / K1, q = i - j * K1;
    uint64_t key = 0ull;
    if (q == 0) {
      float sc = lae(lae(s.pb[j], s.pnb[j]) + xb, stay_pnb(j)) + lw * s.lm[j] + a.ins_bonus * (float)s.len[j];
      if constexpr (BIAS) sc += s.b[j];
      key = mk_key(sc, i);
    } else if (!((s.merged[j] >> (q - 1)) & 1ull)) {
      float sc = ext_pnb(j, q - 1) + lw * ext_lm(j, q - 1) + a.ins_bonus * (float)(s.len[j] + 1);
      if constexpr (BIAS) {  // one automaton step per live extension, each on its own lane
        const CgStep st = cg_step(g, s.q[j], s.ctok[q - 1], CgRoot{s.rchild[q - 1], s.rboost[q - 1]});
        const float nb = s.b[j] + st.inc;
        s.cq[i] = st.q; s.cb[i] = nb;
        sc += nb;
      }
      key = mk_key(sc, i);
    }
    s.key[i] = key;
  }
  __syncthreads();

  // 3. the `beam` best candidates
  const uint64_t cth = select_nth([&](int i) { return s.key[i]; }, N, beam, s.sel);
  if (tid == 0) s.nsel = 0;
  __syncthreads();
  for (int i = tid; i < N; i += 256) {
    const uint64_t k = s.key[i];
    if (k && k >= cth) s.sel_idx[atomicAdd(&s.nsel, 1)] = i;
  }
  __syncthreads();
  const int ns = s.nsel;

  // 4. new state (wave 0: lane = one selected candidate, written to slot = its rank)
  float n_pb = 0.f, n_pnb = 0.f, n_lm = 0.f;
  int n_len = 0, n_last = -1, n_node = 0, n_pnode = -1, slot = 0, par = 0, ext = 0, fresh = 0, tslot = -1;
  int n_q = 0;
  float n_b = 0.f;
  [[maybe_unused]] float n_vb = 0.f;
  [[maybe_unused]] int n_eb = 0;
  [[maybe_unused]] Vit n_nb{0.f, 0, false};
  if (tid < ns) {
    const int i = s.sel_idx[tid];
    const uint64_t k = s.key[i];
    for (int m = 0; m < ns; ++m) slot += s.key[s.sel_idx[m]] > k;
    const int j = i / K1, q = i - j * K1;
    par = j;
    if (q == 0) {
      n_pb = lae(s.pb[j], s.pnb[j]) + xb; n_pnb = stay_pnb(j); n_lm = s.lm[j];
      n_len = s.len[j]; n_last = s.last[j]; n_node = s.node[j]; n_pnode = s.pnode[j];
      if constexpr (BIAS) { n_q = s.q[j]; n_b = s.b[j]; }
      if constexpr (kTimes) {
        n_vb = fmaxf(s.vb[j], s.vnb[j]) + xb; n_eb = s.vnb[j] > s.vb[j] ? s.enb[j] : s.eb[j];
        n_nb = stay_vit(j);
      }
    } else {
      ext = 1;
      if constexpr (kTimes) { n_vb = -INFINITY; n_nb = ext_vit(j, q - 1); }
      if constexpr (BIAS) { n_q = s.cq[i]; n_b = s.cb[i]; }
      const int r = q - 1;
      n_pb = -INFINITY; n_pnb = ext_pnb(j, r); n_lm = ext_lm(j, r);
      n_len = s.len[j] + 1; n_last = s.ctok[r]; n_pnode = s.node[j];
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
      const int id = s.nnodes + __popcll(fm & ((1ull << tid) - 1ull));
      n_node = id;
      w.tab_val[tslot] = id;
      if (id < w.cap) { w.node_par[id] = n_pnode; w.node_tok[id] = n_last; }
    }
    if (tid == 0) s.nfresh = __popcll(fm);
    if constexpr (kTimes) {  // fresh time nodes likewise; an extension's blank pointer is its new node too (vb = -inf)
      const unsigned long long tm = __ballot(n_nb.fresh);
      if (n_nb.fresh) {
        const int id = s.ntn + __popcll(tm & ((1ull << tid) - 1ull));
        if (id < tw.cap) { tw.tpar[id] = n_nb.e; tw.tfrm[id] = t; }
        n_nb.e = id;
        if (ext) n_eb = id;
      }
      if (tid == 0) s.ntfresh = __popcll(tm);
    }
  }
  __syncthreads();
  if constexpr (kTimes) {
    if (tid < ns) { s.vb[slot] = n_vb; s.vnb[slot] = n_nb.v; s.eb[slot] = n_eb; s.enb[slot] = n_nb.e; }
    if (tid == 0) s.ntn += s.ntfresh;
  }
  if (tid < ns) {
    s.pb[slot] = n_pb; s.pnb[slot] = n_pnb; s.lm[slot] = n_lm;
    s.len[slot] = n_len; s.last[slot] = n_last; s.node[slot] = n_node; s.pnode[slot] = n_pnode;
    if constexpr (BIAS) { s.q[slot] = n_q; s.b[slot] = n_b; }
    if (a.lm_parent) {
      a.lm_parent[row0 + slot] = (int)(row0 + par);
      a.lm_token[row0 + slot] = ext ? n_last : a.blank;
      a.lm_keep[row0 + slot] = (uint8_t)!ext;
    }
  } else if (a.lm_parent && tid < beam) {  // empty slot: any valid row
    a.lm_parent[row0 + tid] = (int)row0; a.lm_token[row0 + tid] = a.blank; a.lm_keep[row0 + tid] = 1;
  }
  if (tid == 0) { s.nhyp = ns; s.nnodes += s.nfresh; }
  __threadfence();  // this frame's table entries, before the next frame's L2 reads
  __syncthreads();
}

// the offline search: one workgroup per utterance of the batch, frames [t0, t1)
template <bool kTimes, class A>
__device__ __forceinline__ void* times_arg(const A& a) {  // the times workspace of a kernel's arguments
  if constexpr (kTimes) return a.tws; else return nullptr;
}

template <typename TX, bool BIAS, bool kTimes = false>
__global__ __launch_bounds__(256) void ctc_beam_step_kernel(
    const std::conditional_t<kTimes, TimesStepArgs, std::conditional_t<BIAS, BiasStepArgs, StepArgs>> a) {
  __shared__ FrameLds<BIAS, kTimes> s;
  const int b = blockIdx.x;
  const int beam = a.p.beam;
  const BeamWs w = beam_ws(a.ws, b, a.T, beam);
  const BiasWs bw = BIAS ? bias_ws(a.ws, gridDim.x, b, a.T, beam) : BiasWs{nullptr, nullptr};
  const TimesOf<kTimes> tw = times_of<kTimes>(times_arg<kTimes>(a), b, a.T, beam);
  const int L = min(a.in_len[b], a.T);
  const long row0 = (long)b * beam;

  if (a.t0 == 0) {
    ctc_beam_init<kTimes>(w, BIAS ? &bw : nullptr, tw);
    __threadfence_block();
    __syncthreads();
  }
  ctc_beam_load<BIAS, kTimes>(s, w, bw, beam, tw);
  __syncthreads();
  for (int t = a.t0; t < a.t1; ++t) {
    if (t >= L) {  // past the end of this utterance: the beam stands still
      ctc_beam_identity(a.p, row0);
      continue;
    }
    ctc_beam_frame<TX, BIAS, kTimes>(s, a.p, w, (const TX*)a.x + ((long)b * a.T + t) * a.ld, row0, graph_of<BIAS>(a), t, tw);
  }
  ctc_beam_store<BIAS, kTimes>(s, w, bw, beam, tw);
}

// final score = s(y) + lm_weight * log P_lm(eos | y) [+ b - phi(q)]; the nbest best, sorted, backtracked into token rows of max_u
// entries (longer hypotheses are cut there).  64 threads; lm_rows: the rows of this beam; nh: its hypotheses
// kTimes: also times [nbest][max_u] (the start frame of every token on the best path, -1 after the hypothesis) and vscores
template <bool BIAS, bool kTimes = false>
__device__ __forceinline__ void ctc_beam_finish(float* s_fin, const BeamWs& w, const BiasWs& bw, int nh, const float* lm_rows,
                                                long ld_lm, float lm_weight, float ins_bonus, int eos, int nbest, int pad, int max_u,
                                                int* tokens, int* lengths, float* scores, int* nhyp, const GraphOf<BIAS>& g,
                                                const TimesOf<kTimes>& tw = {}, [[maybe_unused]] int* times = nullptr,
                                                [[maybe_unused]] float* vscores = nullptr) {
  const int j = threadIdx.x;
  if (j < nh) {
    float s = lae(w.pb[j], w.pnb[j]) + ins_bonus * (float)w.len[j];
    if (lm_rows) s += lm_weight * (w.lm[j] + lm_rows[j * ld_lm + eos]);
    if constexpr (BIAS) s += bw.b[j] - cg_phi(g, bw.q[j]);
    s_fin[j] = s;
  }
  __syncthreads();
  if (j == 0) *nhyp = min(nh, nbest);
  if (j < nh) {
    const float s = s_fin[j];
    int rank = 0;
    for (int m = 0; m < nh; ++m) rank += s_fin[m] > s || (s_fin[m] == s && m < j);
    if (rank < nbest) {
      int* out = tokens + (long)rank * max_u;
      const int n = w.len[j];
      for (int u = n; u < max_u; ++u) out[u] = pad;
      int node = w.node[j];
      for (int u = n - 1; u >= 0 && node > 0 && node < w.cap; --u) {
        if (u < max_u) out[u] = w.node_tok[node];
        node = w.node_par[node];
      }
      lengths[rank] = min(n, max_u);
      scores[rank] = s;
      if constexpr (kTimes) {
        int* tout = times + (long)rank * max_u;
        for (int u = 0; u < max_u; ++u) tout[u] = -1;
        const float vb = tw.vb[j], vnb = tw.vnb[j];
        int e = vnb > vb ? tw.enb[j] : tw.eb[j];
        for (int u = n - 1; u >= 0 && e > 0 && e < tw.cap; --u) {
          if (u < max_u) tout[u] = tw.tfrm[e];
          e = tw.tpar[e];
        }
        vscores[rank] = fmaxf(vb, vnb);
      }
    }
  }
  for (int r = nh + j; r < nbest; r += 64) {
    int* out = tokens + (long)r * max_u;
    for (int u = 0; u < max_u; ++u) out[u] = pad;
    lengths[r] = 0;
    scores[r] = -INFINITY;
    if constexpr (kTimes) {
      for (int u = 0; u < max_u; ++u) times[(long)r * max_u + u] = -1;
      vscores[r] = -INFINITY;
    }
  }
}

template <bool BIAS>
__global__ __launch_bounds__(64) void ctc_beam_finish_kernel(void* ws, const float* lm_rows, long ld_lm, float lm_weight,
                                                             float ins_bonus, int eos, int T, int beam, int nbest, int pad,
                                                             int* tokens, int* lengths, float* scores, int* nhyp,
                                                             const GraphOf<BIAS> g) {
  __shared__ float s_fin[kMaxBeam];
  const int b = blockIdx.x;
  const BeamWs w = beam_ws(ws, b, T, beam);
  const BiasWs bw = BIAS ? bias_ws(ws, gridDim.x, b, T, beam) : BiasWs{nullptr, nullptr};
  ctc_beam_finish<BIAS>(s_fin, w, bw, w.cnt[0], lm_rows ? lm_rows + (long)b * beam * ld_lm : nullptr, ld_lm, lm_weight, ins_bonus, eos,
                        nbest, pad, T, tokens + (long)b * nbest * T, lengths + b * nbest, scores + b * nbest, nhyp + b, g);
}

struct TimesFinishArgs {
  void *ws, *tws;
  const float* lm_rows; long ld_lm;
  float lm_weight, ins_bonus;
  int eos, T, beam, nbest, pad;
  int *tokens, *lengths; float* scores; int* nhyp;
  int* times; float* vscores;
  CgTables g;
};
template <bool BIAS>
__global__ __launch_bounds__(64) void ctc_beam_times_finish_kernel(const TimesFinishArgs a) {
  __shared__ float s_fin[kMaxBeam];
  const int b = blockIdx.x, T = a.T, beam = a.beam, nbest = a.nbest;
  const BeamWs w = beam_ws(a.ws, b, T, beam);
  const BiasWs bw = BIAS ? bias_ws(a.ws, gridDim.x, b, T, beam) : BiasWs{nullptr, nullptr};
  ctc_beam_finish<BIAS, true>(s_fin, w, bw, w.cnt[0], a.lm_rows ? a.lm_rows + (long)b * beam * a.ld_lm : nullptr, a.ld_lm, a.lm_weight,
                              a.ins_bonus, a.eos, nbest, a.pad, T, a.tokens + (long)b * nbest * T, a.lengths + b * nbest,
                              a.scores + b * nbest, a.nhyp + b, graph_of<BIAS>(a), times_ws(a.tws, b, T, beam),
                              a.times + (long)b * nbest * T, a.vscores + b * nbest);
}

// ------------------------------------------------------------------------------------------------ the streamed search
// State of one stream slot, int32 words: [0] frames consumed, [1] 0, then the offline workspace of one utterance of max_frames
// frames, then (q, b) per beam slot, which every slot has room for whether the search is biased or not.
__host__ __device__ __forceinline__ long ctc_state_words(int max_frames, int beam) {
  return 2 + beam_ws_words(max_frames, beam) + 2L * beam;
}

struct CtcSlot {
  int* head;
  BeamWs w;
  BiasWs bw;
};
__device__ __forceinline__ CtcSlot ctc_slot(void* state, int slot, int max_frames, int beam) {
  CtcSlot q;
  q.head = (int*)state + (long)slot * ctc_state_words(max_frames, beam);
  q.w = beam_ws(q.head + 2, 0, max_frames, beam);
  q.bw = bias_ws_at(q.head + 2 + beam_ws_words(max_frames, beam), beam);
  return q;
}

// (tstate: the times slots, one void* with kTimes and nothing without: the kernel without times keeps its parameter list)
template <bool kTimes = false, class... TS>
__global__ __launch_bounds__(256) void ctc_beam_stream_reset_kernel(void* state, const int* slots, int max_streams, int max_frames,
                                                                    int beam, TS... tstate) {
  static_assert(sizeof...(TS) == (kTimes ? 1 : 0));
  const int slot = slots[blockIdx.x];
  if (slot < 0 || slot >= max_streams) return;
  const CtcSlot q = ctc_slot(state, slot, max_frames, beam);
  if constexpr (kTimes) ctc_beam_init<true>(q.w, &q.bw, times_ws(tstate..., slot, max_frames, beam));
  else ctc_beam_init(q.w, &q.bw);
  if (threadIdx.x == 0) { q.head[0] = 0; q.head[1] = 0; }
}

struct StreamStepArgs {
  const void* x; long ld, total_rows;
  const int *slot_idx, *n_new, *row_off;
  void* state;
  FrameParams p;
  int max_streams, max_frames, j0, j1;
};
struct BiasStreamStepArgs : StreamStepArgs { CgTables g; };
struct TimesStreamStepArgs : BiasStreamStepArgs { void* tws; };

// One workgroup per listed stream: the frames [j0, min(j1, n_new)) of its piece over its slot's state.  An entry without such a
// frame, one with out-of-range values and one whose piece would pass max_frames leave the slot untouched (identity triple).
// The slot's counter stands at its value before the piece plus j0 (the LM path steps through the piece one launch per frame),
// so the whole piece fits iff counter - j0 + n_new <= max_frames; that also bounds the frames of this launch, hence the nodes.
// kTimes: the times slot goes with the slot (untouched where the slot is); frame numbers count from the stream's first frame.
template <typename TX, bool BIAS, bool kTimes = false>
__global__ __launch_bounds__(256) void ctc_beam_stream_step_kernel(
    const std::conditional_t<kTimes, TimesStreamStepArgs, std::conditional_t<BIAS, BiasStreamStepArgs, StreamStepArgs>> a) {
  __shared__ FrameLds<BIAS, kTimes> s;
  const int b = blockIdx.x;
  const int beam = a.p.beam;
  const long row0 = (long)b * beam;
  const int slot = a.slot_idx[b], n = a.n_new[b];
  const long r0 = a.row_off[b];
  const int j1 = min(a.j1, n);
  bool due = slot >= 0 && slot < a.max_streams && a.j0 < j1 && r0 >= 0 && r0 + n <= a.total_rows;
  const CtcSlot q = ctc_slot(a.state, due ? slot : 0, a.max_frames, beam);
  const int frames = due ? q.head[0] : -1;
  due = due && frames >= a.j0 && (long)frames - a.j0 + n <= a.max_frames;
  if (!due) {
    ctc_beam_identity(a.p, row0);
    return;
  }
  const TimesOf<kTimes> tw = times_of<kTimes>(times_arg<kTimes>(a), slot, a.max_frames, beam);
  ctc_beam_load<BIAS, kTimes>(s, q.w, q.bw, beam, tw);
  __syncthreads();
  for (int j = a.j0; j < j1; ++j)
    ctc_beam_frame<TX, BIAS, kTimes>(s, a.p, q.w, (const TX*)a.x + (r0 + j) * a.ld, row0, graph_of<BIAS>(a), frames + (j - a.j0), tw);
  ctc_beam_store<BIAS, kTimes>(s, q.w, q.bw, beam, tw);
  if (threadIdx.x == 0) q.head[0] = frames + (j1 - a.j0);
}

struct StreamReadArgs {
  const void* state; const int* slots;
  const float* lm_rows; long ld_lm;
  float lm_weight, ins_bonus;
  int eos, biased, max_streams, max_frames, beam, nbest, pad, max_u;
  int *tokens, *lengths; float* scores; int* aux;  // aux: nhyp (finish) / stable_len (partial)
};
struct BiasStreamReadArgs : StreamReadArgs { CgTables g; };
struct TimesStreamReadArgs : BiasStreamReadArgs { const void* tws; int* times; float* vscores; };

// readout of the given slots, as the offline kernel finishes; the state is read only
template <bool BIAS>
__global__ __launch_bounds__(64) void ctc_beam_stream_finish_kernel(const std::conditional_t<BIAS, BiasStreamReadArgs, StreamReadArgs> a) {
  __shared__ float s_fin[kMaxBeam];
  const int b = blockIdx.x, slot = a.slots[b];
  const bool valid = slot >= 0 && slot < a.max_streams;  // no such slot: no hypothesis
  const CtcSlot q = ctc_slot((void*)a.state, valid ? slot : 0, a.max_frames, a.beam);
  ctc_beam_finish<BIAS>(s_fin, q.w, q.bw, valid ? min(max(q.w.cnt[0], 0), a.beam) : 0,
                        a.lm_rows ? a.lm_rows + (long)b * a.beam * a.ld_lm : nullptr, a.ld_lm, a.lm_weight, a.ins_bonus, a.eos, a.nbest,
                        a.pad, a.max_u, a.tokens + (long)b * a.nbest * a.max_u, a.lengths + b * a.nbest, a.scores + b * a.nbest,
                        a.aux + b, graph_of<BIAS>(a));
}
template <bool BIAS>
__global__ __launch_bounds__(64) void ctc_beam_stream_times_finish_kernel(const TimesStreamReadArgs a) {
  __shared__ float s_fin[kMaxBeam];
  const int b = blockIdx.x, slot = a.slots[b];
  const bool valid = slot >= 0 && slot < a.max_streams;
  const CtcSlot q = ctc_slot((void*)a.state, valid ? slot : 0, a.max_frames, a.beam);
  ctc_beam_finish<BIAS, true>(s_fin, q.w, q.bw, valid ? min(max(q.w.cnt[0], 0), a.beam) : 0,
                              a.lm_rows ? a.lm_rows + (long)b * a.beam * a.ld_lm : nullptr, a.ld_lm, a.lm_weight, a.ins_bonus, a.eos,
                              a.nbest, a.pad, a.max_u, a.tokens + (long)b * a.nbest * a.max_u, a.lengths + b * a.nbest,
                              a.scores + b * a.nbest, a.aux + b, graph_of<BIAS>(a),
                              times_ws((void*)a.tws, valid ? slot : 0, a.max_frames, a.beam),
                              a.times + (long)b * a.nbest * a.max_u, a.vscores + b * a.nbest);
}

// The live hypothesis with the best in-beam score log(pb + pnb) + lm_weight * lm + ins_bonus * len (+ b when biased; ties: the
// lower slot) and the length of the longest common prefix of the live hypotheses with a finite score (of all of them when none
// is finite): the depth of their lowest common ancestor in node_par.  Nodes are numbered in creation order, so a parent's id is
// below its child's: lifting the highest node until all are equal ends at that ancestor.  One wave per slot; the state is read
// only.
__global__ __launch_bounds__(64) void ctc_beam_stream_partial_kernel(const StreamReadArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, slot = a.slots[b];
  int* out = a.tokens + (long)b * a.max_u;
  const bool valid = slot >= 0 && slot < a.max_streams;
  const CtcSlot q = ctc_slot((void*)a.state, valid ? slot : 0, a.max_frames, a.beam);
  const int nh = valid ? min(max(q.w.cnt[0], 0), a.beam) : 0;
  float sc = -INFINITY;
  int len = 0, node = 0;
  if (lane < nh) {
    len = q.w.len[lane];
    node = q.w.node[lane];
    sc = lae(q.w.pb[lane], q.w.pnb[lane]) + a.lm_weight * q.w.lm[lane] + a.ins_bonus * (float)len;
    if (a.biased) sc += q.bw.b[lane];
  }
  const bool finite = lane < nh && sc != -INFINITY && sc == sc;
  const unsigned long long fin_mask = __ballot(finite);
  const bool in_set = fin_mask ? finite : lane < nh;
  // best: the highest score, then the lower slot (a nan score ranks below everything)
  const uint64_t key = lane < nh ? mk_key(sc == sc ? sc : -INFINITY, lane) : 0ull;
  uint64_t best = key;
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  const bool is_best = nh > 0 && key == best;
  if (is_best) {
    const int n = min(len, a.max_u);
    for (int u = n; u < a.max_u; ++u) out[u] = a.pad;
    int nd = node;
    for (int u = len - 1; u >= 0 && nd > 0 && nd < q.w.cap; --u) {
      if (u < a.max_u) out[u] = q.w.node_tok[nd];
      nd = q.w.node_par[nd];
    }
    a.lengths[b] = n;
    a.scores[b] = sc;
  }
  int depth = len, cur = in_set ? node : -1;
  for (int it = 0; it < q.w.cap; ++it) {  // every pass lowers the highest node: fewer than `cap` passes
    int hi = cur;
    for (int o = 32; o > 0; o >>= 1) hi = max(hi, __shfl_xor(hi, o, 64));
    if (hi <= 0 || !__ballot(in_set && cur != hi)) break;  // the root, or every member at the same node
    if (in_set && cur == hi) { cur = cur < q.w.cap ? q.w.node_par[cur] : 0; --depth; }
  }
  if (is_best) a.aux[b] = depth;  // the best hypothesis is a member (or none is finite): its depth is the ancestor's
  if (nh == 0 && lane == 0) {
    for (int u = 0; u < a.max_u; ++u) out[u] = a.pad;
    a.lengths[b] = 0; a.scores[b] = -INFINITY; a.aux[b] = 0;
  }
}

struct StreamEndpointArgs {
  const void *state, *tws; const int* slots;
  float lm_weight, ins_bonus;
  int biased, max_streams, max_frames, beam, silence_frames, empty_frames, segment_frames;
  int* out;
};

// The endpoint probe: per listed slot out[b] = (rule, F, L, E) for F = the slot's frame counter and the live hypothesis the partial
// kernel above reports (the same score, tie rule and handling of non-finite scores, restated here so that the partial kernel's code
// stays what it is): L = its length, E = the frame of its last token on its best path, which is what the times finish writes as
// times[L - 1] for it (the pointer of the larger of (vb, eb), (vnb, enb); tie: eb), -1 when L == 0.  A slot without frames or
// without a hypothesis has the empty hypothesis; a slot out of range writes (0, 0, 0, -1).  One wave per slot, no LDS; the state
// and the times state are read only.
__global__ __launch_bounds__(64) void ctc_beam_stream_endpoint_kernel(const StreamEndpointArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, slot = a.slots[b];
  int* out = a.out + 4L * b;
  if (slot < 0 || slot >= a.max_streams) {
    if (lane == 0) { out[0] = 0; out[1] = 0; out[2] = 0; out[3] = -1; }
    return;
  }
  const CtcSlot q = ctc_slot((void*)a.state, slot, a.max_frames, a.beam);
  const TimesWs tw = times_ws((void*)a.tws, slot, a.max_frames, a.beam);
  const int F = max(q.head[0], 0);
  const int nh = F > 0 ? min(max(q.w.cnt[0], 0), a.beam) : 0;
  float sc = -INFINITY;
  int len = 0;
  if (lane < nh) {
    len = q.w.len[lane];
    sc = lae(q.w.pb[lane], q.w.pnb[lane]) + a.lm_weight * q.w.lm[lane] + a.ins_bonus * (float)len;
    if (a.biased) sc += q.bw.b[lane];
  }
  const uint64_t key = lane < nh ? mk_key(sc == sc ? sc : -INFINITY, lane) : 0ull;
  uint64_t best = key;
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if (nh > 0 ? key == best : lane == 0) {
    const int L = nh > 0 ? max(len, 0) : 0;
    int E = -1;
    if (L > 0) {
      const int e = tw.vnb[lane] > tw.vb[lane] ? tw.enb[lane] : tw.eb[lane];
      if (e > 0 && e < tw.cap) E = tw.tfrm[e];
    }
    out[0] = endpoint_rule(F, L, E, a.silence_frames, a.empty_frames, a.segment_frames);
    out[1] = F; out[2] = L; out[3] = E;
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

static int frame_args_ok(long ld, const float* lm_rows, long ld_lm, const int* lm_parent, const int* lm_token, const void* lm_keep,
                         int V, int beam, int K, int blank) {
  return !(V < 2 || V > 65535 || ld < V || beam < 1 || beam > kMaxBeam || K < 1 || K > kMaxK || K > V - 1 || blank < 0 || blank >= V ||
           (lm_rows && (ld_lm < V || !lm_parent || !lm_token || !lm_keep)));
}
static int step_args_ok(long ld, const float* lm_rows, long ld_lm, const int* lm_parent, const int* lm_token, const void* lm_keep,
                        int T, int V, int beam, int K, int blank, int t0, int t1) {
  return frame_args_ok(ld, lm_rows, ld_lm, lm_parent, lm_token, lm_keep, V, beam, K, blank) && !(T < 0 || t0 < 0 || t1 < t0 || t1 > T);
}

static FrameParams frame_params(const float* lm_rows, long ld_lm, int* lm_parent, int* lm_token, void* lm_keep, int V, int beam, int K,
                                int blank, float lm_weight, float ins_bonus) {
  FrameParams p;
  p.lm_rows = lm_rows; p.ld_lm = ld_lm;
  p.lm_parent = lm_parent; p.lm_token = lm_token; p.lm_keep = (uint8_t*)lm_keep;
  p.V = V; p.beam = beam; p.K = K; p.blank = blank;
  p.lm_weight = lm_weight; p.ins_bonus = ins_bonus;
  return p;
}

static void fill_step_args(StepArgs& a, const void* x, long ld, const int* in_len, void* workspace, const float* lm_rows, long ld_lm,
                           int* lm_parent, int* lm_token, void* lm_keep, int T, int V, int beam, int K, int blank, float lm_weight,
                           float ins_bonus, int t0, int t1) {
  a.x = x; a.ld = ld; a.in_len = in_len; a.ws = workspace;
  a.p = frame_params(lm_rows, ld_lm, lm_parent, lm_token, lm_keep, V, beam, K, blank, lm_weight, ins_bonus);
  a.T = T; a.t0 = t0; a.t1 = t1;
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

// ------------------------------------------------------------------------------------------------ C ABI: the streamed search
extern "C" long ea_ctc_prefix_beam_stream_state_bytes(int max_frames, int beam) {
  if (max_frames < 1 || beam < 1 || beam > kMaxBeam) return 0;
  return ctc_state_words(max_frames, beam) * 4L;
}

extern "C" int ea_ctc_prefix_beam_stream_reset(void* state, const int* slots, int n, int max_streams, int max_frames, int beam,
                                               hipStream_t stream) {
  if (n <= 0) return 0;
  if (!state || !slots || max_streams < 1 || max_frames < 1 || beam < 1 || beam > kMaxBeam) return -2;
  hipLaunchKernelGGL(ctc_beam_stream_reset_kernel, dim3(n), dim3(256), 0, stream, state, slots, max_streams, max_frames, beam);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_prefix_beam_stream_step(const void* x, long ld, int x_bf16, long total_rows, const int* slot_idx,
                                              const int* n_new, const int* row_off, int j0, int j1, int n, void* state,
                                              const float* lm_rows, long ld_lm, int* lm_parent, int* lm_token, void* lm_keep,
                                              const int* cg_nodes, const int* cg_edges, const int* cg_root, int cg_n_nodes,
                                              int cg_n_edges, int max_streams, int max_frames, int V, int beam, int K, int blank,
                                              float lm_weight, float ins_bonus, hipStream_t stream) {
  if (n <= 0) return 0;
  BiasStreamStepArgs a;
  if (!x || !slot_idx || !n_new || !row_off || !state || total_rows < 0 || j0 < 0 || j1 < j0 || (lm_rows && j1 != j0 + 1) ||
      max_streams < 1 || max_frames < 1 || !frame_args_ok(ld, lm_rows, ld_lm, lm_parent, lm_token, lm_keep, V, beam, K, blank) ||
      (cg_nodes && !cg_tables(a.g, cg_nodes, cg_edges, cg_root, cg_n_nodes, cg_n_edges, V)))
    return -2;
  a.x = x; a.ld = ld; a.total_rows = total_rows;
  a.slot_idx = slot_idx; a.n_new = n_new; a.row_off = row_off;
  a.state = state;
  a.p = frame_params(lm_rows, ld_lm, lm_parent, lm_token, lm_keep, V, beam, K, blank, lm_weight, ins_bonus);
  a.max_streams = max_streams; a.max_frames = max_frames; a.j0 = j0; a.j1 = j1;
  const StreamStepArgs& u = a;
  if (cg_nodes) {
    if (x_bf16)
      hipLaunchKernelGGL((ctc_beam_stream_step_kernel<bf16_t, true>), dim3(n), dim3(256), 0, stream, a);
    else
      hipLaunchKernelGGL((ctc_beam_stream_step_kernel<float, true>), dim3(n), dim3(256), 0, stream, a);
  } else {
    if (x_bf16)
      hipLaunchKernelGGL((ctc_beam_stream_step_kernel<bf16_t, false>), dim3(n), dim3(256), 0, stream, u);
    else
      hipLaunchKernelGGL((ctc_beam_stream_step_kernel<float, false>), dim3(n), dim3(256), 0, stream, u);
  }
  return EA_CHECK_LAUNCH();
}

static bool stream_read_args_bad(const void* state, const int* slots, int max_streams, int max_frames, int beam, int max_u,
                                 const int* tokens, const int* lengths, const float* scores, const int* aux) {
  return !state || !slots || !tokens || !lengths || !scores || !aux || max_streams < 1 || max_frames < 1 || beam < 1 ||
         beam > kMaxBeam || max_u < 0;
}

static void stream_read_args(StreamReadArgs& a, const void* state, const int* slots, const float* lm_rows, long ld_lm, float lm_weight,
                             float ins_bonus, int eos, int biased, int max_streams, int max_frames, int beam, int nbest, int pad,
                             int max_u, int* tokens, int* lengths, float* scores, int* aux) {
  a.state = state; a.slots = slots;
  a.lm_rows = lm_rows; a.ld_lm = ld_lm;
  a.lm_weight = lm_weight; a.ins_bonus = ins_bonus;
  a.eos = eos; a.biased = biased; a.max_streams = max_streams; a.max_frames = max_frames; a.beam = beam; a.nbest = nbest; a.pad = pad;
  a.max_u = max_u;
  a.tokens = tokens; a.lengths = lengths; a.scores = scores; a.aux = aux;
}

extern "C" int ea_ctc_prefix_beam_stream_finish(const void* state, const int* slots, int n, const float* lm_rows, long ld_lm,
                                                float lm_weight, float ins_bonus, int eos, const int* cg_nodes, int cg_n_nodes,
                                                int max_streams, int max_frames, int beam, int nbest, int pad, int max_u, int* tokens,
                                                int* lengths, float* scores, int* nhyp, hipStream_t stream) {
  if (n <= 0) return 0;
  if (stream_read_args_bad(state, slots, max_streams, max_frames, beam, max_u, tokens, lengths, scores, nhyp) || nbest < 1 ||
      nbest > beam || (lm_rows && (eos < 0 || ld_lm <= eos)) || (cg_nodes && cg_n_nodes < 1))
    return -2;
  BiasStreamReadArgs a;
  stream_read_args(a, state, slots, lm_rows, ld_lm, lm_weight, ins_bonus, eos, cg_nodes != nullptr, max_streams, max_frames, beam,
                   nbest, pad, max_u, tokens, lengths, scores, nhyp);
  if (cg_nodes) {
    a.g = cg_nodes_only(cg_nodes, cg_n_nodes);
    hipLaunchKernelGGL(ctc_beam_stream_finish_kernel<true>, dim3(n), dim3(64), 0, stream, a);
  } else {
    const StreamReadArgs& u = a;
    hipLaunchKernelGGL(ctc_beam_stream_finish_kernel<false>, dim3(n), dim3(64), 0, stream, u);
  }
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_prefix_beam_stream_partial(const void* state, const int* slots, int n, float lm_weight, float ins_bonus,
                                                 int biased, int max_streams, int max_frames, int beam, int pad, int max_u,
                                                 int* tokens, int* lengths, float* scores, int* stable_len, hipStream_t stream) {
  if (n <= 0) return 0;
  if (stream_read_args_bad(state, slots, max_streams, max_frames, beam, max_u, tokens, lengths, scores, stable_len)) return -2;
  StreamReadArgs a;
  stream_read_args(a, state, slots, nullptr, 0, lm_weight, ins_bonus, -1, biased != 0, max_streams, max_frames, beam, 1, pad, max_u,
                   tokens, lengths, scores, stable_len);
  hipLaunchKernelGGL(ctc_beam_stream_partial_kernel, dim3(n), dim3(64), 0, stream, a);
  return EA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------ C ABI: time stamps
extern "C" long ea_ctc_prefix_beam_times_workspace_bytes(int B, int T, int beam) {
  if (B <= 0 || T < 0 || beam < 1 || beam > kMaxBeam) return 0;
  return (long)B * times_ws_words(T, beam) * 4L;
}

extern "C" int ea_ctc_prefix_beam_times_step(const void* x, long ld, int x_bf16, const int* in_len, void* workspace,
                                             void* times_workspace, const float* lm_rows, long ld_lm, int* lm_parent, int* lm_token,
                                             void* lm_keep, const int* cg_nodes, const int* cg_edges, const int* cg_root,
                                             int cg_n_nodes, int cg_n_edges, int B, int T, int V, int beam, int K, int blank,
                                             float lm_weight, float ins_bonus, int t0, int t1, hipStream_t stream) {
  if (B <= 0) return 0;
  TimesStepArgs a;
  if (!x || !in_len || !workspace || !times_workspace ||
      !step_args_ok(ld, lm_rows, ld_lm, lm_parent, lm_token, lm_keep, T, V, beam, K, blank, t0, t1) ||
      (cg_nodes && !cg_tables(a.g, cg_nodes, cg_edges, cg_root, cg_n_nodes, cg_n_edges, V)))
    return -2;
  fill_step_args(a, x, ld, in_len, workspace, lm_rows, ld_lm, lm_parent, lm_token, lm_keep, T, V, beam, K, blank, lm_weight,
                 ins_bonus, t0, t1);
  a.tws = times_workspace;
  if (cg_nodes) {
    if (x_bf16)
      hipLaunchKernelGGL((ctc_beam_step_kernel<bf16_t, true, true>), dim3(B), dim3(256), 0, stream, a);
    else
      hipLaunchKernelGGL((ctc_beam_step_kernel<float, true, true>), dim3(B), dim3(256), 0, stream, a);
  } else {
    if (x_bf16)
      hipLaunchKernelGGL((ctc_beam_step_kernel<bf16_t, false, true>), dim3(B), dim3(256), 0, stream, a);
    else
      hipLaunchKernelGGL((ctc_beam_step_kernel<float, false, true>), dim3(B), dim3(256), 0, stream, a);
  }
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_prefix_beam_times_finish(void* workspace, const void* times_workspace, const float* lm_rows, long ld_lm,
                                               float lm_weight, float ins_bonus, int eos, const int* cg_nodes, int cg_n_nodes, int B,
                                               int T, int beam, int nbest, int pad, int* tokens, int* lengths, float* scores,
                                               int* nhyp, int* times, float* vscores, hipStream_t stream) {
  if (B <= 0) return 0;
  if (!workspace || !times_workspace || !tokens || !lengths || !scores || !nhyp || !times || !vscores || T < 0 || beam < 1 ||
      beam > kMaxBeam || nbest < 1 || nbest > beam || (lm_rows && eos < 0) || (cg_nodes && cg_n_nodes < 1))
    return -2;
  TimesFinishArgs a;
  a.ws = workspace; a.tws = (void*)times_workspace;
  a.lm_rows = lm_rows; a.ld_lm = ld_lm; a.lm_weight = lm_weight; a.ins_bonus = ins_bonus;
  a.eos = eos; a.T = T; a.beam = beam; a.nbest = nbest; a.pad = pad;
  a.tokens = tokens; a.lengths = lengths; a.scores = scores; a.nhyp = nhyp; a.times = times; a.vscores = vscores;
  if (cg_nodes) {
    a.g = cg_nodes_only(cg_nodes, cg_n_nodes);
    hipLaunchKernelGGL(ctc_beam_times_finish_kernel<true>, dim3(B), dim3(64), 0, stream, a);
  } else {
    a.g = CgTables{};
    hipLaunchKernelGGL(ctc_beam_times_finish_kernel<false>, dim3(B), dim3(64), 0, stream, a);
  }
  return EA_CHECK_LAUNCH();
}

extern "C" long ea_ctc_prefix_beam_stream_times_state_bytes(int max_frames, int beam) {
  if (max_frames < 1 || beam < 1 || beam > kMaxBeam) return 0;
  return times_ws_words(max_frames, beam) * 4L;
}

extern "C" int ea_ctc_prefix_beam_stream_times_reset(void* state, void* times_state, const int* slots, int n, int max_streams,
                                                     int max_frames, int beam, hipStream_t stream) {
  if (n <= 0) return 0;
  if (!state || !times_state || !slots || max_streams < 1 || max_frames < 1 || beam < 1 || beam > kMaxBeam) return -2;
  hipLaunchKernelGGL((ctc_beam_stream_reset_kernel<true, void*>), dim3(n), dim3(256), 0, stream, state, slots, max_streams, max_frames,
                     beam, times_state);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_prefix_beam_stream_times_step(const void* x, long ld, int x_bf16, long total_rows, const int* slot_idx,
                                                    const int* n_new, const int* row_off, int j0, int j1, int n, void* state,
                                                    void* times_state, const float* lm_rows, long ld_lm, int* lm_parent,
                                                    int* lm_token, void* lm_keep, const int* cg_nodes, const int* cg_edges,
                                                    const int* cg_root, int cg_n_nodes, int cg_n_edges, int max_streams,
                                                    int max_frames, int V, int beam, int K, int blank, float lm_weight,
                                                    float ins_bonus, hipStream_t stream) {
  if (n <= 0) return 0;
  TimesStreamStepArgs a;
  if (!x || !slot_idx || !n_new || !row_off || !state || !times_state || total_rows < 0 || j0 < 0 || j1 < j0 ||
      (lm_rows && j1 != j0 + 1) || max_streams < 1 || max_frames < 1 ||
      !frame_args_ok(ld, lm_rows, ld_lm, lm_parent, lm_token, lm_keep, V, beam, K, blank) ||
      (cg_nodes && !cg_tables(a.g, cg_nodes, cg_edges, cg_root, cg_n_nodes, cg_n_edges, V)))
    return -2;
  a.x = x; a.ld = ld; a.total_rows = total_rows;
  a.slot_idx = slot_idx; a.n_new = n_new; a.row_off = row_off;
  a.state = state; a.tws = times_state;
  a.p = frame_params(lm_rows, ld_lm, lm_parent, lm_token, lm_keep, V, beam, K, blank, lm_weight, ins_bonus);
  a.max_streams = max_streams; a.max_frames = max_frames; a.j0 = j0; a.j1 = j1;
  if (cg_nodes) {
    if (x_bf16)
      hipLaunchKernelGGL((ctc_beam_stream_step_kernel<bf16_t, true, true>), dim3(n), dim3(256), 0, stream, a);
    else
      hipLaunchKernelGGL((ctc_beam_stream_step_kernel<float, true, true>), dim3(n), dim3(256), 0, stream, a);
  } else {
    if (x_bf16)
      hipLaunchKernelGGL((ctc_beam_stream_step_kernel<bf16_t, false, true>), dim3(n), dim3(256), 0, stream, a);
    else
      hipLaunchKernelGGL((ctc_beam_stream_step_kernel<float, false, true>), dim3(n), dim3(256), 0, stream, a);
  }
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_prefix_beam_stream_times_finish(const void* state, const void* times_state, const int* slots, int n,
                                                      const float* lm_rows, long ld_lm, float lm_weight, float ins_bonus, int eos,
                                                      const int* cg_nodes, int cg_n_nodes, int max_streams, int max_frames, int beam,
                                                      int nbest, int pad, int max_u, int* tokens, int* lengths, float* scores,
                                                      int* nhyp, int* times, float* vscores, hipStream_t stream) {
  if (n <= 0) return 0;
  if (stream_read_args_bad(state, slots, max_streams, max_frames, beam, max_u, tokens, lengths, scores, nhyp) || !times_state ||
      !times || !vscores || nbest < 1 || nbest > beam || (lm_rows && (eos < 0 || ld_lm <= eos)) || (cg_nodes && cg_n_nodes < 1))
    return -2;
  TimesStreamReadArgs a;
  stream_read_args(a, state, slots, lm_rows, ld_lm, lm_weight, ins_bonus, eos, cg_nodes != nullptr, max_streams, max_frames, beam,
                   nbest, pad, max_u, tokens, lengths, scores, nhyp);
  a.tws = times_state; a.times = times; a.vscores = vscores;
  if (cg_nodes) {
    a.g = cg_nodes_only(cg_nodes, cg_n_nodes);
    hipLaunchKernelGGL(ctc_beam_stream_times_finish_kernel<true>, dim3(n), dim3(64), 0, stream, a);
  } else {
    a.g = CgTables{};
    hipLaunchKernelGGL(ctc_beam_stream_times_finish_kernel<false>, dim3(n), dim3(64), 0, stream, a);
  }
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_prefix_beam_stream_endpoint(const void* state, const void* times_state, const int* slots, int n,
                                                  float lm_weight, float ins_bonus, int biased, int max_streams, int max_frames,
                                                  int beam, int silence_frames, int empty_frames, int segment_frames, int* out,
                                                  hipStream_t stream) {
  if (n <= 0) return 0;
  if (!state || !times_state || !slots || !out || max_streams < 1 || max_frames < 1 || beam < 1 || beam > kMaxBeam) return -2;
  StreamEndpointArgs a;
  a.state = state; a.tws = times_state; a.slots = slots;
  a.lm_weight = lm_weight; a.ins_bonus = ins_bonus;
  a.biased = biased != 0; a.max_streams = max_streams; a.max_frames = max_frames; a.beam = beam;
  a.silence_frames = silence_frames; a.empty_frames = empty_frames; a.segment_frames = segment_frames;
  a.out = out;
  hipLaunchKernelGGL(ctc_beam_stream_endpoint_kernel, dim3(n), dim3(64), 0, stream, a);
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
