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
//      without a blank entry (lm_no_blank): token v > blank reads column v - 1.  The rows are the caller's: the LSTM LM's
//      log-softmax, or a sub-word n-gram LM's (ngram_rows.hip; V columns, -inf where the model has no entry: such a token's f_v
//      is -inf and it is no candidate).  Word-level LMs and a lexicon stay outside the transducer searches;
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
//
// The streamed search (ea_rnnt_frame_beam_stream_*): the same frames, one per call, for streams that come and go.  What the
// offline workspace holds per utterance is kept per stream SLOT in a caller-allocated buffer, behind a two-word head (frames
// consumed, 0); the frame number comes from that counter instead of `t` and `in_len`.  State of one slot, int32 words:
//   words(max_frames, beam) = 2 + even(3 * tsize + 5 * beam + 2 + 2 * cap + 2 * beam + 2 * beam * 64)
//   cap = 1 + max_frames * beam,  tsize = the smallest power of two >= max(64, 2 * cap),  even(w) = w rounded up to even
// (hash keys 2 * tsize, hash values tsize; score / len / last / node / pnode; the two counters; node_par and node_tok; and the
// row-to-select hand-over rblank, rnc, ctok, cval, which lives in the slot as it lives in the offline workspace).
//
// One body, two wrappers.  Row phase, select phase, the state before frame 0 and the finish each exist once, as __device__
// functions over a view of that state (RnntWs) and structs of the LDS arrays: rnnt_row_phase, rnnt_select_phase, rnnt_init,
// rnnt_finish.  The offline and the streamed kernels only decide where the view points and whether a frame is due (offline:
// workspace b, t < min(in_len[b], T), frame 0 initialises; streamed: slot in range, j < n_new[b], fewer than max_frames frames
// in the slot head), then call the phase.  The phases are templates on <kStreamed> so that each wrapper gets an instantiation
// of its own: select_nth (ctc_beam_common.h) is not __forceinline__ and is inlined only while every instantiation of it has a
// single caller, and the flag drops from the offline finish the two guards only a caller-sized streamed readout needs.  An
// earlier build whose offline kernels shared the streamed kernels' instantiation was 1.9 % slower per offline step; this one
// is not slower than the separate bodies it replaces (measured).  The tests still hold the two searches to
// each other with torch.equal, which now checks the wrappers: a stream fed in any pieces gives, bit for bit, what the offline
// search gives for the whole utterance, and a state sized for max_frames
// what a workspace sized for T gives (node ids are creation order; no rule looks at the table size).  Within one frame the
// order in which the fresh nodes get their ids is arbitrary (the selected candidates reach their lanes through an atomic
// counter); no result depends on it, only parent id < child id does.  "Bit for bit" is a statement about results (triples,
// finish, partial), not about the bytes of a state buffer: do not compare those across runs.  Table entries are
// published by atomics and read through L1-bypassing loads; everything else is ordered by the kernel boundaries.
//
// Kernels, LDS and occupancy (gfx950: 160 KB LDS per CU); no kernel uses scratch:
//   rnnt_beam_row_kernel, rnnt_beam_stream_row_kernel        256 threads, 21848 B LDS (RowLds), 46 VGPRs -> 7 workgroups per CU by LDS
//   rnnt_beam_select_kernel, rnnt_beam_stream_select_kernel  256 threads, 69912 B LDS (SelLds), 39 VGPRs -> 2 workgroups per CU by LDS
//   rnnt_beam_finish_kernel, rnnt_beam_stream_finish_kernel  64 threads, 256 B LDS, 18 VGPRs
//   rnnt_beam_stream_reset_kernel    256 threads, no LDS, 6 VGPRs
//   rnnt_beam_stream_partial_kernel  64 threads (one wave per slot), no LDS, 22 VGPRs
//   rnnt_beam_stream_endpoint_kernel 64 threads (one wave per slot), no LDS; reads the slot and its times slot only
// RowLds and SelLds are left at their natural alignment of 8: aligning the row to 16 turns the radix passes' ds_read2_b64 into
// ds_read_b128, which measured 0.1 - 0.2 us per frame slower, not faster.
//
// Hotword biasing (kBias instantiations, ea_rnnt_frame_beam_bias_* / ea_rnnt_frame_beam_stream_bias_*): the context graph of
// ctc_beam.hip's BIAS kernels (ctc_beam_common.h: cg_step) on this beam.  Every hypothesis also carries a graph node q and a
// running bias b, (root, 0) for the empty hypothesis, both functions of the token sequence alone: a stay changes neither, an
// extension takes one automaton step, and a merge (decided by node equality, log-add-exp on s only) keeps the stay's, which
// are what the extension would have computed.  The row phase is untouched (the K candidate tokens of a row stay the K with the
// largest fused r_v: biasing re-ranks, it does not bring a token back).  In the select phase the lane that owns candidate
// (j, v) walks the graph inside the candidate loop (cg_root[v], then for a slot off the root its node record, a binary search
// over the node's edge records and the failure hops), s + b' is the ranking key (a candidate is live iff s is finite), and
// (q', b') of ALL candidates wait in LDS for the <= beam selected ones: 33 280 B more, rather than a second walk of dependent
// global loads by wave 0 on the path that already waits for the hash claim -- one workgroup per utterance leaves the CU's LDS
// to it alone, so the size buys nothing back.  The finish adds b - phi(q); the partial ranks by and reports s + b.  (q, b) per
// beam slot live BEHIND the unbiased state, whose layout stays what it is: offline behind the B workspaces (2 * beam words per
// utterance, as ctc_beam.hip does it), streamed behind the slot, so
//   bias words(max_frames, beam) = words(max_frames, beam) + 2 * beam.
// The flag is a second template parameter of the four phases (the row phase ignores it: the streamed bias row kernel needs its
// own slot stride, hence its own kernel, hence its own instantiation of select_nth).  kBias = false: arguments, layout, LDS
// and instructions as before.  One search uses the bias calls for all of its steps, its finish and its partials.
//   rnnt_beam_select_kernel<true>, rnnt_beam_stream_select_kernel<true>  256 threads, 103704 B LDS (SelLdsBias) -> 1 workgroup per CU
//   (the offline bias step launches the unbiased row kernel; the other bias kernels: LDS of their unbiased twins)
//
// Time stamps (kTimes instantiations, ea_rnnt_frame_beam_times_* / ea_rnnt_frame_beam_stream_times_*): every hypothesis also
// carries v, which accumulates the same fused r as s with max in place of log-add-exp at a merge (the score of its best single
// alignment path), and e, a pointer into a per-utterance pool of time nodes (parent time node, frame); node 0 = no tokens.
// Stay: v' = v + r_blank, e' = e.  Extension by u: v'' = v + r_u and a NEW time node (e, t).  An extension that merges into a
// stay replaces the stay's (v', e') only if it is strictly larger.  Time nodes are made for selected candidates only, numbered
// in lane order: at most `beam` per frame, so the pool has the prefix table's cap.  Nothing of this enters a ranking key:
// tokens, scores and triples are those of the search without times, bit for bit.  The finish walks the chain of e into
// times[u] = the frame at which token u is emitted on that path, and returns v (never normalised).  The flag is a third
// template parameter of the select phase, the init and the finish; the row phase is untouched (the times step launches the
// twin's row kernel).  The state lives in a SEPARATE caller-allocated times workspace; the beam workspace / stream state is
// the twin's (biased or not), unchanged.  Per utterance (T frames) or per stream slot (T = max_frames), 4-byte words:
//   times words(T, beam) = 2 * beam + 2 + 2 * cap,  cap = 1 + T * beam
// (v fp32 [beam]; e int32 [beam]; the node counter and a pad word; tpar [cap], tfrm [cap]).  The select kernels write tpar /
// tfrm and only the finish reads them, across a kernel boundary.  LDS: 1 032 bytes more than the twin's select kernel.
//
// Endpointing (ea_rnnt_frame_beam_stream_endpoint): a read-only probe of a slot and its times slot after an accept: for the live
// hypothesis the partial kernel reports, its length L and E = tfrm[e], the frame of its last token on its best path (what the
// times finish writes as times[L - 1]), and the first rule that holds of silence (F - 1 - E frames without a token), empty and
// length (endpoint_rule, ctc_beam_common.h).  The caller then reads the finish and resets the slot: the stream goes on in a new
// segment, whose results are those of the offline search over its frames alone.
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

__device__ __forceinline__ RnntWs rnnt_ws_at(int* base, int T, int beam) {
  RnntWs w;
  w.cap = (int)rnnt_ws_cap(T, beam);
  w.tsize = (int)rnnt_ws_tsize(T, beam);
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

// ------------------------------------------------------------------------------------------------ the phases
// (templates on <kStreamed, kBias>: one instantiation per wrapper, see the header)
// (q, b) of the biased search per beam slot, and the graph; nothing without kBias
template <bool kBias> struct RnntBias {};
template <> struct RnntBias<true> {
  int* q; float* b;
  CgTables g;
};
struct NoGraph {};
template <bool kBias, class G>
__device__ __forceinline__ RnntBias<kBias> rnnt_bias_at(int* base, int beam, const G& g) {
  if constexpr (kBias) return {base, (float*)(base + beam), g}; else return {};
}
template <bool kBias, class A>
__device__ __forceinline__ auto rnnt_graph_of(const A& a) {  // the graph of a kernel's bias arguments
  if constexpr (kBias) return a.g; else return NoGraph{};
}

// the times workspace of one utterance / stream slot (see the header); nothing without kTimes
struct RnntTimesWs {
  float* v;
  int *e, *cnt /*[0] = time nodes*/, *tpar, *tfrm;
  int cap, t;  // t: the number of the frame a step is at
};
struct NoTimes {};
template <bool kTimes> using RnntTimes = std::conditional_t<kTimes, RnntTimesWs, NoTimes>;
__host__ __device__ __forceinline__ long rnnt_times_words(int T, int beam) { return 2L * beam + 2 + 2 * rnnt_ws_cap(T, beam); }
__device__ __forceinline__ RnntTimesWs rnnt_times_at(void* tws, long idx, int T, int beam, int t) {
  RnntTimesWs w;
  w.cap = (int)rnnt_ws_cap(T, beam);
  w.t = t;
  int* base = (int*)tws + idx * rnnt_times_words(T, beam);
  w.v = (float*)base;
  w.e = base + beam;
  w.cnt = w.e + beam;
  w.tpar = w.cnt + 2;
  w.tfrm = w.tpar + w.cap;
  return w;
}

struct RowParams {  // what the row phase needs besides its row, the same for the offline and the streamed search
  int V, K, blank, eos, lm_no_blank;
  float temperature, lm_weight;
};

struct RowLds {
  float row[kRowLds];
  SelectScratch sel;
  float red[16];
  int cunsorted[kMaxK];
  int nc;
};

// steps 1 - 3 of the contract and the top K of the row x (LM row m or null) of live slot j; leaves the hand-over in w.
// kBias is not read here: it only gives the streamed bias row kernel, whose slots are 2 * beam words longer, a body of its own.
// One streamed row kernel for both families would need the slot stride among the unbiased kernel's arguments, which are kept as
// they are; and two kernels on one instantiation would share one select_nth, which is then called instead of inlined -- what
// cost the offline step 1.9 % when the search was first streamed (see the header).  The price is a second copy of this phase.
template <bool kStreamed, bool kBias = false>
__device__ __forceinline__ void rnnt_row_phase(RowLds& s, const RowParams& a, const RnntWs& w, const float* x, const float* m, int j) {
  const int tid = threadIdx.x;
  const int V = a.V, blank = a.blank, eos = a.eos;
  const float temp = a.temperature, lw = a.lm_weight;
  auto lm_col = [&](int v) { return a.lm_no_blank && v > blank ? v - 1 : v; };

  // 1. z = logits / temperature to LDS; max, log-sum-exp, and the non-blank part of the sum
  float mx = -INFINITY;
  for (int v = tid; v < V; v += 256) {
    const float z = x[v] / temp;
    if (v < kRowLds) s.row[v] = z;
    mx = fmaxf(mx, z);
  }
  mx = block_max(mx, s.red);
  auto z_of = [&](int v) { return v < kRowLds ? s.row[v] : x[v] / temp; };
  float sa = 0.f, snb = 0.f;
  for (int v = tid; v < V; v += 256) {
    const float e = expf(z_of(v) - mx);
    sa += e;
    snb += v == blank ? 0.f : e;
  }
  sa = block_sum(sa, s.red);
  snb = block_sum(snb, s.red);
  const float lse = mx + logf(sa);
  float rb = z_of(blank) - lse;
  float shift = -lse;  // r_v = (what LDS holds for v) + shift

  // 2. fusion: f_v replaces z_v for v != blank; the shift gives the fused row the non-blank mass of the unfused one
  if (m) {
    float fm = -INFINITY;
    for (int v = tid; v < V; v += 256) {
      if (v == blank) continue;
      const float f = z_of(v) - lse + lw * m[lm_col(v)];
      if (v < kRowLds) s.row[v] = f;
      fm = fmaxf(fm, f);
    }
    fm = block_max(fm, s.red);
    auto f_of = [&](int v) { return v < kRowLds ? s.row[v] : x[v] / temp - lse + lw * m[lm_col(v)]; };
    float sf = 0.f;
    for (int v = tid; v < V; v += 256) sf += v == blank ? 0.f : expf(f_of(v) - fm);
    sf = block_sum(sf, s.red);
    shift = logf(snb) - logf(sa) - (fm + logf(sf));
  }
  auto r_of = [&](int v) {
    if (v < kRowLds) return s.row[v] + shift;
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
  const uint64_t kth = select_nth(tok_key, V, a.K, s.sel);
  if (tid == 0) s.nc = 0;
  __syncthreads();
  for (int v = tid; v < V; v += 256) {
    const uint64_t k = tok_key(v);
    if (k && k >= kth) s.cunsorted[atomicAdd(&s.nc, 1)] = v;
  }
  __syncthreads();
  const int nc = s.nc;  // <= K: the keys are unique
  if (tid < nc) {
    const int v = s.cunsorted[tid];
    int r = 0;
    for (int i = 0; i < nc; ++i) r += s.cunsorted[i] < v;
    w.ctok[(long)j * kMaxK + r] = v;
    w.cval[(long)j * kMaxK + r] = r_of(v);
  }
  if (tid == 0) { w.rblank[j] = rb; w.rnc[j] = nc; }
}

// the state before frame 0: the empty hypothesis with score 0 in slot 0, node 0 in an empty table (blockDim 256; the caller
// synchronises)
template <bool kBias, bool kTimes = false>
__device__ __forceinline__ void rnnt_init(const RnntWs& w, const RnntBias<kBias>& wb, const RnntTimes<kTimes>& tw = {}) {
  const int tid = threadIdx.x;
  for (int i = tid; i < w.tsize; i += 256) w.tab_key[i] = 0ull;
  if (tid == 0) {
    w.score[0] = 0.f; w.len[0] = 0; w.last[0] = -1; w.node[0] = 0; w.pnode[0] = -1;
    w.cnt[0] = 1; w.cnt[1] = 1;
    w.node_par[0] = -1; w.node_tok[0] = -1;
    if constexpr (kBias) { wb.q[0] = 0; wb.b[0] = 0.f; }
    if constexpr (kTimes) {
      tw.v[0] = 0.f; tw.e[0] = 0;
      tw.cnt[0] = 1; tw.cnt[1] = 0;
      tw.tpar[0] = -1; tw.tfrm[0] = -1;
    }
  }
}

// the triple of a beam that stands still: parent = identity, no token, every state kept
__device__ __forceinline__ void rnnt_identity(int* parent, int* token, uint8_t* keep, long row0, int beam, int blank) {
  const int tid = threadIdx.x;
  if (tid < beam) { parent[row0 + tid] = (int)(row0 + tid); token[row0 + tid] = blank; keep[row0 + tid] = 1; }
}

struct SelLds {
  uint64_t key[kMaxCand];
  SelectScratch sel;
  int ctok[kMaxBeam * kMaxK];  // [slot][K]
  float cval[kMaxBeam * kMaxK];
  float score[kMaxBeam], rb[kMaxBeam], stay[kMaxBeam];
  int len[kMaxBeam], last[kMaxBeam], node[kMaxBeam], pnode[kMaxBeam], nc[kMaxBeam];
  unsigned long long merged[kMaxBeam];  // bit r of slot j: extension (j, r) merged into a stay
  int sel_idx[kMaxBeam];
  int nsel, nfresh;
};
struct SelLdsBias : SelLds {
  int q[kMaxBeam]; float b[kMaxBeam];    // per slot
  int cq[kMaxCand]; float cb[kMaxCand];  // per candidate extension: the node and the running bias after it
};
template <bool kBias> using SelLdsOf = std::conditional_t<kBias, SelLdsBias, SelLds>;
template <bool kBias>
struct SelLdsTimes : SelLdsOf<kBias> {
  float v[kMaxBeam], vstay[kMaxBeam];  // per slot: the Viterbi score; that of its stay
  int e[kMaxBeam], esrc[kMaxBeam];     // its time node; the slot whose extension beat the stay (-1: none)
  int ntfresh;
};
template <bool kBias, bool kTimes> using SelLdsT = std::conditional_t<kTimes, SelLdsTimes<kBias>, SelLdsOf<kBias>>;

// merge, selection and the new state of one beam with nh hypotheses and nnodes table nodes; the triples go to rows row0 ...
template <bool kStreamed, bool kBias, bool kTimes = false>
__device__ __forceinline__ void rnnt_select_phase(SelLdsT<kBias, kTimes>& s, const RnntWs& w, const RnntBias<kBias>& wb, int beam, int K,
                                                  int blank, int nh, int nnodes, int* parent, int* token, uint8_t* keep, long row0,
                                                  const RnntTimes<kTimes>& tw = {}) {
  const int tid = threadIdx.x;
  const int K1 = K + 1;
  [[maybe_unused]] int ntn = 0;
  if constexpr (kTimes) {
    ntn = tw.cnt[0];
    if (tid < nh) { s.v[tid] = tw.v[tid]; s.e[tid] = tw.e[tid]; }
  }
  if (tid < nh) {
    s.score[tid] = w.score[tid]; s.len[tid] = w.len[tid]; s.last[tid] = w.last[tid]; s.node[tid] = w.node[tid];
    s.pnode[tid] = w.pnode[tid]; s.rb[tid] = w.rblank[tid]; s.nc[tid] = w.rnc[tid];
    s.merged[tid] = 0ull;
    if constexpr (kBias) { s.q[tid] = wb.q[tid]; s.b[tid] = wb.b[tid]; }
  }
  for (int i = tid; i < nh * K; i += 256) {  // (entries at or beyond a row's count are never used)
    const int j = i / K, r = i - j * K;
    s.ctok[i] = w.ctok[(long)j * kMaxK + r];
    s.cval[i] = w.cval[(long)j * kMaxK + r];
  }
  __syncthreads();

  // stays; a stay absorbs the extension y' + v == y (y' in the beam, v among its candidates)
  if (tid < nh) {
    float st = s.score[tid] + s.rb[tid];
    [[maybe_unused]] float vst = 0.f;
    [[maybe_unused]] int esrc = -1;
    if constexpr (kTimes) vst = s.v[tid] + s.rb[tid];
    if (s.len[tid] > 0) {
      int src = -1;
      for (int j = 0; j < nh; ++j) src = s.node[j] == s.pnode[tid] ? j : src;
      if (src >= 0) {
        const int nc = min(s.nc[src], K);
        for (int r = 0; r < nc; ++r)
          if (s.ctok[src * K + r] == s.last[tid]) {
            atomicOr(&s.merged[src], 1ull << r);
            st = lae(st, s.score[src] + s.cval[src * K + r]);
            if constexpr (kTimes) {
              const float vx = s.v[src] + s.cval[src * K + r];
              if (vx > vst) { vst = vx; esrc = src; }
            }
          }
      }
    }
    s.stay[tid] = st;
    if constexpr (kTimes) { s.vstay[tid] = vst; s.esrc[tid] = esrc; }
  }
  __syncthreads();

  // candidates; index i = slot * (K + 1) + (0: stay, 1 + r: extension by the slot's r-th candidate token)
  const int N = nh * K1;
  for (int i = tid; i < N; i += 256) {
    const int j = i / K1, q = i - j * K1;
    float sc = NAN;
    if (q == 0) sc = s.stay[j];
    else if (q - 1 < s.nc[j] && !((s.merged[j] >> (q - 1)) & 1ull)) sc = s.score[j] + s.cval[j * K + q - 1];
    // ranked by s + b'; one automaton step per live extension, on the lane that owns it.  cg_root[v] is loaded for every
    // extension, not only for slots in the root: cg_step wants it as the fall-back of a walk that ends at the root, and loading
    // it up front keeps it off the dependent chain of the walk (one 8-byte load per off-root candidate more than strictly needed)
    if constexpr (kBias) {
      float nb = s.b[j];
      if (q > 0 && isfinite(sc)) {
        const int v = s.ctok[j * K + q - 1];
        const CgStep st = cg_step(wb.g, s.q[j], v, cg_root(wb.g, v));
        nb += st.inc;
        s.cq[i] = st.q; s.cb[i] = nb;
      }
      s.key[i] = isfinite(sc) ? mk_key(sc + nb, i) : 0ull;
    } else {
      s.key[i] = isfinite(sc) ? mk_key(sc, i) : 0ull;
    }
  }
  __syncthreads();
  const uint64_t cth = select_nth([&](int i) { return s.key[i]; }, N, beam, s.sel);
  if (tid == 0) s.nsel = 0;
  __syncthreads();
  for (int i = tid; i < N; i += 256) {
    const uint64_t k = s.key[i];
    if (k && k >= cth) s.sel_idx[atomicAdd(&s.nsel, 1)] = i;
  }
  __syncthreads();
  const int ns = s.nsel;

  // the new state (wave 0: lane = one selected candidate, written to slot = its rank)
  float n_score = 0.f;
  int n_len = 0, n_last = -1, n_node = 0, n_pnode = -1, slot = 0, par = 0, ext = 0, fresh = 0, tslot = -1;
  [[maybe_unused]] int n_q = 0;
  [[maybe_unused]] float n_b = 0.f;
  [[maybe_unused]] float n_v = 0.f;
  [[maybe_unused]] int n_e = 0, tfresh = 0;
  if (tid < ns) {
    const int i = s.sel_idx[tid];
    const uint64_t k = s.key[i];
    for (int m = 0; m < ns; ++m) slot += s.key[s.sel_idx[m]] > k;
    const int j = i / K1, q = i - j * K1;
    par = j;
    if (q == 0) {
      n_score = s.stay[j]; n_len = s.len[j]; n_last = s.last[j]; n_node = s.node[j]; n_pnode = s.pnode[j];
      if constexpr (kBias) { n_q = s.q[j]; n_b = s.b[j]; }
      if constexpr (kTimes) {
        const int es = s.esrc[j];
        n_v = s.vstay[j]; tfresh = es >= 0; n_e = s.e[es >= 0 ? es : j];
      }
    } else {
      ext = 1;
      if constexpr (kBias) { n_q = s.cq[i]; n_b = s.cb[i]; }
      if constexpr (kTimes) { n_v = s.v[j] + s.cval[j * K + q - 1]; tfresh = 1; n_e = s.e[j]; }
      n_score = s.score[j] + s.cval[j * K + q - 1];
      n_len = s.len[j] + 1; n_last = s.ctok[j * K + q - 1]; n_pnode = s.node[j];
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
  if (tid < 64) {  // fresh nodes numbered in lane order (which candidate a lane holds is arbitrary: see the header)
    const unsigned long long fm = __ballot(fresh);
    if (fresh) {
      const int id = nnodes + __popcll(fm & ((1ull << tid) - 1ull));
      n_node = id;
      w.tab_val[tslot] = id;
      if (id < w.cap) { w.node_par[id] = n_pnode; w.node_tok[id] = n_last; }
    }
    if (tid == 0) s.nfresh = __popcll(fm);
    if constexpr (kTimes) {  // fresh time nodes likewise
      const unsigned long long tm = __ballot(tfresh);
      if (tfresh) {
        const int id = ntn + __popcll(tm & ((1ull << tid) - 1ull));
        if (id < tw.cap) { tw.tpar[id] = n_e; tw.tfrm[id] = tw.t; }
        n_e = id;
      }
      if (tid == 0) s.ntfresh = __popcll(tm);
    }
  }
  __syncthreads();
  if constexpr (kTimes) {
    if (tid < ns) { tw.v[slot] = n_v; tw.e[slot] = n_e; }
    if (tid == 0) tw.cnt[0] = ntn + s.ntfresh;
  }
  if (tid < ns) {
    w.score[slot] = n_score; w.len[slot] = n_len; w.last[slot] = n_last; w.node[slot] = n_node; w.pnode[slot] = n_pnode;
    if constexpr (kBias) { wb.q[slot] = n_q; wb.b[slot] = n_b; }
    parent[row0 + slot] = (int)(row0 + par);
    token[row0 + slot] = ext ? n_last : blank;
    keep[row0 + slot] = (uint8_t)!ext;
  } else if (tid < beam) {  // empty slot: any valid row
    parent[row0 + tid] = (int)row0; token[row0 + tid] = blank; keep[row0 + tid] = 1;
  }
  if (tid == 0) { w.cnt[0] = ns; w.cnt[1] = nnodes + s.nfresh; }
}

// final score = s [+ b - phi(q)], or that / max(1, |y|); the nbest best of the nh hypotheses by (-final, slot), backtracked into tokens
// [nbest][max_u] (pad-filled), lengths / scores [nbest] and *nhyp.  fresh: no step has run, the beam is the empty hypothesis
// and w is not read.  Reads the state only (blockDim 64).
// kTimes: also times [nbest][max_u] (the frame at which every token is emitted on the best path, -1 after the hypothesis) and
// vscores [nbest] (v, not normalised)
template <bool kStreamed, bool kBias, bool kTimes = false>
__device__ __forceinline__ void rnnt_finish(float* s_fin, const RnntWs& w, const RnntBias<kBias>& wb, int nh, bool fresh, int nbest, int pad, int normalize,
                                            int max_u, int* tokens, int* lengths, float* scores, int* nhyp,
                                            const RnntTimes<kTimes>& tw = {}, [[maybe_unused]] int* times = nullptr,
                                            [[maybe_unused]] float* vscores = nullptr) {
  const int j = threadIdx.x;
  if (j < nh) {
    float s = fresh ? 0.f : w.score[j];
    if constexpr (kBias) s += fresh ? 0.f : wb.b[j] - cg_phi(wb.g, wb.q[j]);
    const int n = fresh ? 0 : w.len[j];
    s_fin[j] = normalize ? s / (float)max(1, n) : s;
  }
  __syncthreads();
  if (j == 0) *nhyp = min(nh, nbest);
  if (j < nh) {
    const float s = s_fin[j];
    int rank = 0;
    for (int m = 0; m < nh; ++m) rank += s_fin[m] > s || (s_fin[m] == s && m < j);
    if (rank < nbest) {
      int* out = tokens + (long)rank * max_u;
      const int len = fresh ? 0 : w.len[j];
      const int n = kStreamed ? min(len, max_u) : len;
      for (int u = n; u < max_u; ++u) out[u] = pad;
      int node = fresh ? 0 : w.node[j];
      for (int u = len - 1; u >= 0 && node > 0 && (!kStreamed || node < w.cap); --u) {
        if (!kStreamed || u < max_u) out[u] = w.node_tok[node];
        node = w.node_par[node];
      }
      lengths[rank] = n;
      scores[rank] = s;
      if constexpr (kTimes) {
        int* tout = times + (long)rank * max_u;
        for (int u = 0; u < max_u; ++u) tout[u] = -1;
        int e = fresh ? 0 : tw.e[j];
        for (int u = len - 1; u >= 0 && e > 0 && e < tw.cap; --u) {
          if (u < max_u) tout[u] = tw.tfrm[e];
          e = tw.tpar[e];
        }
        vscores[rank] = fresh ? 0.f : tw.v[j];
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

// ------------------------------------------------------------------------------------------------ the offline search
// One workspace per utterance b; a frame is due while t < min(in_len[b], T); frame 0 starts from the empty hypothesis, which
// the select kernel writes before it runs the phase (the row kernel of frame 0 only needs the count, 1).
__device__ __forceinline__ RnntWs rnnt_ws_of(void* ws, int b, int T, int beam) {
  return rnnt_ws_at((int*)ws + (long)b * rnnt_ws_words(T, beam), T, beam);
}

struct RowArgs {
  const float* logits; long ld;
  const float* lm_rows; long ld_lm;
  const int* in_len; void* ws;
  RowParams p;
  int T, beam, t;
};

// the row phase, one workgroup per (utterance, slot)
__global__ __launch_bounds__(256) void rnnt_beam_row_kernel(const RowArgs a) {
  __shared__ RowLds s;
  const int n = blockIdx.x, b = n / a.beam, j = n - b * a.beam;
  const RnntWs w = rnnt_ws_of(a.ws, b, a.T, a.beam);
  if (a.t >= min(a.in_len[b], a.T)) return;  // past the end of this utterance
  if (j >= (a.t == 0 ? 1 : w.cnt[0])) return;  // dead slot: the row is not read
  rnnt_row_phase<false>(s, a.p, w, a.logits + (long)n * a.ld, a.lm_rows ? a.lm_rows + (long)n * a.ld_lm : nullptr, j);
}

struct SelArgs {
  const int* in_len; void* ws;
  int* parent; int* token; uint8_t* keep;
  int T, beam, K, blank, t;
};
struct BiasSelArgs : SelArgs { CgTables g; };
struct TimesSelArgs : BiasSelArgs { void* tws; };

// (q, b) of utterance b of B: behind the B unbiased workspaces
template <bool kBias, class G, class... Unused>
__device__ __forceinline__ RnntBias<kBias> rnnt_bias_of(void* ws, int B, int b, int T, int beam, const G& g, const Unused&...) {
  return rnnt_bias_at<kBias>((int*)ws + (long)B * rnnt_ws_words(T, beam) + 2L * b * beam, beam, g);
}

// the select phase, one workgroup per utterance
template <bool kTimes, class A>
__device__ __forceinline__ RnntTimes<kTimes> rnnt_times_of(const A& a, long idx, int T, int beam, int t) {
  if constexpr (kTimes) return rnnt_times_at((void*)a.tws, idx, T, beam, t); else return NoTimes{};
}

template <bool kBias, bool kTimes = false>
__global__ __launch_bounds__(256) void rnnt_beam_select_kernel(
    const std::conditional_t<kTimes, TimesSelArgs, std::conditional_t<kBias, BiasSelArgs, SelArgs>> a) {
  __shared__ SelLdsT<kBias, kTimes> s;
  const int b = blockIdx.x;
  const RnntWs w = rnnt_ws_of(a.ws, b, a.T, a.beam);
  const RnntBias<kBias> wb = rnnt_bias_of<kBias>(a.ws, gridDim.x, b, a.T, a.beam, rnnt_graph_of<kBias>(a));
  const RnntTimes<kTimes> tw = rnnt_times_of<kTimes>(a, b, a.T, a.beam, a.t);
  const long row0 = (long)b * a.beam;
  if (a.t == 0) {
    rnnt_init<kBias, kTimes>(w, wb, tw);
    __threadfence_block();
    __syncthreads();
  }
  if (a.t >= min(a.in_len[b], a.T)) {  // past the end of this utterance: the beam stands still
    rnnt_identity(a.parent, a.token, a.keep, row0, a.beam, a.blank);
    return;
  }
  rnnt_select_phase<false, kBias, kTimes>(s, w, wb, a.beam, a.K, a.blank, a.t == 0 ? 1 : w.cnt[0], a.t == 0 ? 1 : w.cnt[1], a.parent,
                                          a.token, a.keep, row0, tw);
}

// the finish of every utterance into tokens [B][nbest][T]; T == 0: no step has run
// (g: the graph, one CgTables, with kBias and nothing without: the unbiased kernel keeps its parameter list)
template <bool kBias, class... G>
__global__ __launch_bounds__(64) void rnnt_beam_finish_kernel(void* ws, int T, int beam, int nbest, int pad, int normalize,
                                                              int* tokens, int* lengths, float* scores, int* nhyp, const G... g) {
  static_assert(sizeof...(G) == (kBias ? 1 : 0));
  __shared__ float s_fin[kMaxBeam];
  const int b = blockIdx.x;
  const RnntWs w = rnnt_ws_of(ws, b, T, beam);
  const RnntBias<kBias> wb = rnnt_bias_of<kBias>(ws, gridDim.x, b, T, beam, g..., NoGraph{});
  rnnt_finish<false, kBias>(s_fin, w, wb, T == 0 ? 1 : w.cnt[0], T == 0, nbest, pad, normalize, T, tokens + (long)b * nbest * T,
                            lengths + b * nbest, scores + b * nbest, nhyp + b);
}

struct TimesFinishArgs {
  void* ws; const void* tws;
  int T, beam, nbest, pad, normalize;
  int *tokens, *lengths; float* scores; int* nhyp;
  int* times; float* vscores;
  CgTables g;
};
template <bool kBias>
__global__ __launch_bounds__(64) void rnnt_beam_times_finish_kernel(const TimesFinishArgs a) {
  __shared__ float s_fin[kMaxBeam];
  const int b = blockIdx.x, T = a.T, beam = a.beam, nbest = a.nbest;
  const RnntWs w = rnnt_ws_of(a.ws, b, T, beam);
  const RnntBias<kBias> wb = rnnt_bias_of<kBias>(a.ws, gridDim.x, b, T, beam, a.g);
  rnnt_finish<false, kBias, true>(s_fin, w, wb, T == 0 ? 1 : w.cnt[0], T == 0, nbest, a.pad, a.normalize, T, a.tokens + (long)b * nbest * T,
                                  a.lengths + b * nbest, a.scores + b * nbest, a.nhyp + b, rnnt_times_at((void*)a.tws, b, T, beam, 0),
                                  a.times + (long)b * nbest * T, a.vscores + b * nbest);
}

// ------------------------------------------------------------------------------------------------ the streamed search
// State of one stream slot, int32 words: [0] frames consumed, [1] 0, then the offline workspace of one utterance of max_frames
// frames (RnntWs: the row-to-select hand-over included), then with kBias (q, b) per beam slot.
template <bool kBias = false>
__host__ __device__ __forceinline__ long rnnt_state_words(int max_frames, int beam) {
  return 2 + rnnt_ws_words(max_frames, beam) + (kBias ? 2L * beam : 0L);
}

template <bool kBias>
struct RnntSlot {
  int* head;
  RnntWs w;
  RnntBias<kBias> wb;
};
template <bool kBias, class G>
__device__ __forceinline__ RnntSlot<kBias> rnnt_slot(void* state, int slot, int max_frames, int beam, const G& g) {
  RnntSlot<kBias> q;
  q.head = (int*)state + (long)slot * rnnt_state_words<kBias>(max_frames, beam);
  q.w = rnnt_ws_at(q.head + 2, max_frames, beam);
  q.wb = rnnt_bias_at<kBias>(q.head + 2 + rnnt_ws_words(max_frames, beam), beam, g);
  return q;
}

// (tstate: the times slots, one void* with kTimes and nothing without: the kernels without times keep their parameter list)
template <bool kBias, bool kTimes = false, class... TS>
__global__ __launch_bounds__(256) void rnnt_beam_stream_reset_kernel(void* state, const int* slots, int max_streams, int max_frames,
                                                                     int beam, TS... tstate) {
  static_assert(sizeof...(TS) == (kTimes ? 1 : 0));
  const int slot = slots[blockIdx.x];
  if (slot < 0 || slot >= max_streams) return;
  const RnntSlot<kBias> q = rnnt_slot<kBias>(state, slot, max_frames, beam, CgTables{});
  if constexpr (kTimes) rnnt_init<kBias, true>(q.w, q.wb, rnnt_times_at(tstate..., slot, max_frames, beam, 0));
  else rnnt_init<kBias>(q.w, q.wb);
  if (threadIdx.x == 0) { q.head[0] = 0; q.head[1] = 0; }
}

struct StreamRowArgs {
  const float* logits; long ld;
  const float* lm_rows; long ld_lm;
  const int *slot_idx, *n_new; void* state;
  RowParams p;
  int max_streams, max_frames, beam, j;
};

// the row phase of the streamed search, one workgroup per (listed stream, slot of its beam); kBias: the slot stride only
template <bool kBias>
__global__ __launch_bounds__(256) void rnnt_beam_stream_row_kernel(const StreamRowArgs a) {
  __shared__ RowLds s;
  const int n = blockIdx.x, b = n / a.beam, j = n - b * a.beam;
  const int slot = a.slot_idx[b];
  if (slot < 0 || slot >= a.max_streams || a.j >= a.n_new[b]) return;
  const RnntSlot<kBias> q = rnnt_slot<kBias>(a.state, slot, a.max_frames, a.beam, CgTables{});
  const int frames = q.head[0];
  if (frames < 0 || frames >= a.max_frames) return;  // a full slot
  if (j >= q.w.cnt[0]) return;                       // dead slot: the row is not read
  rnnt_row_phase<true, kBias>(s, a.p, q.w, a.logits + (long)n * a.ld, a.lm_rows ? a.lm_rows + (long)n * a.ld_lm : nullptr, j);
}

struct StreamSelArgs {
  const int *slot_idx, *n_new; void* state;
  int* parent; int* token; uint8_t* keep;
  int max_streams, max_frames, beam, K, blank, j;
};
struct BiasStreamSelArgs : StreamSelArgs { CgTables g; };
struct TimesStreamSelArgs : BiasStreamSelArgs { void* tws; };
// the select phase of the streamed search, one workgroup per listed stream; counts the frame
// (kTimes: the times slot goes with the slot, untouched where the slot is; the frame's number is the slot's counter)
template <bool kBias, bool kTimes = false>
__global__ __launch_bounds__(256) void rnnt_beam_stream_select_kernel(
    const std::conditional_t<kTimes, TimesStreamSelArgs, std::conditional_t<kBias, BiasStreamSelArgs, StreamSelArgs>> a) {
  __shared__ SelLdsT<kBias, kTimes> s;
  const int b = blockIdx.x;
  const long row0 = (long)b * a.beam;
  const int slot = a.slot_idx[b];
  bool due = slot >= 0 && slot < a.max_streams && a.j < a.n_new[b];
  const RnntSlot<kBias> q = rnnt_slot<kBias>(a.state, due ? slot : 0, a.max_frames, a.beam, rnnt_graph_of<kBias>(a));
  const int frames = due ? q.head[0] : -1;
  due = due && frames >= 0 && frames < a.max_frames;
  if (!due) {  // idle, no such slot, or a full slot: the slot is untouched
    rnnt_identity(a.parent, a.token, a.keep, row0, a.beam, a.blank);
    return;
  }
  const int nh = min(max(q.w.cnt[0], 0), a.beam);
  rnnt_select_phase<true, kBias, kTimes>(s, q.w, q.wb, a.beam, a.K, a.blank, nh, q.w.cnt[1], a.parent, a.token, a.keep, row0,
                                         rnnt_times_of<kTimes>(a, slot, a.max_frames, a.beam, frames));
  if (threadIdx.x == 0) q.head[0] = frames + 1;
}

struct StreamReadArgs {
  const void* state; const int* slots;
  int max_streams, max_frames, beam, nbest, pad, normalize, max_u;
  int *tokens, *lengths; float* scores; int* aux;  // aux: nhyp (finish) / stable_len (partial)
};
struct BiasStreamReadArgs : StreamReadArgs { CgTables g; };
struct TimesStreamReadArgs : BiasStreamReadArgs { const void* tws; int* times; float* vscores; };

// readout of the given slots, as the offline kernel finishes; the state is read only
template <bool kBias>
__global__ __launch_bounds__(64) void rnnt_beam_stream_finish_kernel(const std::conditional_t<kBias, BiasStreamReadArgs, StreamReadArgs> a) {
  __shared__ float s_fin[kMaxBeam];
  const int b = blockIdx.x, slot = a.slots[b];
  const bool valid = slot >= 0 && slot < a.max_streams;  // no such slot: no hypothesis
  const RnntSlot<kBias> q = rnnt_slot<kBias>((void*)a.state, valid ? slot : 0, a.max_frames, a.beam, rnnt_graph_of<kBias>(a));
  rnnt_finish<true, kBias>(s_fin, q.w, q.wb, valid ? min(max(q.w.cnt[0], 0), a.beam) : 0, false, a.nbest, a.pad, a.normalize, a.max_u,
              a.tokens + (long)b * a.nbest * a.max_u, a.lengths + b * a.nbest, a.scores + b * a.nbest, a.aux + b);
}

template <bool kBias>
__global__ __launch_bounds__(64) void rnnt_beam_stream_times_finish_kernel(const TimesStreamReadArgs a) {
  __shared__ float s_fin[kMaxBeam];
  const int b = blockIdx.x, slot = a.slots[b];
  const bool valid = slot >= 0 && slot < a.max_streams;
  const RnntSlot<kBias> q = rnnt_slot<kBias>((void*)a.state, valid ? slot : 0, a.max_frames, a.beam, a.g);
  rnnt_finish<true, kBias, true>(s_fin, q.w, q.wb, valid ? min(max(q.w.cnt[0], 0), a.beam) : 0, false, a.nbest, a.pad, a.normalize,
                                 a.max_u, a.tokens + (long)b * a.nbest * a.max_u, a.lengths + b * a.nbest, a.scores + b * a.nbest,
                                 a.aux + b, rnnt_times_at((void*)a.tws, valid ? slot : 0, a.max_frames, a.beam, 0),
                                 a.times + (long)b * a.nbest * a.max_u, a.vscores + b * a.nbest);
}

// The live hypothesis with the best score s (kBias: s + b; what the search prunes by; ties: the lower slot) and the length of the longest
// common prefix of all live hypotheses: the depth of their lowest common ancestor in node_par.  Nodes are numbered in creation
// order, so a parent's id is below its child's: lifting the highest node until all are equal ends at that ancestor.  One wave
// per slot; the state is read only.
template <bool kBias>
__global__ __launch_bounds__(64) void rnnt_beam_stream_partial_kernel(const StreamReadArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, slot = a.slots[b];
  int* out = a.tokens + (long)b * a.max_u;
  const bool valid = slot >= 0 && slot < a.max_streams;
  const RnntSlot<kBias> q = rnnt_slot<kBias>((void*)a.state, valid ? slot : 0, a.max_frames, a.beam, CgTables{});
  const int nh = valid ? min(max(q.w.cnt[0], 0), a.beam) : 0;
  float sc = -INFINITY;
  int len = 0, node = 0;
  if (lane < nh) { sc = q.w.score[lane]; len = q.w.len[lane]; node = q.w.node[lane]; }
  if constexpr (kBias) sc += lane < nh ? q.wb.b[lane] : 0.f;
  const bool in_set = lane < nh;
  // best: the highest score, then the lower slot (a nan score ranks below everything)
  const uint64_t key = in_set ? mk_key(sc == sc ? sc : -INFINITY, lane) : 0ull;
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
  if (is_best) a.aux[b] = depth;  // the best hypothesis is a member: its depth after the lifts is the ancestor's
  if (nh == 0 && lane == 0) {
    for (int u = 0; u < a.max_u; ++u) out[u] = a.pad;
    a.lengths[b] = 0; a.scores[b] = -INFINITY; a.aux[b] = 0;
  }
}

struct StreamEndpointArgs {
  const void *state, *tws; const int* slots;
  int max_streams, max_frames, beam, silence_frames, empty_frames, segment_frames;
  int* out;
};

// The endpoint probe: per listed slot out[b] = (rule, F, L, E) for F = the slot's frame counter and the live hypothesis the partial
// kernel above reports (the same score and tie rule, restated here so that the partial kernel's code stays what it is): L = its
// length, E = tfrm[e], the frame at which its last token is emitted on its best path, which is what the times finish writes as
// times[L - 1] for it, -1 when L == 0.  A slot without frames or without a hypothesis has the empty hypothesis; a slot out of
// range writes (0, 0, 0, -1).  One wave per slot, no LDS; the state and the times state are read only.  kBias: the slot stride
// and the + b of the ranking.
template <bool kBias>
__global__ __launch_bounds__(64) void rnnt_beam_stream_endpoint_kernel(const StreamEndpointArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, slot = a.slots[b];
  int* out = a.out + 4L * b;
  if (slot < 0 || slot >= a.max_streams) {
    if (lane == 0) { out[0] = 0; out[1] = 0; out[2] = 0; out[3] = -1; }
    return;
  }
  const RnntSlot<kBias> q = rnnt_slot<kBias>((void*)a.state, slot, a.max_frames, a.beam, CgTables{});
  const RnntTimesWs tw = rnnt_times_at((void*)a.tws, slot, a.max_frames, a.beam, 0);
  const int F = max(q.head[0], 0);
  const int nh = F > 0 ? min(max(q.w.cnt[0], 0), a.beam) : 0;
  float sc = -INFINITY;
  int len = 0;
  if (lane < nh) { sc = q.w.score[lane]; len = q.w.len[lane]; }
  if constexpr (kBias) sc += lane < nh ? q.wb.b[lane] : 0.f;
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
      const int e = tw.e[lane];
      if (e > 0 && e < tw.cap) E = tw.tfrm[e];
    }
    out[0] = endpoint_rule(F, L, E, a.silence_frames, a.empty_frames, a.segment_frames);
    out[1] = F; out[2] = L; out[3] = E;
  }
}

}  // namespace

// weight 0 is no fusion: the LM rows are not read (an entry of -inf times 0 would be NaN)
static RowParams rnnt_row_params(const float*& lm_rows, int lm_no_blank, int V, int K, int blank, int eos, float temperature,
                                 float lm_weight) {
  RowParams p;
  p.V = V; p.K = K; p.blank = blank; p.eos = eos; p.lm_no_blank = lm_no_blank;
  p.temperature = temperature; p.lm_weight = lm_rows ? lm_weight : 0.f;
  if (lm_weight == 0.f) lm_rows = nullptr;
  return p;
}

static bool rnnt_step_args_bad(long ld, const float* lm_rows, long ld_lm, int lm_no_blank, int V, int beam, int K, int blank, int eos,
                               float temperature) {
  return V < 2 || V > 65535 || ld < V || beam < 1 || beam > kMaxBeam || K < 1 || K > kMaxK || K > V - 1 || blank < 0 || blank >= V ||
         eos < -1 || eos >= V || eos == blank || !(temperature > 0.f) || (lm_rows && ld_lm < (lm_no_blank ? V - 1 : V));
}

extern "C" long ea_rnnt_frame_beam_workspace_bytes(int B, int T, int beam) {
  if (B <= 0 || T < 0 || beam < 1 || beam > kMaxBeam) return 0;
  return (long)B * rnnt_ws_words(T, beam) * 4L;
}

extern "C" int ea_rnnt_frame_beam_step(const float* logits, long ld, const float* lm_rows, long ld_lm, int lm_no_blank,
                                       const int* in_len, void* workspace, int* parent, int* token, void* keep, int B, int T, int V,
                                       int beam, int K, int blank, int eos, float temperature, float lm_weight, int t,
                                       hipStream_t stream) {
  if (B <= 0) return 0;
  if (!logits || !in_len || !workspace || !parent || !token || !keep || T < 1 || t < 0 || t >= T ||
      rnnt_step_args_bad(ld, lm_rows, ld_lm, lm_no_blank, V, beam, K, blank, eos, temperature))
    return -2;
  RowArgs r;
  r.p = rnnt_row_params(lm_rows, lm_no_blank, V, K, blank, eos, temperature, lm_weight);
  r.logits = logits; r.ld = ld; r.lm_rows = lm_rows; r.ld_lm = ld_lm;
  r.in_len = in_len; r.ws = workspace;
  r.T = T; r.beam = beam; r.t = t;
  hipLaunchKernelGGL(rnnt_beam_row_kernel, dim3(B * beam), dim3(256), 0, stream, r);
  SelArgs s;
  s.in_len = in_len; s.ws = workspace; s.parent = parent; s.token = token; s.keep = (uint8_t*)keep;
  s.T = T; s.beam = beam; s.K = K; s.blank = blank; s.t = t;
  hipLaunchKernelGGL(rnnt_beam_select_kernel<false>, dim3(B), dim3(256), 0, stream, s);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_rnnt_frame_beam_finish(void* workspace, int B, int T, int beam, int nbest, int pad, int normalize, int* tokens,
                                         int* lengths, float* scores, int* nhyp, hipStream_t stream) {
  if (B <= 0) return 0;
  if (!workspace || !tokens || !lengths || !scores || !nhyp || T < 0 || beam < 1 || beam > kMaxBeam || nbest < 1 || nbest > beam)
    return -2;
  hipLaunchKernelGGL(rnnt_beam_finish_kernel<false>, dim3(B), dim3(64), 0, stream, workspace, T, beam, nbest, pad, normalize, tokens,
                     lengths, scores, nhyp);
  return EA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------ C ABI: hotword biasing
extern "C" long ea_rnnt_frame_beam_bias_workspace_bytes(int B, int T, int beam) {
  const long base = ea_rnnt_frame_beam_workspace_bytes(B, T, beam);
  return base ? base + (long)B * 2L * beam * 4L : 0;
}

extern "C" int ea_rnnt_frame_beam_bias_step(const float* logits, long ld, const float* lm_rows, long ld_lm, int lm_no_blank,
                                            const int* in_len, void* workspace, int* parent, int* token, void* keep,
                                            const int* cg_nodes, const int* cg_edges, const int* cg_root, int cg_n_nodes,
                                            int cg_n_edges, int B, int T, int V, int beam, int K, int blank, int eos,
                                            float temperature, float lm_weight, int t, hipStream_t stream) {
  if (B <= 0) return 0;
  BiasSelArgs s;
  if (!logits || !in_len || !workspace || !parent || !token || !keep || T < 1 || t < 0 || t >= T ||
      rnnt_step_args_bad(ld, lm_rows, ld_lm, lm_no_blank, V, beam, K, blank, eos, temperature) ||
      !cg_tables(s.g, cg_nodes, cg_edges, cg_root, cg_n_nodes, cg_n_edges, V))
    return -2;
  RowArgs r;  // the row phase knows nothing of the graph: the unbiased row kernel on the unbiased part of the workspace
  r.p = rnnt_row_params(lm_rows, lm_no_blank, V, K, blank, eos, temperature, lm_weight);
  r.logits = logits; r.ld = ld; r.lm_rows = lm_rows; r.ld_lm = ld_lm;
  r.in_len = in_len; r.ws = workspace;
  r.T = T; r.beam = beam; r.t = t;
  hipLaunchKernelGGL(rnnt_beam_row_kernel, dim3(B * beam), dim3(256), 0, stream, r);
  s.in_len = in_len; s.ws = workspace; s.parent = parent; s.token = token; s.keep = (uint8_t*)keep;
  s.T = T; s.beam = beam; s.K = K; s.blank = blank; s.t = t;
  hipLaunchKernelGGL(rnnt_beam_select_kernel<true>, dim3(B), dim3(256), 0, stream, s);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_rnnt_frame_beam_bias_finish(void* workspace, const int* cg_nodes, int cg_n_nodes, int B, int T, int beam, int nbest,
                                              int pad, int normalize, int* tokens, int* lengths, float* scores, int* nhyp,
                                              hipStream_t stream) {
  if (B <= 0) return 0;
  if (!workspace || !tokens || !lengths || !scores || !nhyp || T < 0 || beam < 1 || beam > kMaxBeam || nbest < 1 || nbest > beam ||
      !cg_nodes || cg_n_nodes < 1)
    return -2;
  hipLaunchKernelGGL((rnnt_beam_finish_kernel<true, CgTables>), dim3(B), dim3(64), 0, stream, workspace, T, beam, nbest, pad, normalize, tokens,
                     lengths, scores, nhyp, cg_nodes_only(cg_nodes, cg_n_nodes));
  return EA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------ C ABI: the streamed search
extern "C" long ea_rnnt_frame_beam_stream_state_bytes(int max_frames, int beam) {
  if (max_frames < 1 || beam < 1 || beam > kMaxBeam) return 0;
  return rnnt_state_words(max_frames, beam) * 4L;
}

extern "C" int ea_rnnt_frame_beam_stream_reset(void* state, const int* slots, int n, int max_streams, int max_frames, int beam,
                                               hipStream_t stream) {
  if (n <= 0) return 0;
  if (!state || !slots || max_streams < 1 || max_frames < 1 || beam < 1 || beam > kMaxBeam) return -2;
  hipLaunchKernelGGL(rnnt_beam_stream_reset_kernel<false>, dim3(n), dim3(256), 0, stream, state, slots, max_streams, max_frames, beam);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_rnnt_frame_beam_stream_step(const float* logits, long ld, const float* lm_rows, long ld_lm, int lm_no_blank,
                                              const int* slot_idx, const int* n_new, int j, int n, void* state, int* parent,
                                              int* token, void* keep, int max_streams, int max_frames, int V, int beam, int K,
                                              int blank, int eos, float temperature, float lm_weight, hipStream_t stream) {
  if (n <= 0) return 0;
  if (!logits || !slot_idx || !n_new || !state || !parent || !token || !keep || j < 0 || max_streams < 1 || max_frames < 1 ||
      rnnt_step_args_bad(ld, lm_rows, ld_lm, lm_no_blank, V, beam, K, blank, eos, temperature))
    return -2;
  StreamRowArgs r;
  r.p = rnnt_row_params(lm_rows, lm_no_blank, V, K, blank, eos, temperature, lm_weight);
  r.logits = logits; r.ld = ld; r.lm_rows = lm_rows; r.ld_lm = ld_lm;
  r.slot_idx = slot_idx; r.n_new = n_new; r.state = state;
  r.max_streams = max_streams; r.max_frames = max_frames; r.beam = beam; r.j = j;
  hipLaunchKernelGGL(rnnt_beam_stream_row_kernel<false>, dim3(n * beam), dim3(256), 0, stream, r);
  StreamSelArgs s;
  s.slot_idx = slot_idx; s.n_new = n_new; s.state = state; s.parent = parent; s.token = token; s.keep = (uint8_t*)keep;
  s.max_streams = max_streams; s.max_frames = max_frames; s.beam = beam; s.K = K; s.blank = blank; s.j = j;
  hipLaunchKernelGGL(rnnt_beam_stream_select_kernel<false>, dim3(n), dim3(256), 0, stream, s);
  return EA_CHECK_LAUNCH();
}

static bool rnnt_read_args_bad(const void* state, const int* slots, int max_streams, int max_frames, int beam, int max_u,
                               const int* tokens, const int* lengths, const float* scores, const int* aux) {
  return !state || !slots || !tokens || !lengths || !scores || !aux || max_streams < 1 || max_frames < 1 || beam < 1 ||
         beam > kMaxBeam || max_u < 0;
}

static void rnnt_read_args(StreamReadArgs& a, const void* state, const int* slots, int max_streams, int max_frames, int beam, int nbest,
                           int pad, int normalize, int max_u, int* tokens, int* lengths, float* scores, int* aux) {
  a.state = state; a.slots = slots;
  a.max_streams = max_streams; a.max_frames = max_frames; a.beam = beam; a.nbest = nbest; a.pad = pad; a.normalize = normalize;
  a.max_u = max_u;
  a.tokens = tokens; a.lengths = lengths; a.scores = scores; a.aux = aux;
}

extern "C" int ea_rnnt_frame_beam_stream_finish(const void* state, const int* slots, int n, int max_streams, int max_frames,
                                                int beam, int nbest, int pad, int normalize, int max_u, int* tokens, int* lengths,
                                                float* scores, int* nhyp, hipStream_t stream) {
  if (n <= 0) return 0;
  if (rnnt_read_args_bad(state, slots, max_streams, max_frames, beam, max_u, tokens, lengths, scores, nhyp) || nbest < 1 || nbest > beam)
    return -2;
  StreamReadArgs a;
  rnnt_read_args(a, state, slots, max_streams, max_frames, beam, nbest, pad, normalize, max_u, tokens, lengths, scores, nhyp);
  hipLaunchKernelGGL(rnnt_beam_stream_finish_kernel<false>, dim3(n), dim3(64), 0, stream, a);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_rnnt_frame_beam_stream_partial(const void* state, const int* slots, int n, int max_streams, int max_frames,
                                                 int beam, int pad, int max_u, int* tokens, int* lengths, float* scores,
                                                 int* stable_len, hipStream_t stream) {
  if (n <= 0) return 0;
  if (rnnt_read_args_bad(state, slots, max_streams, max_frames, beam, max_u, tokens, lengths, scores, stable_len)) return -2;
  StreamReadArgs a;
  rnnt_read_args(a, state, slots, max_streams, max_frames, beam, 1, pad, 0, max_u, tokens, lengths, scores, stable_len);
  hipLaunchKernelGGL(rnnt_beam_stream_partial_kernel<false>, dim3(n), dim3(64), 0, stream, a);
  return EA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------ C ABI: the streamed search, biased
extern "C" long ea_rnnt_frame_beam_stream_bias_state_bytes(int max_frames, int beam) {
  if (max_frames < 1 || beam < 1 || beam > kMaxBeam) return 0;
  return rnnt_state_words<true>(max_frames, beam) * 4L;
}

extern "C" int ea_rnnt_frame_beam_stream_bias_reset(void* state, const int* slots, int n, int max_streams, int max_frames, int beam,
                                                    hipStream_t stream) {
  if (n <= 0) return 0;
  if (!state || !slots || max_streams < 1 || max_frames < 1 || beam < 1 || beam > kMaxBeam) return -2;
  hipLaunchKernelGGL(rnnt_beam_stream_reset_kernel<true>, dim3(n), dim3(256), 0, stream, state, slots, max_streams, max_frames, beam);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_rnnt_frame_beam_stream_bias_step(const float* logits, long ld, const float* lm_rows, long ld_lm, int lm_no_blank,
                                                   const int* slot_idx, const int* n_new, int j, int n, void* state, int* parent,
                                                   int* token, void* keep, const int* cg_nodes, const int* cg_edges,
                                                   const int* cg_root, int cg_n_nodes, int cg_n_edges, int max_streams,
                                                   int max_frames, int V, int beam, int K, int blank, int eos, float temperature,
                                                   float lm_weight, hipStream_t stream) {
  if (n <= 0) return 0;
  BiasStreamSelArgs s;
  if (!logits || !slot_idx || !n_new || !state || !parent || !token || !keep || j < 0 || max_streams < 1 || max_frames < 1 ||
      rnnt_step_args_bad(ld, lm_rows, ld_lm, lm_no_blank, V, beam, K, blank, eos, temperature) ||
      !cg_tables(s.g, cg_nodes, cg_edges, cg_root, cg_n_nodes, cg_n_edges, V))
    return -2;
  StreamRowArgs r;
  r.p = rnnt_row_params(lm_rows, lm_no_blank, V, K, blank, eos, temperature, lm_weight);
  r.logits = logits; r.ld = ld; r.lm_rows = lm_rows; r.ld_lm = ld_lm;
  r.slot_idx = slot_idx; r.n_new = n_new; r.state = state;
  r.max_streams = max_streams; r.max_frames = max_frames; r.beam = beam; r.j = j;
  hipLaunchKernelGGL(rnnt_beam_stream_row_kernel<true>, dim3(n * beam), dim3(256), 0, stream, r);
  s.slot_idx = slot_idx; s.n_new = n_new; s.state = state; s.parent = parent; s.token = token; s.keep = (uint8_t*)keep;
  s.max_streams = max_streams; s.max_frames = max_frames; s.beam = beam; s.K = K; s.blank = blank; s.j = j;
  hipLaunchKernelGGL(rnnt_beam_stream_select_kernel<true>, dim3(n), dim3(256), 0, stream, s);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_rnnt_frame_beam_stream_bias_finish(const void* state, const int* slots, int n, int max_streams, int max_frames,
                                                     int beam, const int* cg_nodes, int cg_n_nodes, int nbest, int pad,
                                                     int normalize, int max_u, int* tokens, int* lengths, float* scores, int* nhyp,
                                                     hipStream_t stream) {
  if (n <= 0) return 0;
  if (rnnt_read_args_bad(state, slots, max_streams, max_frames, beam, max_u, tokens, lengths, scores, nhyp) || nbest < 1 ||
      nbest > beam || !cg_nodes || cg_n_nodes < 1)
    return -2;
  BiasStreamReadArgs a;
  rnnt_read_args(a, state, slots, max_streams, max_frames, beam, nbest, pad, normalize, max_u, tokens, lengths, scores, nhyp);
  a.g = cg_nodes_only(cg_nodes, cg_n_nodes);
  hipLaunchKernelGGL(rnnt_beam_stream_finish_kernel<true>, dim3(n), dim3(64), 0, stream, a);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_rnnt_frame_beam_stream_bias_partial(const void* state, const int* slots, int n, int max_streams, int max_frames,
                                                      int beam, int pad, int max_u, int* tokens, int* lengths, float* scores,
                                                      int* stable_len, hipStream_t stream) {
  if (n <= 0) return 0;
  if (rnnt_read_args_bad(state, slots, max_streams, max_frames, beam, max_u, tokens, lengths, scores, stable_len)) return -2;
  StreamReadArgs a;
  rnnt_read_args(a, state, slots, max_streams, max_frames, beam, 1, pad, 0, max_u, tokens, lengths, scores, stable_len);
  hipLaunchKernelGGL(rnnt_beam_stream_partial_kernel<true>, dim3(n), dim3(64), 0, stream, a);
  return EA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------ C ABI: time stamps
extern "C" long ea_rnnt_frame_beam_times_workspace_bytes(int B, int T, int beam) {
  if (B <= 0 || T < 0 || beam < 1 || beam > kMaxBeam) return 0;
  return (long)B * rnnt_times_words(T, beam) * 4L;
}

extern "C" int ea_rnnt_frame_beam_times_step(const float* logits, long ld, const float* lm_rows, long ld_lm, int lm_no_blank,
                                             const int* in_len, void* workspace, void* times_workspace, int* parent, int* token,
                                             void* keep, const int* cg_nodes, const int* cg_edges, const int* cg_root,
                                             int cg_n_nodes, int cg_n_edges, int B, int T, int V, int beam, int K, int blank, int eos,
                                             float temperature, float lm_weight, int t, hipStream_t stream) {
  if (B <= 0) return 0;
  TimesSelArgs s;
  if (!logits || !in_len || !workspace || !times_workspace || !parent || !token || !keep || T < 1 || t < 0 || t >= T ||
      rnnt_step_args_bad(ld, lm_rows, ld_lm, lm_no_blank, V, beam, K, blank, eos, temperature) ||
      (cg_nodes && !cg_tables(s.g, cg_nodes, cg_edges, cg_root, cg_n_nodes, cg_n_edges, V)))
    return -2;
  RowArgs r;  // the row phase knows nothing of times or the graph: the twin's row kernel
  r.p = rnnt_row_params(lm_rows, lm_no_blank, V, K, blank, eos, temperature, lm_weight);
  r.logits = logits; r.ld = ld; r.lm_rows = lm_rows; r.ld_lm = ld_lm;
  r.in_len = in_len; r.ws = workspace;
  r.T = T; r.beam = beam; r.t = t;
  hipLaunchKernelGGL(rnnt_beam_row_kernel, dim3(B * beam), dim3(256), 0, stream, r);
  s.in_len = in_len; s.ws = workspace; s.parent = parent; s.token = token; s.keep = (uint8_t*)keep;
  s.T = T; s.beam = beam; s.K = K; s.blank = blank; s.t = t;
  s.tws = times_workspace;
  if (cg_nodes)
    hipLaunchKernelGGL((rnnt_beam_select_kernel<true, true>), dim3(B), dim3(256), 0, stream, s);
  else
    hipLaunchKernelGGL((rnnt_beam_select_kernel<false, true>), dim3(B), dim3(256), 0, stream, s);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_rnnt_frame_beam_times_finish(void* workspace, const void* times_workspace, const int* cg_nodes, int cg_n_nodes,
                                               int B, int T, int beam, int nbest, int pad, int normalize, int* tokens, int* lengths,
                                               float* scores, int* nhyp, int* times, float* vscores, hipStream_t stream) {
  if (B <= 0) return 0;
  if (!workspace || !times_workspace || !tokens || !lengths || !scores || !nhyp || !times || !vscores || T < 0 || beam < 1 ||
      beam > kMaxBeam || nbest < 1 || nbest > beam || (cg_nodes && cg_n_nodes < 1))
    return -2;
  TimesFinishArgs a;
  a.ws = workspace; a.tws = times_workspace;
  a.T = T; a.beam = beam; a.nbest = nbest; a.pad = pad; a.normalize = normalize;
  a.tokens = tokens; a.lengths = lengths; a.scores = scores; a.nhyp = nhyp; a.times = times; a.vscores = vscores;
  if (cg_nodes) {
    a.g = cg_nodes_only(cg_nodes, cg_n_nodes);
    hipLaunchKernelGGL(rnnt_beam_times_finish_kernel<true>, dim3(B), dim3(64), 0, stream, a);
  } else {
    a.g = CgTables{};
    hipLaunchKernelGGL(rnnt_beam_times_finish_kernel<false>, dim3(B), dim3(64), 0, stream, a);
  }
  return EA_CHECK_LAUNCH();
}

extern "C" long ea_rnnt_frame_beam_stream_times_state_bytes(int max_frames, int beam) {
  if (max_frames < 1 || beam < 1 || beam > kMaxBeam) return 0;
  return rnnt_times_words(max_frames, beam) * 4L;
}

extern "C" int ea_rnnt_frame_beam_stream_times_reset(void* state, void* times_state, const int* slots, int n, int biased,
                                                     int max_streams, int max_frames, int beam, hipStream_t stream) {
  if (n <= 0) return 0;
  if (!state || !times_state || !slots || max_streams < 1 || max_frames < 1 || beam < 1 || beam > kMaxBeam) return -2;
  if (biased)
    hipLaunchKernelGGL((rnnt_beam_stream_reset_kernel<true, true, void*>), dim3(n), dim3(256), 0, stream, state, slots, max_streams,
                       max_frames, beam, times_state);
  else
    hipLaunchKernelGGL((rnnt_beam_stream_reset_kernel<false, true, void*>), dim3(n), dim3(256), 0, stream, state, slots, max_streams,
                       max_frames, beam, times_state);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_rnnt_frame_beam_stream_times_step(const float* logits, long ld, const float* lm_rows, long ld_lm, int lm_no_blank,
                                                    const int* slot_idx, const int* n_new, int j, int n, void* state,
                                                    void* times_state, int* parent, int* token, void* keep, const int* cg_nodes,
                                                    const int* cg_edges, const int* cg_root, int cg_n_nodes, int cg_n_edges,
                                                    int max_streams, int max_frames, int V, int beam, int K, int blank, int eos,
                                                    float temperature, float lm_weight, hipStream_t stream) {
  if (n <= 0) return 0;
  TimesStreamSelArgs s;
  if (!logits || !slot_idx || !n_new || !state || !times_state || !parent || !token || !keep || j < 0 || max_streams < 1 ||
      max_frames < 1 || rnnt_step_args_bad(ld, lm_rows, ld_lm, lm_no_blank, V, beam, K, blank, eos, temperature) ||
      (cg_nodes && !cg_tables(s.g, cg_nodes, cg_edges, cg_root, cg_n_nodes, cg_n_edges, V)))
    return -2;
  StreamRowArgs r;
  r.p = rnnt_row_params(lm_rows, lm_no_blank, V, K, blank, eos, temperature, lm_weight);
  r.logits = logits; r.ld = ld; r.lm_rows = lm_rows; r.ld_lm = ld_lm;
  r.slot_idx = slot_idx; r.n_new = n_new; r.state = state;
  r.max_streams = max_streams; r.max_frames = max_frames; r.beam = beam; r.j = j;
  s.slot_idx = slot_idx; s.n_new = n_new; s.state = state; s.parent = parent; s.token = token; s.keep = (uint8_t*)keep;
  s.max_streams = max_streams; s.max_frames = max_frames; s.beam = beam; s.K = K; s.blank = blank; s.j = j;
  s.tws = times_state;
  if (cg_nodes) {
    hipLaunchKernelGGL(rnnt_beam_stream_row_kernel<true>, dim3(n * beam), dim3(256), 0, stream, r);
    hipLaunchKernelGGL((rnnt_beam_stream_select_kernel<true, true>), dim3(n), dim3(256), 0, stream, s);
  } else {
    hipLaunchKernelGGL(rnnt_beam_stream_row_kernel<false>, dim3(n * beam), dim3(256), 0, stream, r);
    hipLaunchKernelGGL((rnnt_beam_stream_select_kernel<false, true>), dim3(n), dim3(256), 0, stream, s);
  }
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_rnnt_frame_beam_stream_times_finish(const void* state, const void* times_state, const int* slots, int n,
                                                      int max_streams, int max_frames, int beam, const int* cg_nodes, int cg_n_nodes,
                                                      int nbest, int pad, int normalize, int max_u, int* tokens, int* lengths,
                                                      float* scores, int* nhyp, int* times, float* vscores, hipStream_t stream) {
  if (n <= 0) return 0;
  if (rnnt_read_args_bad(state, slots, max_streams, max_frames, beam, max_u, tokens, lengths, scores, nhyp) || !times_state || !times ||
      !vscores || nbest < 1 || nbest > beam || (cg_nodes && cg_n_nodes < 1))
    return -2;
  TimesStreamReadArgs a;
  rnnt_read_args(a, state, slots, max_streams, max_frames, beam, nbest, pad, normalize, max_u, tokens, lengths, scores, nhyp);
  a.tws = times_state; a.times = times; a.vscores = vscores;
  if (cg_nodes) {
    a.g = cg_nodes_only(cg_nodes, cg_n_nodes);
    hipLaunchKernelGGL(rnnt_beam_stream_times_finish_kernel<true>, dim3(n), dim3(64), 0, stream, a);
  } else {
    a.g = CgTables{};
    hipLaunchKernelGGL(rnnt_beam_stream_times_finish_kernel<false>, dim3(n), dim3(64), 0, stream, a);
  }
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_rnnt_frame_beam_stream_endpoint(const void* state, const void* times_state, const int* slots, int n, int biased,
                                                  int max_streams, int max_frames, int beam, int silence_frames, int empty_frames,
                                                  int segment_frames, int* out, hipStream_t stream) {
  if (n <= 0) return 0;
  if (!state || !times_state || !slots || !out || max_streams < 1 || max_frames < 1 || beam < 1 || beam > kMaxBeam) return -2;
  StreamEndpointArgs a;
  a.state = state; a.tws = times_state; a.slots = slots;
  a.max_streams = max_streams; a.max_frames = max_frames; a.beam = beam;
  a.silence_frames = silence_frames; a.empty_frames = empty_frames; a.segment_frames = segment_frames;
  a.out = out;
  if (biased)
    hipLaunchKernelGGL(rnnt_beam_stream_endpoint_kernel<true>, dim3(n), dim3(64), 0, stream, a);
  else
    hipLaunchKernelGGL(rnnt_beam_stream_endpoint_kernel<false>, dim3(n), dim3(64), 0, stream, a);
  return EA_CHECK_LAUNCH();
}
