// Lexicon-constrained CTC prefix beam search with shallow fusion of a word n-gram LM (ARPA), for gfx950 — the search the
// reference gets from Flashlight's KenLM lexicon decoder (espresso/tools/ctc_decoder.py:24-71), built here on the prefix
// beam of ctc_beam.hip: the same candidates (K best non-blank tokens per frame), stays and extensions of every hypothesis,
// merging of equal token sequences only, and the same tie rules.
//
// Scoring contract.  A hypothesis y is completed words w_1..w_m and a partial word p (a node of the lexicon trie):
//   score(y) = log(p_b + p_nb) + alpha * (L(y) + S(p)) + beta * m + gamma * |y|
// with L(y) = sum ln P(w_i | w_{i-n+1..i-1}) (<s> as the sentence-start context) and S(p) = max ln P_1(w) over the lexicon
// words below p (S(root) = 0).  The LM part is kept as a running sum of increments:
//   a token moves p down the trie:  alpha * (S(child) - S(node));
//   a word is completed:            alpha * (ln P(w | ctx) - S(node)) + beta;
//   at the end:                     the pending word is completed, then alpha * ln P(</s> | ctx).
// A word ends on <space> (space mode, `space` >= 0) or before a token that starts a word (word-start mode, `word_start`
// flags).  Closed vocabulary: leaving the trie, ending a word on a node that is no word, an empty word, and a pending
// non-word at the end score -inf.  Prefixes merge only when their token sequences are equal, so the LM state is a function
// of the prefix.
//
// ARPA tables (host loader below): a sorted-array trie.  Order 1 is indexed by word
// id; every order k >= 2 holds its records sorted by (record of the (k-1)-gram context, word id).  A record of order k < n
// carries a child range into order k + 1.  ln P(w | h) is the standard backoff: the longest suffix h' of h with (h', w)
// present, plus the backoff weights of the longer suffixes (0 where a suffix is absent).  Every lookup is a chain of binary
// searches over these arrays: dependent, latency-bound loads.
//
// The search (ctc_lexicon_beam_kernel): one 256-thread workgroup per utterance walks every frame in one launch and
// finishes in the same launch.  The beam state (with trie node, word context and LM sum per slot) lives in LDS; the
// per-utterance prefix table and its (parent, token) hash are in the workspace, as in ctc_beam.hip.  Per frame the n-gram
// lookup of a slot's pending word is done once, by one lane per slot, and only if a candidate token ends a word; the trie
// step of every extension runs on its own lane.
//
// The streamed search (ea_ctc_lexicon_stream_*): the same frames, a piece at a time.  What the kernel above has live between
// two frames is kept per stream slot in a caller-allocated buffer; a step loads a slot's beam into LDS, runs lex_frame over
// the new frames and stores it back.  The frame, the initial state and the finish are the functions the offline kernel is
// made of (lex_frame, lex_init, lex_finish), so both searches return the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "ctc_beam_common.h"
#include "espresso_amd.h"
#include "ngram_common.h"

namespace {

constexpr int kLexMaxBeam = 64;
constexpr int kLexMaxK = 64;
constexpr int kLexMaxCand = kLexMaxBeam * (kLexMaxK + 1);
constexpr int kLexRowLds = 5120;

__global__ __launch_bounds__(256) void ngram_score_kernel(const NgramDev m, const int* ctx, const int* words, int N, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int W = m.order - 1;
  const int* h = ctx + (long)i * W;
  const int L = ctx_len(h, W);
  out[i] = ng_logp(m, h + W - L, L, words[i]);
}

// ------------------------------------------------------------------------------------------------ ARPA parser (host)
struct ArpaError {
  std::string msg;
};

[[noreturn]] void arpa_fail(long line, const std::string& what) {
  char buf[64];
  snprintf(buf, sizeof(buf), "line %ld: ", line);
  throw ArpaError{line > 0 ? buf + what : what};
}

bool is_space(char c) { return c == ' ' || c == '\t' || c == '\r'; }

void split_fields(const char* s, const char* e, std::vector<std::pair<const char*, const char*>>& out) {
  out.clear();
  while (s < e) {
    while (s < e && is_space(*s)) ++s;
    const char* b = s;
    while (s < e && !is_space(*s)) ++s;
    if (s > b) out.emplace_back(b, s);
  }
}

double parse_num(std::pair<const char*, const char*> f, long line) {
  std::string t(f.first, f.second);
  char* end = nullptr;
  const double v = strtod(t.c_str(), &end);
  if (t.empty() || *end) arpa_fail(line, "'" + t + "' is not a number");
  return v;
}

void arpa_parse(const std::string& text, NgramLM& lm) {
  constexpr double kLn10 = 2.302585092994045684;
  std::vector<std::pair<const char*, const char*>> f;
  std::unordered_map<std::string, int> ids;
  const char* p = text.data();
  const char* const end = p + text.size();
  long line = 0;
  auto next_line = [&](const char*& b, const char*& e) {
    if (p >= end) return false;
    b = p;
    e = (const char*)memchr(p, '\n', end - p);
    if (!e) e = end;
    p = e < end ? e + 1 : end;
    ++line;
    while (e > b && is_space(e[-1])) --e;
    while (b < e && is_space(*b)) ++b;
    return true;
  };
  const char *b, *e;
  bool found = false;
  while (next_line(b, e))
    if (std::string(b, e) == "\\data\\") { found = true; break; }
  if (!found) arpa_fail(0, "no \\data\\ header");
  // ngram k=count lines
  long data_line = line;
  while (next_line(b, e)) {
    if (b == e) continue;
    std::string s(b, e);
    if (s.rfind("ngram ", 0) != 0) { p = b; --line; break; }
    const size_t eq = s.find('=');
    if (eq == std::string::npos) arpa_fail(line, "expected 'ngram N=count'");
    const int k = atoi(s.c_str() + 6);
    const long c = atol(s.c_str() + eq + 1);
    if (k < 1) arpa_fail(line, "bad n-gram order in '" + s + "'");
    if (k > kMaxOrder) arpa_fail(line, "order " + std::to_string(k) + " exceeds the supported maximum of 6");
    if (k != lm.order + 1) arpa_fail(line, "n-gram counts must be listed for orders 1, 2, ... in turn");
    if (c < 1 || c >= (1L << 31) - 1) arpa_fail(line, "bad count in '" + s + "'");
    lm.order = k;
    lm.counts[k] = c;
  }
  if (lm.order == 0) arpa_fail(data_line, "\\data\\ lists no n-gram counts");
  for (int k = 1; k <= lm.order; ++k) {
    const std::string head = "\\" + std::to_string(k) + "-grams:";
    while (next_line(b, e) && b == e) {}
    if (std::string(b, e) != head) arpa_fail(line, "expected '" + head + "'");
    const long head_line = line, n = lm.counts[k];
    std::vector<int> words;  // k per record, in file order
    std::vector<int> lines;
    std::vector<float> lp, bw;
    words.reserve(n * k);
    lp.reserve(n);
    bw.reserve(n);
    if (k > 1) lines.reserve(n);
    while (p < end) {
      const char* save = p;
      const long save_line = line;
      next_line(b, e);
      if (b == e) break;
      if (*b == '\\') { p = save; line = save_line; break; }
      split_fields(b, e, f);
      const int nf = (int)f.size();
      if (nf != k + 1 && !(nf == k + 2 && k < lm.order))
        arpa_fail(line, "a " + std::to_string(k) + "-gram line has " + std::to_string(nf) + " fields, expected " +
                            std::to_string(k + 1) + (k < lm.order ? " or " + std::to_string(k + 2) : std::string()));
      if ((long)lp.size() >= n) arpa_fail(line, "more " + std::to_string(k) + "-grams than the " + std::to_string(n) + " \\data\\ declares");
      lp.push_back((float)(parse_num(f[0], line) * kLn10));
      bw.push_back(nf == k + 2 ? (float)(parse_num(f[k + 1], line) * kLn10) : 0.f);
      for (int i = 0; i < k; ++i) {
        std::string wd(f[1 + i].first, f[1 + i].second);
        if (k == 1) {
          if (!ids.emplace(wd, (int)lm.vocab.size()).second) arpa_fail(line, "unigram '" + wd + "' listed twice");
          lm.vocab.push_back(wd);
          words.push_back((int)lm.vocab.size() - 1);
        } else {
          auto it = ids.find(wd);
          if (it == ids.end()) arpa_fail(line, "word '" + wd + "' is not a unigram");
          words.push_back(it->second);
        }
      }
      if (k > 1) lines.push_back((int)line);
    }
    if ((long)lp.size() != n)
      arpa_fail(head_line, head + " has " + std::to_string(lp.size()) + " entries, \\data\\ declares " + std::to_string(n));
    if (k == 1) {
      lm.logp[1] = std::move(lp);
      lm.bow[1] = std::move(bw);
      continue;
    }
    // parent record (the (k-1)-gram context) of every k-gram, then sort by (parent, word)
    const int n1 = (int)lm.counts[1];
    const int* cp[kMaxOrder + 1] = {};
    const int* wp[kMaxOrder + 1] = {};
    for (int j = 1; j < k; ++j) { cp[j] = lm.child[j].data(); wp[j] = lm.word[j].data(); }
    std::vector<std::pair<unsigned long long, int>> key(n);
    for (long i = 0; i < n; ++i) {
      const int* t = &words[i * k];
      int r = 0;
      for (int j = 0; j < k - 1 && r >= 0; ++j) r = ng_find(cp, wp, n1, j, r, t[j]);
      if (r < 0) {
        std::string ctx;
        for (int j = 0; j < k - 1; ++j) ctx += (j ? " " : "") + lm.vocab[t[j]];
        arpa_fail(lines[i], std::to_string(k) + "-gram context '" + ctx + "' is not a " + std::to_string(k - 1) + "-gram");
      }
      key[i] = {((unsigned long long)r << 32) | (unsigned)t[k - 1], (int)i};
    }
    std::sort(key.begin(), key.end());
    for (long i = 1; i < n; ++i)
      if (key[i].first == key[i - 1].first)
        arpa_fail(lines[key[i].second], std::to_string(k) + "-gram listed twice (first on line " +
                                           std::to_string(lines[key[i - 1].second]) + ")");
    lm.logp[k].resize(n);
    lm.bow[k].resize(n);
    lm.word[k].resize(n);
    lm.parent[k].resize(n);
    for (long i = 0; i < n; ++i) {
      const int src = key[i].second;
      lm.logp[k][i] = lp[src];
      lm.bow[k][i] = bw[src];
      lm.word[k][i] = words[(long)src * k + k - 1];
      lm.parent[k][i] = (int)(key[i].first >> 32);
    }
    std::vector<int>& ch = lm.child[k - 1];
    ch.assign(lm.counts[k - 1] + 1, 0);
    for (long i = 0; i < n; ++i) ch[lm.parent[k][i] + 1]++;
    for (long i = 0; i < lm.counts[k - 1]; ++i) ch[i + 1] += ch[i];
  }
  while (next_line(b, e) && b == e) {}
  if (std::string(b, e) != "\\end\\") arpa_fail(line, "expected '\\end\\'");
  auto id = [&](const char* w) { auto it = ids.find(w); return it == ids.end() ? -1 : it->second; };
  lm.unk = id("<unk>");
  lm.bos = id("<s>");
  lm.eos = id("</s>");
  if (lm.bos < 0 || lm.eos < 0) arpa_fail(0, "the ARPA file has no <s> or no </s> unigram");
}

}  // namespace

namespace {

// ------------------------------------------------------------------------------------------------ the search
struct LexDev {  // the lexicon trie in CSR form (node 0 = root): children of n are tok/child[off[n] .. off[n + 1]), tok sorted
  const int *off, *tok, *child, *word;  // word: LM word id of the node, -1 if no word ends there
  const float* smear;                   // S(node), S(root) = 0
  const uint8_t* word_start;            // [V] word-start mode: 1 = the token starts a word; NULL in space mode
  int space;                            // space mode: the <space> token, else -1
};

__device__ __forceinline__ int lex_child(const LexDev& x, int node, int c) {
  int lo = x.off[node];
  const int end = x.off[node + 1];
  int hi = end;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (x.tok[mid] < c) lo = mid + 1; else hi = mid;
  }
  return (lo < end && x.tok[lo] == c) ? x.child[lo] : -1;
}

// per utterance: hash table (parent node, token) -> node and the prefix table of 1 + T * beam nodes, as in ctc_beam.hip
struct LexWs {
  unsigned long long* tab_key;
  int *tab_val, *node_par, *node_tok;
  int cap, tsize;
};
__host__ __device__ __forceinline__ long lex_ws_cap(int T, int beam) { return 1L + (long)T * beam; }
__host__ __device__ __forceinline__ long lex_ws_tsize(int T, int beam) {
  long n = 64;
  while (n < 2 * lex_ws_cap(T, beam)) n <<= 1;
  return n;
}
__host__ __device__ __forceinline__ long lex_ws_words(int T, int beam) {
  return (3 * lex_ws_tsize(T, beam) + 2 * lex_ws_cap(T, beam) + 1) & ~1L;
}
__device__ __forceinline__ LexWs lex_ws_at(int* base, int T, int beam) {  // the tables of T frames laid out from `base`
  LexWs w;
  w.cap = (int)lex_ws_cap(T, beam);
  w.tsize = (int)lex_ws_tsize(T, beam);
  w.tab_key = (unsigned long long*)base;
  w.tab_val = base + 2L * w.tsize;
  w.node_par = w.tab_val + w.tsize;
  w.node_tok = w.node_par + w.cap;
  return w;
}
__device__ __forceinline__ LexWs lex_ws(void* ws, int b, int T, int beam) {
  return lex_ws_at((int*)ws + (long)b * lex_ws_words(T, beam), T, beam);
}

struct LexParams {  // what every frame and the finish need, the same for the offline and the streamed search
  NgramDev lm; LexDev lex;
  int V, beam, K, blank, W /* context width = order - 1 */;
  float alpha, beta, gamma;
};

struct LexArgs {  // the offline search
  const void* x; long ld; const int* in_len; void* ws;
  LexParams p;
  int T, nbest, pad;
  int *tokens, *lengths; float* scores; int* nhyp;
};

// the increment of completing the word at trie node `node` after context h (W words, front-padded with -1); -inf when
// the node is the root (an empty word) or no word
__device__ float word_end(const LexParams& a, int node, const int* h, int& w) {
  w = node > 0 ? a.lex.word[node] : -1;
  if (w < 0) return -INFINITY;
  const int L = ctx_len(h, a.W);
  return a.alpha * (ng_logp(a.lm, h + a.W - L, L, w) - a.lex.smear[node]) + a.beta;
}

// The beam between two frames: everything the search keeps besides the prefix table.  The offline kernel holds it in LDS
// from its first frame to its finish; the streamed search (below) loads and stores it around the frames of one call.
struct LexBeam {
  float pb[kLexMaxBeam], pnb[kLexMaxBeam], lm[kLexMaxBeam];
  int len[kLexMaxBeam], last[kLexMaxBeam], node[kLexMaxBeam], pnode[kLexMaxBeam], tn[kLexMaxBeam];
  int ctx[kLexMaxBeam][kMaxCtx];
  float fin[kLexMaxBeam];  // scratch of lex_finish
  int nhyp, nnodes;
};

struct LexLds : LexBeam {  // + the scratch of one frame
  uint64_t key[kLexMaxCand];
  float nlm[kLexMaxCand];  // LM sum of extension i
  int ntn[kLexMaxCand];    // trie node of extension i
  SelectScratch sel;
  float wend[kLexMaxBeam];  // increment of ending the slot's pending word this frame
  int wid[kLexMaxBeam];     // that word (-1: none / nothing pending)
  int lrank[kLexMaxBeam], msrc[kLexMaxBeam];
  unsigned long long merged[kLexMaxBeam];
  int ctok[kLexMaxK], cunsorted[kLexMaxK], cbound[kLexMaxK];
  float cx[kLexMaxK];
  int sel_idx[kLexMaxBeam];
  float row[kLexRowLds];
  int ncand, nsel, nfresh, anybound;
};

// the state before frame 0: the empty prefix with <s> as its context in slot 0, node 0 in an empty table.  The caller
// fences and synchronises.
__device__ __forceinline__ void lex_init(LexBeam& s, const LexWs& w, int bos, int W) {
  const int tid = threadIdx.x;
  for (int i = tid; i < w.tsize; i += 256) w.tab_key[i] = 0ull;
  if (tid == 0) {
    s.pb[0] = 0.f; s.pnb[0] = -INFINITY; s.lm[0] = 0.f;
    s.len[0] = 0; s.last[0] = -1; s.node[0] = 0; s.pnode[0] = -1; s.tn[0] = 0;
    for (int i = 0; i < W; ++i) s.ctx[0][i] = i == W - 1 ? bos : -1;
    s.nhyp = 1; s.nnodes = 1;
    w.node_par[0] = -1; w.node_tok[0] = -1;
  }
}

// One frame (the log-prob row xr) of the search over the beam in `s` and the prefix table `w`; all 256 threads call, after a
// barrier that follows the last write of the beam, and leave through one.
template <typename TX>
__device__ __forceinline__ void lex_frame(LexLds& s, const LexParams& a, const LexWs& w, const TX* xr) {
  const int tid = threadIdx.x;
  const int beam = a.beam, K = a.K, K1 = a.K + 1, W = a.W;
  const bool space_mode = a.lex.space >= 0;
  for (int v = tid; v < min(a.V, kLexRowLds); v += 256) s.row[v] = ldx(xr, v);
  __syncthreads();
  auto xv = [&](int v) { return v < kLexRowLds ? s.row[v] : ldx(xr, v); };
  const int nh = s.nhyp;
  const int V = a.V, blank = a.blank;

  // 1. top-K non-blank tokens of the frame, in token-id order; which of them end a word
  auto tok_key = [&](int v) -> uint64_t { return v == blank ? 0ull : mk_key(xv(v), v); };
  const uint64_t kth = select_nth(tok_key, V, K, s.sel);
  if (tid == 0) { s.ncand = 0; s.anybound = 0; }
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
    const int bound = a.lex.space >= 0 ? v == a.lex.space : (int)a.lex.word_start[v];
    s.ctok[r] = v;
    s.cx[r] = xv(v);
    s.cbound[r] = bound;
    if (bound) s.anybound = 1;
  }
  if (tid < kLexMaxBeam) s.merged[tid] = 0ull;
  __syncthreads();

  // 2a. stays that absorb an extension (as ctc_beam.hip); the word-end increment of every slot, if a candidate ends words
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
    float inc = -INFINITY;
    int wd = -1;
    if (s.anybound) {
      if (!space_mode && s.tn[tid] == 0) inc = 0.f;  // word-start mode, nothing pending: nothing to end
      else inc = word_end(a, s.tn[tid], s.ctx[tid], wd);
    }
    s.wend[tid] = inc;
    s.wid[tid] = wd;
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
  const int N = nh * K1;
  for (int i = tid; i < N; i += 256) {
    const int j = i / K1, q = i - j * K1;
    uint64_t key = 0ull;
    if (q == 0) {
      key = mk_key(lae(lae(s.pb[j], s.pnb[j]) + xb, stay_pnb(j)) + s.lm[j] + a.gamma * (float)s.len[j], i);
    } else if (!((s.merged[j] >> (q - 1)) & 1ull)) {
      const int r = q - 1, c = s.ctok[r];
      float lm = s.lm[j];  // -inf exactly when the slot's trie node is -1
      int tn = 0;
      if (space_mode && s.cbound[r]) {  // <space>: end the pending word
        lm += s.wend[j];
      } else {
        int node = s.tn[j];
        if (s.cbound[r]) { lm += s.wend[j]; node = 0; }  // word-start mode: end the pending word, c starts one
        tn = lm == -INFINITY ? -1 : lex_child(a.lex, node, c);
        lm = tn < 0 ? -INFINITY : lm + a.alpha * (a.lex.smear[tn] - a.lex.smear[node]);
      }
      s.nlm[i] = lm;
      s.ntn[i] = tn;
      key = mk_key(ext_pnb(j, r) + lm + a.gamma * (float)(s.len[j] + 1), i);
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
  int n_len = 0, n_last = -1, n_node = 0, n_pnode = -1, n_tn = 0, slot = 0, fresh = 0, tslot = -1, n_done = -1;
  int n_ctx[kMaxCtx];
  if (tid < ns) {
    const int i = s.sel_idx[tid];
    const uint64_t k = s.key[i];
    for (int m = 0; m < ns; ++m) slot += s.key[s.sel_idx[m]] > k;
    const int j = i / K1, q = i - j * K1;
    for (int m = 0; m < W; ++m) n_ctx[m] = s.ctx[j][m];
    if (q == 0) {
      n_pb = lae(s.pb[j], s.pnb[j]) + xb; n_pnb = stay_pnb(j); n_lm = s.lm[j];
      n_len = s.len[j]; n_last = s.last[j]; n_node = s.node[j]; n_pnode = s.pnode[j]; n_tn = s.tn[j];
    } else {
      const int r = q - 1;
      n_pb = -INFINITY; n_pnb = ext_pnb(j, r); n_lm = s.nlm[i]; n_tn = s.ntn[i];
      n_len = s.len[j] + 1; n_last = s.ctok[r]; n_pnode = s.node[j];
      if (s.cbound[r]) n_done = s.wid[j];
      const unsigned long long key = ((unsigned long long)(n_pnode + 1) << 32) | (uint32_t)n_last;
      const uint32_t mask = (uint32_t)w.tsize - 1u;
      for (uint32_t h = tab_hash(key) & mask;; h = (h + 1) & mask) {
        const unsigned long long cur = ld_l2(w.tab_key + h);
        if (cur == key) { n_node = ld_l2(w.tab_val + h); break; }
        if (cur == 0ull && atomicCAS(w.tab_key + h, 0ull, key) == 0ull) { fresh = 1; tslot = (int)h; break; }
      }
    }
    if (n_done >= 0 && W > 0) {
      for (int m = 0; m + 1 < W; ++m) n_ctx[m] = n_ctx[m + 1];
      n_ctx[W - 1] = n_done;
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
  }
  __syncthreads();
  if (tid < ns) {
    s.pb[slot] = n_pb; s.pnb[slot] = n_pnb; s.lm[slot] = n_lm;
    s.len[slot] = n_len; s.last[slot] = n_last; s.node[slot] = n_node; s.pnode[slot] = n_pnode; s.tn[slot] = n_tn;
    for (int m = 0; m < W; ++m) s.ctx[slot][m] = n_ctx[m];
  }
  if (tid == 0) { s.nhyp = ns; s.nnodes += s.nfresh; }
  __threadfence();  // this frame's table entries, before the next frame's L2 reads
  __syncthreads();
}

// The finish: end the pending word, add ln P(</s> | ctx); the nbest best finite hypotheses, sorted, backtracked into
// tokens [nbest][max_u] (pad-filled), lengths / scores [nbest] and *nhyp of this utterance.  Reads the beam, changes only
// s.fin.  has_frames false (an empty utterance) returns no hypothesis.
__device__ __forceinline__ void lex_finish(LexBeam& s, const LexParams& a, const LexWs& w, bool has_frames, int nbest, int pad,
                                           int max_u, int* tokens, int* lengths, float* scores, int* nhyp) {
  const int tid = threadIdx.x, W = a.W;
  const int nh = s.nhyp;
  if (tid < nh) {
    float sc = lae(s.pb[tid], s.pnb[tid]) + s.lm[tid] + a.gamma * (float)s.len[tid];
    int h[kMaxCtx];
    for (int m = 0; m < W; ++m) h[m] = s.ctx[tid][m];
    if (s.tn[tid] > 0) {
      int wd;
      sc += word_end(a, s.tn[tid], h, wd);
      if (wd >= 0 && W > 0) {
        for (int m = 0; m + 1 < W; ++m) h[m] = h[m + 1];
        h[W - 1] = wd;
      }
    }
    if (sc != -INFINITY) {
      const int Lh = ctx_len(h, W);
      sc += a.alpha * ng_logp(a.lm, h + W - Lh, Lh, a.lm.eos);
    }
    s.fin[tid] = has_frames ? sc : -INFINITY;
  }
  __syncthreads();
  if (tid < 64) {
    const bool ok = tid < nh && s.fin[tid] != -INFINITY && s.fin[tid] == s.fin[tid];
    const int nfin = __popcll(__ballot(ok));
    if (tid == 0) *nhyp = min(nfin, nbest);
    int rank = nbest;
    if (ok) {
      const float sc = s.fin[tid];
      rank = 0;
      for (int m = 0; m < nh; ++m) rank += s.fin[m] > sc || (s.fin[m] == sc && m < tid);
    }
    if (rank < nbest) {
      int* out = tokens + (long)rank * max_u;
      const int n = min(s.len[tid], max_u);
      for (int u = n; u < max_u; ++u) out[u] = pad;
      int node = s.node[tid];
      for (int u = s.len[tid] - 1; u >= 0 && node > 0; --u) {
        if (u < max_u) out[u] = ld_l2(w.node_tok + node);
        node = ld_l2(w.node_par + node);
      }
      lengths[rank] = n;
      scores[rank] = s.fin[tid];
    }
    for (int r = min(nfin, nbest) + tid; r < nbest; r += 64) {
      int* out = tokens + (long)r * max_u;
      for (int u = 0; u < max_u; ++u) out[u] = pad;
      lengths[r] = 0;
      scores[r] = -INFINITY;
    }
  }
}

template <typename TX>
__global__ __launch_bounds__(256) void ctc_lexicon_beam_kernel(const LexArgs a) {
  __shared__ LexLds s;
  const int b = blockIdx.x;
  const LexWs w = lex_ws(a.ws, b, a.T, a.p.beam);
  const int L = min(a.in_len[b], a.T);
  lex_init(s, w, a.p.lm.bos, a.p.W);
  __threadfence();
  __syncthreads();
  for (int t = 0; t < L; ++t) lex_frame(s, a.p, w, (const TX*)a.x + ((long)b * a.T + t) * a.ld);
  lex_finish(s, a.p, w, L > 0, a.nbest, a.pad, a.T, a.tokens + (long)b * a.nbest * a.T, a.lengths + b * a.nbest,
             a.scores + b * a.nbest, a.nhyp + b);
}

// ------------------------------------------------------------------------------------------------ the streamed search
// State of one stream slot, int32 words: [0] hypotheses in the beam, [1] prefix-table nodes, [2] frames consumed, [3] 0;
// then beam-sized arrays pb, pnb, lm (fp32), len, last, node, pnode, tn and ctx [beam][kMaxCtx]; then, 8-byte aligned, the
// prefix table and its hash sized for max_frames frames (the LexWs layout).  It is what the offline kernel has live between
// two frames, so a step that loads it, runs lex_frame and stores it computes what the offline kernel computes.
__host__ __device__ __forceinline__ long lex_state_head_words(int beam) { return (4L + (8 + kMaxCtx) * (long)beam + 1) & ~1L; }
__host__ __device__ __forceinline__ long lex_state_words(int max_frames, int beam) {
  return lex_state_head_words(beam) + lex_ws_words(max_frames, beam);
}

struct LexSlot {
  int* head;
  LexWs w;
};
__device__ __forceinline__ LexSlot lex_slot(void* state, int slot, int max_frames, int beam) {
  LexSlot q;
  q.head = (int*)state + (long)slot * lex_state_words(max_frames, beam);
  q.w = lex_ws_at(q.head + lex_state_head_words(beam), max_frames, beam);
  return q;
}

// beam <-> state; the caller synchronises
__device__ __forceinline__ void lex_load(LexBeam& s, const int* st, int beam, int W) {
  const int tid = threadIdx.x;
  const int nh = min(max(st[0], 0), beam);
  if (tid < nh) {
    const float* f = (const float*)(st + 4);
    const int* q = st + 4 + 3 * beam;
    s.pb[tid] = f[tid]; s.pnb[tid] = f[beam + tid]; s.lm[tid] = f[2 * beam + tid];
    s.len[tid] = q[tid]; s.last[tid] = q[beam + tid]; s.node[tid] = q[2 * beam + tid]; s.pnode[tid] = q[3 * beam + tid];
    s.tn[tid] = q[4 * beam + tid];
    for (int m = 0; m < W; ++m) s.ctx[tid][m] = q[5 * beam + tid * kMaxCtx + m];
  }
  if (tid == 0) { s.nhyp = nh; s.nnodes = st[1]; }
}
__device__ __forceinline__ void lex_store(int* st, const LexBeam& s, int beam, int W, int frames) {
  const int tid = threadIdx.x;
  if (tid < s.nhyp) {
    float* f = (float*)(st + 4);
    int* q = st + 4 + 3 * beam;
    f[tid] = s.pb[tid]; f[beam + tid] = s.pnb[tid]; f[2 * beam + tid] = s.lm[tid];
    q[tid] = s.len[tid]; q[beam + tid] = s.last[tid]; q[2 * beam + tid] = s.node[tid]; q[3 * beam + tid] = s.pnode[tid];
    q[4 * beam + tid] = s.tn[tid];
    for (int m = 0; m < W; ++m) q[5 * beam + tid * kMaxCtx + m] = s.ctx[tid][m];
  }
  if (tid == 0) { st[0] = s.nhyp; st[1] = s.nnodes; st[2] = frames; st[3] = 0; }
}

__global__ __launch_bounds__(256) void lexicon_stream_reset_kernel(void* state, const int* slots, int max_streams, int max_frames,
                                                                   int beam, int bos, int W) {
  __shared__ LexBeam s;
  const int slot = slots[blockIdx.x];
  if (slot < 0 || slot >= max_streams) return;
  const LexSlot q = lex_slot(state, slot, max_frames, beam);
  lex_init(s, q.w, bos, W);
  __syncthreads();
  lex_store(q.head, s, beam, W, 0);
}

struct LexStreamArgs {
  const void* x; long ld, total_rows;
  const int *slot_idx, *n_new, *row_off;
  void* state;
  LexParams p;
  int max_streams, max_frames;
};

// one workgroup per ready stream: its n_new frames over its slot's state.  An idle entry (n_new 0), one with out-of-range
// values and one that would pass max_frames leave the slot untouched.
template <typename TX>
__global__ __launch_bounds__(256) void ctc_lexicon_stream_step_kernel(const LexStreamArgs a) {
  __shared__ LexLds s;
  const int b = blockIdx.x;
  const int slot = a.slot_idx[b], n = a.n_new[b];
  const long r0 = a.row_off[b];
  if (n <= 0 || slot < 0 || slot >= a.max_streams || r0 < 0 || r0 + n > a.total_rows) return;
  const LexSlot q = lex_slot(a.state, slot, a.max_frames, a.p.beam);
  const int frames = q.head[2];
  if (frames < 0 || frames + n > a.max_frames) return;
  lex_load(s, q.head, a.p.beam, a.p.W);
  __syncthreads();
  for (int t = 0; t < n; ++t) lex_frame(s, a.p, q.w, (const TX*)a.x + (r0 + t) * a.ld);
  lex_store(q.head, s, a.p.beam, a.p.W, frames + n);
}

struct LexReadArgs {
  const void* state; const int* slots;
  LexParams p;
  int max_streams, max_frames, nbest, pad, max_u;
  int *tokens, *lengths; float* scores; int* aux;  // aux: nhyp (finish) / stable_len (partial)
};

// readout of the given slots, as the offline kernel finishes; the state is read only
__global__ __launch_bounds__(256) void ctc_lexicon_stream_finish_kernel(const LexReadArgs a) {
  __shared__ LexBeam s;
  const int b = blockIdx.x, slot = a.slots[b];
  const bool valid = slot >= 0 && slot < a.max_streams;  // no such slot: no hypothesis
  const LexSlot q = lex_slot((void*)a.state, valid ? slot : 0, a.max_frames, a.p.beam);
  if (valid) lex_load(s, q.head, a.p.beam, a.p.W);
  else if (threadIdx.x == 0) s.nhyp = 0;
  __syncthreads();
  lex_finish(s, a.p, q.w, valid && q.head[2] > 0, a.nbest, a.pad, a.max_u, a.tokens + (long)b * a.nbest * a.max_u,
             a.lengths + b * a.nbest, a.scores + b * a.nbest, a.aux + b);
}

// The live hypothesis with the best in-beam score log(pb + pnb) + lm + gamma * len (ties: the lower slot) and the length of
// the longest common prefix of the live hypotheses with a finite score (of all of them when none is finite): the depth of
// their lowest common ancestor in node_par.  Nodes are numbered in creation order, so a parent's id is below its child's:
// lifting the highest node until all are equal ends at that ancestor.  One wave per slot; the state is read only.
__global__ __launch_bounds__(64) void ctc_lexicon_stream_partial_kernel(const LexReadArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, slot = a.slots[b];
  int* out = a.tokens + (long)b * a.max_u;
  const bool valid = slot >= 0 && slot < a.max_streams;
  const int beam = a.p.beam;
  const LexSlot q = lex_slot((void*)a.state, valid ? slot : 0, a.max_frames, beam);
  const int nh = valid ? min(max(q.head[0], 0), beam) : 0;
  float sc = -INFINITY;
  int len = 0, node = 0;
  if (lane < nh) {
    const float* f = (const float*)(q.head + 4);
    const int* qi = q.head + 4 + 3 * beam;
    len = qi[lane];
    node = qi[2 * beam + lane];
    sc = lae(f[lane], f[beam + lane]) + f[2 * beam + lane] + a.p.gamma * (float)len;
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
    for (int u = len - 1; u >= 0 && nd > 0; --u) {
      if (u < a.max_u) out[u] = ld_l2(q.w.node_tok + nd);
      nd = ld_l2(q.w.node_par + nd);
    }
    a.lengths[b] = n;
    a.scores[b] = sc;
  }
  int depth = len, cur = in_set ? node : -1;
  for (int it = 0; it < q.w.cap; ++it) {  // every pass lowers the highest node: fewer than `cap` passes
    int hi = cur;
    for (int o = 32; o > 0; o >>= 1) hi = max(hi, __shfl_xor(hi, o, 64));
    if (hi <= 0 || !__ballot(in_set && cur != hi)) break;  // the root, or every member at the same node
    if (in_set && cur == hi) { cur = cur < q.w.cap ? ld_l2(q.w.node_par + cur) : 0; --depth; }
  }
  if (is_best) a.aux[b] = depth;  // the best hypothesis is a member (or none is finite): its depth is the ancestor's
  if (nh == 0 && lane == 0) {
    for (int u = 0; u < a.max_u; ++u) out[u] = a.pad;
    a.lengths[b] = 0; a.scores[b] = -INFINITY; a.aux[b] = 0;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI: the n-gram LM
extern "C" int ea_ngram_create(const char* path, void* handle_host, char* err_host, long err_cap) {
  auto err = [&](const std::string& m) {
    if (err_host && err_cap > 0) snprintf(err_host, err_cap, "%s", m.c_str());
  };
  *(void**)handle_host = nullptr;
  FILE* fp = fopen(path, "rb");
  if (!fp) { err(std::string("cannot open ") + path); return -1; }
  std::string text;
  char buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) text.append(buf, n);
  fclose(fp);
  auto* lm = new NgramLM();
  try {
    arpa_parse(text, *lm);
  } catch (const ArpaError& e) {
    err(std::string(path) + ": " + e.msg);
    delete lm;
    return -3;
  }
  NgramDev& h = lm->host;
  h.order = lm->order; h.n1 = (int)lm->counts[1]; h.unk = lm->unk; h.bos = lm->bos; h.eos = lm->eos;
  for (int k = 1; k <= lm->order; ++k) {
    h.logp[k] = lm->logp[k].data(); h.bow[k] = lm->bow[k].data(); h.word[k] = lm->word[k].data(); h.child[k] = lm->child[k].data();
  }
  lm->dev = h;
  *(void**)handle_host = lm;
  return 0;
}

extern "C" int ea_ngram_destroy(void* handle) {
  auto* lm = (NgramLM*)handle;
  if (!lm) return 0;
  if (lm->dev_buf) hipFree(lm->dev_buf);
  delete lm;
  return 0;
}

extern "C" int ea_ngram_info(const void* handle, int* meta_host, long* counts_host) {
  const auto* lm = (const NgramLM*)handle;
  if (!lm) return -2;
  meta_host[0] = lm->order; meta_host[1] = lm->unk; meta_host[2] = lm->bos; meta_host[3] = lm->eos;
  for (int k = 1; k <= kMaxOrder; ++k) counts_host[k - 1] = lm->counts[k];
  return 0;
}

extern "C" long ea_ngram_vocab(const void* handle, char* buf_host, long cap) {
  const auto* lm = (const NgramLM*)handle;
  if (!lm) return -2;
  long need = 0;
  for (const auto& w : lm->vocab) need += (long)w.size() + 1;
  if (buf_host && cap >= need) {
    char* o = buf_host;
    for (const auto& w : lm->vocab) { memcpy(o, w.data(), w.size()); o += w.size(); *o++ = '\n'; }
  }
  return need;
}

extern "C" long ea_ngram_records(const void* handle, int order, int* ngrams_host, float* logp_host, float* bow_host) {
  const auto* lm = (const NgramLM*)handle;
  if (!lm || order < 1 || order > lm->order) return -2;
  const long n = lm->counts[order];
  for (long i = 0; i < n; ++i) {
    int r = (int)i;
    for (int k = order; k >= 1; --k) {
      ngrams_host[i * order + k - 1] = k == 1 ? r : lm->word[k][r];
      if (k > 1) r = lm->parent[k][r];
    }
    logp_host[i] = lm->logp[order][i];
    bow_host[i] = lm->bow[order][i];
  }
  return n;
}

extern "C" int ea_ngram_upload(void* handle) {
  auto* lm = (NgramLM*)handle;
  if (!lm) return -2;
  if (lm->dev_buf) return 0;
  std::vector<std::pair<const void*, size_t>> parts;
  for (int k = 1; k <= lm->order; ++k) {
    parts.emplace_back(lm->logp[k].data(), lm->logp[k].size() * 4);
    parts.emplace_back(lm->bow[k].data(), lm->bow[k].size() * 4);
    parts.emplace_back(lm->word[k].data(), lm->word[k].size() * 4);
    parts.emplace_back(lm->child[k].data(), lm->child[k].size() * 4);
  }
  size_t total = 0;
  for (auto& q : parts) total += (q.second + 255) & ~(size_t)255;
  char* base = nullptr;
  if (hipMalloc(&base, total ? total : 256) != hipSuccess) return -1;
  size_t off = 0;
  std::vector<char*> at;
  for (auto& q : parts) {
    at.push_back(base + off);
    if (q.second && hipMemcpy(base + off, q.first, q.second, hipMemcpyHostToDevice) != hipSuccess) { hipFree(base); return -1; }
    off += (q.second + 255) & ~(size_t)255;
  }
  for (int k = 1; k <= lm->order; ++k) {
    lm->dev.logp[k] = (const float*)at[4 * (k - 1)];
    lm->dev.bow[k] = (const float*)at[4 * (k - 1) + 1];
    lm->dev.word[k] = (const int*)at[4 * (k - 1) + 2];
    lm->dev.child[k] = (const int*)at[4 * (k - 1) + 3];
  }
  lm->dev_buf = base;
  return 0;
}

extern "C" int ea_ngram_score_host(const void* handle, const int* ctx_host, const int* words_host, int N, float* out_host) {
  const auto* lm = (const NgramLM*)handle;
  if (!lm || N < 0) return -2;
  const int W = lm->order - 1;
  for (int i = 0; i < N; ++i) {
    const int* h = ctx_host + (long)i * W;
    const int L = ctx_len(h, W);
    out_host[i] = ng_logp(lm->host, h + W - L, L, words_host[i]);
  }
  return 0;
}

extern "C" int ea_ngram_score(const void* handle, const int* ctx, const int* words, int N, float* out, ea_stream_t stream) {
  const auto* lm = (const NgramLM*)handle;
  if (!lm || !lm->dev_buf || N < 0) return -2;
  if (N == 0) return 0;
  hipLaunchKernelGGL(ngram_score_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, lm->dev, ctx, words, N, out);
  return EA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------ C ABI: the search
namespace {
LexParams lex_params(const NgramLM* lm, const int* trie_off, const int* trie_tok, const int* trie_child, const int* trie_word,
                     const float* trie_smear, const void* word_start, int space, int V, int beam, int K, int blank, float lm_weight,
                     float word_score, float ins_bonus) {
  LexParams p;
  p.lm = lm->dev;
  p.lex.off = trie_off; p.lex.tok = trie_tok; p.lex.child = trie_child; p.lex.word = trie_word; p.lex.smear = trie_smear;
  p.lex.word_start = space >= 0 ? nullptr : (const uint8_t*)word_start;
  p.lex.space = space;
  p.V = V; p.beam = beam; p.K = K; p.blank = blank; p.W = lm->order - 1;
  p.alpha = lm_weight; p.beta = word_score; p.gamma = ins_bonus;
  return p;
}
}  // namespace

extern "C" long ea_ctc_lexicon_beam_workspace_bytes(int B, int T, int beam) {
  if (B <= 0 || T < 0 || beam < 1 || beam > kLexMaxBeam) return 0;
  return (long)B * lex_ws_words(T, beam) * 4L;
}

extern "C" int ea_ctc_lexicon_beam_search(const void* x, long ld, int x_bf16, const int* in_len, void* workspace, const void* ngram,
                                          const int* trie_off, const int* trie_tok, const int* trie_child, const int* trie_word,
                                          const float* trie_smear, const void* word_start, int space, int B, int T, int V, int beam,
                                          int K, int blank, float lm_weight, float word_score, float ins_bonus, int nbest, int pad,
                                          int* tokens, int* lengths, float* scores, int* nhyp, ea_stream_t stream) {
  const auto* lm = (const NgramLM*)ngram;
  if (!lm || !lm->dev_buf) return -2;
  if (B <= 0) return 0;
  if (T < 0 || V < 2 || V > 65535 || ld < V || beam < 1 || beam > kLexMaxBeam || K < 1 || K > kLexMaxK || K > V - 1 || blank < 0 ||
      blank >= V || nbest < 1 || nbest > beam || space >= V || (space < 0 && !word_start) || lm->order < 1 ||
      lm->order > kMaxOrder || !trie_off || !trie_word || !trie_smear)
    return -2;
  LexArgs a;
  a.x = x; a.ld = ld; a.in_len = in_len; a.ws = workspace;
  a.p = lex_params(lm, trie_off, trie_tok, trie_child, trie_word, trie_smear, word_start, space, V, beam, K, blank, lm_weight,
                   word_score, ins_bonus);
  a.T = T; a.nbest = nbest; a.pad = pad;
  a.tokens = tokens; a.lengths = lengths; a.scores = scores; a.nhyp = nhyp;
  if (x_bf16)
    hipLaunchKernelGGL(ctc_lexicon_beam_kernel<bf16_t>, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(ctc_lexicon_beam_kernel<float>, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  return EA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------ C ABI: the streamed search
extern "C" long ea_ctc_lexicon_stream_state_bytes(int max_frames, int beam) {
  if (max_frames < 0 || beam < 1 || beam > kLexMaxBeam) return 0;
  return lex_state_words(max_frames, beam) * 4L;
}

extern "C" int ea_ctc_lexicon_stream_reset(void* state, const int* slots, int n, const void* ngram, int max_streams, int max_frames,
                                           int beam, ea_stream_t stream) {
  const auto* lm = (const NgramLM*)ngram;
  if (!lm || !state || max_streams < 1 || max_frames < 0 || beam < 1 || beam > kLexMaxBeam || lm->order < 1 || lm->order > kMaxOrder)
    return -2;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(lexicon_stream_reset_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, state, slots, max_streams, max_frames,
                     beam, lm->bos, lm->order - 1);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_lexicon_stream_step(const void* x, long ld, int x_bf16, long total_rows, const int* slot_idx, const int* n_new,
                                          const int* row_off, int n, void* state, const void* ngram, const int* trie_off,
                                          const int* trie_tok, const int* trie_child, const int* trie_word, const float* trie_smear,
                                          const void* word_start, int space, int max_streams, int max_frames, int V, int beam, int K,
                                          int blank, float lm_weight, float word_score, float ins_bonus, ea_stream_t stream) {
  const auto* lm = (const NgramLM*)ngram;
  if (!lm || !lm->dev_buf || !state) return -2;
  if (n <= 0) return 0;
  if (total_rows < 0 || max_streams < 1 || max_frames < 0 || V < 2 || V > 65535 || ld < V || beam < 1 || beam > kLexMaxBeam || K < 1 ||
      K > kLexMaxK || K > V - 1 || blank < 0 || blank >= V || space >= V || (space < 0 && !word_start) || lm->order < 1 ||
      lm->order > kMaxOrder || !trie_off || !trie_word || !trie_smear)
    return -2;
  LexStreamArgs a;
  a.x = x; a.ld = ld; a.total_rows = total_rows;
  a.slot_idx = slot_idx; a.n_new = n_new; a.row_off = row_off;
  a.state = state;
  a.p = lex_params(lm, trie_off, trie_tok, trie_child, trie_word, trie_smear, word_start, space, V, beam, K, blank, lm_weight,
                   word_score, ins_bonus);
  a.max_streams = max_streams; a.max_frames = max_frames;
  if (x_bf16)
    hipLaunchKernelGGL(ctc_lexicon_stream_step_kernel<bf16_t>, dim3(n), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(ctc_lexicon_stream_step_kernel<float>, dim3(n), dim3(256), 0, (hipStream_t)stream, a);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_lexicon_stream_finish(const void* state, const int* slots, int n, const void* ngram, const int* trie_word,
                                            const float* trie_smear, int max_streams, int max_frames, int beam, float lm_weight,
                                            float word_score, float ins_bonus, int nbest, int pad, int max_u, int* tokens,
                                            int* lengths, float* scores, int* nhyp, ea_stream_t stream) {
  const auto* lm = (const NgramLM*)ngram;
  if (!lm || !lm->dev_buf || !state) return -2;
  if (n <= 0) return 0;
  if (max_streams < 1 || max_frames < 0 || beam < 1 || beam > kLexMaxBeam || nbest < 1 || nbest > beam || max_u < 0 || lm->order < 1 ||
      lm->order > kMaxOrder || !trie_word || !trie_smear)
    return -2;
  LexReadArgs a;
  a.state = state; a.slots = slots;
  a.p = lex_params(lm, nullptr, nullptr, nullptr, trie_word, trie_smear, nullptr, 0, 0, beam, 0, 0, lm_weight, word_score, ins_bonus);
  a.max_streams = max_streams; a.max_frames = max_frames; a.nbest = nbest; a.pad = pad; a.max_u = max_u;
  a.tokens = tokens; a.lengths = lengths; a.scores = scores; a.aux = nhyp;
  hipLaunchKernelGGL(ctc_lexicon_stream_finish_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, a);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_lexicon_stream_partial(const void* state, const int* slots, int n, int max_streams, int max_frames, int beam,
                                             float ins_bonus, int pad, int max_u, int* tokens, int* lengths, float* scores,
                                             int* stable_len, ea_stream_t stream) {
  if (!state) return -2;
  if (n <= 0) return 0;
  if (max_streams < 1 || max_frames < 0 || beam < 1 || beam > kLexMaxBeam || max_u < 0) return -2;
  LexReadArgs a{};
  a.state = state; a.slots = slots;
  a.p.beam = beam; a.p.gamma = ins_bonus;
  a.max_streams = max_streams; a.max_frames = max_frames; a.nbest = 1; a.pad = pad; a.max_u = max_u;
  a.tokens = tokens; a.lengths = lengths; a.scores = scores; a.aux = stable_len;
  hipLaunchKernelGGL(ctc_lexicon_stream_partial_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, a);
  return EA_CHECK_LAUNCH();
}
