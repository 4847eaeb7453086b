// Log-prob rows of a sub-word n-gram LM (ARPA) for the token-level beam searches, for gfx950: per hypothesis its n-gram
// context is advanced from the (parent, token, keep) triple a search step writes and turned into the full row
// ln P(. | context) over the model's dictionary, in one launch per frame.  The four searches (ctc_beam.hip, rnnt_beam.hip and
// their streamed forms) read such rows as `lm_rows`, exactly as they read the LSTM LM's.  The reference gets an n-gram LM only
// through Flashlight's KenLM hand-off (espresso/tools/ctc_decoder.py:24-71), word-level and behind a lexicon; this is the
// same ARPA model queried over sub-word units, with no lexicon.
//
// Contract (W = order - 1; a context is int32 [W], oldest first, front-padded with -1, as ea_ngram_score takes it; tok2word
// int32 [V]: >= 0 an ARPA word id, -1 no ARPA entry, -2 a column that is always -inf).  For row i < N:
//   1. c = ctx_in[parent[i]] when keep[i], else ctx_in[parent[i]] shifted left by one with word(token[i]) appended, where
//      word(t) = tok2word[t] if >= 0, else the file's <unk>, else n1 (an id that matches no n-gram);
//   2. ctx_out[i] = c (ctx_in and ctx_out are distinct buffers: the gather by parent forbids an in-place update);
//   3. rows[i * ld + v] = ng_logp(c, tok2word[v]) for v < V, bit for bit (ngram_common.h); -1 columns get the value of <unk>
//      in that context (-inf without one), -2 columns -inf.
// ea_ngram_token_rows_host is this contract as a loop of ng_logp over v on the host tables: the yardstick of the kernel.
//
// The kernel (ngram_rows_kernel): one 256-thread workgroup per row.  ng_logp for one word is a chain of dependent binary
// searches: longest context first, falling back order by order and adding backoff weights.  For a whole row the searches
// turn into scatters, because the children of a context record are contiguous and sorted by word id:
//   a. threads 0 .. W-1 build c; lane l <= L (L = the valid words of c) of wave 0 walks the suffix of length l down the trie
//      (l dependent searches) to its record r_l, or -1 if the suffix is absent;
//   b. lane 0 forms acc_l, the backoff sum ng_logp holds when it reaches suffix length l: 0 at l = L, then bow[l][r_l] of every
//      present suffix added longest first (an absent suffix adds nothing) -- the same additions in the same order;
//   c. unigram pass, coalesced over v: row[v] = acc_0 + logp[1][tok2word[v]] (-inf for the -1 and -2 columns);
//   d. for l = 1 .. L in that order, a barrier between two orders: every child c of r_l overwrites column word2tok[word[c]] with
//      acc_l + logp[l + 1][c].  The longest suffix that has the word writes last: that is ng_logp's answer, one fp32 addition
//      of the same two operands.  Within one order the children of one record have distinct words: no two threads write one
//      column between two barriers, and no atomics touch the row.  The value of <unk> takes the same passes in one LDS word;
//   e. the row leaves LDS with 16-byte stores (ld a multiple of 4 and an aligned base; 4-byte stores otherwise); the -1
//      columns take the <unk> value on the way out.
// (L + 1) * V coalesced accesses at most instead of V * (L + 1) search chains; in practice far fewer, since a context has few
// children.  The row is staged in LDS up to kNgRowLds = 5120 columns (the recipe's V = 5004 fits); columns beyond are written
// to `rows` directly by the same passes (the barriers order them) and patched there for -1.  Every row is recomputed every
// frame, the rows of kept hypotheses included.
//
//   ngram_rows_kernel<false>, <true> (the start rows)   256 threads, 20560 B LDS, 20 VGPRs, no scratch
//     -> 7 workgroups per CU by LDS (160 KB): 7 waves per SIMD of the 8 the registers would allow
#include <vector>

#include "common.h"
#include "espresso_amd.h"
#include "ngram_common.h"

namespace {

constexpr int kNgRowLds = 5120;  // row columns staged in LDS; columns beyond live in global memory only

struct TokenMap {  // the uploaded pair
  int V = 0, n1 = 0;
  int* dev = nullptr;  // tok2word [V], then word2tok [n1]: the token of an ARPA word, -1 if none
};

struct RowsArgs {
  NgramDev m;
  const int *tok2word, *word2tok;
  const int *ctx_in, *parent, *token;
  const uint8_t* keep;
  int* ctx_out;
  float* rows;
  long ld;
  int V, N;
};

struct RowsLds {
  float row[kNgRowLds];
  int ctx[kMaxCtx + 1];
  int rec[kMaxOrder];    // [l]: the record of the suffix of length l, -1 if absent ([0]: the root)
  float acc[kMaxOrder];  // [l]: the backoff sum in front of order l + 1
  float unk;             // the value of <unk> in this context
  int L;
};

template <bool kStart>
__global__ __launch_bounds__(256) void ngram_rows_kernel(const RowsArgs a) {
  __shared__ __attribute__((aligned(16))) RowsLds s;
  const int tid = threadIdx.x, i = blockIdx.x;
  const NgramDev& m = a.m;
  const int W = m.order - 1, V = a.V, n1 = m.n1;
  float* const out = a.rows + (long)i * a.ld;

  // a. the context
  if (tid < W) {
    int c;
    if constexpr (kStart) {
      c = tid == W - 1 ? m.bos : -1;
    } else {
      int p = a.parent[i];
      if (p < 0 || p >= a.N) p = i;
      const int* h = a.ctx_in + (long)p * W;
      if (a.keep[i]) {
        c = h[tid];
      } else if (tid < W - 1) {
        c = h[tid + 1];
      } else {
        const int t = a.token[i];
        c = t >= 0 && t < V ? a.tok2word[t] : -1;
        if (c < 0) c = m.unk >= 0 ? m.unk : n1;
      }
    }
    s.ctx[tid] = c;
    a.ctx_out[(long)i * W + tid] = c;
  }
  __syncthreads();
  if (tid < 64) {
    const int L = ctx_len(s.ctx, W);
    int r = tid <= L ? 0 : -1;
    for (int k = 0; k < tid && r >= 0; ++k) r = ng_find(m.child, m.word, n1, k, r, s.ctx[W - tid + k]);
    if (tid <= L) s.rec[tid] = r;
    if (tid == 0) s.L = L;
  }
  __syncthreads();
  const int L = s.L;
  // b. the backoff sums, in ng_logp's order
  if (tid == 0) {
    float acc = 0.f;
    for (int l = L; l >= 0; --l) {
      s.acc[l] = acc;
      if (l > 0 && s.rec[l] >= 0) acc += m.bow[l][s.rec[l]];
    }
    s.unk = m.unk >= 0 ? s.acc[0] + m.logp[1][m.unk] : -INFINITY;
  }
  __syncthreads();

  // c. unigrams
  const float acc0 = s.acc[0];
  for (int v = tid; v < V; v += 256) {
    const int w = a.tok2word[v];
    const float x = w >= 0 ? acc0 + m.logp[1][w] : -INFINITY;
    if (v < kNgRowLds) s.row[v] = x; else out[v] = x;
  }
  __syncthreads();

  // d. the children of every present suffix, shortest first: the longest one that has the word writes last
  for (int l = 1; l <= L; ++l) {
    const int r = s.rec[l];
    if (r < 0) continue;  // (uniform: no barrier is skipped by part of the workgroup)
    const float acc = s.acc[l];
    const int* wd = m.word[l + 1];
    const float* lp = m.logp[l + 1];
    const int end = m.child[l][r + 1];
    for (int c = m.child[l][r] + tid; c < end; c += 256) {
      const int w = wd[c];
      const int v = a.word2tok[w];
      const float x = acc + lp[c];
      if (w == m.unk) s.unk = x;
      if (v >= 0) {
        if (v < kNgRowLds) s.row[v] = x; else out[v] = x;
      }
    }
    __syncthreads();
  }

  // e. out; the columns without an ARPA entry score as <unk>
  const float unk = s.unk;
  const int Vl = min(V, kNgRowLds);
  int v0 = 0;
  if ((a.ld & 3) == 0 && ((uintptr_t)a.rows & 15) == 0) {
    v0 = Vl & ~3;
    for (int v = 4 * tid; v < v0; v += 1024) {
      float4 x = *(const float4*)&s.row[v];
      const int4 w = *(const int4*)&a.tok2word[v];  // (the map's allocation is 256-byte aligned)
      if (w.x == -1) x.x = unk;
      if (w.y == -1) x.y = unk;
      if (w.z == -1) x.z = unk;
      if (w.w == -1) x.w = unk;
      *(float4*)&out[v] = x;
    }
  }
  for (int v = v0 + tid; v < Vl; v += 256) out[v] = a.tok2word[v] == -1 ? unk : s.row[v];
  for (int v = kNgRowLds + tid; v < V; v += 256)
    if (a.tok2word[v] == -1) out[v] = unk;
}

// the contract on the host tables: context i of the step, then the row by ng_logp
void host_row(const NgramDev& m, const int* tok2word, int V, const int* c, float* out) {
  const int W = m.order - 1;
  const int L = ctx_len(c, W);
  for (int v = 0; v < V; ++v) out[v] = tok2word[v] == -2 ? -INFINITY : ng_logp(m, c + W - L, L, tok2word[v]);
}

int map_ok(const NgramLM* lm, const int* tok2word, int V) {
  if (!lm || !tok2word || V < 1) return 0;
  const int n1 = (int)lm->counts[1];
  std::vector<char> seen(n1, 0);
  for (int v = 0; v < V; ++v) {
    const int w = tok2word[v];
    if (w < -2 || w >= n1) return 0;
    if (w >= 0 && seen[w]++) return 0;  // two tokens on one word: the scatter needs the inverse map
  }
  return 1;
}

}  // namespace

extern "C" int ea_ngram_token_map_create(const void* handle, const int* tok2word_host, int V, void* map_host) {
  const auto* lm = (const NgramLM*)handle;
  *(void**)map_host = nullptr;
  if (!map_ok(lm, tok2word_host, V)) return -2;
  const int n1 = (int)lm->counts[1];
  std::vector<int> both(tok2word_host, tok2word_host + V);
  both.resize((size_t)V + n1, -1);
  for (int v = 0; v < V; ++v)
    if (tok2word_host[v] >= 0) both[V + tok2word_host[v]] = v;
  auto* mp = new TokenMap();
  mp->V = V; mp->n1 = n1;
  if (hipMalloc(&mp->dev, both.size() * 4) != hipSuccess ||
      hipMemcpy(mp->dev, both.data(), both.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    if (mp->dev) hipFree(mp->dev);
    delete mp;
    return -1;
  }
  *(void**)map_host = mp;
  return 0;
}

extern "C" int ea_ngram_token_map_destroy(void* map) {
  auto* mp = (TokenMap*)map;
  if (!mp) return 0;
  if (mp->dev) hipFree(mp->dev);
  delete mp;
  return 0;
}

namespace {
int rows_launch(bool start, const void* handle, const void* tok2word, int V, const int* ctx_in, const int* parent, const int* token,
                const void* keep, int N, int* ctx_out, float* rows, long ld, ea_stream_t stream) {
  const auto* lm = (const NgramLM*)handle;
  const auto* mp = (const TokenMap*)tok2word;
  if (!lm || !lm->dev_buf || !mp || mp->V != V || mp->n1 != (int)lm->counts[1] || N < 0 || !rows || ld < V) return -2;
  const int W = lm->order - 1;
  if (W > 0 && !ctx_out) return -2;
  if (!start && (!parent || !token || !keep || (W > 0 && (!ctx_in || ctx_in == ctx_out)))) return -2;
  if (N == 0) return 0;
  RowsArgs a;
  a.m = lm->dev;
  a.tok2word = mp->dev; a.word2tok = mp->dev + V;
  a.ctx_in = ctx_in; a.parent = parent; a.token = token; a.keep = (const uint8_t*)keep;
  a.ctx_out = ctx_out; a.rows = rows; a.ld = ld; a.V = V; a.N = N;
  if (start) hipLaunchKernelGGL(ngram_rows_kernel<true>, dim3(N), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(ngram_rows_kernel<false>, dim3(N), dim3(256), 0, (hipStream_t)stream, a);
  return EA_CHECK_LAUNCH();
}
}  // namespace

extern "C" int ea_ngram_token_rows_step(const void* handle, const void* tok2word, int V, const int* ctx_in, const int* parent,
                                        const int* token, const void* keep, int N, int* ctx_out, float* rows, long ld,
                                        ea_stream_t stream) {
  return rows_launch(false, handle, tok2word, V, ctx_in, parent, token, keep, N, ctx_out, rows, ld, stream);
}

extern "C" int ea_ngram_token_rows_start(const void* handle, const void* tok2word, int V, int N, int* ctx, float* rows, long ld,
                                         ea_stream_t stream) {
  return rows_launch(true, handle, tok2word, V, nullptr, nullptr, nullptr, nullptr, N, ctx, rows, ld, stream);
}

extern "C" int ea_ngram_token_rows_host(const void* handle, const int* tok2word_host, int V, const int* ctx_in_host,
                                        const int* parent_host, const int* token_host, const void* keep_host, int N,
                                        int* ctx_out_host, float* rows_host, long ld) {
  const auto* lm = (const NgramLM*)handle;
  if (!map_ok(lm, tok2word_host, V) || N < 0 || !rows_host || ld < V) return -2;
  const NgramDev& m = lm->host;
  const int W = m.order - 1;
  const bool start = !parent_host;  // no triple: the start rows
  if (W > 0 && !ctx_out_host) return -2;
  if (!start && (!token_host || !keep_host || (W > 0 && (!ctx_in_host || ctx_in_host == ctx_out_host)))) return -2;
  const auto* keep = (const uint8_t*)keep_host;
  int c[kMaxCtx + 1];
  for (int i = 0; i < N; ++i) {
    if (start) {
      for (int j = 0; j < W; ++j) c[j] = j == W - 1 ? m.bos : -1;
    } else {
      int p = parent_host[i];
      if (p < 0 || p >= N) p = i;
      const int* h = ctx_in_host + (long)p * W;
      for (int j = 0; j < W; ++j) c[j] = keep[i] ? h[j] : j < W - 1 ? h[j + 1] : -1;
      if (!keep[i] && W > 0) {
        const int t = token_host[i];
        int w = t >= 0 && t < V ? tok2word_host[t] : -1;
        if (w < 0) w = m.unk >= 0 ? m.unk : m.n1;
        c[W - 1] = w;
      }
    }
    for (int j = 0; j < W; ++j) ctx_out_host[(long)i * W + j] = c[j];
    host_row(m, tok2word_host, V, c, rows_host + (long)i * ld);
  }
  return 0;
}
