// The ARPA n-gram tables and their lookup, shared by the searches that fuse an n-gram LM: the lexicon search with a word LM
// (ctc_lexicon_beam.hip, which also holds the parser and the upload) and the per-hypothesis log-prob rows of a sub-word LM
// (ngram_rows.hip).  A sorted-array trie: order 1 is indexed by word id; every order k >= 2 holds its records sorted by
// (record of the (k-1)-gram context, word id), and a record of order k < n carries a child range into order k + 1.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

constexpr int kMaxOrder = 6;
constexpr int kMaxCtx = kMaxOrder - 1;

// ------------------------------------------------------------------------------------------------ n-gram tables
struct NgramDev {  // device pointers of the tables, passed by value
  int order, n1, unk, bos, eos;
  const float* logp[kMaxOrder + 1];  // [k]: records of order k (natural log)
  const float* bow[kMaxOrder + 1];   // [k], k < order (0 where the ARPA line has none)
  const int* word[kMaxOrder + 1];    // [k], k >= 2: last word of the record (order 1: record i is word i)
  const int* child[kMaxOrder + 1];   // [k], k < order: records [child[i], child[i + 1]) of order k + 1 extend record i
};

struct NgramLM {
  int order = 0, unk = -1, bos = -1, eos = -1;
  long counts[kMaxOrder + 1] = {};
  std::vector<std::string> vocab;
  std::vector<float> logp[kMaxOrder + 1], bow[kMaxOrder + 1];
  std::vector<int> word[kMaxOrder + 1], child[kMaxOrder + 1], parent[kMaxOrder + 1];
  void* dev_buf = nullptr;
  NgramDev dev{}, host{};  // the same tables: device copy, host vectors
};

// the record of order k + 1 that extends record r of order k by word w (order 0: the root), -1 if none
__host__ __device__ __forceinline__ int ng_find(const int* const* child, const int* const* word, int n1, int k, int r, int w) {
  if (k == 0) return (w >= 0 && w < n1) ? w : -1;
  const int* wd = word[k + 1];
  int lo = child[k][r];
  const int end = child[k][r + 1];
  int hi = end;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (wd[mid] < w) lo = mid + 1; else hi = mid;
  }
  return (lo < end && wd[lo] == w) ? lo : -1;
}

// ln P(w | h[0..L)), h oldest first; w outside the vocabulary scores as <unk> (-inf without one)
__host__ __device__ inline float ng_logp(const NgramDev& m, const int* h, int L, int w) {
  if (w < 0 || w >= m.n1) w = m.unk;
  if (w < 0) return -INFINITY;
  if (L > m.order - 1) { h += L - (m.order - 1); L = m.order - 1; }
  float acc = 0.f;
  for (int l = L; l >= 0; --l) {
    int r = 0, k = 0;
    for (; k < l; ++k) {
      r = ng_find(m.child, m.word, m.n1, k, r, h[L - l + k]);
      if (r < 0) break;
    }
    if (k < l) continue;  // the context h[L-l..L) is absent: its backoff weight counts as 0
    const int rw = ng_find(m.child, m.word, m.n1, l, r, w);
    if (rw >= 0) return acc + m.logp[l + 1][rw];
    if (l > 0) acc += m.bow[l][r];
  }
  return -INFINITY;  // not reached: every w in [0, n1) is a unigram
}

// contexts: fixed width W = order - 1, oldest first, front-padded with -1; the valid words are those after the last -1
__host__ __device__ __forceinline__ int ctx_len(const int* h, int W) {
  int L = 0;
  while (L < W && h[W - 1 - L] >= 0) ++L;
  return L;
}
