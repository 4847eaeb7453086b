// Device helpers shared by the CTC prefix beam searches (ctc_beam.hip, ctc_lexicon_beam.hip): 48-bit ordering keys,
// the workgroup-wide radix select over them, log-add-exp, the prefix hash and L2 loads of the workgroup's own writes; and the
// one step of the hotword context graph (an Aho-Corasick automaton over the phrase trie) that the biased searches (ctc_beam.hip,
// rnnt_beam.hip), the replay kernel and its host twin share.
#pragma once
#include "common.h"

namespace {

// L1-bypassing loads of what this workgroup's own atomics and stores wrote earlier
__device__ __forceinline__ unsigned long long ld_l2(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_l2(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t tab_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  return (uint32_t)k;
}

__device__ __forceinline__ float lae(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + log1pf(expf(-fabsf(a - b)));
}

// order-preserving map of a float to 32 unsigned bits (-0 folded into +0)
__device__ __forceinline__ uint64_t ord32(float f) {
  const uint32_t u = __float_as_uint(f + 0.f);
  return (uint64_t)(u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u));
}
// unique 48-bit key: larger value first, then lower index (0 = absent)
__device__ __forceinline__ uint64_t mk_key(float v, int idx) { return (ord32(v) << 16) | (uint64_t)(0xFFFF - idx); }

// The endpoint rule of the streamed searches (ea_*_stream_endpoint) for a slot with F frames whose best live hypothesis has L
// tokens, the last of them starting at frame E of its best path (-1 when L == 0): the first that holds of 1 "silence" (L > 0 and
// F - 1 - E >= silence), 2 "empty" (L == 0 and F >= empty), 3 "length" (F >= segment), else 0; a threshold <= 0 is switched off.
__host__ __device__ __forceinline__ int endpoint_rule(int F, int L, int E, int silence, int empty, int segment) {
  if (silence > 0 && L > 0 && F - 1 - E >= silence) return 1;
  if (empty > 0 && L == 0 && F >= empty) return 2;
  if (segment > 0 && F >= segment) return 3;
  return 0;
}

struct SelectScratch {
  unsigned hist[256];
  uint64_t prefix;
  int need, done;
};

// The n-th largest of the nonzero keys key(0..N) (blockDim 256, all threads call).  Returns 1 when there are n or fewer
// nonzero keys (then every nonzero key is selected).  MSB-first radix select, 8 bits per pass over 48-bit keys.
template <class KeyFn>
__device__ uint64_t select_nth(KeyFn key, int N, int n, SelectScratch& s) {
  const int tid = threadIdx.x;
  if (tid == 0) { s.prefix = 0; s.need = n; s.done = 0; }
  for (int shift = 40; shift >= 0; shift -= 8) {
    s.hist[tid] = 0u;
    __syncthreads();
    const uint64_t prefix = s.prefix;
    const uint64_t hi = ~0ull << (shift + 8);
    for (int i = tid; i < N; i += 256) {
      const uint64_t k = key(i);
      if (k && (k & hi) == prefix) atomicAdd(&s.hist[(k >> shift) & 255], 1u);
    }
    __syncthreads();
    if (tid < 64) {  // wave 0: lane L holds digits 255-4L .. 252-4L, scanned from the top
      unsigned c[4], tot = 0;
#pragma unroll
      for (int m = 0; m < 4; ++m) { c[m] = s.hist[255 - 4 * tid - m]; tot += c[m]; }
      unsigned incl = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o, 64);
        if (tid >= o) incl += v;
      }
      const unsigned all = __shfl(incl, 63, 64);
      const unsigned need = (unsigned)s.need;
      if (shift == 40 && all <= need) {
        if (tid == 0) s.done = 1;
      } else {
        unsigned run = incl - tot;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          if (run < need && run + c[m] >= need) {
            s.prefix = prefix | ((uint64_t)(255 - 4 * tid - m) << shift);
            s.need = (int)(need - run);
          }
          run += c[m];
        }
      }
    }
    __syncthreads();
    if (s.done) return 1;
  }
  return s.prefix;
}

// Context graph (tools/context_graph.py), packed for one 16-byte load per visited node and per probed edge:
//   nodes int32 [n_nodes][4] = (first edge, end edge, fail node, bits of phi);  node 0 = root
//   edges int32 [n_edges][4] = (token, child node, bits of the edge boost, 0), the edges of a node ascending by token
//   root  int32 [V][2]       = (child of the root by token or -1, bits of its edge boost): the first level, direct-indexed
struct CgTables {
  const int* nodes; const int* edges; const int* root;
  int n_nodes, n_edges, V;
};
struct CgStep { int q; float inc; };  // the state after the token, and b' - b
struct CgRoot { int child; float boost; };

__host__ __device__ __forceinline__ float cg_bits(int i) {
  float f;
  __builtin_memcpy(&f, &i, 4);
  return f;
}
__host__ __device__ __forceinline__ CgRoot cg_root(const CgTables& g, int v) {
  if ((unsigned)v >= (unsigned)g.V) return {-1, 0.f};
  const int2 r = *(const int2*)(g.root + 2L * v);
  return {r.x, cg_bits(r.y)};
}
// Appending token v in state q: down the failure links from q until a node has the edge v (the root's edge comes from
// `root_of_v`, which the search keeps in LDS for the frame's candidates).  inc = phi(m) + e(q') - phi(q), or -phi(q) when the
// automaton falls back to the root.  Out-of-range table entries end the walk at the root (malformed tables cannot hang it).
__host__ __device__ __forceinline__ CgStep cg_step(const CgTables& g, int q, int v, CgRoot root_of_v) {
  float phi_q = 0.f;
  if (q > 0 && q < g.n_nodes) {
    int4 nm = *(const int4*)(g.nodes + 4L * q);
    phi_q = cg_bits(nm.w);
    for (int hops = 0; hops < g.n_nodes; ++hops) {
      int lo = nm.x > 0 ? nm.x : 0, hi = nm.y < g.n_edges ? nm.y : g.n_edges;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int4 e = *(const int4*)(g.edges + 4L * mid);
        if (e.x == v) return {e.y, cg_bits(nm.w) + cg_bits(e.z) - phi_q};
        if (e.x < v) lo = mid + 1; else hi = mid;
      }
      const int m = nm.z;
      if (m <= 0 || m >= g.n_nodes) break;
      nm = *(const int4*)(g.nodes + 4L * m);
    }
  }
  if (root_of_v.child >= 0) return {root_of_v.child, root_of_v.boost - phi_q};
  return {0, -phi_q};
}
__host__ __device__ __forceinline__ float cg_phi(const CgTables& g, int q) {
  return q > 0 && q < g.n_nodes ? cg_bits(g.nodes[4L * q + 3]) : 0.f;
}

// one token row through the graph: running[u] = b after token u (may be NULL), *final_bias = b - phi(q) = B(y), *q_out = q
__host__ __device__ __forceinline__ void cg_replay(const CgTables& g, const int* tokens, int len, float* running, float* final_bias,
                                                   int* q_out) {
  int q = 0;
  float b = 0.f;
  for (int u = 0; u < len; ++u) {
    const CgStep st = cg_step(g, q, tokens[u], cg_root(g, tokens[u]));
    q = st.q;
    b += st.inc;
    if (running) running[u] = b;
  }
  *final_bias = b - cg_phi(g, q);
  *q_out = q;
}

// the table arguments of a C entry point -> g; 0 = malformed.  A trie: one edge into every node but the root; an empty graph is
// the root alone, and then the edge table may be NULL
inline int cg_tables(CgTables& g, const int* nodes, const int* edges, const int* root, int n_nodes, int n_edges, int V) {
  if (!nodes || !root || n_nodes < 1 || n_edges < 0 || (n_edges > 0 && !edges) || n_edges != n_nodes - 1 || V < 1) return 0;
  g.nodes = nodes; g.edges = edges; g.root = root;
  g.n_nodes = n_nodes; g.n_edges = n_edges; g.V = V;
  return 1;
}
// what a finish needs of the graph: phi of a node
inline CgTables cg_nodes_only(const int* nodes, int n_nodes) {
  CgTables g;
  g.nodes = nodes; g.edges = nullptr; g.root = nullptr;
  g.n_nodes = n_nodes; g.n_edges = 0; g.V = 0;
  return g;
}

template <typename TX>
__device__ __forceinline__ float ldx(const TX* p, int i) {
  if constexpr (sizeof(TX) == 2) return bf2f(p[i]); else return p[i];
}

}  // namespace
