// The CTC lattice (blank y1 blank ... yU blank, S = 2U + 1 states) as the aligner and posterior kernels walk it: every rule that
// ctc_viterbi_kernel (align.hip), ctc_long_tile_kernel (align_long.hip), ctc_prefix_kernel (prefix_posterior.hip) and
// ctc_prefix_long_tile_kernel (prefix_posterior_long.hip) have in common is stated here, once.  The tiled kernels equal the
// one-workgroup kernels bit for bit because both call the same frame function, not because two copies agree.
//
// The frame loop.  A thread owns 16 consecutive states (thread g of the state axis: states 16g .. 16g + 15, tokens 8g .. 8g + 7).
// The score vector lives in LDS, double-buffered, with two entries in front of it for the two states left of the thread's first
// (-inf in front of state 0, the neighbouring tile's in a tiled kernel); a frame ends in one raw barrier (lds_barrier).  The columns
// a frame needs (blank + the thread's 8 labels, an Emis) are requested four frames ahead into four register sets, every lane loading
// from a clamped row and a clamped column: no load sits in a divergent branch (hipcc would wait vmcnt(0) for it, DESIGN section 3
// item 4), and the frame functions hold no global load.  One frame in a kernel is
//   word = viterbi_frame(prev + s0, ...) or prefix_frame(prev + s0, ...);  ctc_fetch(row t + 4, q);  ctc_store(cur + s0 + 2, o);
//   [tile_handover]  [backpointer store]  lds_barrier();  swap(prev, cur)
// with the refill of a register set AFTER its last use (the load can then take the same registers: no copy that waits for it) and
// no branch around it: the loop runs the frame count rounded up to 4, frames past the end (`live` false) keep the scores.
//
// The tiled part (from kTB on) cuts the lattice into tiles of kTB frames x kTS states, one wave per tile, one launch per
// anti-diagonal; DESIGN sections 3.9 and 3.10.
#pragma once
#include <algorithm>

#include "common.h"
#include "wave_prims.h"

constexpr int kCtcMaxS = 2048;  // states of a one-workgroup kernel (Lmax <= 1023)

// threads of a one-workgroup kernel = backpointer words per frame row: one per 16 states, whole waves (64 or 128)
__host__ __device__ __forceinline__ int ctc_threads(int Lmax) {
  const int w = (2 * Lmax + 1 + 15) / 16;
  return (w + 63) & ~63;
}

template <typename TX>
__device__ __forceinline__ float ldx(const TX* p, long i) {
  if constexpr (sizeof(TX) == 2) return bf2f(p[i]); else return p[i];
}

struct Emis {  // the columns one thread needs in one frame: blank and the labels of its 8 odd states
  float b, y[8];
};

__device__ __forceinline__ void lds_barrier() {
  wait_lgkmcnt0();  // the LDS hand-off only: prefetched global loads stay in flight
  __builtin_amdgcn_s_barrier();
}

// log(exp(a) + exp(b)), -inf safe, on the hardware exp2 / log2 (v_exp_f32, v_log_f32): a frame of the posterior kernels is 32 of
// these per thread in series, and common.h's log_add (log1pf: ~40 instructions) made it 12x the aligner's frame.  The argument of
// the log is in [1, 2], where the instruction's error (1 ulp of a result <= 1) is below half an ulp of any |score| >= 1.
__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  const float r = m + __logf(1.f + __expf(-fabsf(a - b)));
  return m == -INFINITY ? -INFINITY : r;
}

__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }

// one factor: Psi_i - Psi_{i-1}, clamped to <= 0; -inf (never NaN) from the first Psi = -inf on
__device__ __forceinline__ float factor(float hi, float lo) { return hi == -INFINITY ? -INFINITY : fminf(hi - lo, 0.f); }

// Labels of thread g's odd states 16g + 2k + 1 (token u = 8g + k), clamped to a valid column: a token past U and an id outside
// [0, V) are read as blank.  Bit k of `skip`: the +2 move into that state is allowed (its label differs from the one two states
// earlier).  Returns whether a real token's id is outside [0, V) or equal to blank.
__device__ __forceinline__ bool ctc_labels(const int* tg, int g, int U, int V, int blank, int (&col)[8], unsigned& skip) {
  bool bad = false;
  skip = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int u = 8 * g + k;
    const int uc = min(u, max(U - 1, 0));
    const int y = U > 0 ? tg[uc] : blank, yp = U > 0 ? tg[max(uc - 1, 0)] : blank;
    const bool real = u < U;
    bad |= real && (y < 0 || y >= V || y == blank);
    col[k] = (real && y >= 0 && y < V) ? y : blank;
    if (real && u > 0 && y != yp) skip |= 1u << k;
  }
  return bad;
}

// one frame's columns from its row r (the caller clamps the row)
template <typename TX>
__device__ __forceinline__ void ctc_fetch(const TX* r, int blank, const int (&col)[8], Emis& e) {
  e.b = ldx(r, blank);
#pragma unroll
  for (int k = 0; k < 8; ++k) e.y[k] = ldx(r, col[k]);
}

// The first four frames' columns, t .. t + 3, requested in frame order; fetch(t, q) is the kernel's ctc_fetch from its clamped row.
// The order is pinned: loads return in order and hipcc's counted wait in the loop (vmcnt(N)) is the smaller of what the loop's entry
// and its back edge allow, so a prologue that the scheduler had interleaved would turn the loop's waits into drains.
template <typename F>
__device__ __forceinline__ void ctc_prefetch(F&& fetch, int t, Emis& q0, Emis& q1, Emis& q2, Emis& q3) {
  fetch(t, q0);
  __builtin_amdgcn_sched_barrier(0);
  fetch(t + 1, q1);
  __builtin_amdgcn_sched_barrier(0);
  fetch(t + 2, q2);
  __builtin_amdgcn_sched_barrier(0);
  fetch(t + 3, q3);
  __builtin_amdgcn_sched_barrier(0);
}

// a thread's window of the frame before: w = buffer + 16 * thread; p[j + 2] is its state j, p[0] and p[1] the two states left of it
__device__ __forceinline__ void ctc_window(const float* w, float (&p)[18]) {
#pragma unroll
  for (int j = 0; j < 18; j += 2) {
    const float2 v = *reinterpret_cast<const float2*>(w + j);
    p[j] = v.x; p[j + 1] = v.y;
  }
}

// the thread's 16 new scores: w = buffer + 16 * thread + 2
__device__ __forceinline__ void ctc_store(float* w, const float (&o)[16]) {
#pragma unroll
  for (int j = 0; j < 16; j += 2) *reinterpret_cast<float2*>(w + j) = make_float2(o[j], o[j + 1]);
}

// Max-plus frame t for the thread whose first state is sg (global) and whose window is w: new[s] = max(stay, +1, +2) + x[t][label(s)]; ties prefer stay,
// then +1.  Frame 0 starts the lattice in states 0 and 1.  States from S on are -inf; a frame that is not live keeps the scores.
// Returns the 2-bit backpointers (0 stay, 1 from s-1, 2 from s-2) of the 16 states.
__device__ __forceinline__ uint32_t viterbi_frame(const float* w, const Emis& e, unsigned skip, int sg, int S, int t, bool live,
                                                  float (&o)[16]) {
  float p[18];
  ctc_window(w, p);
  uint32_t word = 0u;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int s = sg + j;
    const float st = p[j + 2], m1 = p[j + 1];
    const float m2 = ((j & 1) && ((skip >> (j >> 1)) & 1u)) ? p[j] : -INFINITY;
    float best = st;
    uint32_t c = 0u;
    if (m1 > best) { best = m1; c = 1u; }
    if (m2 > best) { best = m2; c = 2u; }
    float v;
    if (t == 0) v = s == 0 ? e.b : (s == 1 && S > 1 ? e.y[0] : -INFINITY);
    else v = best + ((j & 1) ? e.y[j >> 1] : e.b);
    o[j] = live ? (s < S ? v : -INFINITY) : st;
    word |= c << (2 * j);
  }
  return word;
}

// Sum-product frame t: new[s] = lse(stay, +1, +2) + x[t][label(s)], and for the odd state of token k, psi[k] = lse(psi[k], enter):
// the mass ENTERING the state (+1 and, where allowed, +2) times the frame's emission, the self-loop left out, so that every
// alignment of a prefix is counted once, at the frame where its last token starts.  Frames that are not live add nothing.
__device__ __forceinline__ void prefix_frame(const float* w, const Emis& e, unsigned skip, int sg, int S, int t, bool live,
                                             float (&psi)[8], float (&o)[16]) {
  float p[18];
  ctc_window(w, p);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int s = sg + j;
    const float st = p[j + 2], m1 = p[j + 1];
    float v;
    if (j & 1) {
      const int k = j >> 1;
      const float m2 = ((skip >> k) & 1u) ? p[j] : -INFINITY;
      float enter = lse2(m1, m2) + e.y[k];
      v = lse2(st + e.y[k], enter);
      if (t == 0) { enter = (s == 1 && S > 1) ? e.y[0] : -INFINITY; v = enter; }
      if (live && s < S) psi[k] = lse2(psi[k], enter);
    } else {
      v = lse2(st, m1) + e.b;
      if (t == 0) v = s == 0 ? e.b : -INFINITY;
    }
    o[j] = live ? (s < S ? v : -INFINITY) : st;
  }
}

// ---- the tiled kernels: tile (i, j) = frame block i, state tile j ----------------------------------------------------------------
// A tile takes the scores of its states in the frame before its block from alpha[S] (left there by tile (i - 1, j), one launch
// earlier) and leaves its own last frame there; it takes the scores of the two states left of it, for every frame of the block and
// the frame before it, from edge[j - 1][t][2] (tile (i, j - 1), one launch earlier, and tile (i - 1, j - 1), two earlier) and leaves
// those of its own two last states in edge[j][t][2].  The edge columns pass through LDS: read once per tile, written once per tile.
// Tiles of one launch touch disjoint parts of every buffer; ORDER BETWEEN WORKGROUPS COMES FROM LAUNCH BOUNDARIES ONLY: no grid
// barrier, no cooperative launch, no flag one workgroup waits on.  Every index into edge is 64-bit.

constexpr int kTB = 128;       // frames per tile (a multiple of 4: the prefetch depth)
constexpr int kTS = 1024;      // states per tile (even; 16 per thread)
constexpr int kNT = kTS / 16;  // threads per tile: one wave
static_assert(kTB % 4 == 0 && kTS % 32 == 0 && kNT % 64 == 0, "tile shape");
constexpr long kMaxT = 1L << 30, kMaxU = 1L << 28;  // frame and state indices stay in 32 bits

// the front of a tiled kernel's workspace: alpha at byte 0, edge at edge_off; a kernel's own buffers follow from `tail` on.  Every
// count is a multiple of 64 elements.
struct TileLayout {
  long nI, nJ;  // frame blocks, state tiles
  long Tp, Sp;  // padded frames, padded states
  long edge_off, tail;
};

__host__ inline TileLayout tile_layout(long T, long U) {
  TileLayout l;
  const long S = 2 * U + 1;
  l.nI = (T + kTB - 1) / kTB;
  l.nJ = (S + kTS - 1) / kTS;
  l.Tp = l.nI * kTB;
  l.Sp = l.nJ * kTS;
  l.edge_off = 4 * l.Sp;
  l.tail = l.edge_off + 8 * l.nJ * l.Tp;
  return l;
}

// anti-diagonal d holds the tiles (i, d - i), i_lo <= i < i_lo + count: launch(d, i_lo, count) for each d in order
template <typename F>
void for_each_antidiagonal(const TileLayout& l, F&& launch) {
  for (long d = 0; l.nI > 0 && d < l.nI + l.nJ - 1; ++d) {
    const long i_lo = std::max(0L, d - (l.nJ - 1)), i_hi = std::min(d, l.nI - 1);
    launch((int)d, (int)i_lo, (unsigned)(i_hi - i_lo + 1));
  }
}

// A tile kernel's LDS: the score vector s_a[2][kTS + 2] ([buffer][2 + local state]: entries 0, 1 are the two states left of the
// tile), s_in[2 * (kTB + 1)] (those two states in the frames t0 - 1 .. t0 + kTB - 1) and s_out[2 * kTB] (the tile's own two last
// states in its frames), each aligned to 16 bytes and declared by the kernel itself.

// (uniform) whether tile (., bj) is above the reachable cone in every frame of the block that starts at t0 (its first state >
// 2 t + 1 for its last frame t).  Such a tile computes nothing: alpha stays -inf, and its edge column eout is written as -inf here.
__device__ __forceinline__ bool tile_above_cone(float* eout, int bj, int t0, int i) {
  if ((long)bj * kTS <= 2L * (t0 + kTB - 1) + 1) return false;
  for (int k = i; k < 2 * kTB / 4; k += kNT) reinterpret_cast<float4*>(eout)[k] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  return true;
}

// the frame before the block into prev: the tile's states from alpha, the two states left of it (and their later frames, into
// s_in) from edge
__device__ __forceinline__ void tile_prologue(float* prev, float* s_in, const float* alpha, const float* edge, long Tp, int bj, int t0,
                                              int i) {
  const float* ain = alpha + (long)bj * kTS + 16 * i;
#pragma unroll
  for (int k = 0; k < 16; k += 4) {
    const float4 v = *reinterpret_cast<const float4*>(ain + k);
    *reinterpret_cast<float2*>(prev + 2 + 16 * i + k) = make_float2(v.x, v.y);
    *reinterpret_cast<float2*>(prev + 4 + 16 * i + k) = make_float2(v.z, v.w);
  }
  const float* ein = edge + (long)max(bj - 1, 0) * Tp * 2;
  for (int k = i; k < 2 * (kTB + 1); k += kNT) {
    const int t = t0 - 1 + (k >> 1);
    const float v = ein[(long)max(t, 0) * 2 + (k & 1)];
    const float w = (bj == 0 || t < 0) ? -INFINITY : v;
    s_in[k] = w;
    if (k < 2) prev[k] = w;
  }
}

// frame tt of the block: the left neighbour's two states of this frame into cur[0..1], the tile's two last states into s_out
// (the last thread is tested with >=: after two equality tests of i in a row hipcc branches on i as on a switch, two levels of
// exec-mask branches in every frame)
__device__ __forceinline__ void tile_handover(float* cur, const float* s_in, float* s_out, const float (&o)[16], int tt, int i) {
  if (i == 0) *reinterpret_cast<float2*>(cur) = *reinterpret_cast<const float2*>(s_in + 2 * (tt + 1));
  if (i >= kNT - 1) *reinterpret_cast<float2*>(s_out + 2 * tt) = make_float2(o[14], o[15]);
}

// the block's last frame (prev) to alpha, s_out to the tile's edge column eout
__device__ __forceinline__ void tile_epilogue(const float* prev, const float* s_out, float* alpha, float* eout, int bj, int i) {
  float* aout = alpha + (long)bj * kTS + 16 * i;
#pragma unroll
  for (int k = 0; k < 16; k += 4) {
    const float2 a = *reinterpret_cast<const float2*>(prev + 2 + 16 * i + k), b = *reinterpret_cast<const float2*>(prev + 4 + 16 * i + k);
    *reinterpret_cast<float4*>(aout + k) = make_float4(a.x, a.y, b.x, b.y);
  }
  for (int k = i; k < 2 * kTB / 4; k += kNT) reinterpret_cast<float4*>(eout)[k] = reinterpret_cast<const float4*>(s_out)[k];
}
