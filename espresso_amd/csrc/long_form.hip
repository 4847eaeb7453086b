// Long-form recognition for offline CTC models on gfx950: the two kernels that join the logits of one recording's overlapping
// windows into one log-prob matrix on the recording's own frame axis (tools/long_form.py).  The reference
// has no long-form path -- its recognizer takes a recording as one utterance -- so these kernels replace nothing of it; without
// them the join is a host loop of per-junction slices, log-softmaxes, mins, argmaxes and index copies over tensors of a few rows.
// The rule is normative in include/espresso_amd.h ("Long-form recognition").
//
// Window n holds global frames n * Hf + [0, counts[n]); its logits are rows (n * Tw + j) * ld of `logits`, bf16 or fp32 as the
// encoder wrote them.
//
//   longform_cuts_kernel: one 256-thread workgroup per junction (windows n and n + 1).  It walks the overlap frames, takes the
//     log-sum-exp of the frame's row in either window with the row routine of ea_log_softmax_* (softmax_row.h: the whole
//     workgroup on one row, so b(j) has the bits of the log-softmax's blank column) and keeps b(j) in LDS -- an overlap is at
//     most Tw - Hf frames.  Then every thread scores candidates c = first + tid, + 256, ..., and thread 0 picks among the 256
//     thread-bests.  Every comparison is on (score, distance from the middle, c), a total order: no dependence on the thread count.
//   longform_stitch_kernel: one workgroup per global frame.  The owner of frame t is window n0 = min(t / Hf, Nw - 1) unless
//     t < cuts[n0 - 1], then n0 - 1 (cuts[n] lies in window n + 1, so one comparison decides); its row goes through the same row
//     routine, with 16-byte loads and stores where the addresses allow them.  Rows of other windows are not touched.  All
//     branches on the window are uniform over the workgroup; a frame whose owner does not hold it (cuts not made by
//     ea_longform_cuts) is left unwritten rather than read out of its window.
//
// Long-form recognition for transducer models (tools/long_form.py LongFormTransducer) joins the windows'
// encoder outputs instead: x [Nw][Tw][ld >= D], bf16 or fp32 as the encoder wrote `_x_bt`.  There is no blank column to cut at,
// so the cut goes where the two windows' rows agree: s(j) = -d(j), d(j) = sum_k (a_k - b_k)^2 / (sum_k a_k^2 + sum_k b_k^2) takes
// the place of b(j); candidates, scores, order and fallbacks are those of the CTC rule, in the one function `choose_cut` that
// both cut kernels call.
//
//   longform_feature_cuts_kernel: one 256-thread workgroup per junction, s(j) in the same LDS array.  Wave w takes the overlap
//     frames j = w, w + 4, ...; its lanes stride the D columns of the frame's row in either window, 16 bytes per load on the
//     vector path (base pointer and row pitch multiples of 16 bytes; the columns past the last whole 16 bytes, and every
//     column on the scalar path, go one element per lane).  Each lane keeps the two fp32 sums of its columns -- at most
//     ceil(D / 64) rounded terms each, in column order -- then the wave adds them in the fixed butterfly of wave_sum (6 steps;
//     lanes without a column add an exact 0), so either sum carries at most D + 3 roundings however D splits over the lanes,
//     and lane 0 writes -num / den (0 for den == 0; the division is correctly rounded).  Rows >= counts[n] are never read.
//   longform_stitch_rows_kernel: one wave per global frame (four frames per 256-thread workgroup), owner rule and guards of
//     longform_stitch_kernel; the owner's D elements are copied bit for bit, 16 bytes per lane and access where the two base
//     pointers and pitches allow it (the row's last bytes, and every byte otherwise, one element per lane).  It moves bytes:
//     any 2- or 4-byte element type.
//
// What the build reports (hipcc -Rpass-analysis=kernel-resource-usage, gfx950); no kernel uses scratch:
//   longform_cuts_kernel<bf16> / <float>          256 threads, 3136 B static LDS + 4 B per overlap frame (<= 48 KB), 33 / 32 VGPRs
//   longform_stitch_kernel<bf16> / <float>        256 threads, 64 B LDS, 24 / 26 VGPRs
//   longform_feature_cuts_kernel<bf16> / <float>  256 threads, 3072 B static LDS + 4 B per overlap frame (<= 48 KB);
//                                                 vector path 58 / 40 VGPRs, scalar path 26 / 24 VGPRs
//   longform_stitch_rows_kernel<2> / <4>          256 threads, no LDS; vector path 16 VGPRs, scalar path 10 VGPRs
// Every one of them leaves 8 waves per SIMD.
#include <climits>

#include "common.h"
#include "espresso_amd.h"
#include "softmax_row.h"

namespace {

constexpr int kLongformMaxOverlap = 12288;  // frames of b(j) in LDS: 48 KB

struct CutKey {
  float score;
  int dist, c;
};

__device__ __forceinline__ bool cut_better(const CutKey& a, const CutKey& b) {
  if (a.score != b.score) return a.score > b.score;
  if (a.dist != b.dist) return a.dist < b.dist;
  return a.c < b.c;
}

// score(c): min of b over [c - guard, c + guard) within the overlap [lo, hi); an empty range falls back to b at the overlap
// frame nearest c (c itself, or hi - 1 for c == hi).
__device__ __forceinline__ float cut_score(const float* b, int c, int lo, int hi, int guard) {
  const int a = max(c - guard, lo), e = min(c + guard, hi);
  if (a >= e) return b[min(max(c, lo), hi - 1) - lo];
  float s = b[a - lo];
  for (int j = a + 1; j < e; ++j) s = fminf(s, b[j - lo]);
  return s;
}

// The rule after b(j) (or s(j)) of an overlap [lo, hi) stands in LDS, for the whole workgroup (256 threads, all of them behind
// the barrier that follows the last write of b): every thread scores the candidates c = first + tid, + 256, ..., thread 0 picks
// among the 256 thread-bests, or takes the middle when there is no candidate.
__device__ __forceinline__ void choose_cut(const float* b, CutKey* best, int lo, int hi, int edge, int guard, int* cut, float* score) {
  const int tid = threadIdx.x;
  const int first = lo + edge, last = hi - edge, mid2 = lo + hi;
  CutKey k = {-INFINITY, INT_MAX, INT_MAX};
  for (int c = first + tid; c <= last; c += 256) {
    const CutKey cand = {cut_score(b, c, lo, hi, guard), abs(2 * c - mid2), c};
    if (cut_better(cand, k)) k = cand;
  }
  best[tid] = k;
  __syncthreads();
  if (tid == 0) {
    if (first > last) {
      k.c = mid2 / 2;
      k.score = cut_score(b, k.c, lo, hi, guard);
    } else {
      for (int i = 1; i < 256; ++i)
        if (cut_better(best[i], k)) k = best[i];
    }
    *cut = k.c;
    *score = k.score;
  }
}

template <typename TIn>
__global__ __launch_bounds__(256) void longform_cuts_kernel(const TIn* __restrict__ logits, long ld, const int* __restrict__ counts,
                                                            int Tw, int V, int Hf, int blank, int edge, int guard,
                                                            int* __restrict__ cuts, float* __restrict__ scores) {
  extern __shared__ float bsh[];  // [Tw - Hf]
  __shared__ float sm[16];
  __shared__ CutKey best[256];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int Tn = min(max(counts[n], 0), Tw), Tn1 = min(max(counts[n + 1], 0), Tw);
  const int lo = (n + 1) * Hf, hi = min(n * Hf + Tn, lo + Tn1);
  if (hi <= lo) {  // (uniform) no overlap: nothing to choose
    if (tid == 0) { cuts[n] = lo; scores[n] = 0.f; }
    return;
  }
  const TIn* wa = logits + ((long)n * Tw + Hf) * ld;  // window n, global frame lo
  const TIn* wb = logits + (long)(n + 1) * Tw * ld;   // window n + 1, global frame lo
  for (int j = 0; j < hi - lo; ++j) {
    const TIn* ra = wa + j * ld;
    const TIn* rb = wb + j * ld;
    const float la = log_softmax_row_lse<TIn, true>(ra, V, sm);
    const float lb = log_softmax_row_lse<TIn, true>(rb, V, sm);
    if (tid == 0) bsh[j] = fminf(lsm_ld(ra, blank) - la, lsm_ld(rb, blank) - lb);
  }
  __syncthreads();
  choose_cut(bsh, best, lo, hi, edge, guard, cuts + n, scores + n);
}

template <typename TIn>
__global__ __launch_bounds__(256) void longform_stitch_kernel(const TIn* __restrict__ logits, long ld, const int* __restrict__ counts,
                                                              const int* __restrict__ cuts, int Nw, int Tw, int V, int Hf,
                                                              float* __restrict__ out, long ldo) {
  __shared__ float sm[16];
  const int t = blockIdx.x;
  int n = min(t / Hf, Nw - 1);
  if (n > 0 && t < cuts[n - 1]) --n;
  const int j = t - n * Hf;
  if (j < 0 || j >= min(counts[n], Tw)) return;  // (uniform) the owner does not hold the frame: never read past a window
  const TIn* x = logits + ((long)n * Tw + j) * ld;
  const float lse = log_softmax_row_lse<TIn, true>(x, V, sm);
  log_softmax_row_write<TIn, true>(x, V, lse, out + (long)t * ldo);
}

// ------------------------------------------------------------------------------------------------ encoder outputs (transducers)
__device__ __forceinline__ float feat_ld(const bf16_t* p, int k) { return bf2f(p[k]); }
__device__ __forceinline__ float feat_ld(const float* p, int k) { return p[k]; }

__device__ __forceinline__ void feat_acc(float a, float b, float& num, float& den) {
  const float d = a - b;
  num = fmaf(d, d, num);
  den = fmaf(b, b, fmaf(a, a, den));
}

// this lane's share of the two sums over one frame's rows a (window n) and b (window n + 1): columns in increasing order
template <typename TIn, bool kVec>
__device__ __forceinline__ void feat_row_sums(const TIn* __restrict__ a, const TIn* __restrict__ b, int D, int lane, float& num,
                                              float& den) {
  constexpr int E = 16 / (int)sizeof(TIn);  // elements of one 16-byte load
  int k0 = 0;
  if constexpr (kVec) {
    const int chunks = D / E;
    for (int c = lane; c < chunks; c += 64) {
      const uint4 va = *reinterpret_cast<const uint4*>(a + (long)c * E);
      const uint4 vb = *reinterpret_cast<const uint4*>(b + (long)c * E);
      const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (sizeof(TIn) == 2) {
          feat_acc(__uint_as_float(wa[i] << 16), __uint_as_float(wb[i] << 16), num, den);
          feat_acc(__uint_as_float(wa[i] & 0xffff0000u), __uint_as_float(wb[i] & 0xffff0000u), num, den);
        } else {
          feat_acc(__uint_as_float(wa[i]), __uint_as_float(wb[i]), num, den);
        }
      }
    }
    k0 = chunks * E;
  }
  for (int k = k0 + lane; k < D; k += 64) feat_acc(feat_ld(a, k), feat_ld(b, k), num, den);
}

template <typename TIn, bool kVec>
__global__ __launch_bounds__(256) void longform_feature_cuts_kernel(const TIn* __restrict__ x, long ld, const int* __restrict__ counts,
                                                                    int Tw, int D, int Hf, int edge, int guard,
                                                                    int* __restrict__ cuts, float* __restrict__ scores) {
  extern __shared__ float bsh[];  // [Tw - Hf]: s(j)
  __shared__ CutKey best[256];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tn = min(max(counts[n], 0), Tw), Tn1 = min(max(counts[n + 1], 0), Tw);
  const int lo = (n + 1) * Hf, hi = min(n * Hf + Tn, lo + Tn1);
  if (hi <= lo) {  // (uniform) no overlap: nothing to choose
    if (tid == 0) { cuts[n] = lo; scores[n] = 0.f; }
    return;
  }
  const TIn* wa = x + ((long)n * Tw + Hf) * ld;  // window n, global frame lo: rows Hf .. Hf + (hi - lo) - 1 < counts[n]
  const TIn* wb = x + (long)(n + 1) * Tw * ld;   // window n + 1, global frame lo: rows 0 .. (hi - lo) - 1 < counts[n + 1]
  for (int j = wave; j < hi - lo; j += 4) {
    float num = 0.f, den = 0.f;
    feat_row_sums<TIn, kVec>(wa + (long)j * ld, wb + (long)j * ld, D, lane, num, den);
    num = wave_sum(num);
    den = wave_sum(den);
    if (lane == 0) bsh[j] = den > 0.f ? -__fdiv_rn(num, den) : 0.f;
  }
  __syncthreads();
  choose_cut(bsh, best, lo, hi, edge, guard, cuts + n, scores + n);
}

// units [first, first + count) of a row, one TUnit per lane and access
template <typename TUnit>
__device__ __forceinline__ void copy_units(const char* __restrict__ src, char* __restrict__ dst, long first, long count, int lane) {
  const TUnit* s = reinterpret_cast<const TUnit*>(src) + first;
  TUnit* d = reinterpret_cast<TUnit*>(dst) + first;
  for (long i = lane; i < count; i += 64) d[i] = s[i];
}

// kVec: both base pointers and both row pitches are multiples of 16 bytes; kElem: the element size in bytes, 2 or 4
template <bool kVec, int kElem>
__global__ __launch_bounds__(256) void longform_stitch_rows_kernel(const char* __restrict__ x, long ld_bytes, const int* __restrict__ counts,
                                                                   const int* __restrict__ cuts, int Nw, int Tw, int D, int Hf, int T,
                                                                   char* __restrict__ out, long ldo_bytes) {
  using TElem = std::conditional_t<kElem == 4, uint32_t, uint16_t>;
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);  // (uniform over the wave)
  if (t >= T) return;
  int n = min(t / Hf, Nw - 1);
  if (n > 0 && t < cuts[n - 1]) --n;
  const int j = t - n * Hf;
  if (j < 0 || j >= min(counts[n], Tw)) return;  // the owner does not hold the frame: never read past a window
  const char* src = x + ((long)n * Tw + j) * ld_bytes;
  char* dst = out + (long)t * ldo_bytes;
  long done = 0;  // elements copied by the 16-byte accesses
  if constexpr (kVec) {
    const long v = (long)D * kElem / 16;
    copy_units<uint4>(src, dst, 0, v, lane);
    done = v * (16 / kElem);
  }
  copy_units<TElem>(src, dst, done, D - done, lane);
}

}  // namespace

extern "C" int ea_longform_cuts(const void* logits, int is_bf16, long ld, const int* counts, int Nw, int Tw, int V, int Hf,
                                int blank, int edge, int guard, int* cuts, float* scores, hipStream_t stream) {
  if (Nw < 1 || Tw < 1 || V < 1 || ld < V || Hf < 1 || Hf > Tw || blank < 0 || blank >= V || edge < 0 || guard < 0) return -2;
  if ((long)Nw * Hf + Tw > INT_MAX) return -2;
  if (Nw == 1) return 0;
  const int ov = Tw - Hf;
  if (ov < 1 || ov > kLongformMaxOverlap) return -2;
  const size_t lds = (size_t)ov * sizeof(float);
  if (is_bf16)
    hipLaunchKernelGGL((longform_cuts_kernel<bf16_t>), dim3((unsigned)(Nw - 1)), dim3(256), lds, stream, (const bf16_t*)logits, ld,
                       counts, Tw, V, Hf, blank, edge, guard, cuts, scores);
  else
    hipLaunchKernelGGL((longform_cuts_kernel<float>), dim3((unsigned)(Nw - 1)), dim3(256), lds, stream, (const float*)logits, ld,
                       counts, Tw, V, Hf, blank, edge, guard, cuts, scores);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_longform_stitch(const void* logits, int is_bf16, long ld, const int* counts, const int* cuts, int Nw, int Tw,
                                  int V, int Hf, long T, float* out, long ldo, hipStream_t stream) {
  if (Nw < 1 || Tw < 1 || V < 1 || ld < V || ldo < V || Hf < 1 || Hf > Tw || T < 0) return -2;
  if (T > (long)(Nw - 1) * Hf + Tw || T > INT_MAX) return -2;  // no frame beyond the last window
  if (Nw > 1 && 2L * Hf <= Tw) return -2;                    // three windows would share a frame: the cuts could cross
  if (T == 0) return 0;
  if (is_bf16)
    hipLaunchKernelGGL((longform_stitch_kernel<bf16_t>), dim3((unsigned)T), dim3(256), 0, stream, (const bf16_t*)logits, ld, counts,
                       cuts, Nw, Tw, V, Hf, out, ldo);
  else
    hipLaunchKernelGGL((longform_stitch_kernel<float>), dim3((unsigned)T), dim3(256), 0, stream, (const float*)logits, ld, counts, cuts,
                       Nw, Tw, V, Hf, out, ldo);
  return EA_CHECK_LAUNCH();
}

static bool aligned16(const void* p, long pitch_bytes) { return ((uintptr_t)p & 15) == 0 && (pitch_bytes & 15) == 0; }

template <typename TIn>
static void launch_feature_cuts(const void* x, long ld, const int* counts, int Nw, int Tw, int D, int Hf, int edge, int guard, int* cuts,
                                float* scores, hipStream_t stream) {
  const size_t lds = (size_t)(Tw - Hf) * sizeof(float);
  const dim3 grid((unsigned)(Nw - 1)), block(256);
  if (aligned16(x, ld * (long)sizeof(TIn)))
    hipLaunchKernelGGL((longform_feature_cuts_kernel<TIn, true>), grid, block, lds, stream, (const TIn*)x, ld, counts, Tw, D, Hf, edge,
                       guard, cuts, scores);
  else
    hipLaunchKernelGGL((longform_feature_cuts_kernel<TIn, false>), grid, block, lds, stream, (const TIn*)x, ld, counts, Tw, D, Hf, edge,
                       guard, cuts, scores);
}

extern "C" int ea_longform_feature_cuts(const void* x, int is_bf16, long ld, const int* counts, int Nw, int Tw, int D, int Hf, int edge,
                                        int guard, int* cuts, float* scores, hipStream_t stream) {
  if (Nw < 1 || Tw < 1 || D < 1 || ld < D || Hf < 1 || Hf > Tw || edge < 0 || guard < 0) return -2;
  if ((long)Nw * Hf + Tw > INT_MAX) return -2;
  if (Nw == 1) return 0;
  const int ov = Tw - Hf;
  if (ov < 1 || ov > kLongformMaxOverlap || !x || !counts || !cuts || !scores) return -2;
  if (is_bf16)
    launch_feature_cuts<bf16_t>(x, ld, counts, Nw, Tw, D, Hf, edge, guard, cuts, scores, stream);
  else
    launch_feature_cuts<float>(x, ld, counts, Nw, Tw, D, Hf, edge, guard, cuts, scores, stream);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_longform_stitch_rows(const void* x, int elem_bytes, long ld, const int* counts, const int* cuts, int Nw, int Tw, int D,
                                       int Hf, long T, void* out, long ldo, hipStream_t stream) {
  if (Nw < 1 || Tw < 1 || D < 1 || ld < D || ldo < D || Hf < 1 || Hf > Tw || T < 0 || (elem_bytes != 2 && elem_bytes != 4)) return -2;
  if (T > (long)(Nw - 1) * Hf + Tw || T > INT_MAX) return -2;  // no frame beyond the last window
  if (Nw > 1 && 2L * Hf <= Tw) return -2;                    // three windows would share a frame: the cuts could cross
  if (T == 0) return 0;
  if (!x || !counts || !out || (Nw > 1 && !cuts)) return -2;
  const long ldb = ld * elem_bytes, ldob = ldo * elem_bytes;
  const dim3 grid((unsigned)((T + 3) / 4)), block(256);
  const bool vec = aligned16(x, ldb) && aligned16(out, ldob);
#define EA_ROWS(kVec, kElem)                                                                                                          \
  hipLaunchKernelGGL((longform_stitch_rows_kernel<kVec, kElem>), grid, block, 0, stream, (const char*)x, ldb, counts, cuts, Nw, Tw, D, \
                     Hf, (int)T, (char*)out, ldob)
  if (elem_bytes == 2) {
    if (vec) EA_ROWS(true, 2); else EA_ROWS(false, 2);
  } else {
    if (vec) EA_ROWS(true, 4); else EA_ROWS(false, 4);
  }
#undef EA_ROWS
  return EA_CHECK_LAUNCH();
}
