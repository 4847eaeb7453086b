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
  const int first = lo + edge, last = hi - edge, mid2 = lo + hi;
  CutKey k = {-INFINITY, INT_MAX, INT_MAX};
  for (int c = first + tid; c <= last; c += 256) {
    const CutKey cand = {cut_score(bsh, c, lo, hi, guard), abs(2 * c - mid2), c};
    if (cut_better(cand, k)) k = cand;
  }
  best[tid] = k;
  __syncthreads();
  if (tid == 0) {
    if (first > last) {
      k.c = mid2 / 2;
      k.score = cut_score(bsh, k.c, lo, hi, guard);
    } else {
      for (int i = 1; i < 256; ++i)
        if (cut_better(best[i], k)) k = best[i];
    }
    cuts[n] = k.c;
    scores[n] = k.score;
  }
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
