// Keyword spotting on CTC log-probs for gfx950, offline and streamed: per (stream, keyword) pair a max-plus scan over the frames
// with a free start frame, the state carried from piece to piece in the stream's slot.  The reference has nothing of the kind;
// it is the family of align.hip (the lattice without its outer blanks, scores relative to the greedy path) with the slot
// conventions of the streamed searches.  The rule -- the frame update, the detection and the emit -- is written once, in the
// __host__ __device__ functions below, and is normative in include/espresso_amd.h: the kernel and ea_ctc_kws_host both go through
// them, and every operation is a max, one add or one subtract, so the two agree bit for bit.
//
// Two launches per step:
//   kws_prepare_kernel: one wave per row of x takes the row maximum g_t (16-byte loads when ld and the base allow them, 4-byte
//     loads otherwise; a maximum does not depend on the order), and the first n threads of the grid do the entries' frame
//     bookkeeping: slot word [1] = the stream frame of the piece's first row, word [0] += n_new.  The scan of one entry is spread
//     over ceil(K / 4) workgroups, so none of them can advance the counter the others still have to read.
//   kws_scan_kernel: 256-thread workgroups, one keyword per wave, grid (ceil(K / 4), n); no LDS and no barrier.  Lane u owns
//     tok_{u+1} and blk_{u+1}, so every move needs the four values (e, b) x (tok, blk) of lane u - 1: one cross-lane shift per
//     frame.  The scan is a dependent chain of n_new steps, but its loads (the lane's token column, the blank column and g_t of a
//     row) do not depend on the state: they are requested kKwsAhead = 8 frames ahead into eight register sets from a frame clamped to
//     the entry's own rows, every lane loading (no load in a divergent branch); the loop runs n_new rounded up
//     to eight frames and the frames past the end keep the state.  The lane that holds tok_L keeps the detection state in registers
//     and writes the hit list with ordinary stores: a (slot, keyword) pair has one owner, no atomics.
#include <vector>

#include "common.h"
#include "espresso_amd.h"

namespace {

constexpr int kKwsMaxL = 64;  // tokens per keyword: one lane each
constexpr int kKwsDetWords = 6;  // open.start, open.end, open.e, last_end, count, 0
constexpr int kKwsAhead = 8;     // frames whose loads are in flight ahead of the scan

// (an even count: the (e, b) pairs of a lane are 8-byte accesses)
__host__ __device__ __forceinline__ long kws_kw_words(int Lmax, int max_hits) { return (4L * Lmax + kKwsDetWords + 3L * max_hits + 1) & ~1L; }
__host__ __device__ __forceinline__ long kws_slot_words(int K, int Lmax, int max_hits) { return 2 + K * kws_kw_words(Lmax, max_hits); }

// ---- the rule (include/espresso_amd.h, "Keyword spotting") ----

__host__ __device__ __forceinline__ void kws_pick(float& e, int& b, float ce, int cb) {
  if (ce > e) { e = ce; b = cb; }  // the first of the candidates with the largest e
}

__host__ __device__ __forceinline__ void kws_close(float& e, int& b, float d) {
  if (e == -INFINITY) b = -1; else e = e + d;
}

// One frame for tok_{u+1} = (te, tb) and blk_{u+1} = (be, bb); (pte, ptb) / (pbe, pbb) are tok_u / blk_u before the frame.
// first: u == 0; skip: the token differs from the one before it; has_blk: u + 1 < L; dtok / dblk: d_t of the token / of blank.
__host__ __device__ __forceinline__ void kws_update(float& te, int& tb, float& be, int& bb, float pte, int ptb, float pbe, int pbb,
                                                    bool first, bool skip, bool has_blk, float dtok, float dblk, int t) {
  float e = te, e2 = be;
  int b = tb, b2 = bb;
  if (first) {
    kws_pick(e, b, 0.f, t);  // a fresh start
  } else {
    kws_pick(e, b, pbe, pbb);            // step, from blk_u
    if (skip) kws_pick(e, b, pte, ptb);  // skip, from tok_u
  }
  kws_pick(e2, b2, te, tb);  // blk: stay, then step from tok_{u+1}
  kws_close(e, b, dtok);
  kws_close(e2, b2, dblk);
  te = e; tb = b;
  if (has_blk) { be = e2; bb = b2; }
}

struct KwsDet {
  int open_s, open_e;  // the open hit, open_s < 0: none
  float open_sc;
  int last_end, count;
};

struct KwsList {
  int *starts, *ends;
  float* scores;
  int max_hits;
};

__host__ __device__ __forceinline__ void kws_emit(KwsDet& d, const KwsList& l) {
  if (d.count < l.max_hits) {
    l.starts[d.count] = d.open_s;
    l.ends[d.count] = d.open_e;
    l.scores[d.count] = d.open_sc;
  }
  ++d.count;
  d.last_end = d.open_e;
  d.open_s = -1;
}

// after the update of frame t: (e, b) of tok_L
__host__ __device__ __forceinline__ void kws_detect(KwsDet& d, const KwsList& l, float e, int b, int t, float tau, int hold) {
  if (e >= tau && b > d.last_end) {
    bool take = true;
    if (d.open_s >= 0) {
      if (b <= d.open_e) take = e >= d.open_sc;  // overlap: the better one, a tie to the later end
      else kws_emit(d, l);
    }
    if (take) { d.open_s = b; d.open_e = t; d.open_sc = e; }
  }
  if (d.open_s >= 0 && t - d.open_e > hold) kws_emit(d, l);
}

__host__ __device__ __forceinline__ KwsDet kws_det_init() { return KwsDet{-1, -1, 0.f, -1, 0}; }

__host__ __device__ __forceinline__ bool kws_token_ok(int y, int V, int blank) { return y >= 0 && y < V && y != blank; }

// ---- device ----

struct KwsArgs {
  const float* x;
  long ld, total_rows;
  float* rowmax;
  const int *slot_idx, *n_new, *row_off;
  int n;
  int* state;
  const int *kw_tokens, *kw_len;
  const float* kw_tau;
  int max_streams, K, Lmax, max_hits, V, blank, hold;
};

__device__ __forceinline__ bool kws_entry_ok(const KwsArgs& a, int ent, int& slot, int& nn, long& r0) {
  slot = a.slot_idx[ent];
  nn = a.n_new[ent];
  r0 = a.row_off[ent];
  return slot >= 0 && slot < a.max_streams && nn > 0 && r0 >= 0 && r0 + nn <= a.total_rows;
}

__global__ __launch_bounds__(256) void kws_prepare_kernel(const KwsArgs a, int vec) {
  const int lane = threadIdx.x & 63;
  const long gtid = (long)blockIdx.x * 256 + threadIdx.x;
  const long slot_words = kws_slot_words(a.K, a.Lmax, a.max_hits);
  for (long i = gtid; i < a.n; i += (long)gridDim.x * 256) {
    int slot, nn;
    long r0;
    if (!kws_entry_ok(a, (int)i, slot, nn, r0)) continue;
    int* w = a.state + slot * slot_words;
    const int c = w[0];
    w[1] = c;
    w[0] = c + nn;
  }
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.total_rows) return;
  const float* r = a.x + row * a.ld;
  float m = -INFINITY;
  int v0 = 0;
  if (vec) {
    v0 = a.V & ~3;
#pragma unroll 4
    for (int v = 4 * lane; v < v0; v += 256) {
      const float4 q = *reinterpret_cast<const float4*>(r + v);
      m = fmaxf(fmaxf(m, fmaxf(q.x, q.y)), fmaxf(q.z, q.w));
    }
  }
#pragma unroll 4
  for (int v = v0 + lane; v < a.V; v += 64) m = fmaxf(m, r[v]);
  m = wave_max(m);
  if (lane == 0) a.rowmax[row] = m;
}

struct KwsFrame {
  float y, b, g;  // x_t[token], x_t[blank], g_t
};

__global__ __launch_bounds__(256) void kws_scan_kernel(const KwsArgs a) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= a.K) return;
  int slot, nn;
  long r0;
  if (!kws_entry_ok(a, blockIdx.y, slot, nn, r0)) return;
  const int L = a.kw_len[k];
  if (L < 1 || L > a.Lmax) return;
  const int y = a.kw_tokens[(long)k * a.Lmax + min(lane, L - 1)];
  if (__ballot(!kws_token_ok(y, a.V, a.blank)) != 0ull) return;  // an inactive keyword: never a candidate
  const int yp = __shfl_up(y, 1, 64);
  const bool act = lane < L, first = lane == 0, skip = lane > 0 && y != yp, has_blk = lane + 1 < L, last = lane == L - 1;
  const float tau = a.kw_tau[k];

  int* slot_w = a.state + slot * kws_slot_words(a.K, a.Lmax, a.max_hits);
  int* kw_w = slot_w + 2 + k * kws_kw_words(a.Lmax, a.max_hits);
  float* st_e = reinterpret_cast<float*>(kw_w);
  int* st_b = kw_w + 2 * a.Lmax;
  int* det_w = kw_w + 4 * a.Lmax;
  const KwsList list{det_w + kKwsDetWords, det_w + kKwsDetWords + a.max_hits,
                     reinterpret_cast<float*>(det_w + kKwsDetWords + 2 * a.max_hits), a.max_hits};
  const int t0 = slot_w[1];  // the stream frame of this piece's first row (kws_prepare_kernel)

  float te = -INFINITY, be = -INFINITY;
  int tb = -1, bb = -1;
  if (act) {
    const float2 e2 = *reinterpret_cast<const float2*>(st_e + 2 * lane);
    const int2 b2 = *reinterpret_cast<const int2*>(st_b + 2 * lane);
    te = e2.x; be = e2.y; tb = b2.x; bb = b2.y;
  }
  KwsDet det = kws_det_init();
  if (last) {
    det.open_s = det_w[0]; det.open_e = det_w[1]; det.open_sc = __int_as_float(det_w[2]);
    det.last_end = det_w[3]; det.count = det_w[4];
  }

  const float* xb = a.x + r0 * a.ld;
  const float* gb = a.rowmax + r0;
  auto fetch = [&](int j, KwsFrame& f) {
    const long jj = min(j, nn - 1);  // clamped to the entry's own rows
    const float* r = xb + jj * a.ld;
    f.y = r[y];
    f.b = r[a.blank];
    f.g = gb[jj];
  };
  auto step = [&](int j, KwsFrame& q) {
    const float dtok = q.y - q.g, dblk = q.b - q.g;
    const bool live = j < nn;
    const float pte = __shfl_up(te, 1, 64), pbe = __shfl_up(be, 1, 64);
    const int ptb = __shfl_up(tb, 1, 64), pbb = __shfl_up(bb, 1, 64);
    fetch(j + kKwsAhead, q);  // (after the last use of the set)
    if (live && act) {
      kws_update(te, tb, be, bb, pte, ptb, pbe, pbb, first, skip, has_blk, dtok, dblk, t0 + j);
      if (last) kws_detect(det, list, te, tb, t0 + j, tau, a.hold);
    }
  };
  KwsFrame q[kKwsAhead];  // (indexed by constants only after the unrolling: registers)
#pragma unroll
  for (int i = 0; i < kKwsAhead; ++i) fetch(i, q[i]);
  for (int j = 0; j < nn; j += kKwsAhead) {
#pragma unroll
    for (int i = 0; i < kKwsAhead; ++i) step(j + i, q[i]);
  }

  if (act) {
    *reinterpret_cast<float2*>(st_e + 2 * lane) = make_float2(te, be);
    *reinterpret_cast<int2*>(st_b + 2 * lane) = make_int2(tb, bb);
  }
  if (last) {
    det_w[0] = det.open_s; det_w[1] = det.open_e; det_w[2] = __float_as_int(det.open_sc);
    det_w[3] = det.last_end; det_w[4] = det.count;
  }
}

// one workgroup per listed slot
__global__ __launch_bounds__(256) void kws_reset_kernel(int* state, const int* slots, int max_streams, int K, int Lmax, int max_hits) {
  const int slot = slots[blockIdx.x];
  if (slot < 0 || slot >= max_streams) return;
  const long kw_words = kws_kw_words(Lmax, max_hits), slot_words = kws_slot_words(K, Lmax, max_hits);
  int* w = state + slot * slot_words;
  if (threadIdx.x < 2) w[threadIdx.x] = 0;
  const int neg_inf = __float_as_int(-INFINITY);
  for (long i = threadIdx.x; i < slot_words - 2; i += 256) {
    const int j = (int)(i % kw_words);
    int v;
    if (j < 2 * Lmax) v = neg_inf;                             // e
    else if (j < 4 * Lmax) v = -1;                             // b
    else if (j < 4 * Lmax + kKwsDetWords) {
      const int d = j - 4 * Lmax;
      v = (d == 0 || d == 1 || d == 3) ? -1 : 0;               // open.start, open.end, last_end; open.e, count, 0
    } else v = j < 4 * Lmax + kKwsDetWords + 2 * max_hits ? -1 : 0;  // starts, ends; scores
    w[2 + i] = v;
  }
}

// one workgroup per listed slot, one thread per keyword
__global__ __launch_bounds__(256) void kws_hits_kernel(int* state, const int* slots, int flush, int clear, int max_streams, int K,
                                                       int Lmax, int max_hits, int* starts, int* ends, float* scores, int* counts) {
  const int i = blockIdx.x, slot = slots[i];
  const bool ok = slot >= 0 && slot < max_streams;
  for (int k = threadIdx.x; k < K; k += 256) {
    const long o = ((long)i * K + k) * max_hits;
    int cnt = 0;
    if (ok) {
      int* det_w = state + slot * kws_slot_words(K, Lmax, max_hits) + 2 + k * kws_kw_words(Lmax, max_hits) + 4 * Lmax;
      const KwsList list{det_w + kKwsDetWords, det_w + kKwsDetWords + max_hits,
                         reinterpret_cast<float*>(det_w + kKwsDetWords + 2 * max_hits), max_hits};
      KwsDet det{det_w[0], det_w[1], __int_as_float(det_w[2]), det_w[3], det_w[4]};
      if (flush && det.open_s >= 0) {
        kws_emit(det, list);
        det_w[0] = det.open_s; det_w[3] = det.last_end;
      }
      cnt = det.count;
      const int m = min(cnt, max_hits);
      for (int h = 0; h < max_hits; ++h) {
        starts[o + h] = h < m ? list.starts[h] : -1;
        ends[o + h] = h < m ? list.ends[h] : -1;
        scores[o + h] = h < m ? list.scores[h] : 0.f;
      }
      det_w[4] = clear ? 0 : cnt;
    } else {
      for (int h = 0; h < max_hits; ++h) { starts[o + h] = -1; ends[o + h] = -1; scores[o + h] = 0.f; }
    }
    counts[(long)i * K + k] = cnt;
  }
}

bool kws_sizes_ok(int K, int Lmax, int max_hits) { return K >= 1 && Lmax >= 1 && Lmax <= kKwsMaxL && max_hits >= 1; }

}  // namespace

extern "C" long ea_ctc_kws_state_bytes(int K, int Lmax, int max_hits) {
  if (!kws_sizes_ok(K, Lmax, max_hits)) return 0;
  return 4L * kws_slot_words(K, Lmax, max_hits);
}

extern "C" int ea_ctc_kws_reset(void* state, const int* slots, int n, int max_streams, int K, int Lmax, int max_hits,
                                ea_stream_t stream) {
  if (n <= 0) return 0;
  if (!state || !slots || max_streams < 1 || !kws_sizes_ok(K, Lmax, max_hits)) return -2;
  hipLaunchKernelGGL(kws_reset_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (int*)state, slots, max_streams, K, Lmax, max_hits);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_kws_step(const float* x, long ld, long total_rows, float* rowmax, const int* slot_idx, const int* n_new,
                               const int* row_off, int n, void* state, const int* kw_tokens, const int* kw_len, const float* kw_tau,
                               int max_streams, int K, int Lmax, int max_hits, int V, int blank, int hold, ea_stream_t stream) {
  if (n <= 0) return 0;
  if (!slot_idx || !n_new || !row_off || !state || !kw_tokens || !kw_len || !kw_tau || max_streams < 1 ||
      !kws_sizes_ok(K, Lmax, max_hits) || V < 1 || ld < V || blank < 0 || blank >= V || hold < 0 || total_rows < 0 ||
      total_rows > (1L << 31) || (total_rows > 0 && (!x || !rowmax)))
    return -2;
  if (total_rows == 0) return 0;  // no entry can have a frame
  KwsArgs a;
  a.x = x; a.ld = ld; a.total_rows = total_rows; a.rowmax = rowmax;
  a.slot_idx = slot_idx; a.n_new = n_new; a.row_off = row_off; a.n = n;
  a.state = (int*)state; a.kw_tokens = kw_tokens; a.kw_len = kw_len; a.kw_tau = kw_tau;
  a.max_streams = max_streams; a.K = K; a.Lmax = Lmax; a.max_hits = max_hits; a.V = V; a.blank = blank; a.hold = hold;
  const int vec = (ld & 3) == 0 && ((uintptr_t)x & 15) == 0;
  hipLaunchKernelGGL(kws_prepare_kernel, dim3((unsigned)((total_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, vec);
  hipLaunchKernelGGL(kws_scan_kernel, dim3((K + 3) / 4, n), dim3(256), 0, (hipStream_t)stream, a);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_kws_hits(void* state, const int* slots, int n, int flush, int clear, int max_streams, int K, int Lmax,
                               int max_hits, int* starts, int* ends, float* scores, int* counts, ea_stream_t stream) {
  if (n <= 0) return 0;
  if (!state || !slots || max_streams < 1 || !kws_sizes_ok(K, Lmax, max_hits) || !starts || !ends || !scores || !counts) return -2;
  hipLaunchKernelGGL(kws_hits_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (int*)state, slots, flush, clear, max_streams, K,
                     Lmax, max_hits, starts, ends, scores, counts);
  return EA_CHECK_LAUNCH();
}

extern "C" int ea_ctc_kws_host(const float* x_host, long ld, int T, int V, const int* kw_tokens, const int* kw_len,
                               const float* kw_tau, int K, int Lmax, int blank, int hold, int max_hits, int* starts, int* ends,
                               float* scores, int* counts) {
  if (T < 0 || (T > 0 && !x_host) || V < 1 || ld < V || !kw_tokens || !kw_len || !kw_tau || !kws_sizes_ok(K, Lmax, max_hits) ||
      blank < 0 || blank >= V || hold < 0 || !starts || !ends || !scores || !counts)
    return -2;
  std::vector<float> rowmax((size_t)T);
  for (int t = 0; t < T; ++t) {
    const float* r = x_host + (long)t * ld;
    float g = -INFINITY;
    for (int v = 0; v < V; ++v) g = fmaxf(g, r[v]);
    rowmax[t] = g;
  }
  std::vector<float> e(2 * (size_t)Lmax);
  std::vector<int> b(2 * (size_t)Lmax);
  for (int k = 0; k < K; ++k) {
    const KwsList list{starts + (long)k * max_hits, ends + (long)k * max_hits, scores + (long)k * max_hits, max_hits};
    for (int h = 0; h < max_hits; ++h) { list.starts[h] = -1; list.ends[h] = -1; list.scores[h] = 0.f; }
    counts[k] = 0;
    const int L = kw_len[k];
    const int* y = kw_tokens + (long)k * Lmax;
    bool active = L >= 1 && L <= Lmax;
    for (int u = 0; active && u < L; ++u) active = kws_token_ok(y[u], V, blank);
    if (!active) continue;
    for (int s = 0; s < 2 * Lmax; ++s) { e[s] = -INFINITY; b[s] = -1; }
    KwsDet det = kws_det_init();
    for (int t = 0; t < T; ++t) {
      const float* r = x_host + (long)t * ld;
      const float g = rowmax[t], dblk = r[blank] - g;
      for (int u = L - 1; u >= 0; --u) {  // downwards: lane u - 1 still holds the values before the frame
        const float pte = u > 0 ? e[2 * u - 2] : -INFINITY, pbe = u > 0 ? e[2 * u - 1] : -INFINITY;
        const int ptb = u > 0 ? b[2 * u - 2] : -1, pbb = u > 0 ? b[2 * u - 1] : -1;
        kws_update(e[2 * u], b[2 * u], e[2 * u + 1], b[2 * u + 1], pte, ptb, pbe, pbb, u == 0, u > 0 && y[u] != y[u - 1], u + 1 < L,
                   r[y[u]] - g, dblk, t);
      }
      kws_detect(det, list, e[2 * L - 2], b[2 * L - 2], t, kw_tau[k], hold);
    }
    if (det.open_s >= 0) kws_emit(det, list);  // the flush at the audio's end
    counts[k] = det.count;
  }
  return 0;
}
