// Stand-alone host check of the keyword spotter's host twin under AddressSanitizer / UBSan (no GPU, nothing loaded into
// Python).  Build, from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//     -Iinclude -Iespresso_amd/csrc espresso_amd/csrc/kws.hip tests/kws_asan_main.cpp -o kws_asan
// Run: kws_asan.  It drives ea_ctc_kws_host over the extreme shapes -- T = 0, L = 1, L = 64 (= Lmax), ld > V, max_hits = 1,
// inactive keywords -- with every array allocated at its exact size, so that an access one element past an end is reported, and
// prints a checksum per case.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "espresso_amd.h"

static uint32_t rng_state = 2024u;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }
static float unif() { return (float)(rnd() >> 8) / 16777216.0f; }

// log-probs [T][ld] of random peaked rows over V; the columns from V on hold +9 (a row maximum that reads them shows up)
static std::vector<float> lprobs(int T, int V, long ld) {
  std::vector<float> x((size_t)T * ld, 9.0f);
  for (int t = 0; t < T; ++t) {
    std::vector<double> z(V);
    double s = 0;
    const int peak = rnd() % V;
    for (int v = 0; v < V; ++v) { z[v] = std::exp(4.0 * unif() + (v == peak ? 5.0 : 0.0)); s += z[v]; }
    for (int v = 0; v < V; ++v) x[(size_t)t * ld + v] = (float)std::log(z[v] / s);
  }
  return x;
}

static int run(const char* name, int T, int V, long ld, int K, int Lmax, int fixed_len, int hold, int max_hits, int spoil) {
  const std::vector<float> x = lprobs(T, V, ld);
  std::vector<int> tok((size_t)K * Lmax), len(K);
  std::vector<float> tau(K);
  for (int k = 0; k < K; ++k) {
    len[k] = fixed_len > 0 ? fixed_len : 1 + (int)(rnd() % Lmax);
    for (int u = 0; u < Lmax; ++u) tok[(size_t)k * Lmax + u] = 1 + (int)(rnd() % (V - 1));
    tau[k] = (float)len[k] * std::log(0.001f);  // (low enough for random phrases to be found: the emit path runs too)
  }
  if (spoil) {  // inactive keywords: a length past Lmax, a zero length, the blank, ids outside [0, V)
    len[0] = Lmax + 1;
    if (K > 1) len[1] = 0;
    if (K > 2) tok[(size_t)2 * Lmax] = 0;
    if (K > 3) tok[(size_t)3 * Lmax + len[3] - 1] = V;
    if (K > 4) tok[(size_t)4 * Lmax] = -1;
  }
  std::vector<int> starts((size_t)K * max_hits), ends((size_t)K * max_hits), counts(K);
  std::vector<float> scores((size_t)K * max_hits);
  const int rc = ea_ctc_kws_host(T ? x.data() : nullptr, ld, T, V, tok.data(), len.data(), tau.data(), K, Lmax, 0, hold, max_hits,
                                 starts.data(), ends.data(), scores.data(), counts.data());
  if (rc != 0) { fprintf(stderr, "%s: ea_ctc_kws_host returned %d\n", name, rc); return 1; }
  long total = 0, stored = 0;
  double sum = 0;
  for (int k = 0; k < K; ++k) {
    total += counts[k];
    for (int h = 0; h < max_hits && h < counts[k]; ++h) {
      const size_t i = (size_t)k * max_hits + h;
      if (starts[i] < 0 || ends[i] < starts[i] || ends[i] >= T || !(scores[i] <= 0.f)) { fprintf(stderr, "%s: bad hit\n", name); return 1; }
      ++stored;
      sum += scores[i];
    }
    if (spoil && k < 5 && counts[k] != 0) { fprintf(stderr, "%s: an inactive keyword has hits\n", name); return 1; }
  }
  printf("%s: %ld hits (%ld stored), checksum %.6f\n", name, total, stored, sum);
  return 0;
}

int main() {
  int bad = 0;
  bad |= run("T=0", 0, 7, 7, 4, 6, 0, 0, 2, 0);
  bad |= run("L=1", 50, 7, 7, 6, 1, 1, 0, 2, 0);
  bad |= run("L=64", 200, 70, 70, 3, 64, 64, 3, 2, 0);
  bad |= run("L=64 of Lmax 64, mixed", 120, 9, 13, 8, 64, 0, 5, 3, 0);
  bad |= run("ld>V", 70, 7, 11, 9, 6, 0, 3, 2, 0);
  bad |= run("max_hits=1", 70, 5, 8, 9, 4, 0, 0, 1, 0);
  bad |= run("inactive", 40, 7, 9, 7, 5, 0, 100, 2, 1);
  bad |= run("T<L", 3, 7, 7, 5, 6, 6, 0, 1, 0);
  // refused arguments launch nothing and touch nothing
  int one = 0;
  float f = 0.f;
  if (ea_ctc_kws_host(&f, 1, 1, 2, &one, &one, &f, 1, 1, 0, 0, 1, &one, &one, &f, &one) != -2) { fprintf(stderr, "ld < V taken\n"); bad = 1; }
  if (ea_ctc_kws_host(&f, 1, 1, 1, &one, &one, &f, 1, 65, 0, 0, 1, &one, &one, &f, &one) != -2) { fprintf(stderr, "Lmax 65 taken\n"); bad = 1; }
  if (ea_ctc_kws_state_bytes(1, 64, 1) != 4L * (2 + 266) || ea_ctc_kws_state_bytes(1, 65, 1) != 0) { fprintf(stderr, "state bytes\n"); bad = 1; }
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
