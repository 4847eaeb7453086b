// Stand-alone host check of the ARPA loader and the host n-gram rows under AddressSanitizer / UBSan (no GPU, nothing loaded
// into Python).  Build, from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//     -Iinclude -Iespresso_amd/csrc espresso_amd/csrc/ctc_lexicon_beam.hip espresso_amd/csrc/ngram_rows.hip \
//     tests/ngram_rows_asan_main.cpp -o ngram_rows_asan
// Run: ngram_rows_asan a.arpa b.arpa ...  For every file: ea_ngram_create, a dictionary of the file's words plus a pad-like
// (-2) and an unknown (-1) column with every seventh word dropped to -1, the start rows, then 40 steps of random
// (parent, token, keep) triples through ea_ngram_token_rows_host with alternating context buffers; prints a checksum per file.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "espresso_amd.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s file.arpa ...\n", argv[0]); return 2; }
  for (int f = 1; f < argc; ++f) {
    void* lm = nullptr;
    char err[512] = "";
    if (ea_ngram_create(argv[f], &lm, err, sizeof(err)) != 0) { fprintf(stderr, "%s\n", err); return 1; }
    int meta[4];
    long counts[6];
    ea_ngram_info(lm, meta, counts);
    const int order = meta[0], bos = meta[2], n1 = (int)counts[0], W = order - 1;
    const int V = n1 + 2;
    std::vector<int> t2w(V);
    for (int v = 0; v < n1; ++v) t2w[v] = v == bos ? -2 : (v % 7 == 6 ? -1 : v);
    t2w[n1] = -2; t2w[n1 + 1] = -1;
    const int N = 13;
    const long ld = V + 3;
    std::vector<int> ctx[2] = {std::vector<int>((size_t)N * W + 1), std::vector<int>((size_t)N * W + 1)};
    std::vector<int> parent(N), token(N);
    std::vector<uint8_t> keep(N);
    std::vector<float> rows((size_t)N * ld);
    if (ea_ngram_token_rows_host(lm, t2w.data(), V, nullptr, nullptr, nullptr, nullptr, N, ctx[0].data(), rows.data(), ld) != 0) return 1;
    double sum = 0;
    long ninf = 0;
    for (int step = 0; step < 40; ++step) {
      for (int i = 0; i < N; ++i) { parent[i] = rnd() % N; token[i] = rnd() % V; keep[i] = rnd() % 3 == 0; }
      if (ea_ngram_token_rows_host(lm, t2w.data(), V, ctx[step & 1].data(), parent.data(), token.data(), keep.data(), N,
                                   ctx[(step + 1) & 1].data(), rows.data(), ld) != 0) return 1;
      for (int i = 0; i < N; ++i)
        for (int v = 0; v < V; ++v) {
          const float x = rows[i * ld + v];
          if (std::isinf(x)) ++ninf; else sum += x;
        }
    }
    printf("%s: order %d, %d unigrams, checksum %.6f, %ld -inf entries\n", argv[f], order, n1, sum, ninf);
    ea_ngram_destroy(lm);
  }
  return 0;
}
