"""Time the lexicon-constrained CTC beam search with ARPA n-gram fusion (`--search ctc_beam --ngram-lm`) next to
`--search ctc_beam` without an LM and with a random `lstm_lm_librispeech`-size LSTM LM, on the same batch; and the load time
of a generated ARPA file of a few million n-grams.

Input: the synthetic batch of tools/bench_ctc_beam.py (seeded, peaked log-probs, B = 24 utterances of T' = 400 encoder
frames over V = 5004 tokens; RTF = batch time / (B * T' * 0.04 s), the search alone, no encoder).  The dictionary's first
2000 pieces start a word (U+2581), the rest continue one (word-start mode).  The ARPA file: `--words` unigrams, `--bigrams`
bigrams and `--trigrams` trigrams of random ids (every n-gram extends a listed one), written to a temporary file; the
lexicon spells every word as one word-start piece and 0-2 continuation pieces.

Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def write_arpa(path, rng, n_words, n_bi, n_tri):
    """A random trigram ARPA file; returns the word list."""
    words = [f"w{i}" for i in range(n_words)]
    uni = ["<s>", "</s>", "<unk>"] + words
    nu = len(uni)
    bi = np.unique(np.stack([rng.integers(0, nu, n_bi), rng.integers(1, nu, n_bi)], 1), axis=0)
    bi = bi[bi[:, 0] != 1]  # nothing follows </s>
    pick = bi[rng.integers(0, len(bi), n_tri)]
    tri = np.unique(np.concatenate([pick, rng.integers(1, nu, (n_tri, 1))], 1), axis=0)
    tri = tri[tri[:, 1] != 1]

    def lp(n):
        return rng.uniform(-4.0, -0.1, n)

    with open(path, "w") as f:
        f.write(f"\\data\\\nngram 1={nu}\nngram 2={len(bi)}\nngram 3={len(tri)}\n\n\\1-grams:\n")
        u_lp, u_bw = lp(nu), rng.uniform(-1.0, 0.0, nu)
        u_lp[0] = -99.0
        f.write("".join(f"{a:.4f}\t{w}\t{b:.4f}\n" for a, w, b in zip(u_lp, uni, u_bw)))
        f.write("\n\\2-grams:\n")
        f.write("".join(f"{a:.4f}\t{uni[x]} {uni[y]}\t{b:.4f}\n" for a, (x, y), b in zip(lp(len(bi)), bi, rng.uniform(-1.0, 0.0, len(bi)))))
        f.write("\n\\3-grams:\n")
        f.write("".join(f"{a:.4f}\t{uni[x]} {uni[y]} {uni[z]}\n" for a, (x, y, z) in zip(lp(len(tri)), tri)))
        f.write("\n\\end\\\n")
    return words, (nu, len(bi), len(tri))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--B", type=int, default=24)
    ap.add_argument("--T", type=int, default=400)
    ap.add_argument("--V", type=int, default=5004)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--lm-weight", type=float, default=0.4)
    ap.add_argument("--words", type=int, default=100000)
    ap.add_argument("--bigrams", type=int, default=1500000)
    ap.add_argument("--trigrams", type=int, default=2000000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    from espresso_amd import kernels as K
    from espresso_amd.data.asr_dictionary import AsrDictionary
    from espresso_amd.models.lstm_lm import LSTMLanguageModelEspresso
    from espresso_amd.models.ngram_lm import NGramLanguageModel
    from espresso_amd.tools.ctc_lexicon_beam_search import CTCLexiconBeamSearchDecoder
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder
    from espresso_amd.tools.lexicon import LexiconTrie

    dev = torch.device("cuda:0")
    B, T = args.B, args.T
    n_start = 2000
    d = AsrDictionary.from_symbols([f"▁p{i}" if i < n_start else f"p{i}" for i in range(args.V - 4)], enable_bos=True, add_space=False)
    V = len(d)
    assert V == args.V, V
    g = torch.Generator(device="cpu").manual_seed(0)
    z = torch.randn(B * T, V, generator=g) * 2.0
    peak = torch.where(torch.rand(B * T, generator=g) < 0.5, torch.zeros(B * T, dtype=torch.long), torch.randint(1, V, (B * T,), generator=g))
    z[torch.arange(B * T), peak] += 8.0
    z = z.to(dev)
    x = K.log_softmax(z, B * T, V, V).view(B, T, V)
    in_len = torch.full((B,), T, dtype=torch.int32, device=dev)
    in_len[B // 2:] = T - T // 4

    rng = np.random.default_rng(0)
    res = {"metric": "ctc_decode_batch_ms", "B": B, "T": T, "V": V, "beam": args.beam, "calls": args.calls,
           "audio_s_per_batch": B * T * 0.04}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "lm.arpa")
        t0 = time.perf_counter()
        words, counts = write_arpa(path, rng, args.words, args.bigrams, args.trigrams)
        res["arpa"] = {"ngrams": list(counts), "total": sum(counts), "MB": round(os.path.getsize(path) / 2 ** 20, 1),
                       "write_s": round(time.perf_counter() - t0, 2)}
        t0 = time.perf_counter()
        ngram = NGramLanguageModel(path)
        res["arpa"]["parse_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    ngram.to(dev)
    torch.cuda.synchronize()
    res["arpa"]["upload_s"] = round(time.perf_counter() - t0, 3)
    spell = {}
    for w in words:
        sp = (int(rng.integers(4, 4 + n_start)),) + tuple(int(t) for t in rng.integers(4 + n_start, V, rng.integers(0, 3)))
        spell.setdefault(sp, w)
    t0 = time.perf_counter()
    trie = LexiconTrie([(w, list(sp)) for sp, w in spell.items()], ngram, d)
    res["lexicon"] = {"words": trie.num_words, "nodes": len(trie), "build_s": round(time.perf_counter() - t0, 2)}

    class _LMTask:
        target_dictionary = source_dictionary = d

    torch.manual_seed(0)
    lstm = LSTMLanguageModelEspresso.build_model(SimpleNamespace(arch="lstm_lm_librispeech", is_wordlm=False), _LMTask).to(dev).eval()
    runs = {f"beam{args.beam}_no_lm": CTCPrefixBeamSearchDecoder([None], d, beam_size=args.beam),
            f"beam{args.beam}_lstm_lm{args.lm_weight:g}": CTCPrefixBeamSearchDecoder([None], d, beam_size=args.beam, lm_model=lstm,
                                                                                  lm_weight=args.lm_weight),
            f"beam{args.beam}_ngram_lexicon": CTCLexiconBeamSearchDecoder([None], d, ngram, trie, beam_size=args.beam, lm_weight=2.0,
                                                                          word_score=-1.0)}
    for name, dec in runs.items():
        for _ in range(args.warmup):
            out = dec.search(x, in_len)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = dec.search(x, in_len)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        med = float(np.median(times))
        res[name] = {"ms_median": round(med, 3), "ms_min": round(min(times), 3), "rtf": med / 1e3 / res["audio_s_per_batch"],
                     "mean_1best_len": round(float(out[1][:, 0].float().mean()), 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
