"""Lexicon-constrained CTC prefix beam search with ARPA n-gram fusion (models/ngram_lm.py, tools/lexicon.py,
tools/ctc_lexicon_beam_search.py, csrc/ctc_lexicon_beam.hip).

tests/ngram_ref.py restates the ARPA backoff and the fusion increments in float64; with them, prefix_beam_oracle of
tests/test_ctc_prefix_beam.py is the whole search.  The CPU tests hold those restatements to hand-computed values and brute
force, and the library's parser to them; the GPU tests hold the HIP search to the oracle."""
import itertools
import math
import os
import wave

import numpy as np
import pytest
import torch

from tests.ngram_ref import LN10, ArpaRef, FusionRef, random_arpa
from tests.test_ctc_prefix_beam import _peaked, prefix_beam_oracle

DEV = "cuda:0"
SCORE_TOL = 1e-4
# prefix_beam_oracle subtracts -inf scores of invalid hypotheses from each other when it computes its margins (nan, ignored)
pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered in scalar subtract:RuntimeWarning")

# a hand-written trigram file: every value below is checked by hand in test_arpa_reference_hand_values
TRIGRAM = """
\\data\\
ngram 1=6
ngram 2=5
ngram 3=2

\\1-grams:
-1.5\t<unk>
-99\t<s>\t-0.5
-0.8\t</s>
-0.6\tthe\t-0.3
-0.9\tcat
-1.1\tsat\t-0.2

\\2-grams:
-0.3\t<s> the\t-0.15
-0.4\tthe cat\t-0.1
-0.7\tthe sat
-0.5\tcat sat
-0.2\tsat </s>

\\3-grams:
-0.1\t<s> the cat
-0.05\tthe cat sat
\\end\\
"""


def _write(tmp_path, name, text):
    p = str(tmp_path / name)
    with open(p, "w", encoding="utf-8") as f:
        f.write(text)
    return p


def _space_dict(letters="abcdef"):
    from espresso_amd.data.asr_dictionary import AsrDictionary

    return AsrDictionary.from_symbols(list(letters), enable_bos=True)  # <space> appended


def _wordstart_dict():
    from espresso_amd.data.asr_dictionary import AsrDictionary

    return AsrDictionary.from_symbols(["▁a", "▁b", "▁c", "a", "b", "c", "d"], enable_bos=True, add_space=False)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_arpa_reference_hand_values():
    r = ArpaRef(TRIGRAM)
    L = LN10
    assert r.logp(["<s>", "the"], "cat") == pytest.approx(-0.1 * L)                    # trigram hit
    assert r.logp(["<s>", "the"], "sat") == pytest.approx((-0.15 - 0.7) * L)          # one step: bow(<s> the) + P(sat | the)
    assert r.logp(["<s>", "the"], "the") == pytest.approx((-0.15 - 0.3 - 0.6) * L)    # two steps down to the unigram
    assert r.logp(["cat", "the"], "cat") == pytest.approx(-0.4 * L)                   # context (cat the) absent: weight 0
    assert r.logp(["the", "cat"], "the") == pytest.approx((-0.1 + 0.0 - 0.6) * L)     # bow(the cat), then cat has no bow
    assert r.logp(["cat", "sat"], "dog") == pytest.approx((0.0 - 0.2 - 1.5) * L)      # unknown word = <unk>; (cat sat) no bow
    assert r.logp(["cat", "sat"], "</s>") == pytest.approx(-0.2 * L)                   # </s> bigram
    assert r.sentence(["the", "cat", "sat"]) == pytest.approx((-0.3 - 0.1 - 0.05 - 0.2) * L)


def test_library_parser_matches_hand_values(tmp_path):
    from espresso_amd.models.ngram_lm import NGramLanguageModel

    lm = NGramLanguageModel(_write(tmp_path, "t.arpa", TRIGRAM))
    assert (lm.order, lm.counts, lm.vocab) == (3, [6, 5, 2], ["<unk>", "<s>", "</s>", "the", "cat", "sat"])
    r = ArpaRef(TRIGRAM)
    queries = [(["<s>", "the"], "cat"), (["cat", "the"], "cat"), (["<s>", "the"], "sat"), (["<s>", "the"], "the"), (["the", "cat"], "the"),
               (["cat", "sat"], "dog"), (["cat", "sat"], "</s>"), ([], "sat"), (["<s>"], "the")]
    got = lm.score_host(lm.encode_contexts([c for c, _ in queries]).numpy(), np.array([lm.index(w) for _, w in queries]))
    for (c, w), g in zip(queries, got):
        assert abs(g - r.logp(c, w)) < 1e-5, (c, w, g, r.logp(c, w))


def test_library_parser_random_order4(tmp_path):
    """Same tables (every n-gram with its log-prob and backoff) and same scores as the float64 scorer."""
    from espresso_amd.models.ngram_lm import NGramLanguageModel

    rng = np.random.default_rng(0)
    words = [f"w{i}" for i in range(40)]
    text = random_arpa(rng, words, 4, per_order=150)
    lm = NGramLanguageModel(_write(tmp_path, "r.arpa", text))
    r = ArpaRef(text)
    assert lm.order == 4
    for k in range(1, 5):
        ng, lp, bw = lm.records(k)
        table = {tuple(lm.vocab[i] for i in row): (p, b) for row, p, b in zip(ng, lp, bw)}
        expect = {g: (p, r.bow.get(g, 0.0)) for g, p in r.prob.items() if len(g) == k}
        assert set(table) == set(expect)
        for g, (p, b) in table.items():
            assert abs(p - expect[g][0]) < 1e-5 * max(1.0, abs(expect[g][0])) and abs(b - expect[g][1]) < 1e-5, g
    N = 4000
    vocab = lm.vocab + ["oov1"]
    ctx = [[vocab[i] for i in rng.integers(0, len(vocab), rng.integers(0, 4))] for _ in range(N)]
    targets = [w for w in vocab if w != "<s>"]  # never predicted (its -99 is ~ -228 in natural log: fp32 ulp 1.5e-5)
    ws = [targets[i] for i in rng.integers(0, len(targets), N)]
    got = lm.score_host(lm.encode_contexts(ctx).numpy(), np.array([lm.index(w) for w in ws]))
    ref = np.array([r.logp(["<unk>" if c not in lm.word2id else c for c in cx], w) for cx, w in zip(ctx, ws)])
    assert np.max(np.abs(got - ref)) < 1e-5


_BAD = {
    "count": ("\\data\\\nngram 1=3\n\n\\1-grams:\n-1 <s>\n-1 </s>\n\n\\end\\\n", "line 4:"),
    "unknown": ("\\data\\\nngram 1=3\nngram 2=1\n\n\\1-grams:\n-1 <s>\n-1 </s>\n-1 a\n\n\\2-grams:\n-1 a b\n\\end\\\n", "line 11:"),
    "number": ("\\data\\\nngram 1=3\n\n\\1-grams:\n-1 <s>\nx </s>\n-1 a\n\\end\\\n", "line 6:"),
    "fields": ("\\data\\\nngram 1=3\n\n\\1-grams:\n-1 <s>\n-1 </s> -0.5\n-1 a\n\\end\\\n", "line 6:"),
    "order": ("\\data\\\n" + "".join(f"ngram {k}=1\n" for k in range(1, 8)), "line 8:"),
    "end": ("\\data\\\nngram 1=3\n\n\\1-grams:\n-1 <s>\n-1 </s>\n-1 a\n\n\\2-grams:\n", "line 9:"),
    "duplicate": ("\\data\\\nngram 1=3\n\n\\1-grams:\n-1 <s>\n-1 </s>\n-1 <s>\n\\end\\\n", "line 7:"),
    "missing_ctx": ("\\data\\\nngram 1=4\nngram 2=1\nngram 3=1\n\n\\1-grams:\n-1 <s>\n-1 </s>\n-1 a\n-1 b\n\n\\2-grams:\n-1 a b\n\n"
                    "\\3-grams:\n-1 b a b\n\\end\\\n", "line 16:"),
}


@pytest.mark.parametrize("case", sorted(_BAD))
def test_malformed_arpa_names_the_line(tmp_path, case):
    from espresso_amd.models.ngram_lm import ArpaFormatError, NGramLanguageModel

    text, where = _BAD[case]
    with pytest.raises(ArpaFormatError) as e:
        NGramLanguageModel(_write(tmp_path, f"{case}.arpa", text))
    assert where in str(e.value), str(e.value)


def test_lexicon_file_and_errors(tmp_path):
    from espresso_amd.models.ngram_lm import NGramLanguageModel
    from espresso_amd.tools.lexicon import LexiconError, LexiconTrie, build_lexicon, read_lexicon

    d = _wordstart_dict()
    lm = NGramLanguageModel(_write(tmp_path, "a.arpa", random_arpa(np.random.default_rng(1), ["x", "y", "z"], 2, 4)))
    lex = _write(tmp_path, "lex.txt", "x ▁a b\nx ▁a c\ny ▁b\n\nz ▁c d a\n")
    sp = read_lexicon(lex, d)
    assert sp == [("x", [d.index("▁a"), d.index("b")]), ("x", [d.index("▁a"), d.index("c")]), ("y", [d.index("▁b")]),
                  ("z", [d.index("▁c"), d.index("d"), d.index("a")])]
    trie = build_lexicon(d, lm, lex)
    assert trie.num_words == 4 and len(trie) == 8  # root; ▁a ▁b ▁c; ▁a-b ▁a-c; ▁c-d ▁c-d-a
    n_a = trie.child_of(0, d.index("▁a"))
    assert trie.word[trie.child_of(n_a, d.index("b"))] == trie.word[trie.child_of(n_a, d.index("c"))] == lm.index("x")
    assert trie.word[n_a] == -1 and trie.child_of(0, d.index("a")) == -1
    uni = lm.unigram_logprobs()
    assert trie.smear[n_a] == uni[lm.index("x")] and trie.smear[0] == 0.0
    assert list(trie.word_start) == [0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0]
    with pytest.raises(LexiconError, match="same spelling"):
        LexiconTrie([("x", [4, 7]), ("y", [4, 7])], lm, d)
    with pytest.raises(LexiconError, match="line 2"):
        read_lexicon(_write(tmp_path, "bad.txt", "x ▁a\ny ▁q\n"), d)
    with pytest.raises(LexiconError, match="--lexicon"):
        build_lexicon(d, lm)  # word-start mode needs a file
    with pytest.warns(UserWarning, match="dropped"):  # no <unk> in the file: an unknown word cannot be scored
        lm2 = NGramLanguageModel(_write(tmp_path, "n.arpa", random_arpa(np.random.default_rng(1), ["x"], 2, 2, unk=False)))
        t2 = LexiconTrie([("x", [4]), ("nope", [5])], lm2, d)
    assert t2.num_words == 1


def test_lexicon_space_mode_spells_the_arpa_words(tmp_path):
    from espresso_amd.models.ngram_lm import NGramLanguageModel
    from espresso_amd.tools.lexicon import build_lexicon

    d = _space_dict("abc")
    lm = NGramLanguageModel(_write(tmp_path, "a.arpa", random_arpa(np.random.default_rng(2), ["ab", "ba", "abc", "cd"], 2, 5)))
    trie = build_lexicon(d, lm)  # "cd": 'd' is no symbol, left out
    assert trie.word_start is None and trie.space == d.space() and trie.num_words == 3
    node = 0
    for ch in "abc":
        node = trie.child_of(node, d.index(ch))
    assert trie.word[node] == lm.index("abc")
    uni = lm.unigram_logprobs()
    assert trie.smear[trie.child_of(0, d.index("a"))] == max(uni[lm.index("ab")], uni[lm.index("abc")])


def _spell_space(d, words):
    return {tuple(d.index(c) for c in w): w for w in words}


def _spell_wordstart(d, words):
    """word -> a spelling: '▁' + first letter, then the rest letters (tokens of _wordstart_dict)."""
    return {tuple([d.index("▁" + w[0])] + [d.index(c) for c in w[1:]]): w for w in words}


def _setup(mode, rng, alpha, beta, n_words=12, order=3):
    if mode == "space":
        d = _space_dict("abcd")
        letters = "abcd"
    else:
        d = _wordstart_dict()
        letters = None
    words = set()
    while len(words) < n_words:
        n = int(rng.integers(1, 4))
        if mode == "space":
            words.add("".join(letters[i] for i in rng.integers(0, 4, n)))
        else:
            words.add("abc"[rng.integers(0, 3)] + "".join("abcd"[i] for i in rng.integers(0, 4, n - 1)))
    words = sorted(words)
    text = random_arpa(rng, words, order, per_order=30)
    spell = _spell_space(d, words) if mode == "space" else _spell_wordstart(d, words)
    ws = None if mode == "space" else np.array([1 if d[i].startswith("▁") else 0 for i in range(len(d))])
    fus = FusionRef(ArpaRef(text), spell, len(d), space=d.space(), word_start=ws, alpha=alpha, beta=beta)
    return d, words, text, spell, fus


@pytest.mark.parametrize("mode", ["space", "wordstart"])
def test_increments_telescope(mode):
    rng = np.random.default_rng(7)
    alpha, beta = 0.7, -1.3
    d, words, text, spell, fus = _setup(mode, rng, alpha, beta)
    inv = {w: sp for sp, w in spell.items()}
    r = ArpaRef(text)
    for _ in range(30):
        sent = [words[i] for i in rng.integers(0, len(words), int(rng.integers(0, 6)))]
        toks = []
        for i, w in enumerate(sent):
            if mode == "space" and i:
                toks.append(d.space())
            toks += list(inv[w])
        if mode == "space" and sent and rng.random() < 0.5:
            toks.append(d.space())  # a trailing <space> changes nothing
        y = tuple(toks)
        total = sum(fus.lm_fn(y[:u])[y[u]] for u in range(len(y))) + fus.lm_fn(y)[len(d)]
        assert total == pytest.approx(alpha * r.sentence(sent) + beta * len(sent), abs=1e-9), (sent, y)


@pytest.mark.parametrize("mode", ["space", "wordstart"])
@pytest.mark.parametrize("T", [1, 3, 5])
def test_oracle_with_fusion_is_exact_without_pruning(mode, T):
    """beam and K exhaustive: the oracle with the fusion lm_fn returns every valid label sequence of length <= T with the
    score -ctc_nll(y) + (sum of increments) + end term, its 1-best the argmax."""
    from oracle.torch_ref import ctc_nll_numpy

    rng = np.random.default_rng(T)
    d, words, text, spell, fus = _setup(mode, rng, 0.8, 0.4, n_words=8)
    V = len(d)
    x = rng.standard_normal((T, V)) * 1.5
    x -= np.logaddexp.reduce(x, axis=1, keepdims=True)
    hyps, _ = prefix_beam_oracle(x, T, beam=10 ** 6, K=V - 1, blank=d.bos(), lm_fn=fus.lm_fn, lm_weight=1.0, eos=V, nbest=10 ** 6)
    hyps = {y: s for y, s in hyps if s > -math.inf}
    brute = {}
    for n in range(T + 1):
        for y in itertools.product([v for v in range(V) if v != d.bos()], repeat=n):
            if fus.state(y) is None:
                continue
            nll = ctc_nll_numpy(x, list(y), blank=d.bos())
            lm = sum(fus.lm_fn(y[:u])[y[u]] for u in range(n)) + fus.lm_fn(y)[V]
            if np.isfinite(nll) and lm > -math.inf:
                brute[y] = -nll + lm
    assert set(hyps) == set(brute) and brute
    for y, s in hyps.items():
        assert abs(s - brute[y]) < 1e-9, (y, s, brute[y])
    assert max(hyps, key=hyps.get) == max(brute, key=brute.get)


def _run(argv):
    from espresso_amd import speech_recognize as sr

    return sr.main(["--path", "missing.pt", "--dict", "missing.txt", "--wav-scp", "missing.scp", *argv])


@pytest.mark.parametrize("extra,match", [(["--search", "ctc"], "ctc_beam"), (["--search", "beam"], "ctc_beam"),
                                         (["--search", "transducer_beam"], "ctc_beam"),
                                         (["--search", "ctc_beam", "--lm-path", "lm.pt"], "--lm-path"),
                                         (["--search", "ctc_beam", "--word-dict", "w.txt"], "--word-dict")])
def test_cli_refuses_ngram_combinations(extra, match):
    with pytest.raises(NotImplementedError, match=match):
        _run(["--ngram-lm", "missing.arpa", *extra])


def test_cli_refuses_ngram_ensembles_and_parses_options():
    from espresso_amd import speech_recognize as sr

    with pytest.raises(NotImplementedError, match="ensembles"):
        sr.main(["--path", os.pathsep.join(["a.pt", "b.pt"]), "--dict", "d.txt", "--wav-scp", "w.scp", "--search", "ctc_beam",
                 "--ngram-lm", "lm.arpa"])
    a = sr.get_parser().parse_args(["--path", "m.pt", "--dict", "d.txt", "--wav-scp", "w.scp", "--search", "ctc_beam"])
    assert (a.ngram_lm, a.lexicon, a.word_score) == (None, None, -1.0)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


@pytest.mark.gpu
def test_ngram_score_kernel_vs_float64(tmp_path):
    _need_gpu()
    from espresso_amd.models.ngram_lm import NGramLanguageModel

    rng = np.random.default_rng(3)
    words = [f"w{i}" for i in range(60)]
    text = random_arpa(rng, words, 4, per_order=400)
    lm = NGramLanguageModel(_write(tmp_path, "r.arpa", text), device=DEV)
    r = ArpaRef(text)
    # contexts: half of them prefixes of listed n-grams (hits and backoff chains at every depth), half random words
    listed = [g for g in r.prob if len(g) >= 2]
    N = 12000
    vocab = lm.vocab + ["oov_a", "oov_b"]
    targets = [w for w in vocab if w != "<s>"]  # never predicted (its -99 is ~ -228 in natural log: fp32 ulp 1.5e-5)
    ctx, ws = [], []
    for i in range(N):
        if i % 2:
            g = listed[rng.integers(len(listed))]
            ctx.append(list(g[:-1]))
            ws.append(g[-1] if rng.random() < 0.5 else targets[rng.integers(len(targets))])
        else:
            ctx.append([vocab[j] for j in rng.integers(0, len(vocab), rng.integers(0, 4))])
            ws.append(targets[rng.integers(len(targets))])
    got = lm.score(ctx, ws).cpu().numpy()
    ref = np.array([r.logp(["<unk>" if c not in lm.word2id else c for c in cx], w) for cx, w in zip(ctx, ws)])
    assert sum(w not in lm.word2id for w in ws) > 100
    err = np.max(np.abs(got - ref))
    print(f"ea_ngram_score: {N} queries, max |device - float64| {err:.2e}")
    assert err < 1e-5


def _decoder(d, lm, trie, beam, K, nbest=1, alpha=1.0, beta=0.0, gamma=0.0):
    from espresso_amd.tools.ctc_lexicon_beam_search import CTCLexiconBeamSearchDecoder

    return CTCLexiconBeamSearchDecoder([None], d, lm, trie, beam_size=beam, nbest=nbest, beam_size_token=K, lm_weight=alpha,
                                       word_score=beta, insertion_bonus=gamma)


def _tables(tmp_path, d, text, spell, mode):
    from espresso_amd.models.ngram_lm import NGramLanguageModel
    from espresso_amd.tools.lexicon import build_lexicon

    lm = NGramLanguageModel(_write(tmp_path, "lm.arpa", text), device=DEV)
    lex = None
    if mode != "space":
        lex = _write(tmp_path, "lex.txt", "".join(f"{w} {' '.join(d[t] for t in sp)}\n" for sp, w in spell.items()))
    return lm, build_lexicon(d, lm, lex)


def _hyps(out, b):
    tokens, lengths, scores, nhyp = (t.cpu() for t in out)
    return [(tuple(tokens[b, i, : int(lengths[b, i])].tolist()), float(scores[b, i])) for i in range(int(nhyp[b]))]


def _compare(out, x, lens, dec, fus):
    """Every returned hypothesis against the oracle's finite ones: scores within SCORE_TOL, sequences equal where the oracle's
    ranking margin exceeds it.  Returns the worst score difference."""
    worst = 0.0
    V = dec.vocab_size
    for b in range(x.shape[0]):
        ref, margin = prefix_beam_oracle(x[b].astype(np.float64), int(lens[b]), dec.beam_size, dec.beam_size_token, dec.blank,
                                         lm_fn=fus.lm_fn, lm_weight=1.0, bonus=dec.insertion_bonus, eos=V, nbest=dec.nbest)
        ref = [(y, s) for y, s in ref if s > -math.inf] if lens[b] > 0 else []
        got = _hyps(out, b)
        assert len(got) == len(ref), (b, got, ref)
        for (gy, gs), (ry, rs) in zip(got, ref):
            assert abs(gs - rs) < SCORE_TOL, (b, got, ref)
            worst = max(worst, abs(gs - rs))
        if margin > SCORE_TOL:
            assert [y for y, _ in got] == [y for y, _ in ref], (b, got, ref)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["space", "wordstart"])
@pytest.mark.parametrize("beam,K", [(1, 1), (4, 4), (16, 4), (10, 6)])
def test_search_vs_oracle(tmp_path, beam, K, mode, dtype):
    _need_gpu()
    worst = 0.0
    for alpha, beta, gamma, seed in [(1.0, 0.0, 0.0, 0), (0.5, -1.0, 0.3, 1), (2.0, 1.5, -0.2, 2), (0.0, -0.5, 0.0, 3)]:
        rng = np.random.default_rng(100 * seed + beam + K)
        d, words, text, spell, fus = _setup(mode, rng, alpha, beta)
        lm, trie = _tables(tmp_path, d, text, spell, mode)
        V = len(d)
        B, T = 5, 12
        x = _peaked(rng, B * T, V, sharp=3.0, scale=1.5).reshape(B, T, V)
        lens = np.array([T, 0, 1, 7, 10], dtype=np.int32)
        xd = torch.from_numpy(x).to(DEV, dtype)
        x_seen = xd.float().cpu().numpy()
        dec = _decoder(d, lm, trie, beam, K, nbest=min(beam, 3), alpha=alpha, beta=beta, gamma=gamma)
        out = dec.search(xd, torch.from_numpy(lens).to(DEV))
        worst = max(worst, _compare(out, x_seen, lens, dec, fus))
        assert int(out[3][1]) == 0  # no frames: no hypothesis
    print(f"{mode} beam {beam} K {K} {dtype}: max |score - oracle| {worst:.2e}")


def _words_of(y, spell, d, mode):
    """Split a token sequence into lexicon words (None if it does not split)."""
    if mode == "space":
        parts, cur = [], []
        for t in y:
            if t == d.space():
                parts.append(tuple(cur))
                cur = []
            else:
                cur.append(t)
        if cur:
            parts.append(tuple(cur))
    else:
        parts = []
        for t in y:
            if d[t].startswith("▁") or not parts:
                parts.append((t,))
            else:
                parts[-1] += (t,)
    return None if any(p not in spell for p in parts) else [spell[p] for p in parts]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["space", "wordstart"])
def test_lexicon_constraint(tmp_path, mode):
    _need_gpu()
    rng = np.random.default_rng(11)
    d, words, text, spell, fus = _setup(mode, rng, 0.5, 0.0)
    lm, trie = _tables(tmp_path, d, text, spell, mode)
    V = len(d)
    B, T = 6, 14
    x = _peaked(rng, B * T, V, sharp=2.0, scale=1.5).reshape(B, T, V).astype(np.float32)
    lens = np.full(B, T, dtype=np.int32)
    dec = _decoder(d, lm, trie, 8, 5, nbest=4, alpha=0.5)
    out = dec.search(torch.from_numpy(x).to(DEV), torch.from_numpy(lens).to(DEV))
    n = 0
    for b in range(B):
        for y, _ in _hyps(out, b):
            assert _words_of(y, spell, d, mode) is not None, (b, y)
            n += 1
    assert n > B


def _two_frame_setup(tmp_path, lm_text, words_lex):
    """Space-mode dictionary a, b, c; frames: 'a' then a near tie of 'b' (slightly ahead) and 'c'."""
    d = _space_dict("abc")
    V = len(d)
    x = np.full((1, 4, V), -9.0)
    x[0, 0, d.index("a")] = -0.05
    x[0, 1, d.index("b")], x[0, 1, d.index("c")] = math.log(0.55), math.log(0.43)
    x[0, 2, d.bos()] = x[0, 3, d.bos()] = -0.02
    x = x - np.logaddexp.reduce(x, axis=2, keepdims=True)
    spell = _spell_space(d, words_lex)
    lm, trie = _tables(tmp_path, d, lm_text, spell, "space")
    return d, x.astype(np.float32), lm, trie


def _arpa(probs):
    """A unigram ARPA file: {word: log10 prob}."""
    lines = ["\\data\\", f"ngram 1={len(probs) + 2}", "", "\\1-grams:", "-99\t<s>", "-0.5\t</s>"]
    lines += [f"{p}\t{w}" for w, p in probs.items()]
    return "\n".join(lines + ["", "\\end\\", ""])


@pytest.mark.gpu
def test_out_of_lexicon_spelling_is_not_returned(tmp_path):
    _need_gpu()
    d, x, lm, trie = _two_frame_setup(tmp_path, _arpa({"ac": -1.0, "b": -1.0}), ["ac", "b"])
    lens = torch.tensor([4], dtype=torch.int32, device=DEV)
    dec = _decoder(d, lm, trie, 4, 3, alpha=0.0, beta=0.0)
    got = _hyps(dec.search(torch.from_numpy(x).to(DEV), lens), 0)
    assert got[0][0] == (d.index("a"), d.index("c")), got  # acoustically "ab" is ahead, but it is no word


@pytest.mark.gpu
def test_fusion_changes_the_answer(tmp_path):
    _need_gpu()
    d, x, lm, trie = _two_frame_setup(tmp_path, _arpa({"ab": -3.0, "ac": -0.1}), ["ab", "ac"])
    lens = torch.tensor([4], dtype=torch.int32, device=DEV)
    best = {}
    for alpha in (0.0, 1.0):
        dec = _decoder(d, lm, trie, 4, 3, alpha=alpha, beta=-1.0)
        best[alpha] = _hyps(dec.search(torch.from_numpy(x).to(DEV), lens), 0)[0][0]
    assert best[0.0] == (d.index("a"), d.index("b")) and best[1.0] == (d.index("a"), d.index("c")), best


@pytest.mark.gpu
def test_no_valid_hypothesis_gives_none(tmp_path):
    """beam 1 follows 'a' into the trie; the utterance ends inside the word 'ab': nothing finite is left."""
    _need_gpu()
    d = _space_dict("abc")
    V = len(d)
    x = np.full((1, 2, V), -9.0)
    x[0, 0, d.index("a")] = -0.01
    x[0, 1, d.bos()] = -0.01
    x = (x - np.logaddexp.reduce(x, axis=2, keepdims=True)).astype(np.float32)
    lm, trie = _tables(tmp_path, d, _arpa({"ab": -1.0}), _spell_space(d, ["ab"]), "space")
    dec = _decoder(d, lm, trie, 1, 1)
    out = dec.search(torch.from_numpy(x).to(DEV), torch.tensor([2], dtype=torch.int32, device=DEV))
    assert int(out[3][0]) == 0 and float(out[2][0, 0]) == -math.inf


@pytest.mark.gpu
def test_one_call_no_synchronisation(tmp_path, monkeypatch):
    _need_gpu()
    from espresso_amd import kernels

    rng = np.random.default_rng(5)
    d, words, text, spell, fus = _setup("wordstart", rng, 1.0, -1.0)
    lm, trie = _tables(tmp_path, d, text, spell, "wordstart")
    V = len(d)
    B, T = 3, 12
    x = torch.from_numpy(_peaked(rng, B * T, V).reshape(B, T, V).astype(np.float32)).to(DEV)
    lens = torch.tensor([12, 5, 0], dtype=torch.int32, device=DEV)
    dec = _decoder(d, lm, trie, 6, 4, nbest=2)
    ref = [t.clone() for t in dec.search(x, lens)]  # warm-up: the lexicon tables go to the device
    calls = []
    real = kernels.ctc_lexicon_beam_search
    monkeypatch.setattr(kernels, "ctc_lexicon_beam_search", lambda *a, **k: calls.append(1) or real(*a, **k))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = dec.search(x, lens)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(calls) == 1
    for a, b in zip(out, ref):
        assert torch.equal(a, b)


def _write_wav(path, samples):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(samples, -32768, 32767).astype("<i2").tobytes())


@pytest.mark.gpu
def test_cli_round_trip(tmp_path, capsys):
    """speech_recognize --search ctc_beam --ngram-lm --lexicon prints, for every utterance, what the decoder returns, and
    the WER summary."""
    _need_gpu()
    from espresso_amd import registry
    from espresso_amd import speech_recognize as sr
    from espresso_amd.data.audio_utils import read_wav
    from espresso_amd.models.ngram_lm import NGramLanguageModel
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from espresso_amd.tools.ctc_lexicon_beam_search import CTCLexiconBeamSearchDecoder
    from espresso_amd.tools.lexicon import build_lexicon

    letters = "abcdefgh"
    dict_path = _write(tmp_path, "dict.txt", "".join(f"{c} 1\n" for c in letters) + "<space> 1\n")
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(dict=dict_path, autoregressive=False,
                                                                                    criterion_name="ctc_loss"))
    d = task.target_dictionary
    assert d.space() >= 0
    rng = np.random.default_rng(0)
    words = sorted({"".join(letters[i] for i in rng.integers(0, 8, rng.integers(1, 4))) for _ in range(40)})
    arpa = _write(tmp_path, "lm.arpa", random_arpa(rng, words, 3, per_order=60))
    lex = _write(tmp_path, "lex.txt", "".join(f"{w} {' '.join(w)}\n" for w in words))
    block = {"_name": "speech_transformer_encoder_model", "encoder": {"conv_channels": "[64, 64, 16, 16]", "embed_dim": 64,
             "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4, "normalize_before": True, "relative_positional_embeddings": True,
             "layer_type": "conformer"}, "dropout": 0.0, "attention_dropout": 0.0, "activation_dropout": 0.0, "layernorm_embedding": True}
    cls = registry.MODEL_REGISTRY["speech_transformer_encoder_model"]
    torch.manual_seed(0)
    model = cls.build_model(cls.config_class.from_dict(block), task)
    torch.save({"model": model.state_dict(), "cfg": {"model": block}}, str(tmp_path / "model.pt"))
    model = model.to(DEV).eval()
    utts = [f"utt{i}" for i in range(4)]
    with open(tmp_path / "wav.scp", "w") as f, open(tmp_path / "text", "w") as g:
        for i, u in enumerate(utts):
            p = str(tmp_path / f"{u}.wav")
            _write_wav(p, rng.standard_normal(int(16000 * (0.6 + 0.3 * i))) * 3000)
            f.write(f"{u} {p}\n")
            g.write(f"{u} {' '.join(words[i])}\n")
    argv = ["--path", str(tmp_path / "model.pt"), "--dict", dict_path, "--wav-scp", str(tmp_path / "wav.scp"), "--text",
            str(tmp_path / "text"), "--search", "ctc_beam", "--beam", "5", "--nbest", "2", "--max-tokens", "500", "--batch-size", "3",
            "--ngram-lm", arpa, "--lexicon", lex, "--lm-weight", "0.7", "--word-score", "-0.5"]
    capsys.readouterr()
    sr.main(argv)
    out = capsys.readouterr().out.splitlines()
    lines = [l.split("\t") for l in out if l.startswith("H-")]
    assert any(l.startswith("WER=") for l in out)

    waves = [read_wav(str(tmp_path / f"{u}.wav")) for u in utts]
    task.build_frontend(torch.device(DEV))
    lm = NGramLanguageModel(arpa, device=DEV)
    gen = CTCLexiconBeamSearchDecoder([model], d, lm, build_lexicon(d, lm, lex), beam_size=5, nbest=2, lm_weight=0.7,
                                      word_score=-0.5)
    expect = []
    for bt in sr.make_batches(utts, [len(w) for w in waves], 500, 3):
        sample = sr.collate(bt, utts, waves, torch.device(DEV))
        hyps = gen.generate([model], task.prepare_sample(sample, train=False))
        for i, u in enumerate(sample["utt_ids"]):
            for h in hyps[i][:2]:
                expect.append((f"H-{u}", d.string(h["tokens"]), float(h["score"]) / math.log(2)))
    assert len(lines) == len(expect) >= len(utts)
    for (hu, text, score), (eu, etext, escore) in zip(lines, expect):
        assert (hu, text) == (eu, etext)
        assert float(score) == escore or abs(float(score) - escore) < 1e-4, (hu, score, escore)
