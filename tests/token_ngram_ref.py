"""Float64 restatement of the sub-word n-gram LM rows (models/token_ngram_lm.py, csrc/ngram_rows.hip) over tests.ngram_ref.ArpaRef,
and the files, dictionaries and random (parent, token, keep) walks the tests of that LM share."""
import math

import numpy as np

from tests.ngram_ref import ArpaRef, random_arpa

# |fp32 row - float64 ArpaRef| per finite entry: the value is a sum of at most 6 fp32 addends (5 backoff weights and one
# log-prob), each |x| <= 7 (random_arpa draws log10 values from [-3, 0.3]; times ln 10).  Rounding an addend to fp32 costs at
# most 2^-22 = 2.4e-7 (|x| < 8), each of the 5 additions at most 2^-20 = 9.5e-7 while the partial sums stay below 32, as they
# do for these files: 6 * 2.4e-7 + 5 * 9.5e-7 = 6.2e-6 < 1e-5
ROW_TOL = 1e-5


def dictionary(n):
    """<s> (blank), <pad>, </s>, <unk>, t0 .. t{n-1}, <space>: V = n + 5."""
    from espresso_amd.data.asr_dictionary import AsrDictionary

    return AsrDictionary.from_symbols([f"t{i}" for i in range(n)], enable_bos=True)


def plain_symbols(d):
    return [s for i, s in enumerate(d.symbols) if i not in (d.bos(), d.pad(), d.eos(), d.unk())]


def write_arpa(tmp_path, name, text):
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write(text)
    return path


def random_lm_text(d, order, unk, seed, per_order=60, absent=0.25):
    """A random_arpa file over the dictionary's symbols without about `absent` of them."""
    rng = np.random.default_rng(seed)
    syms = plain_symbols(d)
    words = [s for s in syms if rng.random() >= absent]
    return random_arpa(rng, words, order, per_order, unk=unk)


def _arpa_text(rng, uni, bi, tri):
    out = ["\\data\\", f"ngram 1={len(uni)}", f"ngram 2={len(bi)}", f"ngram 3={len(tri)}", ""]
    for k, gs in enumerate((([(w,) for w in uni]), bi, tri), 1):
        out.append(f"\\{k}-grams:")
        for g in gs:
            lp = -99.0 if g == ("<s>",) else round(float(rng.uniform(-3.0, -0.05)), 4)
            out.append(f"{lp}\t{' '.join(g)}" + (f"\t{round(float(rng.uniform(-1.0, 0.3)), 4)}" if k < 3 else ""))
        out.append("")
    return "\n".join(out + ["\\end\\"]) + "\n"


def dense_arpa(words, seed=0):
    """Order 3.  The unigram context `words[0]` has every word as a child; after (words[0], words[0]) a trigram and the bigram
    hit the same columns, and after (words[1], words[0]) likewise: the later order must win."""
    uni = ["<s>", "</s>", "<unk>"] + list(words)
    a, b = words[0], words[1]
    bi = [(a, w) for w in uni[1:]] + [("<s>", a), (b, a), (b, words[2])]
    tri = [(a, a, w) for w in words[::2]] + [(a, a, "</s>"), (b, a, words[3]), (b, a, a), ("<s>", a, a), ("<s>", a, words[4])]
    return _arpa_text(np.random.default_rng(seed), uni, bi, tri)


def wide_tail_arpa(words, tail, seed=0):
    """Order 3 over `words` (which include `tail`, the symbols of the dictionary's last columns).  After words[0] every tail
    word is a bigram child; after (words[0], words[0]) every second tail word is a trigram child too, so both orders land on
    one column and the trigram must win; (words[1], words[0]) and (<s>, words[0]) have one tail child each; <unk> is a child
    of both orders as well."""
    uni = ["<s>", "</s>", "<unk>"] + list(words)
    a, b = words[0], words[1]
    bi = [(a, w) for w in tail] + [(a, a), (b, a), ("<s>", a), (a, "<unk>")]
    tri = [(a, a, w) for w in tail[::2]] + [(b, a, tail[1]), ("<s>", a, tail[0]), (a, a, "<unk>"), (a, a, a)]
    return _arpa_text(np.random.default_rng(seed), uni, bi, tri)


class TokenRowsRef:
    """Rows over the dictionary from an ArpaRef, by the map rules of TokenNGramLM: eos is </s>, pad and blank are -inf, the
    dictionary's <unk> and every symbol the file lacks score as the file's <unk> (-inf without one); a context token the file
    lacks is <unk>, or without one a word that matches no n-gram."""

    def __init__(self, text, d, blank=None):
        self.ref, self.d = ArpaRef(text), d
        self.blank = d.bos() if blank is None else blank
        self.has_unk = ("<unk>",) in self.ref.prob
        self._cache = {}

    def word(self, t):
        d = self.d
        if t == d.eos():
            return "</s>"
        s = d.symbols[t]
        if t in (d.pad(), self.blank, d.unk()) or s in ("<s>", "</s>", "<unk>") or (s,) not in self.ref.prob:
            return "<unk>" if self.has_unk else "\0none"
        return s

    def row(self, ctx_words):
        """float64 [V] after the context words (strings, <s> first)."""
        d = self.d
        # (ArpaRef.logp slices the last order - 1 words with a start index that goes negative for a shorter context: words
        # that match no n-gram in front keep the index at or above 0 and change no value)
        ctx_words = ["\0front"] * self.ref.order + list(ctx_words)
        out = np.full(len(d), -math.inf)
        for v in range(len(d)):
            if v in (d.pad(), self.blank) and v != d.eos():
                continue
            w = self.word(v)
            out[v] = self.ref.logp(ctx_words, w) if w != "\0none" else -math.inf
        return out

    def lm_fn(self, prefix):
        """For prefix_beam_oracle / frame_beam_oracle: token prefix -> row."""
        prefix = tuple(prefix)
        if prefix not in self._cache:
            self._cache[prefix] = self.row(["<s>"] + [self.word(t) for t in prefix])
        return self._cache[prefix]


def random_triples(rng, N, V, steps, blank, pad):
    """`steps` triples: parent a random non-permutation of the rows, token any id but blank and pad, keep mixed."""
    toks = np.array([v for v in range(V) if v not in (blank, pad)])
    for _ in range(steps):
        yield (rng.integers(0, N, N).astype(np.int32), toks[rng.integers(0, len(toks), N)].astype(np.int32),
               (rng.random(N) < 0.35).astype(np.uint8))


def steered_triples(lm, rng, N):
    """Triples that walk row i along one of the file's highest-order n-grams, a word per step (parent = identity, keep = 0):
    the contexts then have present and absent suffixes of every length, which random tokens almost never reach."""
    ng = lm.ngram.records(lm.order)[0]
    word2tok = {int(w): v for v, w in enumerate(lm.tok2word) if w >= 0}
    ok = [g for g in ng.tolist() if all(w in word2tok for w in g)]
    if lm.order < 2 or not ok:
        return
    pick = [ok[i] for i in rng.integers(0, len(ok), N)]
    for k in range(lm.order):
        yield (np.arange(N, dtype=np.int32), np.array([word2tok[g[k]] for g in pick], dtype=np.int32), np.zeros(N, dtype=np.uint8))


def walk_triples(lm, rng, N, steps):
    """`steps` triples for N rows: first along n-grams of the file, then at random."""
    d = lm.dictionary
    out = list(steered_triples(lm, rng, N))[:steps]
    return out + list(random_triples(rng, N, len(d), steps - len(out), d.bos(), d.pad()))
