"""Float64 restatements for tests/test_ngram_lexicon_ctc.py: an ARPA scorer over Python dicts, a random ARPA writer, and the
lexicon + n-gram fusion increments of tools/ctc_lexicon_beam_search.py as an `lm_fn` for
tests.test_ctc_prefix_beam.prefix_beam_oracle."""
import math

import numpy as np

LN10 = math.log(10.0)


class ArpaRef:
    """ln P(w | h) by the ARPA backoff rules, from dicts of the file's values (converted to natural log)."""

    def __init__(self, text):
        self.prob, self.bow, self.order = {}, {}, 0
        self.vocab = []
        section = 0
        for line in text.splitlines():
            line = line.strip()
            if not line or line.startswith("ngram ") or line == "\\data\\" or line == "\\end\\":
                continue
            if line.startswith("\\") and line.endswith("-grams:"):
                section = int(line[1:].split("-")[0])
                self.order = max(self.order, section)
                continue
            if section == 0:
                continue
            f = line.split()
            ng = tuple(f[1: 1 + section])
            self.prob[ng] = float(f[0]) * LN10
            if len(f) == section + 2:
                self.bow[ng] = float(f[-1]) * LN10
            if section == 1:
                self.vocab.append(ng[0])

    def logp(self, ctx, w):
        if (w,) not in self.prob:
            w = "<unk>"
            if (w,) not in self.prob:
                return -math.inf
        h = tuple(ctx)[len(ctx) - (self.order - 1):] if self.order > 1 else ()
        acc = 0.0
        for l in range(len(h), -1, -1):
            hh = h[len(h) - l:]
            if hh + (w,) in self.prob:
                return acc + self.prob[hh + (w,)]
            acc += self.bow.get(hh, 0.0)
        raise AssertionError("unreachable: every word is a unigram")

    def sentence(self, words):
        """L(y) + ln P(</s> | ...) of a word sequence, <s> as the start."""
        ctx, s = ["<s>"], 0.0
        for w in list(words) + ["</s>"]:
            s += self.logp(ctx, w)
            ctx.append(w)
        return s


def random_arpa(rng, words, order, per_order, unk=True, bow_p=0.7):
    """Text of a random ARPA file over `words` (+ <s>, </s>, optionally <unk>): every n-gram extends an existing
    (n-1)-gram, so that contexts are present; about bow_p of the records below the top order carry a backoff weight."""
    uni = ["<s>", "</s>"] + (["<unk>"] if unk else []) + list(words)
    grams = [[(w,) for w in uni]]
    for k in range(2, order + 1):
        seen, prev = set(), [g for g in grams[-1] if g[-1] != "</s>"]
        for _ in range(per_order * 4):
            if len(seen) >= per_order:
                break
            g = prev[rng.integers(len(prev))] + (uni[1 + rng.integers(len(uni) - 1)],)
            seen.add(g)
        seen = sorted(seen)  # (set order depends on the string hash seed)
        grams.append([seen[i] for i in rng.permutation(len(seen))])
    out = ["", "\\data\\"] + [f"ngram {k + 1}={len(g)}" for k, g in enumerate(grams)] + [""]
    for k, gs in enumerate(grams, 1):
        out.append(f"\\{k}-grams:")
        for g in gs:
            lp = -99.0 if g == ("<s>",) else round(float(rng.uniform(-3.0, -0.05)), 4)
            line = f"{lp}\t{' '.join(g)}"
            if k < order and rng.random() < bow_p:
                line += f"\t{round(float(rng.uniform(-1.0, 0.3)), 4)}"
            out.append(line)
        out.append("")
    out.append("\\end\\")
    return "\n".join(out) + "\n"


class FusionRef:
    """The increments of the scoring contract, float64, over a token dictionary: spell = {token tuple: word};
    `space` >= 0 = space mode, else word_start[v] marks the tokens that start a word.  `lm_fn(prefix)` returns V + 1 values:
    [v] = the increment of appending v (lm_weight and word_score applied), [V] = the end term; use it with
    prefix_beam_oracle(..., lm_weight=1.0, eos=V)."""

    def __init__(self, ref, spell, V, space=-1, word_start=None, alpha=1.0, beta=0.0):
        self.ref, self.spell, self.V, self.space, self.ws = ref, dict(spell), V, space, word_start
        self.alpha, self.beta = alpha, beta
        self.smear = {(): 0.0}
        for sp, w in self.spell.items():
            u = ref.logp((), w)
            for i in range(1, len(sp) + 1):
                self.smear[sp[:i]] = max(self.smear.get(sp[:i], -math.inf), u)
        self._cache = {}

    def _bound(self, c):
        return c == self.space if self.space >= 0 else bool(self.ws[c])

    def _end_word(self, words, part):
        """(increment, word) of completing `part` after `words`; None if it is no word (or empty)."""
        if part not in self.spell:
            return None
        w = self.spell[part]
        return self.alpha * (self.ref.logp(["<s>"] + words, w) - self.smear[part]) + self.beta, w

    def step(self, state, c):
        """(increment, new state) of appending token c to state (words list, partial tuple); increment -inf = invalid."""
        words, part = state
        inc = 0.0
        if self._bound(c):
            if self.space >= 0 or part:
                e = self._end_word(words, part)
                if e is None:
                    return -math.inf, None
                inc, words = e[0], words + [e[1]]
            part = ()
            if self.space >= 0:
                return inc, (words, part)
        nxt = part + (c,)
        if nxt not in self.smear:
            return -math.inf, None
        return inc + self.alpha * (self.smear[nxt] - self.smear[part]), (words, nxt)

    def end(self, state):
        words, part = state
        inc = 0.0
        if part:
            e = self._end_word(words, part)
            if e is None:
                return -math.inf
            inc, words = e[0], words + [e[1]]
        return inc + self.alpha * self.ref.logp(["<s>"] + words, "</s>")

    def state(self, prefix):
        if prefix not in self._cache:
            if not prefix:
                self._cache[prefix] = ([], ())
            else:
                prev = self.state(prefix[:-1])
                self._cache[prefix] = None if prev is None else self.step(prev, prefix[-1])[1]
        return self._cache[prefix]

    def lm_fn(self, prefix):
        row = np.full(self.V + 1, -math.inf)
        st = self.state(tuple(prefix))
        if st is not None:
            for c in range(self.V):
                row[c] = self.step(st, c)[0]
            row[self.V] = self.end(st)
        return row
