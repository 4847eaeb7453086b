"""Float64 numpy statement of the frame-synchronous transducer beam search contract (csrc/rnnt_beam.hip),
and the seeded table model the tests drive it with.  tests/test_transducer_frame_beam.py holds the HIP search to
`frame_beam_oracle` and the oracle itself to brute force over every alignment."""
import math

import numpy as np


def _lae(a, b):
    m = max(a, b)
    return -math.inf if m == -math.inf else m + math.log1p(math.exp(-abs(a - b)))


def _lse(x):
    m = np.max(x)
    return -math.inf if m == -math.inf else float(m + np.log(np.sum(np.exp(x - m))))


def fused_row(logits, blank, temperature=1.0, lm_row=None, lm_weight=0.0, eos=None, predicts_eos=False):
    """Steps 1 - 3 of the contract on one logits row [V] -> float64 r [V].  lm_row: [V], or [V - 1] (no blank entry: token
    v > blank reads column v - 1)."""
    z = np.asarray(logits, dtype=np.float64) / temperature
    V = z.shape[0]
    r = z - _lse(z)
    if lm_row is not None:
        m = np.asarray(lm_row, dtype=np.float64)
        nb = np.arange(V) != blank
        if m.shape[0] == V - 1:
            m = np.concatenate((m[:blank], [0.0], m[blank:]))
        assert m.shape[0] == V
        f = r[nb] + lm_weight * m[nb]
        r[nb] = f + _lse(r[nb]) - _lse(f)
    if predicts_eos:
        r[blank] = _lae(r[blank], r[eos])
        r[eos] = -math.inf
    return r


def frame_beam_oracle(logits_fn, length, beam, K, blank, lm_fn=None, lm_weight=0.0, eos=None, predicts_eos=False, temperature=1.0,
                      normalize=True, nbest=1):
    """logits_fn(t, y) -> the joint's logits row [V] of hypothesis y (a tuple) at frame t; lm_fn(y) -> log P_lm(. | eos + y), [V]
    or [V - 1].  Returns ([(tokens, final score)] best first, triples, margin): triples[t] = [(parent slot, token, keep)] of the
    live slots after frame t; margin = the smallest difference the search's decisions rested on (between neighbours of the
    ranked candidates up to the first pruned one, between the K-th and the (K + 1)-th token of a row, between neighbours of
    the final ranking up to the first one not returned)."""
    hyps = [((), 0.0)]
    triples = []
    margin = math.inf
    for t in range(length):
        cands = {}  # y -> [score, key, parent, token, keep]
        exts = []
        for j, (y, s) in enumerate(hyps):
            r = fused_row(logits_fn(t, y), blank, temperature, lm_fn(y) if lm_fn is not None else None, lm_weight, eos, predicts_eos)
            cands[y] = [s + r[blank], (j, 0, 0), j, blank, 1]
            idx = np.flatnonzero(np.isfinite(r) & (np.arange(r.shape[0]) != blank))
            order = [int(v) for v in idx[np.lexsort((idx, -r[idx]))][: K + 1]]  # by (-r, id)
            if len(order) > K:
                margin = min(margin, r[order[K - 1]] - r[order[K]])
            exts += [(y + (v,), s + r[v], (j, 1, v), j, v) for v in order[:K]]
        for y, s, key, j, v in exts:
            if y in cands:  # an extension meets a stay: the stay's key and state win
                cands[y][0] = _lae(cands[y][0], s)
            else:
                cands[y] = [s, key, j, v, 0]
        ranked = sorted(((y, c) for y, c in cands.items() if np.isfinite(c[0])), key=lambda e: (-e[1][0], e[1][1]))
        for a, b in zip(ranked[:beam], ranked[1:beam + 1]):
            margin = min(margin, a[1][0] - b[1][0])
        hyps = [(y, c[0]) for y, c in ranked[:beam]]
        triples.append([(c[2], c[3], c[4]) for _, c in ranked[:beam]])
    fin = sorted(((s / max(1, len(y)) if normalize else s, j, y) for j, (y, s) in enumerate(hyps)), key=lambda e: (-e[0], e[1]))
    for a, b in zip(fin[:nbest], fin[1:nbest + 1]):
        margin = min(margin, a[0] - b[0])
    return [(y, s) for s, _, y in fin[:nbest]], triples, margin


class TableModel:
    """A seeded "joint": the logits row of (utterance b, frame t, hypothesis y) is fp32 noise that depends on all three, plus a
    peak on a token that depends on (b, t // 2) only (blank half of the time) — neighbouring frames and all hypotheses of an
    utterance agree on the likely token, so extensions meet stays as they do with a trained model.  Rows are cached; values
    are float32-representable, so a device copy holds exactly what the oracle reads."""

    def __init__(self, V, seed, blank=0, sharp=6.0, scale=3.0):
        self.V, self.seed, self.blank, self.sharp, self.scale = V, seed, blank, sharp, scale
        self._rows = {}

    def row(self, b, t, y):
        k = (b, t, y)
        if k not in self._rows:
            z = self.scale * np.random.default_rng([self.seed, b, t, len(y), *y]).standard_normal(self.V)
            g = np.random.default_rng([self.seed, b, t // 2, 1 << 20])
            peak = self.blank if g.random() < 0.5 else int(g.integers(0, self.V))
            z[peak] += self.sharp
            self._rows[k] = z.astype(np.float32)
        return self._rows[k]

    def logits_fn(self, b):
        return lambda t, y: self.row(b, t, y).astype(np.float64)


class TableLM:
    """A seeded "LM": log-softmax rows over n entries that depend on the hypothesis alone (fp32-representable)."""

    def __init__(self, n, seed, scale=1.5):
        self.n, self.seed, self.scale = n, seed, scale
        self._rows = {}

    def row(self, y):
        if y not in self._rows:
            z = self.scale * np.random.default_rng([self.seed, 7, len(y), *y]).standard_normal(self.n)
            self._rows[y] = (z - _lse(z)).astype(np.float32)
        return self._rows[y]

    def __call__(self, y):
        return self.row(y).astype(np.float64)
