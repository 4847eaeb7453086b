"""Float64 oracles of the time-stamp contract of the four token-level beam searches (DESIGN.md sections 3.3b / 3.4 / 3.5, "Time
stamps"): tests.streaming_beam_ref.StepwiseBeamOracle (and so tests.test_ctc_prefix_beam.prefix_beam_oracle) and
tests.transducer_hotword_ref.biased_beam (and so tests.transducer_frame_beam_ref.frame_beam_oracle) restated, expression by
expression and in the same order, with what the contract adds: per hypothesis the same sums with max in place of log-add-exp (the
Viterbi score) and the frames at which its tokens start on that best path, kept here as a tuple per score instead of a pointer
into a pool of time nodes.  Every max the times rest on records the gap between its two sides (`vgap`), as the pruning decisions
record theirs (`margin`): a test that compares fp32 kernels with these oracles asserts both clear of its bound.
tests/test_beam_time_stamps.py holds the oracles equal to the ones they restate on tokens and scores, and their times and Viterbi
scores to brute force over every alignment."""
import math

import numpy as np

from tests.test_ctc_prefix_beam import _lae
from tests.transducer_frame_beam_ref import fused_row

NEG = -math.inf


class _Gaps:
    """The smallest gap any max-decision rested on; a decision between two -inf is none (the tie rule decides it exactly)."""

    def __init__(self):
        self.vgap = math.inf

    def larger(self, a, b):
        """Of two (score, times) pairs the one with the larger score; `a` wins ties."""
        if a[0] == NEG and b[0] == NEG:
            return a
        self.vgap = min(self.vgap, abs(a[0] - b[0]))
        return b if b[0] > a[0] else a


class PrefixBeamTimesOracle(_Gaps):
    """StepwiseBeamOracle with the CTC time-stamp contract.  A hypothesis is (prefix, pb, pnb, lm, B, NB): B = (vb, times of the
    path behind vb), NB likewise for vnb.  `lm_fn` may be tests.hotword_ref.bias_lm_fn: LM, bonus and bias are per-token terms and
    stay out of the Viterbi scores."""

    def __init__(self, beam, K, blank, lm_fn=None, lm_weight=0.0, bonus=0.0, eos=None):
        super().__init__()
        self.beam, self.K, self.blank, self.lm_fn, self.bonus, self.eos = beam, K, blank, lm_fn, bonus, eos
        self.lw = lm_weight if lm_fn is not None else 0.0
        self.hyps = [((), 0.0, NEG, 0.0, (0.0, ()), (NEG, ()))]
        self.margin = math.inf
        self.frames = 0

    def feed(self, x):
        x = np.asarray(x, dtype=np.float64)
        blank, K, beam, lm_fn, lw, bonus = self.blank, self.K, self.beam, self.lm_fn, self.lw, self.bonus
        for i in range(x.shape[0]):
            row, t = x[i], self.frames
            cands = sorted(sorted((v for v in range(x.shape[1]) if v != blank), key=lambda v: (-row[v], v))[:K])
            nxt = {}  # prefix -> [pb, pnb, lm, order key, B, NB]

            def add(y, pb, pnb, lm, key, stay, B, NB):
                if y in nxt:
                    e = nxt[y]
                    e[0], e[1] = _lae(e[0], pb), _lae(e[1], pnb)
                    if stay:  # the entry so far is the merging extension: it replaces the stay's NB only if strictly larger
                        e[2], e[3], e[4] = lm, key, B
                        e[5] = self.larger(NB, e[5])
                    else:
                        e[5] = self.larger(e[5], NB)
                else:
                    nxt[y] = [pb, pnb, lm, key, B, NB]

            for j, (y, pb, pnb, lm, B, NB) in enumerate(self.hyps):
                sc = _lae(pb, pnb)
                last = y[-1] if y else None
                big = self.larger(B, NB)  # tie: the blank one
                add(y, sc + row[blank], pnb + row[last] if (y and last in cands) else NEG, lm, (j, 0, 0), True,
                    (big[0] + row[blank], big[1]), (NB[0] + row[last] if (y and last in cands) else NEG, NB[1]))
                lrow = lm_fn(y) if lm_fn is not None else None
                for c in cands:
                    src = B if c == last else big
                    times = src[1] + (t,)  # the new time node
                    add(y + (c,), NEG, (pb if c == last else sc) + row[c], lm + (lrow[c] if lrow is not None else 0.0),
                        (j, 1, c), False, (NEG, times), (src[0] + row[c], times))
            scored = sorted(((_lae(e[0], e[1]) + lw * e[2] + bonus * len(y), e[3], y, e) for y, e in nxt.items()),
                            key=lambda r: (-r[0], r[1]))
            if len(scored) > beam:
                self.margin = min(self.margin, scored[beam - 1][0] - scored[beam][0])
            self.hyps = [(y, e[0], e[1], e[2], e[4], e[5]) for _, _, y, e in scored[:beam]]
            self.frames += 1

    def finish(self, nbest=1):
        """([(tokens, final score, times, Viterbi score)] best first, margin, vgap); the beam is left as it is."""
        margin = self.margin
        fin = []
        for j, (y, pb, pnb, lm, B, NB) in enumerate(self.hyps):
            s = _lae(pb, pnb) + self.lw * lm + self.bonus * len(y)
            if self.lm_fn is not None:
                s += self.lw * self.lm_fn(y)[self.eos]
            fin.append((s, j, y, self.larger(B, NB)))
        fin.sort(key=lambda r: (-r[0], r[1]))
        top = fin[: nbest + 1]
        for a, b in zip(top, top[1:]):
            margin = min(margin, a[0] - b[0])
        return [(y, s, best[1], best[0]) for s, _, y, best in fin[:nbest]], margin, self.vgap


def prefix_beam_times_oracle(x, length, beam, K, blank, lm_fn=None, lm_weight=0.0, bonus=0.0, eos=None, nbest=1):
    """prefix_beam_oracle with times: ([(tokens, final score, times, Viterbi score)], margin, vgap)."""
    o = PrefixBeamTimesOracle(beam, K, blank, lm_fn, lm_weight, bonus, eos)
    o.feed(np.asarray(x, dtype=np.float64)[:length])
    return o.finish(nbest)


def frame_beam_times_oracle(logits_fn, length, beam, K, blank, graph=None, lm_fn=None, lm_weight=0.0, eos=None, predicts_eos=False,
                            temperature=1.0, normalize=True, nbest=1):
    """frame_beam_oracle (graph None) / biased_frame_beam_oracle with the transducer time-stamp contract:
    ([(tokens, final score, times, Viterbi score)] best first, triples, margin, vgap, pmargin).  v accumulates the fused r that s
    does.  margin is frame_beam_oracle's (it also covers the order of the slots inside the beam, which the triples show); pmargin
    covers only what decides which hypotheses exist and which are returned: the K-th against the (K + 1)-th token of a row, the
    last kept candidate against the first pruned one, and the neighbours of the final ranking up to the first one not returned."""
    g = _Gaps()
    pmargin = math.inf
    hyps = [((), 0.0, 0, 0.0, (0.0, ()))]  # (tokens, s, q, b, (v, times))
    triples = []
    margin = math.inf
    for t in range(length):
        cands = {}  # y -> [s, key, parent, token, keep, q, b, (v, times)]
        exts = []
        for j, (y, s, q, b, vt) in enumerate(hyps):
            r = fused_row(logits_fn(t, y), blank, temperature, lm_fn(y) if lm_fn is not None else None, lm_weight, eos, predicts_eos)
            cands[y] = [s + r[blank], (j, 0, 0), j, blank, 1, q, b, (vt[0] + r[blank], vt[1])]
            idx = np.flatnonzero(np.isfinite(r) & (np.arange(r.shape[0]) != blank))
            order = [int(v) for v in idx[np.lexsort((idx, -r[idx]))][: K + 1]]  # by (-r, id)
            if len(order) > K:
                margin = min(margin, r[order[K - 1]] - r[order[K]])
                pmargin = min(pmargin, r[order[K - 1]] - r[order[K]])
            for v in order[:K]:
                q2, inc = graph.step(q, v) if graph is not None else (0, 0.0)
                exts.append((y + (v,), s + r[v], (j, 1, v), j, v, q2, b + inc, (vt[0] + r[v], vt[1] + (t,))))
        for y, s, key, j, v, q2, b2, vt in exts:
            if y in cands:  # an extension meets a stay: it replaces the stay's (v, times) only if strictly larger
                cands[y][0] = _lae(cands[y][0], s)
                cands[y][7] = g.larger(cands[y][7], vt)
            else:
                cands[y] = [s, key, j, v, 0, q2, b2, vt]
        ranked = sorted(((y, c) for y, c in cands.items() if np.isfinite(c[0])), key=lambda e: (-(e[1][0] + e[1][6]), e[1][1]))
        for a, b_ in zip(ranked[:beam], ranked[1:beam + 1]):
            margin = min(margin, (a[1][0] + a[1][6]) - (b_[1][0] + b_[1][6]))
        if len(ranked) > beam:
            pmargin = min(pmargin, (ranked[beam - 1][1][0] + ranked[beam - 1][1][6]) - (ranked[beam][1][0] + ranked[beam][1][6]))
        hyps = [(y, c[0], c[5], c[6], c[7]) for y, c in ranked[:beam]]
        triples.append([(c[2], c[3], c[4]) for _, c in ranked[:beam]])
    pend = (lambda q: graph.pending(q)) if graph is not None else (lambda q: 0.0)
    fin = sorted((((s + b - pend(q)) / (max(1, len(y)) if normalize else 1), j, y, vt) for j, (y, s, q, b, vt) in enumerate(hyps)),
                 key=lambda e: (-e[0], e[1]))
    for a, b_ in zip(fin[:nbest], fin[1:nbest + 1]):
        margin = min(margin, a[0] - b_[0])
        pmargin = min(pmargin, a[0] - b_[0])
    return [(y, s, vt[1], vt[0]) for s, _, y, vt in fin[:nbest]], triples, margin, g.vgap, pmargin


# ------------------------------------------------------------------------------------------------ brute force
def ctc_best_alignments(x, blank):
    """Every frame-labelling of x (T, V): label sequence -> (best path score, start frame of every token on that path, lead over
    the second-best path of the same sequence).  A token starts where its run of equal non-blank labels begins."""
    import itertools

    T, V = x.shape
    best = {}
    for path in itertools.product(range(V), repeat=T):
        y, starts, prev = [], [], blank
        for t, v in enumerate(path):
            if v != blank and v != prev:
                y.append(v)
                starts.append(t)
            prev = v
        sc = float(sum(x[t, v] for t, v in enumerate(path)))
        cur = best.get(tuple(y))
        if cur is None or sc > cur[0]:
            best[tuple(y)] = (sc, tuple(starts), sc - cur[0] if cur is not None else math.inf)
        elif sc > cur[0] - cur[2]:
            best[tuple(y)] = (cur[0], cur[1], cur[0] - sc)
    return best


def transducer_best_alignments(logits_fn, T, V, blank, lm_fn=None, lm_weight=0.0):
    """Every alignment (blank or one token per frame): token sequence -> (best path score, the frames that emit, lead)."""
    import itertools

    best = {}
    for path in itertools.product(range(V), repeat=T):
        y, emit, sc = (), [], 0.0
        for t, v in enumerate(path):
            r = fused_row(logits_fn(t, y), blank, 1.0, lm_fn(y) if lm_fn is not None else None, lm_weight)
            sc += r[v]
            if v != blank:
                y = y + (v,)
                emit.append(t)
        cur = best.get(y)
        if cur is None or sc > cur[0]:
            best[y] = (sc, tuple(emit), sc - cur[0] if cur is not None else math.inf)
        elif sc > cur[0] - cur[2]:
            best[y] = (cur[0], cur[1], cur[0] - sc)
    return best


# ------------------------------------------------------------------------------------------------ state sizes (the headers')
def ctc_times_words(T, beam):
    return 4 * beam + 2 + 2 * (1 + T * beam)


def rnnt_times_words(T, beam):
    return 2 * beam + 2 + 2 * (1 + T * beam)
