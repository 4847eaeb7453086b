"""Float64 restatement of the streamed lexicon beam search for tests/test_streaming_lexicon_beam.py:
tests.test_ctc_prefix_beam.prefix_beam_oracle with the beam kept between calls, so that it can be fed frame ranges, asked
for a finish at any moment, and asked for what `partial` reports.  The arithmetic of a frame and of the finish is that of
prefix_beam_oracle, expression by expression, in the same order: test_stepwise_oracle_equals_prefix_beam_oracle holds the
two equal as float64."""
import math

import numpy as np

from tests.test_ctc_prefix_beam import _lae


class StepwiseBeamOracle:
    def __init__(self, beam, K, blank, lm_fn, lm_weight=1.0, bonus=0.0, eos=None):
        self.beam, self.K, self.blank, self.lm_fn, self.bonus, self.eos = beam, K, blank, lm_fn, bonus, eos
        self.lw = lm_weight if lm_fn is not None else 0.0
        self.hyps = [((), 0.0, -math.inf, 0.0)]  # (prefix, pb, pnb, lm), best first
        self.margin = math.inf                   # the smallest pruning margin met so far
        self.frames = 0

    def feed(self, x):
        """x (n, V) log-prob rows: the next n frames."""
        x = np.asarray(x, dtype=np.float64)
        blank, K, beam, lm_fn, lw, bonus = self.blank, self.K, self.beam, self.lm_fn, self.lw, self.bonus
        for t in range(x.shape[0]):
            row = x[t]
            cands = sorted(sorted((v for v in range(x.shape[1]) if v != blank), key=lambda v: (-row[v], v))[:K])
            nxt = {}

            def add(y, pb, pnb, lm, key, stay):
                if y in nxt:
                    e = nxt[y]
                    e[0], e[1] = _lae(e[0], pb), _lae(e[1], pnb)
                    if stay:
                        e[2], e[3] = lm, key
                else:
                    nxt[y] = [pb, pnb, lm, key]

            for j, (y, pb, pnb, lm) in enumerate(self.hyps):
                sc = _lae(pb, pnb)
                last = y[-1] if y else None
                add(y, sc + row[blank], pnb + row[last] if (y and last in cands) else -math.inf, lm, (j, 0, 0), True)
                lrow = lm_fn(y) if lm_fn is not None else None
                for c in cands:
                    add(y + (c,), -math.inf, (pb if c == last else sc) + row[c], lm + (lrow[c] if lrow is not None else 0.0),
                        (j, 1, c), False)
            scored = sorted(((_lae(e[0], e[1]) + lw * e[2] + bonus * len(y), e[3], y, e) for y, e in nxt.items()),
                            key=lambda r: (-r[0], r[1]))
            if len(scored) > beam:
                self.margin = min(self.margin, scored[beam - 1][0] - scored[beam][0])
            self.hyps = [(y, e[0], e[1], e[2]) for _, _, y, e in scored[:beam]]
            self.frames += 1

    def finish(self, nbest=1):
        """([(tokens, final score)] best first, the smallest pruning / ranking margin met); the beam is left as it is."""
        margin = self.margin
        fin = []
        for j, (y, pb, pnb, lm) in enumerate(self.hyps):
            s = _lae(pb, pnb) + self.lw * lm + self.bonus * len(y)
            if self.lm_fn is not None:
                s += self.lw * self.lm_fn(y)[self.eos]
            fin.append((s, j, y))
        fin.sort(key=lambda r: (-r[0], r[1]))
        top = fin[: nbest + 1]
        for a, b in zip(top, top[1:]):
            margin = min(margin, a[0] - b[0])
        return [(y, s) for s, _, y in fin[:nbest]], margin

    def in_beam_scores(self):
        return [_lae(pb, pnb) + self.lw * lm + self.bonus * len(y) for y, pb, pnb, lm in self.hyps]

    def partial(self):
        """(best tokens, its in-beam score, stable prefix, margin): the live hypothesis with the best in-beam score (ties: the
        lower slot), the longest common prefix of the live hypotheses with a finite in-beam score (of all when none is), and
        the smallest of the pruning margins so far and the lead of the best hypothesis over the second."""
        sc = self.in_beam_scores()
        j = min(range(len(sc)), key=lambda i: (-sc[i], i))
        members = [y for (y, _, _, _), s in zip(self.hyps, sc) if s > -math.inf] or [h[0] for h in self.hyps]
        n = 0
        while all(len(y) > n for y in members) and len({y[n] for y in members}) == 1:
            n += 1
        margin = self.margin
        rest = sorted(sc, reverse=True)
        if len(rest) > 1:
            margin = min(margin, rest[0] - rest[1])
        return self.hyps[j][0], sc[j], members[0][:n], margin
