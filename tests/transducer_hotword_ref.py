"""Float64 reference of hotword biasing of the frame-synchronous transducer beam search ("Hotword
biasing"): tests.transducer_frame_beam_ref.frame_beam_oracle restated with the automaton state (q, b) of every hypothesis, through
ContextGraph.step / pending (the dict-of-nodes replay, not the packed tables the kernels walk), and the phrase recipe the CPU and
GPU tests share.  B(y) itself is held to tests.hotword_ref.locked_bonus, which knows no automaton."""
import math

import numpy as np

from tests.hotword_ref import BOOSTS
from tests.transducer_frame_beam_ref import _lae, frame_beam_oracle, fused_row


def biased_beam(logits_fn, length, beam, K, blank, graph, lm_fn=None, lm_weight=0.0, eos=None, predicts_eos=False, temperature=1.0):
    """The live beam [(tokens, s, q, b)] in slot order after `length` frames, the triples of every frame and the smallest
    margin of the decisions so far (per-row top K on r, as in the unbiased search; ranking on s + b)."""
    hyps = [((), 0.0, 0, 0.0)]
    triples = []
    margin = math.inf
    for t in range(length):
        cands = {}  # y -> [s, key, parent, token, keep, q, b]
        exts = []
        for j, (y, s, q, b) in enumerate(hyps):
            r = fused_row(logits_fn(t, y), blank, temperature, lm_fn(y) if lm_fn is not None else None, lm_weight, eos, predicts_eos)
            cands[y] = [s + r[blank], (j, 0, 0), j, blank, 1, q, b]
            idx = np.flatnonzero(np.isfinite(r) & (np.arange(r.shape[0]) != blank))
            order = [int(v) for v in idx[np.lexsort((idx, -r[idx]))][: K + 1]]  # by (-r, id): the row phase knows no bias
            if len(order) > K:
                margin = min(margin, r[order[K - 1]] - r[order[K]])
            for v in order[:K]:
                q2, inc = graph.step(q, v)
                exts.append((y + (v,), s + r[v], (j, 1, v), j, v, q2, b + inc))
        for y, s, key, j, v, q2, b2 in exts:
            if y in cands:  # an extension meets a stay: log-add-exp on s; key, predictor state and (q, b) are the stay's
                assert cands[y][5] == q2 and abs(cands[y][6] - b2) < 1e-9, (y, cands[y], q2, b2)  # functions of the tokens
                cands[y][0] = _lae(cands[y][0], s)
            else:
                cands[y] = [s, key, j, v, 0, q2, b2]
        ranked = sorted(((y, c) for y, c in cands.items() if np.isfinite(c[0])), key=lambda e: (-(e[1][0] + e[1][6]), e[1][1]))
        for a, b_ in zip(ranked[:beam], ranked[1:beam + 1]):
            margin = min(margin, (a[1][0] + a[1][6]) - (b_[1][0] + b_[1][6]))
        hyps = [(y, c[0], c[5], c[6]) for y, c in ranked[:beam]]
        triples.append([(c[2], c[3], c[4]) for _, c in ranked[:beam]])
    return hyps, triples, margin


def biased_frame_beam_oracle(logits_fn, length, beam, K, blank, graph, lm_fn=None, lm_weight=0.0, eos=None, predicts_eos=False,
                             temperature=1.0, normalize=True, nbest=1):
    """frame_beam_oracle with a context graph: ([(tokens, final score)] best first, triples, margin).  final = s + b - phi(q),
    divided by max(1, |y|) with normalize; the nbest best by (-final, slot)."""
    hyps, triples, margin = biased_beam(logits_fn, length, beam, K, blank, graph, lm_fn, lm_weight, eos, predicts_eos, temperature)
    fin = sorted((((s + b - graph.pending(q)) / (max(1, len(y)) if normalize else 1), j, y) for j, (y, s, q, b) in enumerate(hyps)),
                 key=lambda e: (-e[0], e[1]))
    for a, b_ in zip(fin[:nbest], fin[1:nbest + 1]):
        margin = min(margin, a[0] - b_[0])
    return [(y, s) for s, _, y in fin[:nbest]], triples, margin


def biased_partial_oracle(hyps):
    """(tokens of the live hypothesis with the best s + b, ties to the lower slot; length of the longest common prefix; s + b)."""
    best = max(range(len(hyps)), key=lambda j: (hyps[j][1] + hyps[j][3], -j))
    k = 0
    while all(len(h[0]) > k for h in hyps) and len({h[0][k] for h in hyps}) == 1:
        k += 1
    return hyps[best][0], k, hyps[best][1] + hyps[best][3]


def cut_phrases(logits_fns, lens, blank, V, **kw):
    """The recipe of tests.hotword_ref.grid_phrases on this search: of every utterance the 2- and 3-grams of the second and third
    best unbiased hypotheses (beam 16, K 4), boosted alternately by BOOSTS; then a proper prefix of the first 3-gram, a phrase that
    ends inside it (reached through a failure link only while the longer one is pending: not credited), and one of 64 tokens,
    which no utterance here is long enough to complete.  [(tokens, boost)]."""
    phrases, n = [], 0
    for fn, L in zip(logits_fns, lens):
        hyps, _, _ = frame_beam_oracle(fn, int(L), 16, min(4, V - 1), blank, nbest=3, **kw)
        for y, _ in hyps[1:]:
            for k in (2, 3):
                for i in range(len(y) - k + 1):
                    phrases.append((list(y[i:i + k]), BOOSTS[n % 2]))
                    n += 1
    long3 = next((p for p, _ in phrases if len(p) == 3), None)
    if long3 is not None:
        phrases.append((long3[:1], 0.41))
        phrases.append((long3[1:2], 0.29))
    first = long3[0] if long3 is not None else 3
    phrases.append(([first] + [3 + (i % 5) for i in range(63)], 0.37))
    return phrases
