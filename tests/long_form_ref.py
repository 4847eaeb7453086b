"""NumPy fp64 restatement of long-form recognition (espresso_amd/tools/long_form.py, csrc/long_form.hip): the window plan, the
cut rule and the stitch, as include/espresso_amd.h ("Long-form recognition") states them.  Written from the rule, not from the
kernel: loops over frames, no vector tricks."""
import math

import numpy as np


# ------------------------------------------------------------------------------------------------------- the plan
def plan(N, W, O):
    """(start, length) of the windows of a recording of N samples: Nw = max(1, ceil((N - O) / H)), H = W - O; window n starts at
    n * H and is W long, the last one runs to the end."""
    H = W - O
    nw = max(1, math.ceil((N - O) / H))
    return [(n * H, W if n < nw - 1 else N - n * H) for n in range(nw)]


# ------------------------------------------------------------------------------------------------------- the rows
def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


# ------------------------------------------------------------------------------------------------------- the cuts
def junction(logits, counts, n, Hf, V, blank, edge, guard):
    """Junction n of logits [Nw][Tw][>= V] (any float dtype): (cut, score, ranked) with `ranked` the candidates' (score, c) best
    first under the rule's order (empty without candidates)."""
    lo = (n + 1) * Hf
    hi = min(n * Hf + counts[n], lo + counts[n + 1])
    if hi <= lo:
        return lo, 0.0, []
    b = {}
    for j in range(lo, hi):
        ba = log_softmax64(logits[n, j - n * Hf, :V])[blank]
        bb = log_softmax64(logits[n + 1, j - (n + 1) * Hf, :V])[blank]
        b[j] = min(ba, bb)

    def score(c):
        js = [j for j in range(c - guard, c + guard) if lo <= j < hi]
        if not js:
            return b[min(max(c, lo), hi - 1)]
        return min(b[j] for j in js)

    cands = list(range(lo + edge, hi - edge + 1))
    if not cands:
        c = (lo + hi) // 2
        return c, score(c), []
    ranked = sorted(((score(c), c) for c in cands), key=lambda sc: (-sc[0], abs(2 * sc[1] - (lo + hi)), sc[1]))
    return ranked[0][1], ranked[0][0], ranked


def cuts(logits, counts, Hf, V, blank, edge, guard):
    """(cuts [Nw - 1], scores [Nw - 1], margin): margin = the least lead, over the junctions, of the best score over the next
    lower score among the candidates (inf where all candidates score alike).  Candidates whose guard ranges cover the same
    overlap frames take their score from the same b(j) and tie exactly, in any precision: the tie rule decides those."""
    cs, ss, margin = [], [], math.inf
    for n in range(len(counts) - 1):
        c, s, ranked = junction(logits, counts, n, Hf, V, blank, edge, guard)
        cs.append(c)
        ss.append(s)
        lower = [sc for sc, _ in ranked if sc < s]
        if lower:
            margin = min(margin, s - max(lower))
    return cs, ss, margin


# ------------------------------------------------------------------------------------------------------- the stitch
def owners(counts, cut_list, Hf):
    """(window, local frame) of every global frame: window 0 before cuts[0], window n from cuts[n - 1] up to cuts[n]."""
    Nw = len(counts)
    T = (Nw - 1) * Hf + counts[-1]
    out = []
    for t in range(T):
        n = 0
        while n < Nw - 1 and t >= cut_list[n]:
            n += 1
        out.append((n, t - n * Hf))
    return out


def stitch(logits, counts, cut_list, Hf, V):
    """fp64 log-probs [T][V] of the recording."""
    return np.stack([log_softmax64(logits[n, j, :V]) for n, j in owners(counts, cut_list, Hf)]) if counts[-1] + len(counts) > 1 else np.zeros((0, V))


def greedy(lp, blank):
    """CTC greedy decode of log-probs [T][V]: argmax per frame, repeats merged, blanks dropped."""
    out, prev = [], None
    for k in np.asarray(lp).argmax(axis=-1).tolist():
        if k != prev and k != blank:
            out.append(k)
        prev = k
    return out
