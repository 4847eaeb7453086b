"""NumPy fp64 restatement of the long-form join of encoder outputs (espresso_amd/tools/long_form.py LongFormTransducer,
csrc/long_form.hip), as include/espresso_amd.h ("Long-form recognition for transducer models") states it.  Written from the
rule, not from the kernel: loops over frames and columns, no vector tricks.  The owner rule is the CTC path's
(tests/long_form_ref.owners).

The error bound.  The kernel accumulates num = sum_k (a_k - b_k)^2 and den = sum_k a_k^2 + sum_k b_k^2 in fp32, u = 2^-24.
Every term is non-negative, so a sum's relative error is at most (the roundings on the longest path from a term to the result)
x u: a term of num carries the rounding of a - b twice (it is squared: 2u) and the fused multiply-add that adds it rounds once;
a term of den is exact until its fused multiply-add rounds.  With the D terms added in any order -- a chain, a tree, lanes then a
butterfly -- a path has at most D - 1 further additions (for den: 2D terms, but the kernel gives a lane at most 2 * ceil(D / 64)
of them and the butterfly adds 6, which stays below D + 3 for every D of these tests; adding a lane's exact 0 does not round), so
each sum is within (D + 3) u relatively, as the header says.  The quotient of two such sums is within
((D + 3) + (D + 3)) u + one rounding of the correctly rounded division <= 2 (D + 4) u relatively (second-order terms are
~D^2 u^2 < 1e-9 at D = 512: covered by the slack of 1 u that 2D + 7 <= 2D + 8 leaves times d <= 2).  d <= 2, hence
|d_fp32 - d_fp64| <= 4 (D + 4) 2^-24 absolutely; a score is a minimum of some s(j) = -d(j), and the minimum of values
each moved by at most e moves by at most e, so the same bound holds for every score, whichever frame gives it."""
import math

import numpy as np

from tests.long_form_ref import owners  # noqa: F401  (re-exported: the stitch's owner rule is the CTC path's)


def bound(D):
    """|d computed in fp32 - d| <= 4 (D + 4) 2^-24 (module docstring)."""
    return 4.0 * (D + 4) * 2.0 ** -24


def distance(a, b, D):
    num = den = 0.0
    for k in range(D):
        ak, bk = float(a[k]), float(b[k])
        num += (ak - bk) * (ak - bk)
        den += ak * ak + bk * bk
    return num / den if den > 0 else 0.0


def junction(x, counts, n, Hf, D, edge, guard):
    """Junction n of x [Nw][Tw][>= D] (any float dtype): (cut, score, ranked) with `ranked` the candidates' (score, c) best first
    under the rule's order (empty without candidates)."""
    lo = (n + 1) * Hf
    hi = min(n * Hf + counts[n], lo + counts[n + 1])
    if hi <= lo:
        return lo, 0.0, []
    s = {}
    for j in range(lo, hi):
        s[j] = -distance(x[n, j - n * Hf], x[n + 1, j - lo], D)

    def score(c):
        js = [j for j in range(c - guard, c + guard) if lo <= j < hi]
        if not js:
            return s[min(max(c, lo), hi - 1)]
        return min(s[j] for j in js)

    cands = list(range(lo + edge, hi - edge + 1))
    if not cands:
        c = (lo + hi) // 2
        return c, score(c), []
    ranked = sorted(((score(c), c) for c in cands), key=lambda sc: (-sc[0], abs(2 * sc[1] - (lo + hi)), sc[1]))
    return ranked[0][1], ranked[0][0], ranked


def cuts(x, counts, Hf, D, edge, guard):
    """(cuts [Nw - 1], scores [Nw - 1], margin): margin = the least lead, over the junctions, of the best score over the next
    lower score among the candidates (inf where all candidates score alike: those tie exactly in any precision, since they take
    their score from the same s(j), and the tie rule decides)."""
    cs, ss, margin = [], [], math.inf
    for n in range(len(counts) - 1):
        c, s, ranked = junction(x, counts, n, Hf, D, edge, guard)
        cs.append(c)
        ss.append(s)
        lower = [sc for sc, _ in ranked if sc < s]
        if lower:
            margin = min(margin, s - max(lower))
    return cs, ss, margin


def stitch_rows(x, counts, cut_list, Hf, D):
    """Rows [T][D] of the recording: the owner's row, as it is."""
    return np.stack([x[n, j, :D] for n, j in owners(counts, cut_list, Hf)])


# ------------------------------------------------------------------------------------------------ the cases of the GPU test
def windows_with_planted_agreement(rng, Nw, Tw, Hf, D, ld, last, plant):
    """x fp64 [Nw][Tw][ld] of a recording whose windows see a common signal plus window-own noise.  In the overlap of junction n
    the noise amplitude grows with the distance from frame lo + plant[n], where it is smallest: a clear best cut.  Columns >= D
    hold large values that must not be read; rows >= counts[n] are the caller's to poison."""
    counts = [Tw] * (Nw - 1) + [last]
    span = max(n * Hf + counts[n] for n in range(Nw))  # (a last window shorter than the overlap ends before its predecessor)
    common = rng.standard_normal((span, D))
    x = np.zeros((Nw, Tw, ld))
    x[:, :, D:] = 1e3
    for n in range(Nw):
        for j in range(counts[n]):
            t = n * Hf + j
            amp = 0.5
            for m in (n - 1, n):  # the junctions this window takes part in
                if 0 <= m < Nw - 1:
                    lo = (m + 1) * Hf
                    hi = min(m * Hf + counts[m], lo + counts[m + 1])
                    if lo <= t < hi:
                        amp = 0.02 + 0.1 * abs(t - (lo + plant[m]))
            x[n, j, :D] = common[t] + amp * rng.standard_normal(D)
    return x, counts


# (name, Nw, Tw, Of, D, ld, last window's frames, element offset of the base pointer, edge, guard)
GPU_CASES = [
    ("D64", 3, 24, 8, 64, 64, 24, 0, 1, 2),
    ("D20-scalar-tail", 3, 24, 8, 20, 20, 24, 0, 1, 2),
    ("D512", 2, 24, 8, 512, 512, 24, 0, 2, 2),
    ("ld>D-vector-tail", 3, 24, 8, 70, 72, 24, 0, 1, 2),
    ("ld-unaligned", 3, 24, 8, 64, 67, 24, 0, 1, 2),
    ("misaligned-base", 3, 24, 8, 64, 64, 24, 1, 1, 2),
    ("Of9", 3, 24, 9, 64, 64, 24, 0, 1, 1),
    ("Of1", 3, 8, 1, 64, 64, 8, 0, 0, 1),
    ("short-last", 3, 24, 8, 64, 64, 5, 0, 1, 1),
    ("no-candidate", 3, 24, 8, 64, 64, 24, 0, 5, 2),
    ("guard0", 3, 24, 8, 64, 64, 24, 0, 1, 0),
    ("five-windows", 5, 16, 5, 40, 40, 9, 0, 0, 1),
]


def gpu_case(case, dtype_name):
    """(x fp64 holding exactly the values the device will hold in `dtype_name`, counts, Hf, plant) of one case."""
    import torch

    name, Nw, Tw, Of, D, ld, last, offset, edge, guard = case
    Hf = Tw - Of
    rng = np.random.default_rng([GPU_CASES.index(case), int(dtype_name == "bf16")])
    plant = [int(rng.integers(0, max(1, min(Of, last if n == Nw - 2 else Of)))) for n in range(Nw - 1)]
    x, counts = windows_with_planted_agreement(rng, Nw, Tw, Hf, D, ld, last, plant)
    dt = torch.bfloat16 if dtype_name == "bf16" else torch.float32
    x = torch.from_numpy(x).to(dt).double().numpy()
    return x, counts, Hf, plant
