"""float64 reference of the long-form forced aligner (csrc/align_long.hip): the CTC Viterbi search of one sequence with the
header's rules -- lattice blank y1 blank ... yU blank, moves stay / +1 / +2 (+2 only into a label that differs from the one two
states earlier), ties stay over +1 over +2, end state S-1 over S-2, frame 0 admits states 0 and 1 -- and the per-frame log-prob
of the chosen label.  The search itself is `ctc_viterbi_oracle` of tests/test_forced_align.py (checked there, and again in
tests/test_long_align.py with frame_lp, against brute-force enumeration)."""
import numpy as np

from tests.test_forced_align import ctc_viterbi_oracle


def align(x, y, blank):
    """x: (T, V) float64 log-probs, y: the target ids.  Returns (frame_label [T], tok_start [U], tok_end [U], frame_lp [T], score,
    margin) with the fills of ea_ctc_viterbi_long_align: nothing aligned -> labels -2, spans -1, frame_lp 0."""
    y = [int(k) for k in y]
    T = x.shape[0]
    fl, ts, te, score, margin = ctc_viterbi_oracle(x, T, y, blank)
    if T == 0 or score == -np.inf:
        return np.full(T, -2), np.full(len(y), -1), np.full(len(y), -1), np.zeros(T), score, margin
    lab = np.where(fl >= 0, np.asarray(y + [blank])[fl], blank)  # (y + [blank]: index -1 of a blank frame stays in range)
    return fl, ts, te, x[np.arange(T), lab], score, margin


def quantised_lprobs(rng, T, V):
    """Multiples of 1/64 in [-16, 0]: every fp32 sum over up to 16 384 frames is exact, so fp32 and float64 agree to the bit and
    ties are frequent."""
    return rng.integers(-1024, 1, size=(T, V)).astype(np.float64) / 64.0


def targets_with_repeats(rng, U, V, blank, p_repeat=0.15):
    """U ids in [0, V) without blank; a token repeats its predecessor with probability p_repeat."""
    ids = [k for k in range(V) if k != blank]
    y = rng.choice(ids, size=U) if U else np.zeros(0, dtype=np.int64)
    rep = rng.random(U) < p_repeat
    for u in range(1, U):
        if rep[u]:
            y[u] = y[u - 1]
    return y.astype(np.int32)
