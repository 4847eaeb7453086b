"""A numpy restatement of the keyword-spotting rule of include/espresso_amd.h ("Keyword spotting on CTC log-probs"), written
from that text and not from csrc/kws.hip: the frame update over the 2L - 1 states tok_1, blk_1, ..., tok_L, the detection with
its open hit, `hold` and `last_end`, and the emit.  The dtype is a parameter (np.float32: the bits the library must give;
np.float64: the yardstick of the fp32 rounding).  `KwsRef.counters` counts the rare branches, so a test can assert that its
cases reach them."""
import math

import numpy as np

COUNTERS = ("replaced", "dropped", "emit_hold", "emit_candidate", "overflow")


def tau_of(theta, L):
    """tau = L * ln(theta), in fp32 as the callers of the library compute it."""
    return np.float32(L) * np.float32(math.log(theta))


class KwsRef:
    """One (stream, keyword) pair.  `feed` takes frames [n][>= V] (any pieces), `flush` ends the audio; `hits` is the list of
    (start, end, e) that fit into max_hits, `count` counts every emit."""

    def __init__(self, tokens, tau, V, blank, hold, max_hits, dtype=np.float32, counters=None):
        self.y = [int(v) for v in tokens]
        self.L = len(self.y)
        self.active = self.L >= 1 and all(0 <= v < V and v != blank for v in self.y)
        self.V, self.blank, self.hold, self.max_hits, self.dtype = V, blank, int(hold), int(max_hits), dtype
        self.tau = dtype(tau)
        S = max(2 * self.L - 1, 0)
        self.e = [dtype(-np.inf)] * S
        self.b = [-1] * S
        self.t = 0
        self.open = None  # (start, end, e)
        self.last_end = -1
        self.hits, self.count = [], 0
        self.counters = counters if counters is not None else dict.fromkeys(COUNTERS, 0)

    def label(self, s):
        return self.y[s // 2] if s % 2 == 0 else self.blank

    def _emit(self):
        if self.count < self.max_hits:
            self.hits.append(self.open)
        else:
            self.counters["overflow"] += 1
        self.count += 1
        self.last_end = self.open[1]
        self.open = None

    def _frame(self, row):
        dtype, t = self.dtype, self.t
        g = dtype(np.max(row[: self.V]))
        ninf = dtype(-np.inf)
        e_old, b_old = self.e, self.b
        e_new, b_new = list(e_old), list(b_old)
        for s in range(len(e_old)):
            cands = [(e_old[s], b_old[s])]  # stay
            if s >= 1:
                cands.append((e_old[s - 1], b_old[s - 1]))  # step
            if s >= 2 and s % 2 == 0 and self.y[s // 2] != self.y[s // 2 - 1]:
                cands.append((e_old[s - 2], b_old[s - 2]))  # skip
            if s == 0:
                cands.append((dtype(0), t))  # a fresh start
            ce, cb = cands[0]
            for e, b in cands[1:]:
                if e > ce:  # the first of the largest
                    ce, cb = e, b
            if ce == ninf:
                e_new[s], b_new[s] = ninf, -1
            else:
                d = dtype(dtype(row[self.label(s)]) - g)
                e_new[s], b_new[s] = dtype(ce + d), cb
        self.e, self.b = e_new, b_new
        # detection
        e, b = e_new[-1], b_new[-1]
        if e >= self.tau:
            if b > self.last_end:
                cand = (b, t, e)
                if self.open is None:
                    self.open = cand
                elif b <= self.open[1]:
                    if e >= self.open[2]:
                        self.open = cand
                        self.counters["replaced"] += 1
                else:
                    self.counters["emit_candidate"] += 1
                    self._emit()
                    self.open = cand
            else:
                self.counters["dropped"] += 1
        if self.open is not None and t - self.open[1] > self.hold:
            self.counters["emit_hold"] += 1
            self._emit()
        self.t += 1

    def feed(self, rows):
        rows = np.asarray(rows)
        if not self.active:
            self.t += len(rows)
            return
        with np.errstate(invalid="ignore"):
            for row in rows:
                self._frame(row.astype(self.dtype))

    def flush(self):
        if self.open is not None:
            self._emit()

    def poll(self):
        """The hits emitted since the last poll (the lists are emptied, as `clear` does)."""
        out, n = self.hits, self.count
        self.hits, self.count = [], 0
        return out, n


def spot(x, keywords, taus, V, blank, hold, max_hits, dtype=np.float32, counters=None):
    """Offline: per keyword (hits [(start, end, e)], count) over the utterance x [T][>= V], flushed at the end."""
    out = []
    for y, tau in zip(keywords, taus):
        r = KwsRef(y, tau, V, blank, hold, max_hits, dtype, counters)
        r.feed(x)
        r.flush()
        out.append((r.hits, r.count))
    return out


def as_arrays(results, max_hits):
    """The lists of `spot` in the layout of ea_ctc_kws_hits: starts / ends int32 [K][max_hits] (-1 past the list), scores fp32
    (0 past the list), counts int32 [K]."""
    K = len(results)
    starts = np.full((K, max_hits), -1, dtype=np.int32)
    ends = np.full((K, max_hits), -1, dtype=np.int32)
    scores = np.zeros((K, max_hits), dtype=np.float32)
    counts = np.zeros(K, dtype=np.int32)
    for k, (hits, n) in enumerate(results):
        counts[k] = n
        for h, (s, e, sc) in enumerate(hits):
            starts[k, h], ends[k, h], scores[k, h] = s, e, sc
    return starts, ends, scores, counts
