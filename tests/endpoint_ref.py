"""Float64 oracle of endpointing in the streamed CTC prefix and transducer frame beam searches (DESIGN.md section 3.4,
"Endpointing"), built on the time-stamp oracles of tests/beam_times_ref.py, which are imported, not restated.

An endpoint oracle follows ONE segment of one stream: it is fed the segment's frames in pieces and `probe` reports, for the live
hypothesis `partial` defines as best (the best in-beam score, ties to the lower slot), its tokens, the frame E at which its last
token starts on its best alignment path (-1 without tokens) and the lead of its in-beam score over the second.  `endpoint_rule`
restates the rule table; `simulate` plays a set of streams, cut into given pieces, through one decoder with a given number of
slot frames and writes down everything a test then holds the device to: every probe, every segment end with its reason
(1 silence, 2 empty, 3 length, 4 room, 0 the end of the audio) and the frames of every segment."""
import math

from tests.beam_times_ref import PrefixBeamTimesOracle, frame_beam_times_oracle
from tests.test_ctc_prefix_beam import _lae
from tests.transducer_hotword_ref import biased_beam

ROOM, FINAL = 4, 0


def endpoint_rule(F, L, E, silence, empty, segment):
    """The rule table: trailing = the frames since the last token's (all of them without a token); thresholds <= 0 are off."""
    trailing = F - 1 - E if L > 0 else F
    if L > 0 and silence > 0 and trailing >= silence:
        return 1
    if L == 0 and empty > 0 and F >= empty:
        return 2
    if segment > 0 and F >= segment:
        return 3
    return 0


class CtcEndpointOracle:
    """PrefixBeamTimesOracle over the frames of one segment; rows(lo, hi) gives the segment's log-prob rows [hi - lo][V]."""

    def __init__(self, rows, beam, K, blank, **kw):
        self.rows, self.o = rows, PrefixBeamTimesOracle(beam, K, blank, **kw)

    @property
    def frames(self):
        return self.o.frames

    def feed(self, n):
        if n > 0:
            self.o.feed(self.rows(self.o.frames, self.o.frames + n))

    def probe(self):
        """(tokens of the best live hypothesis, E, its lead over the second in-beam score)."""
        o = self.o
        sc = [_lae(pb, pnb) + o.lw * lm + o.bonus * len(y) for y, pb, pnb, lm, _, _ in o.hyps]
        j = min(range(len(sc)), key=lambda i: (-sc[i], i))
        y, _, _, _, B, NB = o.hyps[j]
        best = o.larger(B, NB)  # the larger Viterbi score, ties to the blank one; the gap goes into o.vgap
        rest = sorted(sc, reverse=True)
        return y, (best[1][-1] if y else -1), (rest[0] - rest[1] if len(rest) > 1 else math.inf)

    def margins(self):
        """(pruning margin, Viterbi gap) of the decisions so far."""
        return self.o.margin, self.o.vgap

    def finish(self, nbest):
        return self.o.finish(nbest)[0]


class TransducerEndpointOracle:
    """frame_beam_times_oracle over the first F frames of one segment, from scratch at every probe; logits_fn(t, y) is the
    segment's (t counts from its first frame).  With a graph the in-beam ranking is s + b (tests.transducer_hotword_ref)."""

    def __init__(self, logits_fn, beam, K, blank, graph=None, **kw):
        self.fn, self.beam, self.K, self.blank, self.graph, self.kw = logits_fn, beam, K, blank, graph, kw
        self.frames = 0
        self._margin = self._vgap = math.inf

    def feed(self, n):
        self.frames += n

    def _search(self, nbest):
        fin, _, _, vgap, pmargin = frame_beam_times_oracle(self.fn, self.frames, self.beam, self.K, self.blank, graph=self.graph,
                                                           normalize=False, nbest=nbest, **self.kw)
        return fin, vgap, pmargin

    def probe(self):
        fin, vgap, _ = self._search(self.beam)
        # pmargin with nbest = beam would also hold the whole final ranking apart; what decides which hypotheses exist is taken
        # with nbest = 1 below, and the lead of the best one is returned
        self._vgap = min(self._vgap, vgap)
        self._margin = min(self._margin, self._search(1)[2] if self.frames else math.inf)
        if self.graph is None:  # final = s: the finish order is the in-beam order
            sc = [(s, y) for y, s, _, _ in fin]
        else:
            live = {y: s + b for y, s, _, b in biased_beam(self.fn, self.frames, self.beam, self.K, self.blank, self.graph, **self.kw)[0]}
            sc = sorted(((live[y], y) for y, _, _, _ in fin), key=lambda e: -e[0])
        times = {y: t for y, _, t, _ in fin}
        y = sc[0][1]
        return y, (times[y][-1] if y else -1), (sc[0][0] - sc[1][0] if len(sc) > 1 else math.inf)

    def margins(self):
        return self._margin, self._vgap

    def finish(self, nbest, normalize=True):
        return frame_beam_times_oracle(self.fn, self.frames, self.beam, self.K, self.blank, graph=self.graph, normalize=normalize,
                                       nbest=nbest, **self.kw)[0]


def simulate(streams, rules, max_frames, make_oracle):
    """streams: [(sid, frames, pieces, after)]: the stream's length, the sizes of its pieces (cycled; the last one cut at the
    end) and the stream whose close it is opened after (None: at the start).  rules: (silence, empty, segment) frames.
    make_oracle(sid, start): the endpoint oracle of the segment of `sid` that begins at its frame `start`.

    Every round gives each open stream its next piece in one accept; before it the streams whose piece would pass max_frames
    end their segment (room); after it every stream is probed and those with a rule end theirs, except a stream whose audio is
    over, which is closed.  Returns (rounds, segments, margins):
      rounds: [dict(open=[sid], room=[sid], accept=[(sid, lo, hi)], probes={sid: (rule, F, L, E, tokens)}, ends=[(sid, rule)],
                    close=[sid])]
      segments: {sid: [(first frame, frames, reason, oracle)]} in order
      margins: (the smallest lead of a best hypothesis at a probe, pruning margin, Viterbi gap) over everything."""
    length = {sid: n for sid, n, _, _ in streams}
    pieces = {sid: list(p) for sid, _, p, _ in streams}
    waiting = [(sid, after) for sid, _, _, after in streams]
    pos, turn, seg, oracle, segments = {}, {}, {}, {}, {sid: [] for sid in length}
    lead = margin = vgap = math.inf
    rounds, closed = [], set()

    def end(sid, reason):
        nonlocal margin, vgap
        o = oracle[sid]
        m, g = o.margins()
        margin, vgap = min(margin, m), min(vgap, g)
        segments[sid].append((seg[sid], o.frames, reason, o))
        seg[sid] += o.frames
        oracle[sid] = make_oracle(sid, seg[sid])

    while waiting or pos:
        r = dict(open=[], room=[], accept=[], probes={}, ends=[], close=[])
        for sid, after in list(waiting):
            if after is None or after in closed:
                waiting.remove((sid, after))
                pos[sid], turn[sid], seg[sid] = 0, 0, 0
                oracle[sid] = make_oracle(sid, 0)
                r["open"].append(sid)
        for sid in pos:
            c = min(pieces[sid][turn[sid] % len(pieces[sid])], length[sid] - pos[sid])
            turn[sid] += 1
            if oracle[sid].frames > 0 and oracle[sid].frames + c > max_frames:
                end(sid, ROOM)
                r["room"].append(sid)
            r["accept"].append((sid, pos[sid], pos[sid] + c))
            oracle[sid].feed(c)
            pos[sid] += c
        for sid in list(pos):
            y, E, ld = oracle[sid].probe()
            F = oracle[sid].frames
            rule = endpoint_rule(F, len(y), E, *rules)
            r["probes"][sid] = (rule, F, len(y), E, y)
            lead = min(lead, ld)
            if pos[sid] >= length[sid]:
                end(sid, FINAL)
                r["close"].append(sid)
                closed.add(sid)
                del pos[sid]
            elif rule:
                end(sid, rule)
                r["ends"].append((sid, rule))
        rounds.append(r)
    return rounds, segments, (lead, margin, vgap)
