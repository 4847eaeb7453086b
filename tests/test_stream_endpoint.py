"""Endpointing of the streamed CTC prefix and transducer frame beam searches (ea_ctc_prefix_beam_stream_endpoint /
ea_rnnt_frame_beam_stream_endpoint; `endpoint=EndpointRules(...)` of the two streamed decoders; `speech_recognize
--stream-endpoint`).

tests/endpoint_ref.py states the contract in float64 on top of the time-stamp oracles.  The CPU tests hold the rule table, the
oracle's E (to brute force over every alignment), `StreamSlots.restart`, the segment joining of `recognize_streaming` (with a
fake encoder and a fake decoder) and the refusals of the command line.  The GPU tests play four streams of 60 / 37 / 25 / 12
frames, cut into uneven pieces of 0 - 7 frames, through three slots of 24 frames under the rules (6, 10, 20): after every accept
the device's (rule, F, L, E) equals the oracle's exactly, agrees with `partial` and with the times of `finish`, and every
segment is torch.equal to the offline search with token_times over that segment's frames alone.

Inputs.  Rows as tests.test_ctc_prefix_beam._peaked (CTC) and the TableModel (transducer), with the blank logit raised by 12 (CTC) / 30
(transducer) where a stream pauses and lowered by 6 where it must not (a peak falls on blank half of the time, which would otherwise leave
pauses of six frames by chance): stream 0 talks for 25 frames, pauses for 11 and talks again, stream 1 has no pause, stream 2 is
silence only, and stream 3 is opened when stream 2 has closed and takes over its slot.

Conditions.  E, L and the rule are compared exactly, which needs the lead of the best hypothesis at every probe, every pruning
margin and every gap a Viterbi max rested on clear of the fp32 error: each case's seed is the first from 0 for which all three
exceed twice the bound tests/test_beam_time_stamps.py uses (CTC: SCORE_TOL, plus LM_TOL per LM term with the LSTM LM; transducer:
SCORE_TOL + 8 * TERM_TOL * terms for the 24 frames and as many bias terms of a segment), and every test asserts that before it
compares.  The LSTM-LM case fuses with weight 0.1: a score carries up to 25 LM terms of LM_TOL x the weight each, and at the
weight 0.4 of tests/test_beam_time_stamps.py no seed below 600 keeps 134 frames of decisions twice that bound apart; the
comparison of every segment with the offline decoder is bit for bit whatever the weight.  Every case must end segments for each of silence, empty, length and room: asserted on the oracle's output."""
import functools
import io
import math

import numpy as np
import pytest
import torch

from tests.beam_times_ref import ctc_best_alignments, transducer_best_alignments
from tests.endpoint_ref import FINAL, ROOM, CtcEndpointOracle, TransducerEndpointOracle, endpoint_rule, simulate
from tests.hotword_ref import bias_lm_fn, grid_phrases
from tests.test_ctc_prefix_beam import LM_TOL, SCORE_TOL, _cpu_lm_fn, _dictionary, _peaked, _tiny_lm
from tests.test_transducer_frame_beam import BLANK, TERM_TOL
from tests.transducer_frame_beam_ref import TableLM, TableModel, frame_beam_oracle

DEV = "cuda:0"
PAD = 1
V = 20
RULES = (6, 10, 20)
MAX_FRAMES, MAX_STREAMS = 24, 3
# (frames, pieces, opened after the close of): a 0-frame piece in every stream; stream 0 reaches 18 frames and is then given 7
# (room); stream 1's third piece ends exactly on the length threshold (20) and stream 2's third on the empty threshold (10)
STREAMS = [(0, 60, [5, 0, 7, 6, 7, 3, 3, 4, 7, 2, 6, 1, 5], None), (1, 37, [7, 7, 6, 1, 0, 4, 7, 5, 3], None),
           (2, 25, [2, 3, 5, 0, 7, 4, 4], None), (3, 12, [3, 0, 4, 5], 2)]
LENGTH = {sid: n for sid, n, _, _ in STREAMS}
PAUSE = {0: range(25, 36), 1: range(0), 2: range(25), 3: range(0)}  # the frames with the blank logit raised; lowered elsewhere
UP, DOWN = {"ctc": 12.0, "transducer": 30.0}, -6.0  # (the TableModel's noise and peak are larger than _peaked's)
LM_WEIGHT, BONUS = 0.1, 0.2  # (every LM term of a score may be off by LM_TOL x the weight: see _ctc_need)


def _shift(search, sid, t):
    return UP[search] if t in PAUSE[sid] else DOWN


def _graph(phrases):
    from espresso_amd.tools.context_graph import ContextGraph

    return ContextGraph(phrases, V)


# =============================================================================================================== CPU: the rule
def test_rule_restatement():
    """EndpointRules.decide against the table: every rule, the order 1 < 2 < 3, thresholds <= 0 switched off."""
    from espresso_amd.tools.beam_common import EndpointRules

    r = EndpointRules(6, 10, 20)
    table = [((0, 0, -1), 0), ((9, 0, -1), 0), ((10, 0, -1), 2), ((19, 0, -1), 2), ((20, 0, -1), 2), ((25, 0, -1), 2),  # empty before length
             ((6, 1, 0), 0), ((7, 1, 0), 1), ((7, 3, 1), 0), ((7, 3, 0), 1), ((12, 2, 6), 0), ((13, 2, 6), 1),  # trailing = F - 1 - E
             ((20, 5, 19), 3), ((20, 5, 14), 3), ((20, 5, 13), 1), ((24, 9, 23), 3), ((19, 5, 18), 0), ((1, 1, 0), 0)]
    for (F, L, E), want in table:
        assert r.decide(F, L, E) == want == endpoint_rule(F, L, E, 6, 10, 20), (F, L, E)
    assert (r.SILENCE, r.EMPTY, r.LENGTH, r.ROOM) == (1, 2, 3, 4) and r.NAMES[1:] == ("silence", "empty", "length", "room")
    assert r.frames() == (6, 10, 20)
    off = EndpointRules(0, -1, 0)
    assert [off.decide(F, L, E) for F, L, E in ((100, 0, -1), (100, 3, 2), (100, 3, 99))] == [0, 0, 0]
    assert EndpointRules(0, 0, 20).decide(50, 0, -1) == 3 and EndpointRules(0, 0, 20).decide(50, 2, 1) == 3
    assert EndpointRules(6, 0, 0).decide(50, 0, -1) == 0 and EndpointRules(0, 10, 0).decide(50, 2, 1) == 0
    rng = np.random.default_rng(0)
    for _ in range(500):
        s, e, g = (int(v) for v in rng.integers(-2, 12, 3))
        F = int(rng.integers(0, 30))
        L = int(rng.integers(0, 3)) if F else 0
        E = int(rng.integers(0, F)) if L else -1
        assert EndpointRules(s, e, g).decide(F, L, E) == endpoint_rule(F, L, E, s, e, g), (s, e, g, F, L, E)


# =============================================================================================================== CPU: the oracle
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("T_", [1, 3, 5])
def test_ctc_oracle_E_against_brute_force(seed, T_):
    """V 3, beam 64, K 2 (no pruning): fed in pieces, E of the best live hypothesis is the last start frame of its best
    alignment among all 3^T frame labellings, after every piece."""
    x = np.random.default_rng(seed).standard_normal((T_, 3)) * 1.5
    x -= np.logaddexp.reduce(x, axis=1, keepdims=True)
    o = CtcEndpointOracle(lambda lo, hi: x[lo:hi], 64, 2, 0)
    assert o.probe() == ((), -1, math.inf)
    for n in (1, 0, 2, 2):
        o.feed(min(n, T_ - o.frames))
        y, E, lead = o.probe()
        if o.frames == 0:
            continue
        brute = ctc_best_alignments(x[: o.frames], 0)
        assert y in brute and lead > 1e-9 and brute[y][2] > 1e-9  # the best hypothesis and its best alignment are unique
        assert E == (brute[y][1][-1] if y else -1), (y, E, brute[y])
    assert o.frames == T_


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("T_", [1, 3, 5])
def test_transducer_oracle_E_against_brute_force(seed, T_, with_lm):
    table = TableModel(3, seed, blank=BLANK, sharp=1.0)
    kw = dict(lm_fn=TableLM(3, seed + 50), lm_weight=0.7) if with_lm else {}
    o = TransducerEndpointOracle(table.logits_fn(0), 10 ** 6, 2, BLANK, **kw)
    assert o.probe()[:2] == ((), -1)
    for n in (1, 2, 2):
        o.feed(min(n, T_ - o.frames))
        y, E, lead = o.probe()
        brute = transducer_best_alignments(table.logits_fn(0), o.frames, 3, BLANK, kw.get("lm_fn"), kw.get("lm_weight", 0.0))
        assert lead > 1e-9 and brute[y][2] > 1e-9
        assert E == (brute[y][1][-1] if y else -1), (y, E, brute[y])


# =============================================================================================================== CPU: the slots
def test_stream_slots_restart():
    from espresso_amd.tools.beam_common import StreamSlots

    s = StreamSlots("test", 3, 24)
    s.open(["a", "b"])
    s._unreset = []
    s.streams["a"][1], s.streams["b"][1] = 17, 9
    slot_a, slot_b = s.streams["a"][0], s.streams["b"][0]
    assert s.room(["a", "b"], [7, 7]) == [] and s.room(["a", "b"], [8, 16]) == ["a", "b"] and s.room(["b", "a"], [0, 8]) == ["a"]
    s.restart("a")
    assert s.streams["a"] == [slot_a, 0] and s.streams["b"] == [slot_b, 9] and s._unreset == [slot_a]
    s.restart("a")
    assert s._unreset == [slot_a]  # listed once
    assert s.room(["a"], [24]) == [] and s.room(["a"], [25]) == []  # nothing to end: the accept itself refuses such a piece
    with pytest.raises(ValueError, match="max_frames"):
        s._check_room(["a"], [25])
    s.open(["c"])
    assert s.streams["c"][0] not in (slot_a, slot_b) and len(s._free) == 0
    with pytest.raises(ValueError, match="endpoint"):
        s.endpoint_tensors = None
        s.end_segment("b")
    with pytest.raises(KeyError):
        s.restart("nobody")


def test_decoders_take_endpoint_rules_and_keep_their_state_size():
    """`endpoint` forces the times family on; state_bytes_per_stream() is that of (max_frames, beam) with and without it."""
    from espresso_amd import _lib
    from espresso_amd.tools.beam_common import EndpointRules
    from espresso_amd.tools.streaming_ctc_prefix_beam_decoder import StreamingCTCPrefixBeamDecoder
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder

    d = _dictionary(8)
    rules = EndpointRules(*RULES)
    on, off = StreamingCTCPrefixBeamDecoder(d, 3, 24, beam_size=4, endpoint=rules), StreamingCTCPrefixBeamDecoder(d, 3, 24, beam_size=4)
    assert on.token_times is True and off.token_times is False and on.endpoint_rules is rules and off.endpoint_rules is None
    ton = StreamingTransducerFrameBeamDecoder(None, d, 4, max_streams=3, max_frames=24, endpoint=rules)
    toff = StreamingTransducerFrameBeamDecoder(None, d, 4, max_streams=3, max_frames=24)
    assert ton.token_times is True and toff.token_times is False and ton.endpoint_rules is rules
    for dec in (off, toff):
        dec.open(["u"])
        with pytest.raises(ValueError, match="endpoint"):
            dec.endpoint(["u"])
        with pytest.raises(ValueError, match="endpoint"):
            dec.end_segment("u")
    try:
        lib = _lib.lib()
    except _lib.EspressoAmdLibraryError:
        pytest.skip("the library is not built")
    assert on.state_bytes_per_stream() == off.state_bytes_per_stream() == lib.ea_ctc_prefix_beam_stream_state_bytes(24, 4)
    assert ton.state_bytes_per_stream() == toff.state_bytes_per_stream() == lib.ea_rnnt_frame_beam_stream_state_bytes(24, 4)
    header = _lib.parse_header()
    assert "ea_ctc_prefix_beam_stream_endpoint" in header and "ea_rnnt_frame_beam_stream_endpoint" in header


# =============================================================================================================== CPU: recognize_streaming
class _FakeFrontend:
    frame_shift, sample_rate = 160, 16000

    @staticmethod
    def num_frames(n):
        return n // 160


class _FakeEncoder:
    """One "encoder frame" per 160 samples, whose single column is the sample value: the token the frame says (0: silence).
    `announce`: what max_rows_per_accept answers (an honest 4 for pieces of 640 samples)."""

    stride, announce = 1, 4

    def __init__(self, model, streams, frontend=None):
        self.open_ids = []

    def open(self, ids):
        self.open_ids += ids

    def close(self, ids):
        for i in ids:
            self.open_ids.remove(i)

    def max_rows_per_accept(self, n_samples):
        assert n_samples == 640
        return self.announce

    def accept_waveform(self, ids, pieces, final):
        counts = [int(p.numel()) // 160 for p in pieces]
        rows = torch.cat([p[: c * 160: 160] for p, c in zip(pieces, counts)])[:, None]
        return (rows if rows.numel() else None), counts


class _FakeDecoder:
    """The endpointed decoder interface over the fake frames: a frame whose value differs from the one before and is not 0 emits
    that value as a token at that frame.  Keeps a log of its calls; `accept` refuses what does not fit, as the real ones do."""

    made = []

    def __init__(self, dictionary, max_streams, max_frames, endpoint=None, **opts):
        self.max_frames, self.rules, self.opts = max_frames, endpoint, opts
        self.frames, self.log = {}, []
        _FakeDecoder.made.append(self)

    def open(self, ids):
        for i in ids:
            self.frames[i] = []

    def accept(self, ids, rows, counts):
        r = 0
        for i, c in zip(ids, counts):
            if len(self.frames[i]) + c > self.max_frames:
                raise ValueError(f"stream {i}: exceeds max_frames {self.max_frames}")
            self.frames[i] += [int(v) for v in rows[r:r + c, 0].tolist()]
            r += c
        self.log.append(("accept", tuple(ids), tuple(counts)))

    def _hyp(self, i):
        f = self.frames[i]
        emit = [(v, t) for t, v in enumerate(f) if v != 0 and (t == 0 or f[t - 1] != v)]
        return {"tokens": torch.tensor([v for v, _ in emit], dtype=torch.long), "score": torch.tensor(-float(len(f))),
                "attention": None, "alignment": None, "times": torch.tensor([t for _, t in emit], dtype=torch.long),
                "viterbi_score": torch.tensor(-2.0 * len(f))}

    def room(self, ids, counts):
        return [i for i, c in zip(ids, counts) if self.frames[i] and len(self.frames[i]) + c > self.max_frames]

    def endpoint(self, ids):
        out = []
        for i in ids:
            h = self._hyp(i)
            F, L = len(self.frames[i]), len(h["tokens"])
            E = int(h["times"][-1]) if L else -1
            out.append((self.rules.decide(F, L, E), F, L, E))
        self.log.append(("endpoint", tuple(ids)))
        return out

    def end_segment(self, i):
        h = self._hyp(i)
        self.log.append(("end_segment", i, len(self.frames[i])))
        self.frames[i] = []
        return [h]

    def partial(self, ids):
        res = []
        for i in ids:
            toks = self._hyp(i)["tokens"].tolist()
            res.append({"tokens": toks, "stable": toks[: max(0, len(toks) - 1)], "score": 0.0})
        return res

    def close(self, i):
        h = self._hyp(i)
        self.log.append(("close", i, len(self.frames.pop(i))))
        return [h]


class _FakeTask:
    frontend = _FakeFrontend()


def _wave(frames):
    return np.repeat(np.asarray(frames, dtype=np.float32), 160)


def _run_fake(monkeypatch, waves, rules, announce=4, partials=False, **kw):
    from espresso_amd import speech_recognize as sr
    from espresso_amd.models.transformer import streaming_encoder
    from espresso_amd.tools import streaming_ctc_prefix_beam_decoder as mod

    monkeypatch.setattr(streaming_encoder, "StreamingEncoder", _FakeEncoder)
    monkeypatch.setattr(mod, "StreamingCTCPrefixBeamDecoder", _FakeDecoder)
    monkeypatch.setattr(_FakeEncoder, "announce", announce)
    _FakeDecoder.made.clear()
    d = _dictionary(8)
    out, ctm = io.StringIO(), {}
    utts = [f"u{i}" for i in range(len(waves))]
    sr.recognize_streaming(_FakeTask(), None, d, utts, waves, "cpu", chunk_ms=40, streams=2, out=out, search="ctc_stream_beam",
                           ctc_stream_beam=dict(beam_size=4, nbest=1), ctm_hyps=ctm, endpoint=rules, partials=partials, **kw)
    return d, out.getvalue().splitlines(), ctm, _FakeDecoder.made[-1]


def test_recognize_streaming_joins_the_segments(monkeypatch):
    """Rules (3, 5, 8) frames, pieces of 4 frames: silence, empty and length ends, the joined H- line, times shifted by each
    segment's first frame, the S- lines in seconds and the stable text of the P- lines."""
    from espresso_amd.tools.beam_common import EndpointRules

    a, b, c = 4, 5, 6  # token ids (t0, t1, t2 of the dictionary)
    #            0  1  2  3 | 4  5  6  7 | 8  9  10 11 | 12 13 14 15 | 16 17 18 19 | 20 21 22 23 | 24 25 26 27 | 28 29
    u0 = _wave([a, b, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, c, a, b, c, a, b, c, a, b, c, a, 0, 0, 0, b, b])
    u1 = _wave([c, c, 0, 0, a])
    d, lines, ctm, dec = _run_fake(monkeypatch, [u0, u1], EndpointRules(3, 5, 8), partials=True)
    assert dec.max_frames == 8 + 4 and dec.rules.frames() == (3, 5, 8) and dec.opts == dict(beam_size=4, nbest=1)
    s0 = [ln.split("\t") for ln in lines if ln.startswith("S-u0\t")]
    # frames 0-8: "t0 t1", trailing 6 >= 3 at F = 8 (a piece boundary; at F = 4 it is 2); 8-16: two tokens at 14, 15: trailing 0, F = 8:
    # length; 16-24: length again; 24-28: t0 at 24, trailing 3: silence; 28-30: the audio's end
    assert s0 == [["S-u0", "0.00", "0.08", "silence", "t0 t1"], ["S-u0", "0.08", "0.16", "length", "t2 t0"],
                  ["S-u0", "0.16", "0.24", "length", "t1 t2 t0 t1 t2 t0 t1 t2"], ["S-u0", "0.24", "0.28", "silence", "t0"],
                  ["S-u0", "0.28", "0.30", "final", "t1"]]
    assert [ln.split("\t") for ln in lines if ln.startswith("S-u1\t")] == [
        ["S-u1", "0.00", "0.04", "silence", "t2"], ["S-u1", "0.04", "0.05", "final", "t0"]]  # t2 at frame 0: trailing 3 at F = 4
    h0 = next(ln.split("\t") for ln in lines if ln.startswith("H-u0\t"))
    assert h0[1] == " ".join(s[4] for s in s0) and float(h0[2]) == pytest.approx(-30.0 / math.log(2))  # the scores summed
    hyp, strip = ctm["u0"]
    assert hyp["tokens"].tolist() == [a, b, c, a, b, c, a, b, c, a, b, c, a, b] and float(hyp["score"]) == -30.0
    assert hyp["times"].tolist() == [0, 1, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 28] and float(hyp["viterbi_score"]) == -60.0
    assert ctm["u1"][0]["times"].tolist() == [0, 4] and float(ctm["u1"][0]["score"]) == -5.0
    # P- lines: the closed segments' text leads the stable field
    p0 = [ln.split("\t") for ln in lines if ln.startswith("P-u0\t")]
    assert p0[0] == ["P-u0", "0.04", "t0", "t1"] and ["P-u0", "0.08", "t0 t1", ""] in p0
    assert ["P-u0", "0.16", "t0 t1 t2 t0", ""] in p0 and p0[-1][2].startswith("t0 t1 t2 t0 t1 t2 t0 t1 t2 t0 t1 t2 t0")
    # one endpoint readback after every accept
    kinds = [e[0] for e in dec.log]
    assert all(kinds[k + 1] == "endpoint" for k, e in enumerate(kinds) if e == "accept") and kinds.count("accept") == kinds.count("endpoint")


def test_recognize_streaming_ends_a_segment_for_room_before_the_accept(monkeypatch):
    """An encoder that brings more frames than it announced (4 per accept against 1): with the segment limit of 10 frames the
    slots hold 11, and the stream at 8 frames ends its segment ("room") before the accept of 4 more, which the decoder would
    refuse.  (With an honest encoder "length" always comes first: room is the safeguard.)"""
    from espresso_amd.tools.beam_common import EndpointRules

    a, b = 4, 5
    u0 = _wave([a, b, a, b, a, b, a, 0, 0, b, a, b, a])
    d, lines, ctm, dec = _run_fake(monkeypatch, [u0], EndpointRules(0, 0, 10), announce=1)
    assert dec.max_frames == 11
    k = dec.log.index(("end_segment", 0, 8))
    assert dec.log[k - 1][0] == "endpoint" and dec.log[k + 1] == ("accept", (0,), (4,))  # ended before the accept that would not fit
    s0 = [ln.split("\t") for ln in lines if ln.startswith("S-u0\t")]
    assert [s[3] for s in s0] == ["room", "final"] and [s[1:3] for s in s0] == [["0.00", "0.08"], ["0.08", "0.13"]]
    assert ctm["u0"][0]["times"].tolist() == [0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12]


def test_slot_size_under_endpointing_does_not_depend_on_the_audio(monkeypatch):
    from espresso_amd.tools.beam_common import EndpointRules

    sizes = set()
    for n in (5, 40, 400):
        _, _, _, dec = _run_fake(monkeypatch, [_wave([5] * n)], EndpointRules(3, 5, 8))
        sizes.add(dec.max_frames)
    assert sizes == {12}
    _, _, _, dec = _run_fake(monkeypatch, [_wave([5] * 40)], None)  # without endpointing: the longest utterance
    assert dec.max_frames == 40 and dec.rules is None


def test_recognize_streaming_refuses_endpointing_elsewhere(monkeypatch):
    from espresso_amd import speech_recognize as sr
    from espresso_amd.models.transformer import streaming_encoder
    from espresso_amd.tools.beam_common import EndpointRules

    monkeypatch.setattr(streaming_encoder, "StreamingEncoder", _FakeEncoder)
    d = _dictionary(8)
    with pytest.raises(NotImplementedError, match="stream-endpoint"):
        sr.recognize_streaming(_FakeTask(), None, d, ["u"], [_wave([5])], "cpu", search="ctc", endpoint=EndpointRules(3, 5, 8))
    with pytest.raises(NotImplementedError, match="nbest"):
        sr.recognize_streaming(_FakeTask(), None, d, ["u"], [_wave([5])], "cpu", search="ctc_stream_beam",
                               ctc_stream_beam=dict(nbest=2), endpoint=EndpointRules(3, 5, 8))


# =============================================================================================================== CPU: the command line
_MISSING = ["--path", "/nonexistent.pt", "--dict", "/nonexistent.txt", "--wav-scp", "/nonexistent.scp"]


def test_cli_options_and_refusals():
    """Every refusal is raised by name before /nonexistent.pt is opened; the accepted forms fail on the missing files."""
    from espresso_amd import speech_recognize as sr

    a = sr.get_parser().parse_args(_MISSING)
    assert (a.stream_endpoint, a.endpoint_silence_s, a.endpoint_empty_s, a.endpoint_max_segment_s) == (False, 0.8, 5.0, 20.0)
    for extra in ([], ["--search", "ctc"], ["--search", "ctc_beam"], ["--search", "transducer_frame_beam"]):
        with pytest.raises(ValueError, match="--stream-endpoint configures --streaming"):
            sr.main(_MISSING + ["--stream-endpoint"] + extra)
    for extra in (["--search", "ctc"], ["--search", "transducer_greedy"], ["--search", "ctc_beam", "--ngram-lm", "lm.arpa"]):
        with pytest.raises(NotImplementedError, match="--stream-endpoint"):
            sr.main(_MISSING + ["--streaming", "--stream-endpoint"] + extra)
    for search in ("ctc_stream_beam", "transducer_stream_beam"):
        with pytest.raises(NotImplementedError, match="--stream-endpoint.*--nbest"):
            sr.main(_MISSING + ["--streaming", "--stream-endpoint", "--search", search, "--nbest", "2", "--beam", "4"])
        with pytest.raises(ValueError, match="--endpoint-max-segment-s"):
            sr.main(_MISSING + ["--streaming", "--stream-endpoint", "--search", search, "--endpoint-max-segment-s", "0"])
        for more in ([], ["--stream-partials"], ["--ctm", "-"]):
            with pytest.raises(FileNotFoundError):
                sr.main(_MISSING + ["--device", "cpu", "--streaming", "--stream-endpoint", "--search", search] + more)
    kw = sr.endpoint_options(sr.get_parser().parse_args(_MISSING + ["--endpoint-empty-s", "0", "--endpoint-silence-s", "0.01"]), 0.04)
    assert kw["endpoint"].frames() == (1, 0, 500) and kw["seconds_per_frame"] == 0.04
    assert sr.endpoint_options(a, 0.04)["endpoint"].frames() == (20, 125, 500)
    help_text = " ".join(sr.get_parser().format_help().split())
    assert "--stream-endpoint" in help_text and "--endpoint-max-segment-s" in help_text


# =============================================================================================================== GPU
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


def _check_coverage(segments):
    """Every rule and room end a segment somewhere, stream 2 never has a token and stream 1 never ends for silence."""
    reasons = {reason for segs in segments.values() for _, _, reason, _ in segs}
    assert reasons >= {1, 2, 3, ROOM, FINAL}, reasons
    assert all(reason in (2, FINAL) for _, _, reason, _ in segments[2]) and all(reason != 1 for _, _, reason, _ in segments[1])
    assert sum(n for _, n, _, _ in segments[0]) == 60 and max(n for segs in segments.values() for _, n, _, _ in segs) <= MAX_FRAMES


# --------------------------------------------------------------------------------------------------------------- CTC
def _ctc_case(beam, mode, seed):
    return dict(beam=beam, K=4, mode=mode, seed=seed)


# the seed of a case: the first from 0 whose lead, pruning margin and Viterbi gap are clear (test_ctc_case_margins_are_clear)
CTC_CASES = [_ctc_case(1, "plain", 0), _ctc_case(4, "plain", 0), _ctc_case(16, "plain", 0), _ctc_case(4, "lm", 4),
             _ctc_case(4, "bonus", 0), _ctc_case(16, "graph", 0)]


def _ctc_id(c):
    return "b{beam}-{mode}".format(**c)


def _ctc_need(c):
    """(what lead and pruning margin must exceed, what every Viterbi gap must exceed): tests.test_beam_time_stamps._ctc_bound for
    segments of at most MAX_FRAMES frames."""
    lm = LM_WEIGHT * LM_TOL * (MAX_FRAMES + 1) if c["mode"] == "lm" else 0.0
    return 2 * (SCORE_TOL + lm), 2 * SCORE_TOL


class _CtcCase:
    def __init__(self, c):
        self.c, self.d = c, _dictionary(V - 5)
        assert len(self.d) == V and self.d.bos() == 0
        self.x = {}
        for sid, n, _, _ in STREAMS:
            z = _peaked(np.random.default_rng([c["seed"], sid]), n, V, sharp=4.0, scale=2.0)
            z[:, 0] += [_shift("ctc", sid, t) for t in range(n)]
            x32 = torch.from_numpy(z - np.logaddexp.reduce(z, axis=1, keepdims=True)).to(torch.float32)
            self.x[sid] = x32
        self.graph = _graph(grid_phrases(self.x[0][None, :25].numpy().astype(np.float64), [25], 0)) if c["mode"] == "graph" else None

    @functools.cached_property
    def oracle_kw(self):
        mode = self.c["mode"]
        if mode == "lm":
            return dict(lm_fn=_cpu_lm_fn(_tiny_lm(self.d, seed=3), self.d), lm_weight=LM_WEIGHT, bonus=BONUS, eos=self.d.eos())
        if mode == "bonus":
            return dict(bonus=BONUS)
        if mode == "graph":
            return dict(lm_fn=bias_lm_fn(self.graph, V), lm_weight=1.0, eos=V)
        return {}

    @functools.cached_property
    def sim(self):
        def make(sid, start):
            x = self.x[sid].numpy().astype(np.float64)
            return CtcEndpointOracle(lambda lo, hi: x[start + lo:start + hi], self.c["beam"], self.c["K"], 0, **self.oracle_kw)

        return simulate(STREAMS, RULES, MAX_FRAMES, make)

    def clear(self):
        lead, margin, vgap = self.sim[2]
        need, need_gap = _ctc_need(self.c)
        return min(lead, margin) > need and vgap > need_gap

    def options(self):
        mode = self.c["mode"]
        lm = _tiny_lm(self.d, seed=3).to(DEV) if mode == "lm" else None
        return dict(beam_size=self.c["beam"], nbest=min(self.c["beam"], 3), beam_size_token=self.c["K"], lm_model=lm,
                    lm_weight=LM_WEIGHT if lm is not None else 0.0, insertion_bonus=BONUS if mode in ("lm", "bonus") else 0.0,
                    context_graph=self.graph)


@functools.lru_cache(maxsize=None)
def _ctc_built(i):
    return _CtcCase(CTC_CASES[i])


def test_ctc_case_margins_are_clear():
    """The cases without the LSTM LM (its oracle takes a while on the CPU: the GPU test asserts that one): margins and coverage."""
    for i, c in enumerate(CTC_CASES):
        if c["mode"] != "lm":
            r = _ctc_built(i)
            assert r.clear(), (_ctc_id(c), r.sim[2])
            _check_coverage(r.sim[1])


def _batch_of_one(rows):
    """[T][V] rows -> a fresh [1][T][V] tensor (the stride of a size-1 dimension of a view is not the batch stride)."""
    out = torch.empty(1, *rows.shape, dtype=rows.dtype, device=rows.device)
    out[0].copy_(rows)
    return out


def _same_hyps(got, want, where):
    """Two hypothesis lists in the generators' format: tokens, scores, times and Viterbi scores torch.equal."""
    assert len(got) == len(want) >= 1, (where, len(got), len(want))
    for g, w in zip(got, want):
        for k in ("tokens", "score", "times", "viterbi_score"):
            assert torch.equal(g[k], w[k]), (where, k, g[k], w[k])


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CTC_CASES)), ids=[_ctc_id(c) for c in CTC_CASES])
def test_ctc_endpoint_vs_oracle_and_segments_vs_offline(i):
    _need_gpu()
    from espresso_amd.tools.beam_common import EndpointRules, hyps_from_tensors
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder
    from espresso_amd.tools.streaming_ctc_prefix_beam_decoder import StreamingCTCPrefixBeamDecoder

    r = _ctc_built(i)
    rounds, segments, (lead, margin, vgap) = r.sim
    assert r.clear(), (lead, margin, vgap)
    _check_coverage(segments)
    opts = r.options()
    dec = StreamingCTCPrefixBeamDecoder(r.d, MAX_STREAMS, MAX_FRAMES, endpoint=EndpointRules(*RULES), **opts)
    off = CTCPrefixBeamSearchDecoder([None], r.d, token_times=True, **opts)
    xd = {sid: x.to(DEV) for sid, x in r.x.items()}
    done = {sid: 0 for sid in LENGTH}  # segments compared so far

    def check_segment(sid, hyps):
        start, n, reason, _ = segments[sid][done[sid]]
        done[sid] += 1
        want = hyps_from_tensors(*(t.cpu() for t in off.search(_batch_of_one(xd[sid][start:start + n]),
                                                               torch.tensor([n], dtype=torch.int32, device=DEV))))[0]
        _same_hyps(hyps, want, (sid, start, n, reason))

    slot_of_2 = None
    for k, rd in enumerate(rounds):
        dec.open(rd["open"])
        if 3 in rd["open"]:
            assert dec.streams[3][0] == slot_of_2  # the restarted slot of stream 2, reused
        ids = [sid for sid, _, _ in rd["accept"]]
        counts = [hi - lo for _, lo, hi in rd["accept"]]
        assert dec.room(ids, counts) == rd["room"], (k, dec.room(ids, counts), rd["room"])
        for sid in rd["room"]:
            check_segment(sid, dec.end_segment(sid))
        if sum(counts):
            dec.accept_lprobs(ids, torch.cat([xd[sid][lo:hi] for sid, lo, hi in rd["accept"]]), counts)
        got = dec.endpoint(ids)
        assert got == [rd["probes"][sid][:4] for sid in ids], (k, got, rd["probes"])
        parts = dec.partial(ids)
        tokens, lengths, _, nhyp, times, _ = (t.cpu() for t in dec.finish(ids, nbest=r.c["beam"]))
        for e, sid in enumerate(ids):
            rule, F, L, E, y = rd["probes"][sid]
            assert tuple(parts[e]["tokens"]) == y and len(y) == L, (k, sid, parts[e], y)
            match = [j for j in range(int(nhyp[e])) if tokens[e, j, : int(lengths[e, j])].tolist() == list(y)]
            assert len(match) == 1 and (E == -1 if L == 0 else int(times[e, match[0], L - 1]) == E), (k, sid, E)
        for sid, rule in rd["ends"]:
            check_segment(sid, dec.end_segment(sid))
            assert dec.streams[sid][1] == 0
        for sid in rd["close"]:
            if sid == 2:
                slot_of_2 = dec.streams[2][0]
            check_segment(sid, dec.close(sid))
    assert done == {sid: len(segs) for sid, segs in segments.items()} and not dec.streams
    print(f"{_ctc_id(r.c)}: lead {lead:.3g}, margin {margin:.3g}, Viterbi gap {vgap:.3g}; segments "
          + "; ".join(f"{sid}: " + " ".join(f"{n}/{reason}" for _, n, reason, _ in segs) for sid, segs in segments.items()))


@pytest.mark.gpu
def test_ctc_decoder_without_endpoint_is_unchanged():
    """Built without `endpoint`: the results of today (the offline search without times, bit for bit), no times state, and the
    ValueError for max_frames."""
    _need_gpu()
    from espresso_amd.tools.beam_common import hyps_from_tensors
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder
    from espresso_amd.tools.streaming_ctc_prefix_beam_decoder import StreamingCTCPrefixBeamDecoder

    r = _ctc_built(1)
    opts = r.options()
    dec = StreamingCTCPrefixBeamDecoder(r.d, MAX_STREAMS, MAX_FRAMES, **opts)
    x = r.x[1].to(DEV)
    dec.open(["u"])
    dec.accept_lprobs(["u"], x[:13], [13])
    dec.accept_lprobs(["u"], x[13:20], [7])
    assert dec.times_state is None and dec.room(["u"], [5]) == ["u"]
    with pytest.raises(ValueError, match="max_frames"):
        dec.accept_lprobs(["u"], x[20:25], [5])
    with pytest.raises(ValueError, match="endpoint"):
        dec.endpoint(["u"])
    want = hyps_from_tensors(*(t.cpu() for t in CTCPrefixBeamSearchDecoder([None], r.d, **opts).search(
        _batch_of_one(x[:20]), torch.tensor([20], dtype=torch.int32, device=DEV))))[0]
    got = dec.close("u")
    assert len(got) == len(want) and all(torch.equal(g["tokens"], w["tokens"]) and torch.equal(g["score"], w["score"]) and "times" not in g
                                         for g, w in zip(got, want))


@pytest.mark.gpu
def test_endpoint_entries_refuse_bad_arguments():
    """-2 before anything is launched, a RuntimeError that names the entry point from the wrappers, (0, 0, 0, -1) for a slot
    out of range, and the empty hypothesis for a reset slot."""
    _need_gpu()
    from espresso_amd import kernels as Kn

    beam, mf = 4, 8
    lib = Kn._lib.lib()
    slots = torch.tensor([1, 7, -1, 0], dtype=torch.int32, device=DEV)
    out = torch.full((4, 4), 77, dtype=torch.int32, device=DEV)
    st, p = Kn._stream(), Kn._p
    cs, _ = Kn.ctc_prefix_beam_stream_state(2, mf, beam, DEV)
    ct, _ = Kn.ctc_prefix_beam_stream_times_state(2, mf, beam, DEV)
    for bad in ((None, p(ct), p(slots), 4, 0.0, 0.0, 0, 2, mf, beam), (p(cs), None, p(slots), 4, 0.0, 0.0, 0, 2, mf, beam),
                (p(cs), p(ct), None, 4, 0.0, 0.0, 0, 2, mf, beam), (p(cs), p(ct), p(slots), 4, 0.0, 0.0, 0, 0, mf, beam),
                (p(cs), p(ct), p(slots), 4, 0.0, 0.0, 0, 2, 0, beam), (p(cs), p(ct), p(slots), 4, 0.0, 0.0, 0, 2, mf, 65),
                (p(cs), p(ct), p(slots), 4, 0.0, 0.0, 0, 2, mf, 0)):
        assert lib.ea_ctc_prefix_beam_stream_endpoint(*bad, 6, 10, 20, p(out), st) == -2
    assert lib.ea_ctc_prefix_beam_stream_endpoint(p(cs), p(ct), p(slots), 4, 0.0, 0.0, 0, 2, mf, beam, 6, 10, 20, None, st) == -2
    assert lib.ea_ctc_prefix_beam_stream_endpoint(p(cs), p(ct), p(slots), 0, 0.0, 0.0, 0, 2, mf, beam, 6, 10, 20, None, st) == 0  # n <= 0
    with pytest.raises(RuntimeError, match="ea_ctc_prefix_beam_stream_endpoint"):
        Kn.ctc_prefix_beam_stream_endpoint(cs, None, slots, mf, beam, 6, 10, 20)
    rs, _ = Kn.rnnt_frame_beam_stream_state(2, mf, beam, DEV)
    rb, _ = Kn.rnnt_frame_beam_stream_bias_state(2, mf, beam, DEV)
    rt, _ = Kn.rnnt_frame_beam_stream_times_state(2, mf, beam, DEV)
    for bad in ((None, p(rt), p(slots), 4, 0, 2, mf, beam), (p(rs), None, p(slots), 4, 0, 2, mf, beam), (p(rs), p(rt), None, 4, 0, 2, mf, beam),
                (p(rs), p(rt), p(slots), 4, 0, 0, mf, beam), (p(rs), p(rt), p(slots), 4, 0, 2, 0, beam), (p(rs), p(rt), p(slots), 4, 0, 2, mf, 65)):
        assert lib.ea_rnnt_frame_beam_stream_endpoint(*bad, 6, 10, 20, p(out), st) == -2
    assert lib.ea_rnnt_frame_beam_stream_endpoint(p(rs), p(rt), p(slots), 4, 0, 2, mf, beam, 6, 10, 20, None, st) == -2
    with pytest.raises(RuntimeError, match="ea_rnnt_frame_beam_stream_endpoint"):
        Kn.rnnt_frame_beam_stream_endpoint(rs, None, slots, mf, beam, 6, 10, 20)
    torch.cuda.synchronize()
    assert out.eq(77).all()  # nothing was launched
    # reset slots: F = 0, the empty hypothesis; slots out of range: (0, 0, 0, -1); thresholds that F = 0 meets only when <= 0 is off
    both = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    Kn.ctc_prefix_beam_stream_times_reset(cs, ct, both, mf, beam)
    assert Kn.ctc_prefix_beam_stream_endpoint(cs, ct, slots, mf, beam, 6, 10, 20).tolist() == [[0, 0, 0, -1]] * 4
    assert Kn.ctc_prefix_beam_stream_endpoint(cs, ct, slots, mf, beam, 0, 0, 0).tolist() == [[0, 0, 0, -1]] * 4
    for state, biased in ((rs, False), (rb, True)):
        Kn.rnnt_frame_beam_stream_times_reset(state, rt, both, mf, beam, biased=biased)
        assert Kn.rnnt_frame_beam_stream_endpoint(state, rt, slots, mf, beam, 6, 10, 20, biased=biased).tolist() == [[0, 0, 0, -1]] * 4


# --------------------------------------------------------------------------------------------------------------- transducer
def _rnnt_case(beam, mode, seed):
    return dict(beam=beam, K=min(4, max(1, beam)), mode=mode, seed=seed)


RNNT_CASES = [_rnnt_case(1, "plain", 0), _rnnt_case(4, "plain", 0), _rnnt_case(16, "plain", 47), _rnnt_case(4, "lm", 2),
              _rnnt_case(4, "biased", 2)]
RNNT_NEED = 2 * (SCORE_TOL + 8 * TERM_TOL * 2 * MAX_FRAMES)  # twice the largest bound: 24 frame terms and as many bias terms


def _rnnt_id(c):
    return "b{beam}-{mode}".format(**c)


class _RnntCase:
    """The TableModel (and TableLM) of a case with the blank logit shifted frame by frame, fp32 rows the oracle reads as they
    are; a segment's hypotheses start from the empty one, so a row is that of (stream, frame of the stream, tokens of the
    segment)."""

    def __init__(self, c):
        self.c = c
        self.table = TableModel(V, c["seed"], blank=BLANK)
        self.lm = TableLM(V, c["seed"] + 1000) if c["mode"] == "lm" else None
        self.kw = dict(lm_fn=self.lm, lm_weight=0.6 if self.lm is not None else 0.0)
        self.step_kw = dict(eos=-1, temperature=1.0, lm_weight=self.kw["lm_weight"], lm_no_blank=False)
        self.graph = None
        if c["mode"] == "biased":
            y = frame_beam_oracle(lambda t, y: self.row(0, t, y).astype(np.float64), 25, 16, 4, BLANK, nbest=2)[0][1][0]
            self.graph = _graph([(list(y[i:i + 2]), 0.73 + 0.64 * (i % 2)) for i in range(len(y) - 1)])

    def row(self, sid, t, y):
        x = self.table.row(sid, t, y).copy()
        x[BLANK] += np.float32(_shift("transducer", sid, t))
        return x

    @functools.cached_property
    def sim(self):
        def make(sid, start):
            return TransducerEndpointOracle(lambda t, y: self.row(sid, start + t, y).astype(np.float64), self.c["beam"], self.c["K"], BLANK,
                                            graph=self.graph, **self.kw)

        return simulate(STREAMS, RULES, MAX_FRAMES, make)

    def clear(self):
        return min(self.sim[2]) > RNNT_NEED


@functools.lru_cache(maxsize=None)
def _rnnt_built(i):
    return _RnntCase(RNNT_CASES[i])


def test_transducer_case_margins_are_clear():
    for i, c in enumerate(RNNT_CASES):
        r = _rnnt_built(i)
        assert r.clear(), (_rnnt_id(c), r.sim[2])
        _check_coverage(r.sim[1])


def _rows_of(r, jobs, beam):
    """Device (logits [n * beam][V], lm rows or None) for jobs = [(stream, frame of the stream or None, live sequences)]; rows
    of dead beam slots and of idle entries are NaN."""
    x = np.full((len(jobs) * beam, V + 3), np.nan, dtype=np.float32)
    m = np.full((len(jobs) * beam, V), np.nan, dtype=np.float32)
    for e, (sid, t, seqs) in enumerate(jobs):
        if t is not None:
            for j, y in enumerate(seqs):
                x[e * beam + j, :V] = r.row(sid, t, y)
                if r.lm is not None:
                    m[e * beam + j] = r.lm.row(y)
    return torch.from_numpy(x).to(DEV)[:, :V], (torch.from_numpy(m).to(DEV) if r.lm is not None else None)


def _advance(seqs, out, e, beam):
    """The live sequences of entry e after a step, from the triple the step wrote for its `beam` rows.  Dead slots carry the filler
    (slot 0, blank, keep) behind the live ones; the stay of slot 0 is one candidate, so at most one live slot looks the same: the
    first of a trailing run of fillers is that stay unless it stands further up (with dead slots nothing was pruned)."""
    rows = [(int(p) - e * beam, int(v), int(k)) for p, v, k in zip(*(o[e * beam:(e + 1) * beam].tolist() for o in out))]
    filler, n = (0, BLANK, 1), beam
    while n > 0 and rows[n - 1] == filler:
        n -= 1
    if n < beam and filler not in rows[:n]:
        n += 1
    return [seqs[p] + (() if k else (v,)) for p, v, k in rows[:n]]


def _offline_segment(r, fam, sid, start, n, nbest):
    """The offline times kernels over frames [start, start + n) of a stream, the rows of every frame built from the kernels' own
    triples: the six finish tensors and the live sequences after the last frame."""
    beam = r.c["beam"]
    ws = fam.workspace(1, n, beam, DEV)
    in_len = torch.tensor([n], dtype=torch.int32, device=DEV)
    out = (torch.empty(beam, dtype=torch.int32, device=DEV), torch.empty(beam, dtype=torch.int32, device=DEV),
           torch.empty(beam, dtype=torch.uint8, device=DEV))
    seqs = [()]
    for t in range(n):
        x, m = _rows_of(r, [(sid, start + t, seqs)], beam)
        fam.step(x, in_len, ws, out, 1, n, V, beam, r.c["K"], BLANK, t, lm_rows=m, **r.step_kw)
        seqs = _advance(seqs, tuple(o.cpu() for o in out), 0, beam)
    return fam.finish(ws, 1, n, beam, nbest, PAD, normalize=True), seqs


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(RNNT_CASES)), ids=[_rnnt_id(c) for c in RNNT_CASES])
def test_transducer_endpoint_vs_oracle_and_segments_vs_offline(i):
    """The streamed times kernels (rows from their own triples, as the decoder's predictor would give them) with the endpoint
    probe after every accept; a segment end is the streamed finish, compared with the offline kernels over the segment, and the
    reset of the slot."""
    _need_gpu()
    from espresso_amd import kernels as Kn
    from tests.test_beam_time_stamps import _TimesFamily

    r = _rnnt_built(i)
    rounds, segments, (lead, margin, vgap) = r.sim
    assert r.clear(), (lead, margin, vgap)
    _check_coverage(segments)
    beam, K, biased = r.c["beam"], r.c["K"], r.graph is not None
    nbest = min(beam, 3)
    fam, off = _TimesFamily(r.graph), _TimesFamily(r.graph)
    state, _ = fam.state(MAX_STREAMS, MAX_FRAMES, beam, DEV)
    state.fill_(0xA5)
    free, slot, seqs, frames = [2, 0, 1], {}, {}, {}
    done = {sid: 0 for sid in LENGTH}

    def reset(sid):
        fam.reset(state, torch.tensor([slot[sid]], dtype=torch.int32, device=DEV), MAX_FRAMES, beam)
        seqs[sid], frames[sid] = [()], 0

    def end_segment(sid):
        start, n, reason, _ = segments[sid][done[sid]]
        done[sid] += 1
        assert frames[sid] == n
        got = fam.sfinish(state, torch.tensor([slot[sid]], dtype=torch.int32, device=DEV), MAX_FRAMES, beam, nbest, PAD, n, normalize=True)
        want, want_seqs = _offline_segment(r, off, sid, start, n, nbest)
        for g, w in zip(got, want):
            assert torch.equal(g, w), (sid, start, n, reason, g, w)
        assert seqs[sid] == want_seqs
        reset(sid)

    def probe(ids):
        slots = torch.tensor([slot[sid] for sid in ids], dtype=torch.int32, device=DEV)
        before, tbefore = state.clone(), fam.tstate.clone()
        got = Kn.rnnt_frame_beam_stream_endpoint(state, fam.tstate, slots, MAX_FRAMES, beam, *RULES, biased=biased)
        assert torch.equal(state, before) and torch.equal(fam.tstate, tbefore)  # read only
        return got.tolist(), slots

    for k, rd in enumerate(rounds):
        for sid in rd["open"]:
            slot[sid] = free.pop()
            reset(sid)
        for sid in rd["room"]:
            end_segment(sid)
        ids = [sid for sid, _, _ in rd["accept"]]
        counts = [hi - lo for _, lo, hi in rd["accept"]]
        slot_idx = torch.tensor([slot[sid] for sid in ids], dtype=torch.int32, device=DEV)
        nn = torch.tensor(counts, dtype=torch.int32, device=DEV)
        out = (torch.empty(len(ids) * beam, dtype=torch.int32, device=DEV), torch.empty(len(ids) * beam, dtype=torch.int32, device=DEV),
               torch.empty(len(ids) * beam, dtype=torch.uint8, device=DEV))
        for j in range(max(counts)):
            x, m = _rows_of(r, [(sid, lo + j if j < hi - lo else None, seqs[sid]) for sid, lo, hi in rd["accept"]], beam)
            fam.sstep(x, slot_idx, nn, j, state, out, MAX_FRAMES, V, beam, K, BLANK, lm_rows=m, **r.step_kw)
            cpu = tuple(o.cpu() for o in out)
            for e, (sid, c) in enumerate(zip(ids, counts)):
                if j < c:
                    seqs[sid] = _advance(seqs[sid], cpu, e, beam)
                    frames[sid] += 1
        got, slots = probe(ids)
        assert got == [list(rd["probes"][sid][:4]) for sid in ids], (k, got, rd["probes"])
        toks, lens_, _, _ = (t.cpu() for t in fam.partial(state, slots, MAX_FRAMES, beam, PAD, MAX_FRAMES))
        fin = [t.cpu() for t in fam.sfinish(state, slots, MAX_FRAMES, beam, beam, PAD, MAX_FRAMES, normalize=False)]
        for e, sid in enumerate(ids):
            rule, F, L, E, y = rd["probes"][sid]
            assert tuple(toks[e, : int(lens_[e])].tolist()) == y and len(y) == L, (k, sid, y)
            match = [j for j in range(int(fin[3][e])) if fin[0][e, j, : int(fin[1][e, j])].tolist() == list(y)]
            assert len(match) == 1 and (E == -1 if L == 0 else int(fin[4][e, match[0], L - 1]) == E), (k, sid, E)
        for sid, rule in rd["ends"]:
            end_segment(sid)
        for sid in rd["close"]:
            end_segment(sid)
            free.append(slot.pop(sid))
    assert done == {sid: len(segs) for sid, segs in segments.items()} and not slot
    print(f"{_rnnt_id(r.c)}: lead {lead:.3g}, margin {margin:.3g}, Viterbi gap {vgap:.3g}; segments "
          + "; ".join(f"{sid}: " + " ".join(f"{n}/{reason}" for _, n, reason, _ in segs) for sid, segs in segments.items()))


# --------------------------------------------------------------------------------------------------------------- end to end
def _cli_lines(out):
    segs, hyps = {}, {}
    for ln in out.splitlines():
        f = ln.split("\t")
        if ln.startswith("S-"):
            segs.setdefault(f[0][2:], []).append((float(f[1]), float(f[2]), f[3], f[4]))
        elif ln.startswith("H-"):
            hyps[f[0][2:]] = f[1]
    return segs, hyps


def _check_cli(out, ctm_path, utts, seconds, limit_s):
    """The H- text is the S- texts joined; the segments tile the audio in order, none longer than the limit plus one piece; the
    CTM times do not decrease across the joins and lie inside the audio."""
    segs, hyps = _cli_lines(out)
    assert set(segs) == set(hyps) == set(utts)
    for u in utts:
        assert hyps[u] == " ".join(t for _, _, _, t in segs[u] if t), (u, hyps[u], segs[u])
        assert segs[u][0][0] == 0.0 and segs[u][-1][2] == "final" and all(r in ("silence", "empty", "length") for _, _, r, _ in segs[u][:-1])
        assert all(a[1] == b[0] for a, b in zip(segs[u], segs[u][1:])) and abs(segs[u][-1][1] - seconds[u]) < 0.1
        assert all(e - s <= limit_s + 0.7 for s, e, _, _ in segs[u])  # the limit, then at most what one accept brings
    assert max(len(s) for s in segs.values()) >= 4  # several times longer than the segment limit
    starts = {u: [] for u in utts}
    for ln in open(ctm_path, encoding="utf-8").read().splitlines():
        f = ln.split()
        starts[f[0]].append((float(f[2]), float(f[3]), f[4]))
    for u in utts:
        assert [w for _, _, w in starts[u]] == hyps[u].split(), u
        t = [s for s, _, _ in starts[u]]
        assert t == sorted(t) and all(0.0 <= s and s + dur <= seconds[u] + 0.05 for s, dur, _ in starts[u]), (u, t)
    return segs


@pytest.mark.gpu
def test_cli_ctc_stream_endpoint_end_to_end(tmp_path, capsys):
    """speech_recognize --streaming --search ctc_stream_beam --stream-endpoint --ctm on the small chunk-streaming CTC checkpoint of
    tests.test_streaming_ctc_prefix_beam with utterances of 2.2 - 3 s and a segment limit of 0.4 s; then with --stream-partials."""
    _need_gpu()
    from espresso_amd import speech_recognize as sr
    from tests.test_streaming_ctc_prefix_beam import _cli_fixture, _tones

    d, utts, base = _cli_fixture(tmp_path, audio=lambda rng, s: _tones(rng, 1.5 + s))
    seconds = {u: 1.5 + 0.7 + 0.4 * i for i, u in enumerate(utts)}
    ctm = tmp_path / "out.ctm"
    argv = base + ["--streaming", "--search", "ctc_stream_beam", "--beam", "5", "--ctc-beam-size-token", "4", "--stream-chunk-ms", "170",
                   "--streams", "2", "--stream-endpoint", "--endpoint-silence-s", "0.2", "--endpoint-empty-s", "0.3",
                   "--endpoint-max-segment-s", "0.4", "--ctm", str(ctm)]
    capsys.readouterr()
    sr.main(argv)
    segs = _check_cli(capsys.readouterr().out, str(ctm), utts, seconds, 0.4)
    sr.main(argv + ["--stream-partials"])
    out = capsys.readouterr().out
    assert _check_cli(out, str(ctm), utts, seconds, 0.4) == segs
    _, hyps = _cli_lines(out)
    closed = {u: "" for u in utts}
    for ln in out.splitlines():  # the stable field carries the closed segments' text, and the final text starts with it
        f = ln.split("\t")
        if ln.startswith("S-") and f[4]:
            closed[f[0][2:]] = (closed[f[0][2:]] + " " + f[4]).strip()
        if ln.startswith("P-"):
            u = f[0][2:]
            assert f[2].startswith(closed[u]) and hyps[u].startswith(f[2]), (ln, closed[u])


@pytest.mark.gpu
def test_cli_transducer_stream_endpoint_end_to_end(tmp_path, capsys):
    """The same with --search transducer_stream_beam on a small random chunk-streaming transducer checkpoint (that of
    tests.test_streaming_transducer_beam.test_cli_streaming_beam_end_to_end)."""
    _need_gpu()
    from espresso_amd import registry
    from espresso_amd import speech_recognize as sr
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from tests.test_streaming_ctc_prefix_beam import _tones, _write_wav

    dict_path = str(tmp_path / "dict.txt")
    open(dict_path, "w").write("".join(f"t{i} 1\n" for i in range(20)))
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(dict=dict_path, autoregressive=False,
                                                                                    criterion_name="transducer_loss"))
    enc = {"conv_channels": "[64, 64, 16, 16]", "embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4,
           "normalize_before": True, "relative_positional_embeddings": True, "layer_type": "transformer", "chunk_size": 8,
           "chunk_left_window": 2, "chunk_right_window": 0}
    name = "speech_transformer_transducer_base"
    block = {"_name": name, "encoder": enc, "decoder": {"embed_dim": 48, "hidden_size": 64, "layers": 1}, "joint_dim": 64,
             "dropout": 0.0, "attention_dropout": 0.0, "activation_dropout": 0.0}
    cls = registry.MODEL_REGISTRY[name]
    torch.manual_seed(0)
    model = cls.build_model(cls.config_class.from_dict(block), task)
    torch.save({"model": model.state_dict(), "cfg": {"model": block}}, str(tmp_path / "model.pt"))
    rng = np.random.default_rng(0)
    utts = [f"utt{i}" for i in range(2)]
    seconds = {u: 2.2 + 0.6 * i for i, u in enumerate(utts)}
    with open(tmp_path / "wav.scp", "w") as f:
        for u in utts:
            p = str(tmp_path / f"{u}.wav")
            _write_wav(p, _tones(rng, seconds[u]))
            f.write(f"{u} {p}\n")
    ctm = tmp_path / "out.ctm"
    capsys.readouterr()
    sr.main(["--path", str(tmp_path / "model.pt"), "--dict", dict_path, "--wav-scp", str(tmp_path / "wav.scp"), "--streaming", "--search",
             "transducer_stream_beam", "--beam", "4", "--transducer-beam-size-token", "3", "--stream-chunk-ms", "170", "--streams", "2",
             "--stream-endpoint", "--endpoint-silence-s", "0.2", "--endpoint-empty-s", "0.3", "--endpoint-max-segment-s", "0.4",
             "--ctm", str(ctm)])
    _check_cli(capsys.readouterr().out, str(ctm), utts, seconds, 0.4)
