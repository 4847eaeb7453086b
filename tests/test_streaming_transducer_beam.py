"""The streamed frame-synchronous transducer beam search (csrc/rnnt_beam.hip ea_rnnt_frame_beam_stream_*,
tools/streaming_transducer_frame_beam_decoder.py, speech_recognize --streaming --search transducer_stream_beam).

The offline search is held to the float64 oracle in tests/test_transducer_frame_beam.py; here the streamed kernels are held to
the offline kernels bit for bit (the same device functions in the same order: an identity, not a tolerance) and to the same
oracle, whose beam after the first t frames (normalize=False, nbest=beam) is the live beam the partial readout describes."""
import math
import os

import numpy as np
import pytest
import torch

from tests.test_transducer_frame_beam import (BLANK, CASES, EOS, SCORE_TOL, TERM_TOL, _case_id, _case_models, _case_oracle, _lens,
                                              case_margin)
from tests.transducer_frame_beam_ref import TableLM, TableModel, frame_beam_oracle

DEV = "cuda:0"
PAD = 1

# V 20, 5004 and 6000 (beyond the LDS-staged columns), beam 1, 4 and 16, the LM with and without a blank column, temperature,
# predicts_eos, unnormalised scores; every case has utterances of 0 and 1 frames (LENS / LENS_WIDE of the offline test file)
SUBSET = ["V20-b1-K1", "V20-b4-K4", "V20-b16-K4", "V20-b4-K4-temperature=1.7", "V20-b4-K4-predicts_eos=True",
          "V20-b16-K4-lm=blank-lm_weight=0.6", "V20-b16-K4-lm=no_blank-lm_weight=0.6", "V20-b4-K4-normalize=False",
          "V20-b16-K4-long=True", "V5004-b1-K4", "V5004-b4-K4", "V5004-b16-K4",
          "V5004-b4-K4-lm=no_blank-lm_weight=0.4-predicts_eos=True-temperature=0.8-normalize=False", "V6000-b4-K4",
          "V6000-b4-K4-lm=blank-lm_weight=0.5"]
STREAM_CASES = [c for c in CASES if _case_id(c) in SUBSET]


def test_subset_covers_the_issue():
    assert len(STREAM_CASES) == len(SUBSET)
    assert {c["V"] for c in STREAM_CASES} == {20, 5004, 6000} and {c["beam"] for c in STREAM_CASES} == {1, 4, 16}
    opts = [c["opts"] for c in STREAM_CASES]
    assert {o.get("lm") for o in opts} == {None, "blank", "no_blank"}
    assert any(o.get("temperature") for o in opts) and any(o.get("predicts_eos") for o in opts)
    assert all(0 in _lens(c) and 1 in _lens(c) for c in STREAM_CASES)


def test_subset_margins_are_clear():
    for c in STREAM_CASES:
        if c["V"] <= 100:  # (the larger ones take a minute on the CPU: the GPU test asserts theirs)
            assert case_margin(c) > 10 * SCORE_TOL, _case_id(c)


# ---------------------------------------------------------------------------------------------------------------- the partial oracle
def live_beam(logits_fn, t, beam, K, **kw):
    """The live hypotheses [(tokens, raw score)] in slot order after the first t frames, and the oracle's margin."""
    hyps, _, margin = frame_beam_oracle(logits_fn, t, beam, K, BLANK, normalize=False, nbest=beam, **kw)
    return hyps, margin


def partial_oracle(hyps):
    """(tokens of the best live hypothesis by raw score, ties to the lower slot; length of the longest common prefix)."""
    best = max(range(len(hyps)), key=lambda j: (hyps[j][1], -j))
    k = 0
    while all(len(y) > k for y, _ in hyps) and len({y[k] for y, _ in hyps}) == 1:
        k += 1
    return hyps[best][0], k, hyps[best][1]


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("beam", [1, 4, 16])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_stable_prefix_never_changes(seed, beam, with_lm):
    """stable_len after frame t never exceeds the length of, and its tokens always prefix, every hypothesis of every later
    frame and of the finish (normalised and not)."""
    V, T, K = 12, 10, min(beam, 4)
    table = TableModel(V, seed, blank=BLANK, sharp=4.0)
    kw = dict(lm_fn=TableLM(V, seed + 77), lm_weight=0.5) if with_lm else {}
    beams = [live_beam(table.logits_fn(0), t, beam, K, **kw)[0] for t in range(T + 1)]
    finals = [frame_beam_oracle(table.logits_fn(0), T, beam, K, BLANK, normalize=n, nbest=beam, **kw)[0] for n in (False, True)]
    grew = 0
    for t in range(T + 1):
        y, k, s = partial_oracle(beams[t])
        assert s == max(s_ for _, s_ in beams[t]) and k <= len(y)
        grew += k > 0
        for later in beams[t:] + finals:
            for y2, _ in later:
                assert len(y2) >= k and y2[:k] == y[:k], (t, y, k, y2)
    assert beams[0] == [((), 0.0)] and partial_oracle(beams[0])[:2] == ((), 0)
    if beam == 1:
        assert grew > 0  # (one hypothesis: all of it is stable)


# ---------------------------------------------------------------------------------------------------------------- CLI, CPU
def _main(argv):
    from espresso_amd import speech_recognize as sr

    return sr.main(["--path", "/nonexistent.pt", "--dict", "d", "--wav-scp", "w", *argv])


def test_cli_new_search_name_builds():
    from espresso_amd import speech_recognize as sr
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder
    from tests.test_ctc_prefix_beam import _tiny_lm
    from tests.test_transducer_frame_beam import _dictionary

    argv = ["--path", "/nonexistent.pt", "--dict", "d", "--wav-scp", "w", "--device", "cpu", "--streaming", "--search",
            "transducer_stream_beam", "--beam", "6", "--nbest", "2", "--transducer-beam-size-token", "3", "--temperature", "1.5",
            "--unnormalized", "--lm-path", "lm.pt", "--lm-weight", "0.3", "--stream-partials", "--streams", "4", "--stream-chunk-ms", "170"]
    args = sr.get_parser().parse_args(argv)
    for check in (sr.check_frame_beam_args, sr.check_stream_beam_args, sr.check_hotword_args, sr.check_ngram_args, sr.check_streaming_args):
        check(args)
    assert sr.lm_fusion_mode(args) == "subword"
    lm = _tiny_lm(_dictionary(8))
    g = StreamingTransducerFrameBeamDecoder(None, _dictionary(8), max_streams=args.streams, max_frames=50, **sr.stream_beam_options(args, lm))
    assert (g.beam_size, g.nbest, g.beam_size_token, g.offline.temperature, g.offline.normalize_scores, g.lm_model, g.lm_weight) == \
        (6, 2, 3, 1.5, False, lm, 0.3)
    assert (g.max_streams, g.max_frames) == (4, 50)
    with pytest.raises(FileNotFoundError):  # both argument checks passed: the failure is the missing checkpoint
        sr.main(argv)


def test_cli_stream_beam_needs_streaming():
    with pytest.raises(ValueError, match="--streaming"):
        _main(["--search", "transducer_stream_beam"])


@pytest.mark.parametrize("extra,named", [
    (["--hotwords", "h.txt"], "--hotwords"), (["--ngram-lm", "lm.arpa"], "--ngram-lm"), (["--word-dict", "w.txt"], "--word-dict"),
    (["--lm-path", "lm.pt", "--word-dict", "w.txt"], "--word-dict"), (["--lm-path", os.pathsep.join(["sub.pt", "word.pt"])], "--lm-path"),
    (["--print-alignment", "--results-path", "res"], "--print-alignment"), (["--print-alignment"], "--print-alignment"),
    (["--path", os.pathsep.join(["a.pt", "b.pt"])], "ensembles")])
def test_cli_stream_beam_refusals(extra, named):
    """Every combination the streamed search does not implement raises, by name, before a file is opened."""
    with pytest.raises(NotImplementedError, match=named):
        _main(["--streaming", "--search", "transducer_stream_beam", *extra])


@pytest.mark.parametrize("extra,exc,named", [
    (["--streaming", "--search", "transducer_frame_beam"], NotImplementedError, "--streaming"),
    (["--streaming", "--search", "ctc", "--lm-path", "lm.pt"], NotImplementedError, "--lm-path"),
    (["--streaming", "--search", "transducer_greedy", "--lm-path", "lm.pt"], NotImplementedError, "--lm-path"),
    (["--streaming", "--search", "ctc", "--stream-partials"], NotImplementedError, "--stream-partials"),
    (["--streaming", "--search", "transducer_greedy", "--stream-partials"], NotImplementedError, "--stream-partials"),
    (["--streaming", "--search", "transducer_beam"], NotImplementedError, "--search transducer_beam"),
    (["--search", "transducer_stream_beam", "--stream-partials"], ValueError, "--streaming"),
    (["--search", "ctc", "--transducer-beam-size-token", "3"], ValueError, "--transducer-beam-size-token")])
def test_cli_pinned_refusals_stay(extra, exc, named):
    with pytest.raises(exc, match=named):
        _main(extra)


def test_decoder_argument_validation():
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder as D
    from tests.test_transducer_frame_beam import _dictionary

    d = _dictionary(8)
    dec = D(None, d, 4, max_streams=2, max_frames=10, nbest=2)
    assert (dec.beam_size, dec.beam_size_token, dec.nbest, dec.blank, dec.bos, dec.pad) == (4, 4, 2, d.bos(), d.eos(), d.pad())
    for kw in (dict(beam_size=65), dict(beam_size=4, nbest=5), dict(beam_size=4, beam_size_token=0), dict(beam_size=4, temperature=0.0),
               dict(beam_size=4, max_streams=0), dict(beam_size=4, max_frames=0)):
        a = dict(max_streams=2, max_frames=10)
        a.update(kw)
        with pytest.raises(ValueError):
            D(None, d, **a)
    with pytest.raises(NotImplementedError, match="ensembles"):
        D([None, None], d, 4, max_streams=2, max_frames=10)
    dec.open(["a", "b"])
    with pytest.raises(ValueError, match="already open"):
        dec.open(["a"])
    with pytest.raises(RuntimeError, match="slots"):
        dec.open(["c"])
    with pytest.raises(ValueError, match="max_frames"):  # refused before anything is launched (there is no device here)
        dec.accept(["a", "b"], torch.zeros(12, 4), [1, 11])
    assert [dec.streams[s][1] for s in ("a", "b")] == [0, 0]


def state_words(max_frames, beam):
    """The documented formula (include/espresso_amd.h)."""
    cap = 1 + max_frames * beam
    tsize = 64
    while tsize < 2 * cap:
        tsize *= 2
    w = 3 * tsize + 5 * beam + 2 + 2 * cap + 2 * beam + 2 * beam * 64
    return 2 + w + (w & 1)


def test_state_bytes_formula():
    from espresso_amd import _lib

    try:
        lib = _lib.lib()
    except _lib.EspressoAmdLibraryError:
        pytest.skip("the library is not built")
    for mf, beam in [(1, 1), (7, 3), (100, 5), (250, 10), (1000, 64), (33, 16)]:
        assert lib.ea_rnnt_frame_beam_stream_state_bytes(mf, beam) == 4 * state_words(mf, beam)
        assert lib.ea_rnnt_frame_beam_stream_state_bytes(mf, beam) == lib.ea_rnnt_frame_beam_workspace_bytes(1, mf, beam) + 8
    assert lib.ea_rnnt_frame_beam_stream_state_bytes(10, 65) == 0
    assert lib.ea_rnnt_frame_beam_stream_state_bytes(0, 4) == 0 and lib.ea_rnnt_frame_beam_stream_state_bytes(10, 0) == 0


# ---------------------------------------------------------------------------------------------------------------- GPU
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


def _triples_out(N):
    return (torch.empty(N, dtype=torch.int32, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV),
            torch.empty(N, dtype=torch.uint8, device=DEV))


class _CaseRows:
    """The logits (and LM) rows of every (utterance, frame) of a case: the table model's rows of the oracle's live hypotheses,
    NaN for dead beam slots (a kernel that read one would not match), with a row stride larger than V."""

    def __init__(self, c):
        self.c, o = c, c["opts"]
        self.V, self.beam, self.K = c["V"], c["beam"], c["K"]
        self.lens = _lens(c)
        self.B, self.T = len(self.lens), max(self.lens)
        self.table, self.lm = _case_models(c)
        self.nlm = self.lm.n if self.lm is not None else 0
        self.step_kw = dict(eos=EOS if o.get("predicts_eos") else -1, temperature=o.get("temperature", 1.0),
                            lm_weight=o.get("lm_weight", 0.0), lm_no_blank=o.get("lm") == "no_blank")
        self.normalize = o.get("normalize", True)
        self.nbest = min(self.beam, 3)
        self.refs = [_case_oracle(c, self.table, self.lm, b, self.nbest) for b in range(self.B)]
        self.margin = min(r[2] for r in self.refs)
        self.logits, self.lm_rows, self.seqs = {}, {}, {}
        for b, L in enumerate(self.lens):
            seqs = [()]
            for t in range(L):
                x = np.full((self.beam, self.V + 3), np.nan, dtype=np.float32)
                m = np.full((self.beam, self.nlm), np.nan, dtype=np.float32)
                for j, y in enumerate(seqs):
                    x[j, : self.V] = self.table.row(b, t, y)
                    if self.lm is not None:
                        m[j] = self.lm.row(y)
                self.logits[b, t], self.lm_rows[b, t], self.seqs[b, t] = x, m, seqs
                seqs = [seqs[p] + (() if k else (v,)) for p, v, k in self.refs[b][1][t]]
            self.seqs[b, L] = seqs

    def rows(self, frames):
        """Device (logits [n*beam][V] view of a wider tensor, lm_rows or None) of the listed (utterance, frame or None) pairs."""
        nan_x = np.full((self.beam, self.V + 3), np.nan, dtype=np.float32)
        nan_m = np.full((self.beam, self.nlm), np.nan, dtype=np.float32)
        x = np.concatenate([self.logits.get(f, nan_x) if f[1] is not None else nan_x for f in frames])
        m = np.concatenate([self.lm_rows.get(f, nan_m) if f[1] is not None else nan_m for f in frames])
        return torch.from_numpy(x).to(DEV)[:, : self.V], (torch.from_numpy(m).to(DEV) if self.lm is not None else None)

    def live(self, b, t):
        """The oracle's live beam of utterance b after its first t frames, and the margin of that search."""
        o = self.c["opts"]
        kw = dict(lm_fn=self.lm, lm_weight=o.get("lm_weight", 0.0), eos=EOS, predicts_eos=o.get("predicts_eos", False),
                  temperature=o.get("temperature", 1.0))
        return live_beam(self.table.logits_fn(b), t, self.beam, self.K, **kw)


def _offline(r):
    """The offline kernels over the case: per frame the triples [B][beam][3] (parent as a beam slot), and after every frame
    count 0 .. T the finish tensors (the finish reads the workspace only: after step t it is the search over t + 1 frames)."""
    from espresso_amd import kernels as Kn

    B, T, V, beam = r.B, r.T, r.V, r.beam
    ws = Kn.rnnt_frame_beam_workspace(B, T, beam, DEV)
    in_len = torch.tensor(r.lens, dtype=torch.int32, device=DEV)
    out = _triples_out(B * beam)
    row0 = (torch.arange(B, device=DEV, dtype=torch.int32) * beam).repeat_interleave(beam)
    triples = []
    # no frame yet: the empty hypothesis with score 0 (what the offline search returns for an utterance without frames)
    scores0 = torch.full((B, r.nbest), -math.inf, device=DEV)
    scores0[:, 0] = 0.0
    fins = [(torch.full((B, r.nbest, T), PAD, dtype=torch.int32, device=DEV), torch.zeros(B, r.nbest, dtype=torch.int32, device=DEV),
             scores0, torch.ones(B, dtype=torch.int32, device=DEV))]
    for t in range(T):
        x, m = r.rows([(b, t if t < r.lens[b] else None) for b in range(B)])
        Kn.rnnt_frame_beam_step(x, in_len, ws, out, B, T, V, beam, r.K, BLANK, t, lm_rows=m, **r.step_kw)
        triples.append(torch.stack([out[0] - row0, out[1], out[2].to(torch.int32)], 1).view(B, beam, 3).clone())
        fins.append(tuple(a.clone() for a in Kn.rnnt_frame_beam_finish(ws, B, T, beam, r.nbest, PAD, normalize=r.normalize)))
    return triples, fins


def _streamed_session(r, offline, max_frames, max_streams, seed, check_partials=False):
    """The streamed kernels over the case in uneven pieces, streams in shuffled slots of a larger buffer, some entries idle;
    every triple, every mid-stream finish and the final finish must equal the offline kernels' bit for bit.  Returns the number
    of partial checkpoints compared on scores and the worst |partial score - oracle|."""
    from espresso_amd import kernels as Kn

    triples, fins = offline
    B, T, V, beam = r.B, r.T, r.V, r.beam
    rng = np.random.default_rng(seed)
    slot_of = rng.permutation(max_streams)[:B].tolist()
    state, nbytes = Kn.rnnt_frame_beam_stream_state(max_streams, max_frames, beam, DEV)
    state.fill_(0xA5)  # any contents: the reset initialises
    Kn.rnnt_frame_beam_stream_reset(state, torch.tensor(slot_of, dtype=torch.int32, device=DEV), max_frames, beam)
    pos = [0] * B
    pieces = [1, 3, 2, 5, 1, 4]
    rounds, compared, worst = 0, 0, 0.0

    def readouts(entries):
        nonlocal compared, worst
        slots = torch.tensor([slot_of[b] for b in entries], dtype=torch.int32, device=DEV)
        before = state.clone()
        fin = Kn.rnnt_frame_beam_stream_finish(state, slots, max_frames, beam, r.nbest, PAD, T, normalize=r.normalize)
        fin2 = Kn.rnnt_frame_beam_stream_finish(state, slots, max_frames, beam, r.nbest, PAD, T, normalize=r.normalize)
        par = Kn.rnnt_frame_beam_stream_partial(state, slots, max_frames, beam, PAD, T)
        par2 = Kn.rnnt_frame_beam_stream_partial(state, slots, max_frames, beam, PAD, T)
        assert torch.equal(state, before)  # both readouts leave the state alone
        assert all(torch.equal(a, b_) for a, b_ in zip(fin + par, fin2 + par2))
        for e, b in enumerate(entries):
            want = fins[pos[b]]
            for got, w in zip(fin, want):  # tokens, lengths, scores, nhyp of the offline search over the frames so far
                assert torch.equal(got[e], w[b]), (b, pos[b], got[e], w[b])
        if check_partials:
            toks, lens_, scores, stable = (t.cpu() for t in par)
            for e, b in enumerate(entries):
                hyps, margin = r.live(b, pos[b])
                y, k, s = partial_oracle(hyps)
                assert tuple(toks[e, : int(lens_[e])].tolist()) == y and int(stable[e]) == k, (b, pos[b], toks[e], stable[e], y, k)
                assert bool((toks[e, int(lens_[e]):] == PAD).all())
                if margin > 10 * SCORE_TOL:
                    compared += 1
                    worst = max(worst, abs(float(scores[e]) - s))

    readouts(list(range(B)))  # before any frame: the empty hypothesis
    while any(pos[b] < r.lens[b] for b in range(B)):
        entries = [b for b in rng.permutation(B).tolist() if rng.random() < 0.8]
        if not entries:
            continue
        n_new = [min(pieces[(rounds + 2 * b) % len(pieces)], r.lens[b] - pos[b]) if rng.random() < 0.85 else 0 for b in entries]
        rounds += 1
        slot_idx = torch.tensor([slot_of[b] for b in entries], dtype=torch.int32, device=DEV)
        nn = torch.tensor(n_new, dtype=torch.int32, device=DEV)
        out = _triples_out(len(entries) * beam)
        idle_before = {b: state[slot_of[b]].clone() for b, c in zip(entries, n_new) if c == 0}
        for j in range(max(n_new)):
            x, m = r.rows([(b, pos[b] + j if j < c else None) for b, c in zip(entries, n_new)])
            Kn.rnnt_frame_beam_stream_step(x, slot_idx, nn, j, state, out, max_frames, V, beam, r.K, BLANK, lm_rows=m, **r.step_kw)
            got = torch.stack([out[0], out[1], out[2].to(torch.int32)], 1).view(len(entries), beam, 3).clone()
            for e, (b, c) in enumerate(zip(entries, n_new)):
                got[e, :, 0] -= e * beam
                if j < c:
                    assert torch.equal(got[e], triples[pos[b] + j][b]), (b, pos[b] + j, got[e], triples[pos[b] + j][b])
                else:
                    ident = torch.tensor([[s, BLANK, 1] for s in range(beam)], dtype=torch.int32, device=DEV)
                    assert torch.equal(got[e], ident), (b, j, got[e])
        for b, c in zip(entries, n_new):
            pos[b] += c
        for b, before in idle_before.items():
            assert torch.equal(state[slot_of[b]], before), b
        readouts(entries)
    assert pos == r.lens
    readouts(list(range(B)))
    # the frame counters on the device are the frames fed
    heads = state.view(torch.int32).view(max_streams, -1)[:, 0].cpu().tolist()
    assert [heads[slot_of[b]] for b in range(B)] == r.lens
    return compared, worst


@pytest.mark.gpu
@pytest.mark.parametrize("c", STREAM_CASES, ids=_case_id)
def test_streamed_kernels_equal_offline_bit_for_bit(c):
    """Per-frame triples, the finish after every piece (tokens, lengths, nhyp, scores) and the final finish: torch.equal with
    the offline kernels on the same table logits, for a state sized for exactly the longest utterance and for a larger one;
    the offline results themselves against the float64 oracle within SCORE_TOL (margin precondition > 10 x SCORE_TOL).

    Measured on an MI355X: every comparison equal; max |score - oracle| over the cases 2.1e-6."""
    _need_gpu()
    r = _CaseRows(c)
    assert r.margin > 10 * SCORE_TOL, r.margin
    offline = _offline(r)
    for max_frames, max_streams, seed in [(r.T, r.B + 3, 1), (r.T + 9, r.B + 1, 2)]:
        _streamed_session(r, offline, max_frames, max_streams, seed)
    tokens, lengths, scores, nhyp = (t.cpu() for t in offline[1][-1])
    worst = 0.0
    for b, (ref, _, _) in enumerate(r.refs):
        got = [(tuple(tokens[b, i, : int(lengths[b, i])].tolist()), float(scores[b, i])) for i in range(int(nhyp[b]))]
        assert [y for y, _ in got] == [y for y, _ in ref], (b, got, ref)
        worst = max([worst] + [abs(s - q) for (_, s), (_, q) in zip(got, ref)])
    print(f"{_case_id(c)}: oracle margin {r.margin:.3g}, max |score - oracle| {worst:.2e}")
    assert worst < SCORE_TOL, worst


PARTIAL_CASES = [c for c in STREAM_CASES if c["V"] == 20] + [c for c in STREAM_CASES if _case_id(c) == "V5004-b4-K4"]


@pytest.mark.gpu
@pytest.mark.parametrize("c", PARTIAL_CASES, ids=_case_id)
def test_partials_equal_the_oracle(c):
    """After every piece: the best live hypothesis and stable_len are the oracle's; where the oracle's margin over the frames so
    far is clear, the score within SCORE_TOL.  (The mid-stream finish and the read-only property are asserted in the same
    session, as in the bit-for-bit test.)"""
    _need_gpu()
    r = _CaseRows(c)
    compared, worst = _streamed_session(r, _offline(r), r.T + 2, r.B + 2, 5, check_partials=True)
    print(f"{_case_id(c)}: {compared} partial checkpoints compared on scores, max |score - oracle| {worst:.2e}")
    assert compared > 0 and worst < SCORE_TOL, (compared, worst)


@pytest.mark.gpu
def test_untouched_slots_and_bad_arguments():
    """n_new = 0, a slot out of range and a full slot: the state bytes stay as they are and the triple is the identity; bad
    arguments are refused with -2 (a RuntimeError naming the entry point)."""
    _need_gpu()
    from espresso_amd import kernels as Kn

    V, beam, K, mf, S = 20, 4, 3, 2, 3
    table = TableModel(V, 0, blank=BLANK)
    state, nbytes = Kn.rnnt_frame_beam_stream_state(S, mf, beam, DEV)
    assert nbytes == 4 * state_words(mf, beam) == state.shape[1]
    Kn.rnnt_frame_beam_stream_reset(state, torch.tensor([0, 1, 2, 7, -1], dtype=torch.int32, device=DEV), mf, beam)  # 7, -1: skipped
    x = torch.from_numpy(np.stack([table.row(0, 0, ())] * (3 * beam))).to(DEV)
    out = _triples_out(3 * beam)
    ident = lambda e: [(e * beam + s, BLANK, 1) for s in range(beam)]  # noqa: E731
    trip = lambda: list(zip(*(o.cpu().tolist() for o in out)))  # noqa: E731

    def step(slots, n_new, j):
        Kn.rnnt_frame_beam_stream_step(x, torch.tensor(slots, dtype=torch.int32, device=DEV), torch.tensor(n_new, dtype=torch.int32, device=DEV),
                                       j, state, out, mf, V, beam, K, BLANK)

    before = state.clone()
    step([0, 5, 2], [0, 1, 1], 0)  # idle, out of range, active
    got = trip()
    assert got[:beam] == ident(0) and got[beam:2 * beam] == ident(1) and got[2 * beam:] != ident(2)
    assert torch.equal(state[:2], before[:2]) and not torch.equal(state[2], before[2])
    step([2, 0, 1], [2, 0, 1], 1)  # j = 1: only the first entry is due
    got = trip()
    assert got[beam:2 * beam] == ident(1) and got[2 * beam:] == ident(2)
    assert torch.equal(state[:2], before[:2])
    heads = lambda: state.view(torch.int32).view(S, -1)[:, 0].cpu().tolist()  # noqa: E731
    assert heads() == [0, 0, 2]
    full = state.clone()
    step([2, -3, 1], [1, 1, 0], 0)  # slot 2 is full (2 of 2 frames), a negative slot, idle
    assert trip() == ident(0) + ident(1) + ident(2) and torch.equal(state, full) and heads() == [0, 0, 2]

    slots = torch.tensor([0], dtype=torch.int32, device=DEV)
    for kw in (dict(K=V), dict(blank=V), dict(eos=BLANK), dict(temperature=0.0), dict(j=-1)):
        a = dict(K=K, blank=BLANK, j=0)
        a.update(kw)
        j = a.pop("j")
        with pytest.raises(RuntimeError, match="ea_rnnt_frame_beam_stream_step"):
            Kn.rnnt_frame_beam_stream_step(x[:beam], slots, slots, j, state, _triples_out(beam), mf, V, beam, **a)
    with pytest.raises(RuntimeError, match="device tensors"):
        Kn.rnnt_frame_beam_stream_step(x[:beam].cpu(), slots, slots, 0, state, _triples_out(beam), mf, V, beam, K, BLANK)
    with pytest.raises(RuntimeError, match="ea_rnnt_frame_beam_stream_finish"):
        Kn.rnnt_frame_beam_stream_finish(state, slots, mf, beam, beam + 1, PAD, 4)
    par = Kn.rnnt_frame_beam_stream_partial(state, torch.tensor([9, 0], dtype=torch.int32, device=DEV), mf, beam, PAD, 3)
    assert par[1].tolist() == [0, 0] and par[3].tolist() == [0, 0] and par[2].tolist() == [-math.inf, 0.0]
    # a slot that does not exist has no hypothesis
    fin = Kn.rnnt_frame_beam_stream_finish(state, torch.tensor([9], dtype=torch.int32, device=DEV), mf, beam, 2, PAD, 3)
    assert int(fin[3][0]) == 0 and bool((fin[0] == PAD).all()) and float(fin[2].max()) == -math.inf
    assert torch.equal(state, full)


# ------------------------------------------------------------------------------------------ the decoder on a chunk transducer
def _chunk_transducer():
    from tests.gpu_checks import _Task
    from tests.streaming_checks import build_chunk_transducer

    model, g = build_chunk_transducer()
    d = _Task(40).target_dictionary
    feats, lengths = torch.from_numpy(g["feats"]).to(DEV), g["lengths"].tolist()
    rows = []
    with torch.no_grad():
        for b in range(feats.shape[0]):
            n = torch.tensor([lengths[b]], device=DEV)
            rows.append(model.encoder(feats[b:b + 1, : lengths[b]], n)["_x_bt"][0])
    return model, d, rows


def _hyp_list(out, b=0):
    tokens, lengths, scores, nhyp = (t.cpu() for t in out)
    return [(tuple(tokens[b, i, : int(lengths[b, i])].tolist()), float(scores[b, i])) for i in range(int(nhyp[b]))]


def _stream_rows(dec, rows, pieces, max_live):
    """Several streams interleaved and opened at different times (one more per round), each fed `pieces` in turn."""
    pos, results, live, pending, k = {}, {}, [], list(range(len(rows))), 0
    while pending or live:
        if pending and len(live) < max_live:
            b = pending.pop(0)
            dec.open([b])
            live.append(b)
            pos[b] = 0
        counts = [min(pieces[(k + b) % len(pieces)], rows[b].shape[0] - pos[b]) for b in live]
        dec.accept(list(live), torch.cat([rows[b][pos[b]:pos[b] + c] for b, c in zip(live, counts)]), counts)
        for b, c in zip(list(live), counts):
            pos[b] += c
            if pos[b] >= rows[b].shape[0]:
                h = dec.close(b)
                results[b] = [(tuple(x["tokens"].tolist()), float(x["score"])) for x in h]
                live.remove(b)
        k += 1
    return results


@pytest.mark.gpu
@pytest.mark.parametrize("beam,lm_weight,lm_seed", [(4, 0.0, None), (4, 0.3, 1)])
def test_decoder_equals_offline_search(beam, lm_weight, lm_seed):
    """The offline encoder rows fed in two piece patterns, several streams interleaved: token sequences and n-best order equal
    TransducerFrameBeamDecoder.search on the same rows; scores within SCORE_TOL + 8 x TERM_TOL x terms (one term per frame, two
    with an LM).  An utterance whose offline oracle margin (the oracle on the same GPU modules, one row at a time) is below
    twice the bound is compared on scores only, and at most one may be.  The measured difference is printed.

    Measured on an MI355X: max |streamed - offline score| 0.0 with and without the LM; smallest oracle margin 5.9e-4 without and
    1.4e-3 with the LM (twice the bound is at most 4.7e-4 and 7.5e-4, at 18 frames): no utterance was compared on scores only."""
    _need_gpu()
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder
    from tests.test_ctc_prefix_beam import _tiny_lm
    from tests.test_transducer_frame_beam import _OneRowModel

    model, d, rows = _chunk_transducer()
    lm = _tiny_lm(d, seed=lm_seed).to(DEV) if lm_weight else None
    kw = dict(nbest=3, normalize_scores=False, lm_model=lm, lm_weight=lm_weight)
    off = TransducerFrameBeamDecoder([model], d, beam_size=beam, **kw)
    want, margins, bounds = [], [], []
    for b, x in enumerate(rows):
        E = model.joint_encoder_branch(x).view(1, x.shape[0], -1)
        want.append(_hyp_list(off.search(E, torch.tensor([x.shape[0]], device=DEV))))
        one = _OneRowModel(off, E)
        margins.append(frame_beam_oracle(one.logits_fn(0), x.shape[0], beam, off.beam_size_token, off.blank, lm_fn=one.lm_fn if lm else None,
                                         lm_weight=lm_weight, normalize=False, nbest=off.nbest)[2])
        bounds.append(SCORE_TOL + 8 * TERM_TOL * x.shape[0] * (2 if lm else 1))
    assert sum(len(w[0][0]) for w in want) > 0  # (something was recognised)
    worst, on_scores_only = 0.0, set()
    for pieces in ([3, 5, 1], [2, 7]):
        dec = StreamingTransducerFrameBeamDecoder(model, d, beam, max_streams=2, max_frames=max(x.shape[0] for x in rows) + 1, **kw)
        got = _stream_rows(dec, rows, pieces, max_live=2)
        assert not dec.streams and sorted(dec._free) == [0, 1]
        for b in range(len(rows)):
            if margins[b] < 2 * bounds[b]:
                on_scores_only.add(b)
                near = [s for y, s in want[b] if y == got[b][0][0]]
                assert near and abs(near[0] - got[b][0][1]) < bounds[b], (b, got[b], want[b])
                continue
            assert [y for y, _ in got[b]] == [y for y, _ in want[b]], (b, pieces, got[b], want[b])
            worst = max([worst] + [abs(s - q) for (_, s), (_, q) in zip(got[b], want[b])])
            assert worst < bounds[b], (b, worst, bounds[b])
    print(f"beam {beam} lm {lm_weight}: oracle margins {[f'{m:.3g}' for m in margins]}, max |streamed - offline score| {worst:.2e}")
    assert len(on_scores_only) <= 1, on_scores_only


@pytest.mark.gpu
def test_decoder_beam1_equals_streaming_greedy():
    _need_gpu()
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder
    from espresso_amd.tools.streaming_transducer_greedy_decoder import StreamingTransducerGreedyDecoder

    model, d, rows = _chunk_transducer()
    dec = StreamingTransducerFrameBeamDecoder(model, d, 1, max_streams=3, max_frames=max(x.shape[0] for x in rows))
    got = _stream_rows(dec, rows, [3, 5, 1], max_live=3)
    n_tok = 0
    for b, x in enumerate(rows):
        greedy = StreamingTransducerGreedyDecoder(model, d, max_num_expansions_per_step=1)
        greedy.open([b])
        greedy.accept([b], x, [x.shape[0]])
        want = [t for t in greedy.close(b)["tokens"].tolist() if t != greedy.blank]
        assert list(got[b][0][0]) == want, (b, got[b], want)
        n_tok += len(want)
    assert n_tok > 0


@pytest.mark.gpu
@pytest.mark.parametrize("with_lm", [False, True])
def test_accept_does_not_synchronise(with_lm, monkeypatch):
    """After a warm-up, accept runs under set_sync_debug_mode("error"); a stream that would pass max_frames raises ValueError
    before anything is launched and every stream goes on as if nothing had happened."""
    _need_gpu()
    from espresso_amd import kernels
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder
    from tests.test_ctc_prefix_beam import _tiny_lm

    model, d, rows = _chunk_transducer()
    lm = _tiny_lm(d, seed=3).to(DEV) if with_lm else None
    mf = max(x.shape[0] for x in rows)
    kw = dict(nbest=2, lm_model=lm, lm_weight=0.3)
    ref_dec = StreamingTransducerFrameBeamDecoder(model, d, 4, max_streams=3, max_frames=mf, **kw)
    ref = _stream_rows(ref_dec, rows, [4], max_live=3)  # (also the warm-up of the cached bf16 weights)
    dec = StreamingTransducerFrameBeamDecoder(model, d, 4, max_streams=3, max_frames=mf, **kw)
    assert dec.state_bytes_per_stream() == dec.state.shape[1] == 4 * state_words(mf, 4)
    ids = [0, 1, 2]
    dec.open(ids)
    dec.accept(ids, torch.cat([rows[b][:2] for b in ids]), [2, 2, 2])  # warm-up: the reset of the opened slots
    counts = [rows[0].shape[0] - 2, 0, 3]
    fed = torch.cat([rows[b][2:2 + c] for b, c in zip(ids, counts)])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        assert dec.accept(ids, fed, counts) is None
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert [dec.streams[b][1] for b in ids] == [rows[0].shape[0], 2, 5]
    calls = []
    for name in ("rnnt_frame_beam_stream_step", "rnnt_frame_beam_stream_reset", "gather_rows", "gemm"):
        real = getattr(kernels, name)
        monkeypatch.setattr(kernels, name, lambda *a, _r=real, **k: calls.append(1) or _r(*a, **k))
    over = mf - dec.streams[0][1] + 1  # one frame more than stream 0 has room for (refused before the rows are looked at)
    with pytest.raises(ValueError, match="max_frames"):
        dec.accept(ids, torch.zeros(over + 2, rows[0].shape[1], dtype=rows[0].dtype, device=DEV), [over, 1, 1])
    assert not calls and [dec.streams[b][1] for b in ids] == [rows[0].shape[0], 2, 5]
    monkeypatch.undo()
    for b in (1, 2):
        dec.accept([b], rows[b][dec.streams[b][1]:], [rows[b].shape[0] - dec.streams[b][1]])
    part = dec.partial(ids)
    for b in ids:
        mid = dec.finish(b)
        h = [(tuple(x["tokens"].tolist()), float(x["score"])) for x in dec.close(b)]
        assert [(tuple(x["tokens"].tolist()), float(x["score"])) for x in mid] == h  # finish leaves the stream as it is
        assert [y for y, _ in h] == [y for y, _ in ref[b]], (b, h, ref[b])
        bound = SCORE_TOL + 8 * TERM_TOL * rows[b].shape[0] * (2 if with_lm else 1)
        assert all(abs(s - q) < bound for (_, s), (_, q) in zip(h, ref[b]))
        toks, k, _ = part[b]
        assert 0 <= k <= len(toks) and all(tuple(toks[:k]) == y[:k] for y, _ in h), (b, part[b], h)


# ------------------------------------------------------------------------------------------ end to end
def _write_wav(path, samples):
    import wave

    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(samples, -32768, 32767).astype("<i2").tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("with_lm", [False, True])
def test_cli_streaming_beam_end_to_end(tmp_path, capsys, with_lm):
    """speech_recognize --streaming --search transducer_stream_beam --stream-partials on synthetic WAVs with a small random
    chunk-streaming transducer checkpoint (with_lm: also --lm-path, an LM of the registered lstm_lm_wsj architecture with small
    random weights, --lm-weight 0.3): one H- line per utterance and hypothesis, equal in text to the offline run of
    --search transducer_frame_beam on the same checkpoint (one utterance per batch: a padded batch is not the utterance
    alone) and to StreamingEncoder + the decoder called directly with another piece size; scores within the bound of the
    decoder test.  The stable text of every P- line prefixes the final H- text."""
    _need_gpu()
    from espresso_amd import registry
    from espresso_amd import speech_recognize as sr
    from espresso_amd.data.audio_utils import read_wav
    from espresso_amd.models.transformer.streaming_encoder import StreamingEncoder
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder
    dict_path = str(tmp_path / "dict.txt")
    open(dict_path, "w").write("".join(f"t{i} 1\n" for i in range(20)))
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(dict=dict_path, autoregressive=False,
                                                                                    criterion_name="transducer_loss"))
    d = task.target_dictionary
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
    utts = [f"utt{i}" for i in range(3)]
    with open(tmp_path / "wav.scp", "w") as f:
        for i, u in enumerate(utts):
            p = str(tmp_path / f"{u}.wav")
            _write_wav(p, rng.standard_normal(int(16000 * (0.9 + 0.7 * i))) * 3000)
            f.write(f"{u} {p}\n")
    opts = ["--beam", "4", "--nbest", "2", "--transducer-beam-size-token", "3"]
    lm = None
    if with_lm:  # an LM of a registered architecture (the CLI rebuilds it from --lm-arch), small random weights
        from espresso_amd.models.lstm_lm import LSTMLanguageModelEspresso

        class _LMTask:
            target_dictionary = source_dictionary = d

        torch.manual_seed(1)
        lm = LSTMLanguageModelEspresso.build_model(dict(arch="lstm_lm_wsj", is_wordlm=False), _LMTask)
        with torch.no_grad():
            for p_ in lm.parameters():
                p_.uniform_(-0.1, 0.1)
            lm.decoder.embed_tokens.weight[d.pad()] = 0.0
        torch.save(lm.state_dict(), str(tmp_path / "lm.pt"))
        lm = lm.to(DEV).eval()
        opts += ["--lm-path", str(tmp_path / "lm.pt"), "--lm-arch", "lstm_lm_wsj", "--lm-weight", "0.3"]
    base = ["--path", str(tmp_path / "model.pt"), "--dict", dict_path, "--wav-scp", str(tmp_path / "wav.scp")] + opts

    def run(extra):
        capsys.readouterr()
        sr.main(base + extra)
        out = capsys.readouterr().out.splitlines()
        lines = {}
        for l in out:
            if l.startswith("H-"):
                lines.setdefault(l.split("\t")[0][2:], []).append(l.split("\t")[1:])
        return lines, [l.split("\t") for l in out if l.startswith("P-")]

    waves = [read_wav(str(tmp_path / f"{u}.wav")) for u in utts]
    model = model.to(DEV).eval()
    offline, _ = run(["--search", "transducer_frame_beam", "--batch-size", "1"])
    streamed, partial_lines = run(["--search", "transducer_stream_beam", "--streaming", "--stream-chunk-ms", "170", "--streams", "2",
                                   "--stream-partials"])
    assert set(offline) == set(utts)
    assert set(streamed) == set(utts)

    # the direct call: StreamingEncoder + the decoder, another piece size
    task.build_frontend(torch.device(DEV))
    se = StreamingEncoder(model, 3, frontend=task.frontend)
    max_frames = max(-(-task.frontend.num_frames(len(w)) // se.stride) for w in waves)
    dec = StreamingTransducerFrameBeamDecoder(model, d, 4, max_streams=3, max_frames=max_frames, nbest=2, beam_size_token=3,
                                              lm_model=lm, lm_weight=0.3 if with_lm else 0.0)
    ids = list(range(len(utts)))
    se.open(ids)
    dec.open(ids)
    pos, direct, piece = [0] * len(utts), {}, 3700
    while len(direct) < len(utts):
        live = [i for i in ids if i not in direct]
        ws = [torch.from_numpy(np.ascontiguousarray(waves[i][pos[i]:pos[i] + piece])).float() for i in live]
        fin = [pos[i] + piece >= len(waves[i]) for i in live]
        y, counts = se.accept_waveform(live, ws, fin)
        if y is not None:
            dec.accept(live, y, counts)
        for i, f in zip(live, fin):
            pos[i] += piece
            if f:
                se.close([i])
                direct[i] = dec.close(i)
    worst = 0.0
    for i, u in enumerate(utts):
        frames = -(-task.frontend.num_frames(len(waves[i])) // se.stride)
        bound = (SCORE_TOL + 8 * TERM_TOL * frames * (2 if with_lm else 1)) / math.log(2)
        texts = [d.string(torch.tensor([t for t in h["tokens"].tolist() if t not in dec.symbols_to_strip_from_output])) for h in direct[i]]
        assert [t for t, _ in streamed[u]] == texts, (u, streamed[u], texts)
        for (_, s), h in zip(streamed[u], direct[i]):
            worst = max(worst, abs(float(s) - float(h["score"]) / math.log(2)))
            assert abs(float(s) - float(h["score"]) / math.log(2)) < bound, (u, s, h["score"])
        assert [t for t, _ in offline[u]] == [t for t, _ in streamed[u]], (u, offline[u], streamed[u])
        for (_, s), (_, q) in zip(streamed[u], offline[u]):
            worst = max(worst, abs(float(s) - float(q)))
            assert abs(float(s) - float(q)) < bound, (u, s, q)
    print(f"lm {with_lm}: H- texts {[streamed[u][0][0] for u in utts]}, max |score difference| (base 2) {worst:.2e}")
    assert partial_lines
    for tag, sec, stable, rest in partial_lines:
        final = streamed[tag[2:]][0][0].split()
        assert final[: len(stable.split())] == stable.split(), (tag, stable, final)
        assert float(sec) > 0
