"""Streamed lexicon + n-gram CTC beam search with partial results (tools/streaming_ctc_lexicon_beam_decoder.py, the
ea_ctc_lexicon_stream_* entries of csrc/ctc_lexicon_beam.hip, speech_recognize --streaming --search ctc_beam --ngram-lm).

tests/streaming_beam_ref.py restates the search step by step in float64.  The CPU tests pin it to prefix_beam_oracle and check
the stable-prefix properties on it; the GPU tests hold the streamed search to the offline kernel bit for bit, to the oracle
within SCORE_TOL, and the partial results to the step-wise oracle."""
import math
import os

import numpy as np
import pytest
import torch

from tests.ngram_ref import random_arpa
from tests.streaming_beam_ref import StepwiseBeamOracle
from tests.test_ctc_prefix_beam import _peaked, prefix_beam_oracle
from tests.test_ngram_lexicon_ctc import SCORE_TOL, _compare, _decoder, _hyps, _setup, _tables

DEV = "cuda:0"
pytestmark = [pytest.mark.filterwarnings("ignore:invalid value encountered in scalar subtract:RuntimeWarning"),
              pytest.mark.filterwarnings("ignore:invalid value encountered in subtract:RuntimeWarning")]
BEAMS = [(1, 1), (4, 4), (16, 4), (10, 6)]
SETTINGS = [(1.0, 0.0, 0.0), (0.5, -1.0, 0.3)]  # lm_weight, word_score, insertion_bonus


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


# ------------------------------------------------------------------------------------------------ a streaming session
class OracleStreams:
    """The streaming decoder's interface over one StepwiseBeamOracle per stream (float64, host)."""

    def __init__(self, make):
        self.make, self.streams = make, {}

    def open(self, ids):
        for i in ids:
            self.streams[i] = self.make()

    def accept_lprobs(self, ids, rows, counts):
        r = 0
        for i, c in zip(ids, counts):
            self.streams[i].feed(rows[r:r + c])
            r += c

    def close(self, i):
        return self.streams.pop(i)


def _session(dec, x, lens, rng, max_streams, whole=(), observe=None, finish=None):
    """Feed the utterances x[b, :lens[b]] through `dec` in random pieces: at most max_streams open at a time (slots are reused),
    streams join and leave at different times, a round takes only some of the open streams, pieces have 0, 1 or a few frames
    and the utterances in `whole` arrive in one piece.  observe(open ids) runs after every round; finish(b) just before a
    stream is closed, its value is returned per utterance.  The schedule depends on rng alone."""
    pending, live, results = list(range(len(lens))), {}, {}
    while pending or live:
        while pending and len(live) < max_streams and (not live or rng.random() < 0.6):
            b = pending.pop(0)
            dec.open([b])
            live[b] = 0
        ids = [b for b in live if rng.random() < 0.7] or [next(iter(live))]
        counts = []
        for b in ids:
            left = int(lens[b]) - live[b]
            counts.append(left if b in whole else min(left, int(rng.choice([0, 1, 1, 2, 3, 5]))))
        rows = [x[b, live[b]:live[b] + n] for b, n in zip(ids, counts)]
        dec.accept_lprobs(ids, torch.cat(rows) if torch.is_tensor(x) else np.concatenate(rows), counts)
        for b, n in zip(ids, counts):
            live[b] += n
        if observe is not None:
            observe(list(live))
        for b in list(live):
            if live[b] >= lens[b] and rng.random() < 0.7:
                results[b] = finish(b) if finish is not None else None
                dec.close(b)
                del live[b]
    return results


def _streaming_decoder(d, lm, trie, max_streams, max_frames, beam, K, nbest=1, alpha=1.0, beta=0.0, gamma=0.0):
    from espresso_amd.tools.streaming_ctc_lexicon_beam_decoder import StreamingCTCLexiconBeamDecoder

    return StreamingCTCLexiconBeamDecoder(d, lm, trie, max_streams, max_frames, beam_size=beam, nbest=nbest, beam_size_token=K,
                                          lm_weight=alpha, word_score=beta, insertion_bonus=gamma)


def _equal_to_offline(results, out):
    """Per utterance: the streamed finish (tokens [1][nbest][U], lengths, scores, nhyp) against row b of the offline search."""
    tokens, lengths, scores, nhyp = out
    for b, (tk, ln, sc, nh) in results.items():
        assert torch.equal(nh[0], nhyp[b]), (b, nh, nhyp[b])
        assert torch.equal(ln[0], lengths[b]), (b, ln, lengths[b])
        assert torch.equal(sc[0], scores[b]), (b, sc, scores[b])
        for i in range(tokens.shape[1]):
            n = int(lengths[b, i])
            assert torch.equal(tk[0, i, :n], tokens[b, i, :n]), (b, i, tk[0, i], tokens[b, i])


def _batched(results, B, nbest, T, pad):
    """The per-utterance streamed results as the offline search's batch tensors."""
    tokens = torch.full((B, nbest, T), pad, dtype=torch.int32)
    lengths = torch.zeros(B, nbest, dtype=torch.int32)
    scores = torch.full((B, nbest), -math.inf)
    nhyp = torch.zeros(B, dtype=torch.int32)
    for b, (tk, ln, sc, nh) in results.items():
        tokens[b, :, :tk.shape[2]] = tk[0].cpu()[:, :T]
        lengths[b], scores[b], nhyp[b] = ln[0].cpu(), sc[0].cpu(), nh[0].cpu()
    return tokens, lengths, scores, nhyp


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("mode", ["space", "wordstart"])
@pytest.mark.parametrize("beam,K", [(1, 1), (3, 2), (4, 4), (10, 6)])
def test_stepwise_oracle_equals_prefix_beam_oracle(mode, beam, K):
    """Fed any split of the frames, the step-wise oracle's n-best is that of prefix_beam_oracle: the same tokens, the scores
    and the margin equal as float64."""
    rng = np.random.default_rng(10 * beam + K)
    for alpha, beta, gamma in SETTINGS + [(2.0, 1.5, -0.2)]:
        d, words, text, spell, fus = _setup(mode, rng, alpha, beta)
        V, T = len(d), 13
        x = _peaked(rng, T, V, sharp=3.0, scale=1.5)
        nbest = min(beam, 3)
        ref, ref_margin = prefix_beam_oracle(x, T, beam, K, d.bos(), lm_fn=fus.lm_fn, lm_weight=1.0, bonus=gamma, eos=V, nbest=nbest)
        for split in ([T], [1] * T, [0, 5, 0, 1, 7], list(np.diff([0] + sorted(rng.integers(0, T + 1, 4).tolist()) + [T]))):
            o = StepwiseBeamOracle(beam, K, d.bos(), fus.lm_fn, lm_weight=1.0, bonus=gamma, eos=V)
            t = 0
            for n in split:
                o.feed(x[t:t + n])
                o.finish(nbest)  # a readout in between changes nothing
                o.partial()
                t += n
            assert t == T and o.frames == T
            got, margin = o.finish(nbest)
            assert got == ref, (split, got, ref)  # tuples of (tokens, float64 score): exact
            assert margin == ref_margin or (math.isnan(margin) and math.isnan(ref_margin))


@pytest.mark.parametrize("mode", ["space", "wordstart"])
def test_oracle_stable_prefix_properties(mode):
    """On random inputs: the stable prefix only grows, each value is a prefix of the next, of the best live hypothesis, and of
    every hypothesis of the final n-best with nbest = beam."""
    grew = 0
    for seed in range(6):
        rng = np.random.default_rng(50 + seed)
        alpha, beta, gamma = SETTINGS[seed % 2]
        d, words, text, spell, fus = _setup(mode, rng, alpha, beta)
        V, T = len(d), 24
        beam, K = [(4, 4), (10, 6), (2, 3)][seed % 3]
        x = _peaked(rng, T, V, sharp=4.0, scale=1.5)
        o = StepwiseBeamOracle(beam, K, d.bos(), fus.lm_fn, lm_weight=1.0, bonus=gamma, eos=V)
        seen = [()]
        for t in range(T):
            o.feed(x[t:t + 1])
            best, _, stable, _ = o.partial()
            assert stable[:len(seen[-1])] == seen[-1], (seed, t, seen[-1], stable)
            assert best[:len(stable)] == stable
            seen.append(stable)
        final = [y for y, s in o.finish(beam)[0] if s > -math.inf]
        for stable in seen:
            for y in final:
                assert y[:len(stable)] == stable, (seed, stable, y)
        grew += len(seen[-1]) > 0
    assert grew >= 3  # the property is not vacuous: the stable prefix does grow


def _partial_case(mode, beam, K, seed):
    rng = np.random.default_rng(seed)
    alpha, beta, gamma = SETTINGS[seed % 2]
    d, words, text, spell, fus = _setup(mode, rng, alpha, beta)
    B, T = 5, 16
    x = _peaked(rng, B * T, len(d), sharp=4.0, scale=1.5).reshape(B, T, len(d)).astype(np.float32)
    lens = np.array([T, 9, 0, T, 12])
    return d, text, spell, fus, x, lens, (alpha, beta, gamma)


def _oracle_checkpoints(mode, beam, K, seed, x_seen):
    """The step-wise oracle through the schedule of _partial_case: per checkpoint (round, stream) its partial."""
    d, text, spell, fus, x, lens, (alpha, beta, gamma) = _partial_case(mode, beam, K, seed)
    dec = OracleStreams(lambda: StepwiseBeamOracle(beam, K, d.bos(), fus.lm_fn, lm_weight=1.0, bonus=gamma, eos=len(d)))
    points = []
    _session(dec, x_seen.astype(np.float64), lens, np.random.default_rng(seed + 1), 3, whole=(3,),
             observe=lambda ids: points.append({b: dec.streams[b].partial() for b in ids}))
    return points


PARTIAL_CASES = [("space", 4, 4, 0), ("wordstart", 10, 6, 1), ("space", 10, 6, 3), ("wordstart", 4, 4, 2)]


@pytest.mark.parametrize("mode,beam,K,seed", PARTIAL_CASES)
def test_oracle_margins_allow_the_partial_comparison(mode, beam, K, seed):
    """At least half of the checkpoints of the GPU partial test have an oracle margin above SCORE_TOL (the oracle alone)."""
    x = _partial_case(mode, beam, K, seed)[4]
    points = [p for rnd in _oracle_checkpoints(mode, beam, K, seed, x) for p in rnd.values()]
    clear = sum(p[3] > SCORE_TOL for p in points)
    print(f"{mode} beam {beam} K {K}: {clear} of {len(points)} checkpoints above the margin")
    assert len(points) >= 20 and 2 * clear >= len(points)


def _main(argv):
    from espresso_amd import speech_recognize as sr

    return sr.main(["--path", "/nonexistent.pt", "--dict", "d", "--wav-scp", "w", *argv])


def test_cli_accepts_streaming_lexicon_beam_arguments():
    """--streaming --search ctc_beam --ngram-lm passes both argument checks: the failure is the missing checkpoint."""
    from espresso_amd import speech_recognize as sr

    argv = ["--path", "/nonexistent.pt", "--dict", "d", "--wav-scp", "w", "--device", "cpu", "--streaming", "--search", "ctc_beam", "--ngram-lm", "x",
            "--lexicon", "l", "--beam", "5", "--nbest", "2", "--lm-weight", "0.7", "--word-score", "-0.5", "--ctc-beam-size-token", "4",
            "--ctc-insertion-bonus", "0.1", "--stream-partials"]
    args = sr.get_parser().parse_args(argv)
    sr.check_ngram_args(args)
    sr.check_streaming_args(args)
    with pytest.raises(FileNotFoundError):
        sr.main(argv)


def test_cli_stream_partials_needs_streaming():
    with pytest.raises(ValueError, match="--stream-partials"):
        _main(["--search", "ctc_beam", "--ngram-lm", "x", "--stream-partials"])
    with pytest.raises(NotImplementedError, match="--stream-partials"):  # the greedy decoders have no partial readout
        _main(["--streaming", "--search", "ctc", "--stream-partials"])


@pytest.mark.parametrize("extra,match", [
    (["--search", "ctc_beam"], "--search ctc_beam.*--ngram-lm"),                                # scope: only the n-gram search
    (["--search", "ctc_beam", "--lm-path", "lm.pt"], "--ngram-lm"),                             # the LSTM-LM prefix beam is not streamed
    (["--search", "ctc_beam", "--ngram-lm", "x", "--lm-path", "lm.pt"], "--lm-path"),
    (["--search", "ctc_beam", "--ngram-lm", "x", "--word-dict", "w.txt"], "--word-dict"),
    (["--search", "ctc_beam", "--ngram-lm", "x", "--print-alignment", "--results-path", "r"], "--print-alignment"),
    (["--search", "beam"], "--search beam"), (["--search", "transducer_beam"], "--search transducer_beam"),
    (["--search", "ctc", "--ngram-lm", "x"], "ctc_beam"), (["--search", "transducer_greedy", "--ngram-lm", "x"], "ctc_beam"),
    (["--search", "ctc", "--lm-path", "lm.pt"], "--lm-path"),
])
def test_cli_streaming_refusals_stay(extra, match):
    with pytest.raises(NotImplementedError, match=match):
        _main(["--streaming", *extra])


def test_cli_streaming_refuses_ensembles():
    from espresso_amd import speech_recognize as sr

    with pytest.raises(NotImplementedError, match="ensembles"):
        sr.main(["--path", os.pathsep.join(["/nonexistent.pt", "/b.pt"]), "--dict", "d", "--wav-scp", "w", "--streaming", "--search",
                 "ctc_beam", "--ngram-lm", "x"])


# ---------------------------------------------------------------------------------------------------------------- GPU
def _run_streamed(d, lm, trie, xd, lens, seed, max_streams, max_frames, beam, K, nbest, alpha, beta, gamma, whole=(0,)):
    dec = _streaming_decoder(d, lm, trie, max_streams, max_frames, beam, K, nbest=nbest, alpha=alpha, beta=beta, gamma=gamma)
    res = _session(dec, xd, lens, np.random.default_rng(seed), max_streams, whole=whole,
                   finish=lambda b: tuple(t.clone() for t in dec.finish([b])))
    assert not dec.streams and sorted(dec._free) == list(range(max_streams))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["space", "wordstart"])
@pytest.mark.parametrize("beam,K", BEAMS)
def test_streamed_equals_offline_bit_for_bit(tmp_path, beam, K, mode, dtype):
    """The same log-probs once through CTCLexiconBeamSearchDecoder.search and once through the streaming decoder in random
    pieces (0- and 1-frame pieces, one utterance whole, 3 slots for 7 utterances, reused; a zero-frame stream): nhyp, lengths,
    scores and tokens are torch.equal, for two prefix-table sizes.  No tolerance: the frames run the same code."""
    _need_gpu()
    for k, (alpha, beta, gamma) in enumerate(SETTINGS):
        rng = np.random.default_rng(1000 * k + 10 * beam + K)
        d, words, text, spell, fus = _setup(mode, rng, alpha, beta)
        lm, trie = _tables(tmp_path, d, text, spell, mode)
        V, B, T = len(d), 7, 14
        x = _peaked(rng, B * T, V, sharp=3.0, scale=1.5).reshape(B, T, V)
        lens = np.array([T, 0, 1, 7, T, 10, 4], dtype=np.int32)
        xd = torch.from_numpy(x).to(DEV, dtype)
        nbest = min(beam, 3)
        off = _decoder(d, lm, trie, beam, K, nbest=nbest, alpha=alpha, beta=beta, gamma=gamma)
        out = off.search(xd, torch.from_numpy(lens).to(DEV))
        assert int(out[3][1]) == 0 and int(out[3].sum()) > 0
        for max_frames in (T, 3 * T + 5):
            res = _run_streamed(d, lm, trie, xd, lens, 7 + k + max_frames, 3, max_frames, beam, K, nbest, alpha, beta, gamma)
            assert sorted(res) == list(range(B))
            _equal_to_offline(res, out)
            assert int(res[1][3][0]) == 0  # the zero-frame stream


def _arpa_unigrams(probs):
    lines = ["\\data\\", f"ngram 1={len(probs) + 2}", "", "\\1-grams:", "-99\t<s>", "-0.5\t</s>"]
    return "\n".join(lines + [f"{p}\t{w}" for w, p in probs.items()] + ["", "\\end\\", ""])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_streamed_utterance_without_finite_hypothesis(tmp_path, dtype):
    """beam 1 follows 'a' into the word 'ab' and the utterance ends inside it: every hypothesis is -inf, nhyp is 0, streamed
    (frame by frame, in a reused slot) as offline; `close` then gives the empty -inf hypothesis of the offline generator."""
    _need_gpu()
    from espresso_amd.data.asr_dictionary import AsrDictionary

    d = AsrDictionary.from_symbols(list("abc"), enable_bos=True)
    V = len(d)
    x = np.full((2, 2, V), -9.0)
    x[:, 0, d.index("a")] = -0.01
    x[:, 1, d.bos()] = -0.01
    x = torch.from_numpy(x - np.logaddexp.reduce(x, axis=2, keepdims=True)).to(DEV, dtype)
    lm, trie = _tables(tmp_path, d, _arpa_unigrams({"ab": -1.0}), {tuple(d.index(c) for c in "ab"): "ab"}, "space")
    lens = torch.tensor([2, 2], dtype=torch.int32, device=DEV)
    out = _decoder(d, lm, trie, 1, 1).search(x, lens)
    assert int(out[3][0]) == 0 and float(out[2][0, 0]) == -math.inf
    dec = _streaming_decoder(d, lm, trie, 1, 4, 1, 1)
    for b in range(2):  # the second stream reuses the slot
        dec.open([b])
        for t in range(2):
            dec.accept_lprobs([b], x[b, t:t + 1], [1])
        res = tuple(t.clone() for t in dec.finish([b]))
        _equal_to_offline({b: res}, out)
        assert int(res[3][0]) == 0
        hyps = dec.close(b)
        assert len(hyps) == 1 and hyps[0]["tokens"].numel() == 0 and float(hyps[0]["score"]) == -math.inf


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["space", "wordstart"])
@pytest.mark.parametrize("beam,K", BEAMS)
def test_streamed_search_vs_oracle(tmp_path, beam, K, mode):
    """The acceptance rule of the offline search's test (_compare): scores within SCORE_TOL of the float64 oracle, sequences
    equal where the oracle's margin exceeds it."""
    _need_gpu()
    worst = 0.0
    for k, (alpha, beta, gamma) in enumerate(SETTINGS + [(2.0, 1.5, -0.2)]):
        rng = np.random.default_rng(200 * k + beam + K)
        d, words, text, spell, fus = _setup(mode, rng, alpha, beta)
        lm, trie = _tables(tmp_path, d, text, spell, mode)
        V, B, T = len(d), 5, 12
        x = _peaked(rng, B * T, V, sharp=3.0, scale=1.5).reshape(B, T, V).astype(np.float32)
        lens = np.array([T, 0, 1, 7, 10], dtype=np.int32)
        nbest = min(beam, 3)
        res = _run_streamed(d, lm, trie, torch.from_numpy(x).to(DEV), lens, k, 2, T, beam, K, nbest, alpha, beta, gamma, whole=())
        off = _decoder(d, lm, trie, beam, K, nbest=nbest, alpha=alpha, beta=beta, gamma=gamma)  # the search's parameters
        worst = max(worst, _compare(_batched(res, B, nbest, T, off.pad), x, lens, off, fus))
    print(f"streamed {mode} beam {beam} K {K}: max |score - oracle| {worst:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,beam,K,seed", PARTIAL_CASES)
def test_partials(tmp_path, mode, beam, K, seed):
    """After every piece, for every open stream: (a) `partial` and a mid-stream `finish` change nothing (final results
    torch.equal to a run without them); (b) the stable prefix only grows and is a prefix of the best live hypothesis, of every
    hypothesis a finish(nbest=beam) returns at that moment and of the final 1-best; (c) best tokens, score and stable prefix
    are the step-wise oracle's wherever its margin so far exceeds SCORE_TOL — at least half of the checkpoints."""
    _need_gpu()
    d, text, spell, fus, x, lens, (alpha, beta, gamma) = _partial_case(mode, beam, K, seed)
    lm, trie = _tables(tmp_path, d, text, spell, mode)
    xd = torch.from_numpy(x).to(DEV)
    T = x.shape[1]
    plain = _run_streamed(d, lm, trie, xd, lens, seed + 1, 3, T, beam, K, beam, alpha, beta, gamma, whole=(3,))

    dec = _streaming_decoder(d, lm, trie, 3, T, beam, K, nbest=beam, alpha=alpha, beta=beta, gamma=gamma)
    points, history = [], {}

    def observe(ids):
        parts = dec.partial(ids)
        fin = dec.finish(ids)
        now = [_hyps(fin, i) for i in range(len(ids))]
        points.append(dict(zip(ids, parts)))
        for b, part, hyps in zip(ids, parts, now):
            stable, prev = part["stable"], history.setdefault(b, [[]])[-1]
            assert stable[:len(prev)] == prev, (b, prev, stable)
            assert part["tokens"][:len(stable)] == stable, (b, part)
            for y, _ in hyps:
                assert list(y[:len(stable)]) == stable, (b, stable, y)
            history[b].append(stable)

    watched = _session(dec, xd, lens, np.random.default_rng(seed + 1), 3, whole=(3,), observe=observe,
                       finish=lambda b: tuple(t.clone() for t in dec.finish([b])))
    assert sorted(watched) == sorted(plain) == list(range(len(lens)))
    for b in watched:                                                     # (a)
        for got, ref in zip(watched[b], plain[b]):
            assert torch.equal(got, ref), (b, got, ref)
    for b, (tk, ln, sc, nh) in watched.items():                           # (b), the final 1-best
        if int(nh[0]) > 0:
            best = tk[0, 0, :int(ln[0, 0])].tolist()
            for stable in history.get(b, []):
                assert best[:len(stable)] == stable, (b, stable, best)
    ref_points = _oracle_checkpoints(mode, beam, K, seed, x)               # (c): the same schedule on the host
    assert len(ref_points) == len(points)
    total = compared = 0
    worst = 0.0
    for got_round, ref_round in zip(points, ref_points):
        assert sorted(got_round) == sorted(ref_round)
        for b, part in got_round.items():
            best, score, stable, margin = ref_round[b]
            total += 1
            if not margin > SCORE_TOL:
                continue
            compared += 1
            assert part["tokens"] == list(best) and part["stable"] == list(stable), (b, part, ref_round[b])
            assert abs(part["score"] - score) < SCORE_TOL or part["score"] == score, (b, part, ref_round[b])
            if math.isfinite(score):
                worst = max(worst, abs(part["score"] - score))
    print(f"partials {mode} beam {beam} K {K}: {compared} of {total} checkpoints compared, max |score - oracle| {worst:.2e}")
    assert total >= 20 and 2 * compared >= total


@pytest.mark.gpu
def test_accept_is_one_launch_without_synchronisation(tmp_path, monkeypatch):
    _need_gpu()
    from espresso_amd import kernels

    rng = np.random.default_rng(5)
    d, words, text, spell, fus = _setup("wordstart", rng, 1.0, -1.0)
    lm, trie = _tables(tmp_path, d, text, spell, "wordstart")
    V, B, T = len(d), 4, 12
    logits = torch.from_numpy(rng.standard_normal((B, T, V)).astype(np.float32) * 2).to(DEV)
    lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
    out = _decoder(d, lm, trie, 6, 4, nbest=2).search(torch.log_softmax(logits, -1), lens)
    dec = _streaming_decoder(d, lm, trie, B, T, 6, 4, nbest=2)
    ids = list(range(B))
    dec.open(ids)
    dec.accept(ids, logits[:, :2].reshape(B * 2, V), [2] * B)  # warm-up: tables, state, the reset of the opened slots
    calls = []
    real = kernels.ctc_lexicon_stream_step
    monkeypatch.setattr(kernels, "ctc_lexicon_stream_step", lambda *a, **k: calls.append(1) or real(*a, **k))
    counts = [10, 0, 3, 10]
    rows = torch.cat([logits[b, 2:2 + n] for b, n in zip(ids, counts)])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        assert dec.accept(ids, rows, counts) is None
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(calls) == 1
    assert [dec.streams[b][1] for b in ids] == [12, 2, 5, 12]
    # the library's log-softmax and torch's differ by rounding: the finished streams against the offline search by score
    got = dec.finish([0, 3])
    for i, b in enumerate((0, 3)):
        assert int(got[3][i]) == int(out[3][b])
        for j in range(int(got[3][i])):
            assert abs(float(got[2][i, j]) - float(out[2][b, j])) < 1e-3


@pytest.mark.gpu
def test_exceeding_max_frames_raises_before_any_launch(tmp_path, monkeypatch):
    _need_gpu()
    from espresso_amd import kernels

    rng = np.random.default_rng(9)
    d, words, text, spell, fus = _setup("space", rng, 1.0, -0.5)
    lm, trie = _tables(tmp_path, d, text, spell, "space")
    V, T = len(d), 10
    x = torch.from_numpy(_peaked(rng, 2 * T, V, sharp=3.0).reshape(2, T, V).astype(np.float32)).to(DEV)
    out = _decoder(d, lm, trie, 4, 4).search(x[:, :8].contiguous(), torch.tensor([8, 8], dtype=torch.int32, device=DEV))
    dec = _streaming_decoder(d, lm, trie, 2, 8, 4, 4)
    dec.open([0, 1])
    dec.accept_lprobs([0, 1], torch.cat([x[0, :6], x[1, :5]]), [6, 5])
    calls = []
    for name in ("ctc_lexicon_stream_step", "ctc_lexicon_stream_reset", "log_softmax"):
        real = getattr(kernels, name)
        monkeypatch.setattr(kernels, name, lambda *a, _r=real, **k: calls.append(1) or _r(*a, **k))
    with pytest.raises(ValueError, match="max_frames"):
        dec.accept_lprobs([0, 1], torch.cat([x[0, 6:9], x[1, 5:8]]), [3, 3])  # stream 0 would reach 9 > 8
    with pytest.raises(ValueError, match="max_frames"):
        dec.accept([0, 1], torch.cat([x[0, 6:9], x[1, 5:8]]), [3, 3])
    assert not calls and [dec.streams[b][1] for b in (0, 1)] == [6, 5]
    dec.accept_lprobs([0, 1], torch.cat([x[0, 6:8], x[1, 5:8]]), [2, 3])  # both go on as if nothing had happened
    _equal_to_offline({b: tuple(t.clone() for t in dec.finish([b])) for b in (0, 1)}, out)
    assert dec.state_bytes_per_stream() == dec.state.shape[1]


def _write_wav(path, samples):
    import wave

    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(samples, -32768, 32767).astype("<i2").tobytes())


@pytest.mark.gpu
def test_cli_streaming_lexicon_beam_round_trip(tmp_path, capsys, golden_dir, monkeypatch):
    """speech_recognize --streaming --search ctc_beam --ngram-lm --lexicon on the repository's FLAC file and two WAV files, a
    small random chunk-streaming CTC checkpoint and a lexicon closed under non-empty prefixes (every 1- and 2-letter word over
    4 letters: every utterance has a finite hypothesis).  Hard requirement: the streamed H- lines are those of the offline
    search over the log-probs the streaming encoder itself produced.  Against the offline CLI run (one utterance per batch) an
    utterance must match whenever its streamed and offline log-probs are torch.equal; otherwise the difference is printed."""
    _need_gpu()
    from espresso_amd import kernels, registry
    from espresso_amd import speech_recognize as sr
    from espresso_amd.data.audio_utils import read_wav
    from espresso_amd.models.ngram_lm import NGramLanguageModel
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from espresso_amd.tools.ctc_lexicon_beam_search import CTCLexiconBeamSearchDecoder
    from espresso_amd.tools.lexicon import build_lexicon
    from espresso_amd.tools.streaming_ctc_lexicon_beam_decoder import StreamingCTCLexiconBeamDecoder

    letters = "abcd"
    dict_path = str(tmp_path / "dict.txt")
    open(dict_path, "w").write("".join(f"{c} 1\n" for c in letters) + "<space> 1\n")
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(dict=dict_path, autoregressive=False,
                                                                                    criterion_name="ctc_loss"))
    d = task.target_dictionary
    assert d.space() >= 0
    rng = np.random.default_rng(0)
    words = list(letters) + [a + b for a in letters for b in letters]
    arpa, lex = str(tmp_path / "lm.arpa"), str(tmp_path / "lex.txt")
    open(arpa, "w", encoding="utf-8").write(random_arpa(rng, words, 2, per_order=60))
    open(lex, "w", encoding="utf-8").write("".join(f"{w} {' '.join(w)}\n" for w in words))
    enc = {"conv_channels": "[64, 64, 16, 16]", "embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4,
           "normalize_before": True, "relative_positional_embeddings": True, "layer_type": "transformer", "chunk_size": 8,
           "chunk_left_window": 2, "chunk_right_window": 0}
    name = "speech_transformer_encoder_model"
    block = {"_name": name, "encoder": enc, "dropout": 0.0, "attention_dropout": 0.0, "activation_dropout": 0.0,
             "layernorm_embedding": True}
    cls = registry.MODEL_REGISTRY[name]
    torch.manual_seed(0)
    model = cls.build_model(cls.config_class.from_dict(block), task)
    torch.save({"model": model.state_dict(), "cfg": {"model": block}}, str(tmp_path / "model.pt"))
    utts = ["flac", "utt0", "utt1"]
    with open(tmp_path / "wav.scp", "w") as f:
        f.write("flac {}\n".format(os.path.join(golden_dir, "6313-76958-0021.flac")))
        for i in range(2):
            p = str(tmp_path / f"utt{i}.wav")
            _write_wav(p, rng.standard_normal(int(16000 * (1.3 + 0.9 * i))) * 3000)
            f.write(f"utt{i} {p}\n")
    opts = ["--beam", "5", "--nbest", "2", "--lm-weight", "0.7", "--word-score", "-0.5", "--ctc-insertion-bonus", "0.1"]
    base = ["--path", str(tmp_path / "model.pt"), "--dict", dict_path, "--wav-scp", str(tmp_path / "wav.scp"), "--search", "ctc_beam",
            "--ngram-lm", arpa, "--lexicon", lex] + opts

    def run(extra):
        capsys.readouterr()
        sr.main(base + extra)
        out = capsys.readouterr().out.splitlines()
        lines = {}
        for l in out:
            if l.startswith("H-"):
                lines.setdefault(l.split("\t")[0][2:], []).append(l.split("\t")[1:])
        return lines, [l.split("\t") for l in out if l.startswith("P-")]

    offline, _ = run(["--batch-size", "1"])
    fed = {}  # utterance index -> the logits the CLI's streaming encoder gave the decoder
    real_accept = StreamingCTCLexiconBeamDecoder.accept

    def recording_accept(self, ids, logits, counts):
        r = 0
        for i, c in zip(ids, counts):
            fed.setdefault(i, []).append(logits[r:r + c].clone())
            r += c
        return real_accept(self, ids, logits, counts)

    monkeypatch.setattr(StreamingCTCLexiconBeamDecoder, "accept", recording_accept)
    stream_args = ["--streaming", "--stream-chunk-ms", "170", "--streams", "2"]
    streamed, partial_lines = run(stream_args + ["--stream-partials"])
    monkeypatch.setattr(StreamingCTCLexiconBeamDecoder, "accept", real_accept)
    assert set(offline) == set(streamed) == set(utts)

    # the hard requirement: the offline search over the streamed log-probs
    lm = NGramLanguageModel(arpa, device=DEV)
    gen = CTCLexiconBeamSearchDecoder([None], d, lm, build_lexicon(d, lm, lex), beam_size=5, nbest=2, lm_weight=0.7, word_score=-0.5,
                                      insertion_bonus=0.1)
    V = len(d)
    streamed_lp = {}
    for i, u in enumerate(utts):
        logits = torch.cat(fed[i])
        lp = kernels.log_softmax(logits, logits.shape[0], V, logits.stride(0))
        streamed_lp[u] = lp
        out = gen.search(lp[None], torch.tensor([lp.shape[0]], dtype=torch.int32, device=DEV))
        hyps = _hyps(out, 0)
        assert len(hyps) >= 1, u
        assert len(streamed[u]) == len(hyps)
        for (text, score), (y, s) in zip(streamed[u], hyps):
            assert text == d.string(torch.tensor(y)), (u, text, y)
            assert float(score) == s / math.log(2), (u, score, s)

    # the offline CLI run: bound by the encoder, which is not under test here
    task.build_frontend(torch.device(DEV))
    m = model.to(DEV).eval()
    scp = sr.read_scp(str(tmp_path / "wav.scp"))
    for u in utts:
        assert len(offline[u]) >= 1 and offline[u][0][1] != "-inf", (u, offline[u])  # nhyp >= 1 offline
        s = task.prepare_sample(sr.collate([0], [u], [read_wav(scp[u])], torch.device(DEV)), train=False)
        with torch.no_grad():
            lp = m.get_normalized_probs(m(**s["net_input"]), log_probs=True)[:, 0].float()
        if lp.shape == streamed_lp[u].shape and torch.equal(lp, streamed_lp[u]):
            assert streamed[u] == offline[u], (u, streamed[u], offline[u])
            with capsys.disabled():
                print(f"{u}: streamed and offline log-probs equal, H- lines equal")
        else:
            diff = float((lp - streamed_lp[u]).abs().max()) if lp.shape == streamed_lp[u].shape else float("nan")
            with capsys.disabled():
                print(f"{u}: max |streamed - offline log-prob| {diff:.3e}; streamed {streamed[u]} offline {offline[u]}")

    # partial lines: the stable column is a prefix of the utterance's final text
    assert partial_lines and {l[0][2:] for l in partial_lines} <= set(utts)
    for l in partial_lines:
        assert len(l) == 4 and float(l[1]) > 0
        final = streamed[l[0][2:]][0][0]
        assert final == l[2] or final.startswith(l[2] + " ") or l[2] == "", (l, final)
    with capsys.disabled():
        print(f"{len(partial_lines)} partial lines, {sum(bool(l[2]) for l in partial_lines)} with a stable text")

    res = str(tmp_path / "res")
    capsys.readouterr()
    sr.main(base + stream_args + ["--results-path", res])
    log = open(os.path.join(res, "decode.log")).read().splitlines()
    got = {}
    for l in log:
        if l.startswith("H-"):
            got.setdefault(l.split("\t")[0][2:], []).append(l.split("\t")[1:])
    assert got == streamed
    for name in ("decoded_results.txt", "decoded_char_results.txt"):
        assert os.path.exists(os.path.join(res, name))
