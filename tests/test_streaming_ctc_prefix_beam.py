"""Streamed CTC prefix beam search: alone, with LSTM-LM fusion, with hotwords, with partial results
(tools/streaming_ctc_prefix_beam_decoder.py, the ea_ctc_prefix_beam_stream_* entries of csrc/ctc_beam.hip, speech_recognize
--streaming --search ctc_stream_beam).

The offline search (CTCPrefixBeamSearchDecoder.search, held to the float64 oracles by tests/test_ctc_prefix_beam.py and
tests/test_ctc_hotword_beam.py) is the reference of the streamed one, bit for bit: both kernels instantiate one frame body.  The
partial results are held to tests/streaming_beam_ref.py, the search restated step by step in float64, with the bias through its
`lm_fn` hook (tests/hotword_ref.bias_lm_fn)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests.hotword_ref import bias_lm_fn, biased_oracle, grid_phrases
from tests.streaming_beam_ref import StepwiseBeamOracle
from tests.test_ctc_prefix_beam import _cpu_lm_fn, _dictionary, _peaked, _tiny_lm
from tests.test_streaming_lexicon_beam import OracleStreams, _need_gpu, _session

DEV = "cuda:0"
SCORE_TOL = 1e-4  # fp32 search vs the float64 oracle on the same log-probs (tests/test_ctc_prefix_beam.py)
pytestmark = [pytest.mark.filterwarnings("ignore:invalid value encountered in scalar subtract:RuntimeWarning"),
              pytest.mark.filterwarnings("ignore:invalid value encountered in subtract:RuntimeWarning")]
BEAMS = [(1, 1), (4, 4), (16, 4), (10, 6), (64, 8)]
B, T = 5, 16
LENS = np.array([16, 9, 0, 16, 12], dtype=np.int32)
LM_WEIGHT, BONUS = 0.5, 0.3
CONFIGS = ["plain", "lm", "graph", "graph_lm"]


def _graph(phrases, V):
    from espresso_amd.tools.context_graph import ContextGraph

    return ContextGraph(phrases, V)


@functools.lru_cache(maxsize=None)
def _inputs(seed=0):
    """(dictionary, float32 log-probs [B][T][V], phrases that occur in them): shared by the tests, never written to."""
    d = _dictionary(20)
    V = len(d)
    x = _peaked(np.random.default_rng(seed), B * T, V, sharp=4.0, scale=2.0).reshape(B, T, V).astype(np.float32)
    x.setflags(write=False)
    return d, x, grid_phrases(x.astype(np.float64), LENS, d.bos())


def _streaming(d, max_streams, max_frames, beam, K, nbest=1, lm=None, lm_weight=0.0, bonus=0.0, graph=None):
    from espresso_amd.tools.streaming_ctc_prefix_beam_decoder import StreamingCTCPrefixBeamDecoder

    return StreamingCTCPrefixBeamDecoder(d, max_streams, max_frames, beam_size=beam, nbest=nbest, beam_size_token=K, lm_model=lm,
                                         lm_weight=lm_weight, insertion_bonus=bonus, context_graph=graph)


def _offline(d, beam, K, nbest=1, lm=None, lm_weight=0.0, bonus=0.0, graph=None):
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder

    return CTCPrefixBeamSearchDecoder([None], d, beam_size=beam, nbest=nbest, beam_size_token=K, lm_model=lm, lm_weight=lm_weight,
                                      insertion_bonus=bonus, context_graph=graph)


def _main(argv):
    from espresso_amd import speech_recognize as sr

    return sr.main(["--path", "/nonexistent.pt", "--dict", "d", "--wav-scp", "w", *argv])


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_cli_accepts_stream_beam_arguments():
    """--streaming --search ctc_stream_beam with an LM, hotwords, partials and the beam options passes every argument check: the
    failure is the missing checkpoint."""
    from espresso_amd import speech_recognize as sr

    argv = ["--path", "/nonexistent.pt", "--dict", "d", "--wav-scp", "w", "--device", "cpu", "--streaming", "--search", "ctc_stream_beam",
            "--lm-path", "lm.pt", "--lm-arch", "lstm_lm_wsj", "--lm-weight", "0.5", "--hotwords", "h.txt", "--hotword-score", "1.2",
            "--bpe", "characters_asr", "--beam", "5", "--nbest", "2", "--ctc-beam-size-token", "4", "--ctc-insertion-bonus", "0.1",
            "--stream-partials", "--streams", "2", "--stream-chunk-ms", "200"]
    args = sr.get_parser().parse_args(argv)
    for check in (sr.check_frame_beam_args, sr.check_stream_beam_args, sr.check_ctc_stream_beam_args, sr.check_hotword_args,
                  sr.check_ngram_args, sr.check_streaming_args):
        check(args)
    assert sr.lm_fusion_mode(args) == "subword"
    with pytest.raises(FileNotFoundError):
        sr.main(argv)


@pytest.mark.parametrize("extra,error,match", [
    (["--search", "ctc_stream_beam"], ValueError, "--search ctc_beam"),                                  # without --streaming
    (["--streaming", "--search", "ctc_stream_beam", "--ngram-lm", "x"], NotImplementedError, "--ngram-lm"),
    (["--streaming", "--search", "ctc_stream_beam", "--lexicon", "l"], NotImplementedError, "--lexicon"),
    (["--streaming", "--search", "ctc_stream_beam", "--word-dict", "w.txt"], NotImplementedError, "--word-dict"),
    (["--streaming", "--search", "ctc_stream_beam", "--lm-path", os.pathsep.join(["a.pt", "b.pt"])], NotImplementedError, "multi-level"),
    (["--streaming", "--search", "ctc_stream_beam", "--print-alignment", "--results-path", "r"], NotImplementedError, "--print-alignment"),
    (["--streaming", "--search", "ctc_stream_beam", "--transducer-hotwords", "h"], NotImplementedError, "--transducer-hotwords"),
])
def test_cli_refusals(extra, error, match):
    with pytest.raises(error, match=match):
        _main(extra)


def test_cli_refuses_ensembles():
    from espresso_amd import speech_recognize as sr

    with pytest.raises(NotImplementedError, match="ensembles"):
        sr.main(["--path", os.pathsep.join(["/nonexistent.pt", "/b.pt"]), "--dict", "d", "--wav-scp", "w", "--streaming", "--search",
                 "ctc_stream_beam"])


@pytest.mark.parametrize("extra", [["--streaming", "--search", "ctc_beam"], ["--streaming", "--search", "ctc_beam", "--lm-path", "lm.pt"],
                                   ["--hotwords", "h", "--search", "ctc_beam", "--streaming"]])
def test_cli_pinned_refusals_stay(extra):
    with pytest.raises(NotImplementedError):
        _main(extra)


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("beam,K", [(1, 1), (4, 4), (10, 6)])
def test_stepwise_oracle_covers_the_biased_search(beam, K, with_lm):
    """The step-wise oracle with the bias as its `lm_fn`, fed any split of the frames, gives biased_oracle's n-best of the whole
    input: the same tokens, the float64 scores and the margin equal."""
    d, x, phrases = _inputs()
    V = len(d)
    g = _graph(phrases, V)
    lm_fn = _cpu_lm_fn(_tiny_lm(d), d) if with_lm else None
    lam = LM_WEIGHT if with_lm else 0.0
    rng = np.random.default_rng(10 * beam + K)
    nbest = min(beam, 3)
    for b in (0, 1, 4):
        n = int(LENS[b])
        xb = x[b, :n].astype(np.float64)
        ref, ref_margin = biased_oracle(xb, n, beam, K, d.bos(), g, lm_fn=lm_fn, lm_weight=lam, bonus=BONUS, eos=d.eos(), nbest=nbest)
        for split in ([n], [1] * n, [0, 3, 0, 1, n - 4], list(np.diff([0] + sorted(rng.integers(0, n + 1, 4).tolist()) + [n]))):
            o = StepwiseBeamOracle(beam, K, d.bos(), bias_lm_fn(g, V, lm_fn, lam, d.eos()), lm_weight=1.0, bonus=BONUS, eos=V)
            t = 0
            for m in split:
                o.feed(xb[t:t + m])
                o.finish(nbest)  # a readout in between changes nothing
                o.partial()
                t += m
            assert t == n and o.frames == n
            got, margin = o.finish(nbest)
            assert got == ref, (b, split, got, ref)  # tuples of (tokens, float64 score): exact
            assert margin == ref_margin or (math.isnan(margin) and math.isnan(ref_margin))


PARTIAL_CASES = [("plain", 4, 4, 0.0), ("plain", 10, 6, 0.3), ("graph", 4, 4, 0.3), ("graph", 10, 6, 0.0)]


def _partial_oracle(kind, beam, K, bonus):
    d, x, phrases = _inputs()
    V = len(d)
    lm_fn = bias_lm_fn(_graph(phrases, V), V) if kind == "graph" else None
    return lambda: StepwiseBeamOracle(beam, K, d.bos(), lm_fn, lm_weight=1.0, bonus=bonus, eos=V)


def _oracle_checkpoints(kind, beam, K, bonus):
    """The step-wise oracle through the schedule of the GPU partial test: per round {stream: its partial}."""
    d, x, phrases = _inputs()
    dec = OracleStreams(_partial_oracle(kind, beam, K, bonus))
    points = []
    _session(dec, x.astype(np.float64), LENS, np.random.default_rng(beam + K), 3, whole=(3,),
             observe=lambda ids: points.append({b: dec.streams[b].partial() for b in ids}))
    return points


@pytest.mark.parametrize("kind,beam,K,bonus", PARTIAL_CASES)
def test_oracle_margins_allow_the_partial_comparison(kind, beam, K, bonus):
    """At least half of the checkpoints of the GPU partial test have an oracle margin above SCORE_TOL (the oracle alone)."""
    points = [p for rnd in _oracle_checkpoints(kind, beam, K, bonus) for p in rnd.values()]
    clear = sum(p[3] > SCORE_TOL for p in points)
    print(f"{kind} beam {beam} K {K}: {clear} of {len(points)} checkpoints above the margin")
    assert len(points) >= 20 and 2 * clear >= len(points)


def test_decoder_argument_checks():
    d = _dictionary(8)
    dec = _streaming(d, 2, 10, 4, 3)
    dec.open([0])
    with pytest.raises(ValueError, match="already open"):
        dec.open([0])
    dec.open(["b"])
    with pytest.raises(RuntimeError, match="slots"):
        dec.open([2])
    assert sorted(st[0] for st in dec.streams.values()) == [0, 1]
    with pytest.raises(ValueError, match="max_streams"):
        _streaming(d, 0, 10, 4, 3)
    with pytest.raises(ValueError, match="max_frames"):
        _streaming(d, 2, 0, 4, 3)
    with pytest.raises(ValueError, match="nbest"):
        _streaming(d, 2, 10, 4, 3, nbest=5)
    with pytest.raises(ValueError, match="beam"):
        _streaming(d, 2, 10, 65, 3)
    with pytest.raises(ValueError, match="context graph"):
        _streaming(d, 2, 10, 4, 3, graph=_graph([], len(d) + 1))


# ---------------------------------------------------------------------------------------------------------------- GPU
def _setup(config, d, phrases):
    """The decoder options of a configuration: (LM on the device or None, lm_weight, insertion bonus, graph or None)."""
    lm = _tiny_lm(d).to(DEV) if "lm" in config else None
    graph = _graph(phrases, len(d)) if "graph" in config else None
    return dict(lm=lm, lm_weight=LM_WEIGHT if lm is not None else 0.0, bonus=BONUS if lm is not None else 0.0, graph=graph)


def _run_streamed(dec, xd, lens, seed, max_streams, whole=(3,), observe=None):
    res = _session(dec, xd, lens, np.random.default_rng(seed), max_streams, whole=whole, observe=observe,
                   finish=lambda b: tuple(t.clone() for t in dec.finish([b])))
    assert not dec.streams and sorted(dec._free) == list(range(max_streams))
    return res


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


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("beam,K", BEAMS)
def test_streamed_equals_offline_bit_for_bit(beam, K, config, dtype):
    """The same log-probs once through CTCPrefixBeamSearchDecoder.search and once through the streaming decoder in random pieces
    (0-, 1-, 2-, 3- and 5-frame pieces, one utterance whole, 3 slots for 5 utterances, reused; a zero-frame stream): nhyp,
    lengths, scores and tokens are torch.equal; without an LM for two prefix-table sizes.  No tolerance: the frames run the same
    code."""
    _need_gpu()
    d, x, phrases = _inputs()
    opts = _setup(config, d, phrases)
    xd = torch.tensor(x).to(DEV, dtype)
    nbest = min(beam, 3)
    out = _offline(d, beam, K, nbest=nbest, **opts).search(xd, torch.from_numpy(LENS).to(DEV))
    assert int(out[3].min()) >= 1 and int(out[1][2, 0]) == 0  # the zero-frame utterance: the empty hypothesis
    for max_frames in ((T, 40) if config == "plain" else (T,)):
        dec = _streaming(d, 3, max_frames, beam, K, nbest=nbest, **opts)
        res = _run_streamed(dec, xd, LENS, 7 + max_frames, 3)
        assert sorted(res) == list(range(B))
        _equal_to_offline(res, out)
        assert dec.state_bytes_per_stream() == dec.state.shape[1]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_streamed_equals_offline_beyond_the_staged_columns(dtype):
    """V = 5200: the columns from 5120 on are not staged in LDS; the frames' best tokens lie there."""
    _need_gpu()
    d = _dictionary(5195)
    V, Bv, Tv = len(d), 2, 3
    assert V == 5200
    rng = np.random.default_rng(4)
    z = rng.standard_normal((Bv * Tv, V))
    z[np.arange(Bv * Tv), rng.integers(5120, V, Bv * Tv)] += 6.0
    z[np.arange(Bv * Tv), rng.integers(5120, V, Bv * Tv)] += 5.0
    x = (z - np.logaddexp.reduce(z, axis=1, keepdims=True)).reshape(Bv, Tv, V).astype(np.float32)
    lens = np.array([3, 2], dtype=np.int32)
    xd = torch.tensor(x).to(DEV, dtype)
    out = _offline(d, 4, 4, nbest=3).search(xd, torch.from_numpy(lens).to(DEV))
    assert int(out[0][0, 0, :int(out[1][0, 0])].max()) >= 5120
    dec = _streaming(d, 2, Tv, 4, 4, nbest=3)
    dec.open([0, 1])
    dec.accept_lprobs([0, 1], torch.cat([xd[0, :1], xd[1, :2]]), [1, 2])
    dec.accept_lprobs([0], xd[0, 1:3], [2])
    _equal_to_offline({b: tuple(t.clone() for t in dec.finish([b])) for b in (0, 1)}, out)


@pytest.mark.gpu
def test_readouts_do_not_depend_on_the_pieces():
    """With the LM and the graph: one utterance to three streams, frame by frame, in pieces with a partial and a finish after
    every piece, and in the same pieces without readouts.  At every common frame count partial_tensors and finish of the first
    two are torch.equal; the final results of all three are."""
    _need_gpu()
    d, x, phrases = _inputs()
    opts = _setup("graph_lm", d, phrases)
    xd = torch.tensor(x).to(DEV)[0]
    dec = _streaming(d, 3, T, 6, 4, nbest=3, **opts)
    dec.open(["frames", "pieces", "quiet"])

    def readout(sid):
        return [t.clone() for t in dec.partial_tensors([sid])] + [t.clone() for t in dec.finish([sid])]

    by_frames = {0: readout("frames")}
    for t in range(T):
        dec.accept_lprobs(["frames"], xd[t:t + 1], [1])
        by_frames[t + 1] = readout("frames")
    t = 0
    for n in (3, 5, 0, 1, 7):
        dec.accept_lprobs(["pieces"], xd[t:t + n], [n])
        dec.accept_lprobs(["quiet"], xd[t:t + n], [n])
        t += n
        for got, ref in zip(readout("pieces"), by_frames[t]):
            assert torch.equal(got, ref), (t, got, ref)
    assert t == T
    final = [dec.finish([sid]) for sid in ("frames", "pieces", "quiet")]
    for other in final[1:]:
        for got, ref in zip(other, final[0]):
            assert torch.equal(got, ref)
    assert int(final[0][1][0, 0]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind,beam,K,bonus", PARTIAL_CASES)
def test_partials(kind, beam, K, bonus):
    """After every piece, for every open stream: the stable prefix only grows and is a prefix of the best live hypothesis; every
    stable prefix is a prefix of every hypothesis of the stream's final result with nbest = beam; best tokens, score and stable
    prefix are the step-wise oracle's wherever its margin so far exceeds SCORE_TOL."""
    _need_gpu()
    d, x, phrases = _inputs()
    graph = _graph(phrases, len(d)) if kind == "graph" else None
    dec = _streaming(d, 3, T, beam, K, nbest=beam, bonus=bonus, graph=graph)
    points, history = [], {}

    def observe(ids):
        parts = dec.partial(ids)
        points.append(dict(zip(ids, parts)))
        for b, part in zip(ids, parts):
            stable, prev = part["stable"], history.setdefault(b, [[]])[-1]
            assert stable[:len(prev)] == prev, (b, prev, stable)
            assert part["tokens"][:len(stable)] == stable, (b, part)
            history[b].append(stable)

    final = _run_streamed(dec, torch.tensor(x).to(DEV), LENS, beam + K, 3, observe=observe)
    assert sorted(final) == list(range(B))
    for b, (tk, ln, sc, nh) in final.items():
        for i in range(int(nh[0])):
            y = tk[0, i, :int(ln[0, i])].tolist()
            for stable in history.get(b, []):
                assert y[:len(stable)] == stable, (b, stable, y)
    assert any(len(h[-1]) > 0 for h in history.values())
    ref_points = _oracle_checkpoints(kind, beam, K, bonus)  # the same schedule on the host
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
            assert abs(part["score"] - score) < SCORE_TOL, (b, part, ref_round[b])
            worst = max(worst, abs(part["score"] - score))
    print(f"partials {kind} beam {beam} K {K}: {compared} of {total} checkpoints compared, max |score - oracle| {worst:.2e}")
    assert total >= 20 and 2 * compared >= total


@pytest.mark.gpu
@pytest.mark.parametrize("with_lm", [False, True])
def test_empty_graph_equals_no_graph(with_lm):
    """A root-only graph (the biased instantiation, every hypothesis in the root with bias 0) against context_graph=None on the
    same session: the same bits, finishes and partials."""
    _need_gpu()
    d, x, phrases = _inputs()
    opts = _setup("lm" if with_lm else "plain", d, phrases)
    xd = torch.tensor(x).to(DEV)
    runs = []
    for graph in (None, _graph([], len(d))):
        dec = _streaming(d, 3, T, 10, 6, nbest=3, **dict(opts, graph=graph))
        seen = []
        res = _run_streamed(dec, xd, LENS, 11, 3, observe=lambda ids: seen.append([t.clone() for t in dec.partial_tensors(ids)]))
        assert (dec.graph is None) == (graph is None)
        runs.append((res, seen))
    (plain, plain_seen), (empty, empty_seen) = runs
    assert sorted(plain) == sorted(empty) == list(range(B)) and len(plain_seen) == len(empty_seen)
    for b in plain:
        for got, ref in zip(empty[b], plain[b]):
            assert torch.equal(got, ref), (b, got, ref)
    for got_round, ref_round in zip(empty_seen, plain_seen):
        for got, ref in zip(got_round, ref_round):
            assert torch.equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("biased", [False, True])
def test_skipped_and_full_slots_leave_the_state_untouched(biased):
    """At kernel level: an entry with a slot id out of range, one with n_new = 0, one whose rows lie beyond total_rows and one
    that would pass max_frames change no byte of the state, and with lm_rows they write the identity triple; a piece that fits
    exactly is searched."""
    _need_gpu()
    from espresso_amd import _lib
    from espresso_amd import kernels as Kn

    d, x, phrases = _inputs()
    V, beam, K, S, mf = len(d), 4, 3, 3, 4
    graph = _graph(phrases, V).cuda(DEV) if biased else None
    xd = torch.tensor(x).to(DEV)[0].contiguous()  # [T][V]
    state, nbytes = Kn.ctc_prefix_beam_stream_state(S, mf, beam, DEV)
    lib = _lib.lib()
    assert nbytes == lib.ea_ctc_prefix_beam_stream_state_bytes(mf, beam) and nbytes % 8 == 0
    cap, tsize = 1 + mf * beam, 64
    assert nbytes == 4 * (2 + ((3 * tsize + 7 * beam + 2 + 2 * cap + 1) // 2) * 2 + 2 * beam)
    assert lib.ea_ctc_prefix_beam_stream_state_bytes(0, beam) == 0 and lib.ea_ctc_prefix_beam_stream_state_bytes(mf, 65) == 0

    def ints(rows):
        return torch.tensor(rows, dtype=torch.int32, device=DEV).t().contiguous()  # [(slot, n_new, row_off)] -> meta [3][n]

    step = dict(max_frames=mf, V=V, beam=beam, K=K, blank=d.bos(), graph=graph)
    Kn.ctc_prefix_beam_stream_reset(state, torch.tensor([0, 1, 2, 9, -1], dtype=torch.int32, device=DEV), mf, beam)
    Kn.ctc_prefix_beam_stream_step(xd, ints([(0, 3, 0), (1, 1, 3)]), state, **step)  # slot 0: 3 frames, slot 1: 1, slot 2: none
    before = state.clone()
    words = before.view(torch.int32)
    assert words[:, 0].tolist() == [3, 1, 0] and words[:, 1].tolist() == [0, 0, 0]
    idle = ints([(S, 2, 0), (-1, 2, 0), (1, 0, 2), (0, 3, 2), (2, 2, T - 1)])  # no such slots, no frames, no room, rows past the end
    Kn.ctc_prefix_beam_stream_step(xd, idle, state, **step)
    assert torch.equal(state, before)
    n = idle.shape[1]
    lm_rows = torch.zeros(n * beam, V, device=DEV)
    for j0 in (0, 1):
        lm_out = (torch.full((n * beam,), -7, dtype=torch.int32, device=DEV), torch.full((n * beam,), -7, dtype=torch.int32, device=DEV),
                  torch.full((n * beam,), 9, dtype=torch.uint8, device=DEV))
        Kn.ctc_prefix_beam_stream_step(xd, idle, state, j0=j0, j1=j0 + 1, lm_rows=lm_rows, lm_weight=0.5, lm_out=lm_out, **step)
        assert torch.equal(state, before)
        assert lm_out[0].tolist() == list(range(n * beam)) and set(lm_out[1].tolist()) == {d.bos()} and set(lm_out[2].tolist()) == {1}
    # bad arguments: -2 and nothing launched
    p = lambda t: t.data_ptr()  # noqa: E731
    lm_out = tuple(t.clone() for t in lm_out)
    args = lambda j0, j1, beam_, lm: (p(xd), V, 0, T, p(idle[0]), p(idle[1]), p(idle[2]), j0, j1, n, p(state), lm, V if lm else 0,  # noqa: E731
                                      p(lm_out[0]), p(lm_out[1]), p(lm_out[2]), None, None, None, 0, 0, S, mf, V, beam_, K, d.bos(), 0.5, 0.0,
                                      None)
    assert lib.ea_ctc_prefix_beam_stream_step(*args(0, 2, beam, p(lm_rows))) == -2   # with an LM: one frame per launch
    assert lib.ea_ctc_prefix_beam_stream_step(*args(2, 1, beam, None)) == -2
    assert lib.ea_ctc_prefix_beam_stream_step(*args(0, 1, 65, None)) == -2
    torch.cuda.synchronize()
    assert torch.equal(state, before)
    # a piece that fits exactly: slot 0 reaches max_frames and equals the offline search of those frames
    Kn.ctc_prefix_beam_stream_step(xd, ints([(0, 1, 3)]), state, **step)
    assert state.view(torch.int32)[0, 0].item() == mf
    slots = torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    got = Kn.ctc_prefix_beam_stream_finish(state, slots, mf, beam, 2, d.pad(), mf, graph=graph)
    if biased:
        ws = Kn.ctc_prefix_beam_bias_workspace(1, mf, beam, DEV)
        lens = torch.tensor([mf], dtype=torch.int32, device=DEV)
        Kn.ctc_prefix_beam_bias_step(xd[:mf], lens, ws, graph, 1, mf, V, beam, K, d.bos(), 0, mf)
        ref = Kn.ctc_prefix_beam_bias_finish(ws, graph, 1, mf, beam, 2, d.pad())
    else:
        ws = Kn.ctc_prefix_beam_workspace(1, mf, beam, DEV)
        lens = torch.tensor([mf], dtype=torch.int32, device=DEV)
        Kn.ctc_prefix_beam_step(xd[:mf], lens, ws, 1, mf, V, beam, K, d.bos(), 0, mf)
        ref = Kn.ctc_prefix_beam_finish(ws, 1, mf, beam, 2, d.pad())
    for g_, r_ in zip(got, ref):
        assert torch.equal(g_[0], r_[0])
    assert int(got[3][1]) == 0 and got[2][1].tolist() == [-math.inf, -math.inf]  # no such slot: no hypothesis
    # longer hypotheses are cut at max_u and their lengths clipped
    cut = Kn.ctc_prefix_beam_stream_finish(state, slots[:1], mf, beam, 2, d.pad(), 1, graph=graph)
    assert torch.equal(cut[1][0], torch.clamp(got[1][0], max=1)) and torch.equal(cut[0][0, :, 0], got[0][0, :, 0])
    assert torch.equal(cut[2], got[2][:1])


@pytest.mark.gpu
def test_exceeding_max_frames_raises_before_any_launch(monkeypatch):
    _need_gpu()
    from espresso_amd import kernels

    d, x, phrases = _inputs()
    xd = torch.tensor(x).to(DEV)
    out = _offline(d, 4, 4).search(xd[:2, :8].contiguous(), torch.tensor([8, 8], dtype=torch.int32, device=DEV))
    dec = _streaming(d, 2, 8, 4, 4)
    dec.open([0, 1])
    dec.accept_lprobs([0, 1], torch.cat([xd[0, :6], xd[1, :5]]), [6, 5])
    calls = []
    for name in ("ctc_prefix_beam_stream_step", "ctc_prefix_beam_stream_reset", "log_softmax"):
        real = getattr(kernels, name)
        monkeypatch.setattr(kernels, name, lambda *a, _r=real, **k: calls.append(1) or _r(*a, **k))
    with pytest.raises(ValueError, match="max_frames"):
        dec.accept_lprobs([0, 1], torch.cat([xd[0, 6:9], xd[1, 5:8]]), [3, 3])  # stream 0 would reach 9 > 8
    with pytest.raises(ValueError, match="max_frames"):
        dec.accept([0, 1], torch.cat([xd[0, 6:9], xd[1, 5:8]]), [3, 3])
    assert not calls and [dec.streams[b][1] for b in (0, 1)] == [6, 5]
    dec.accept_lprobs([0, 1], torch.cat([xd[0, 6:8], xd[1, 5:8]]), [2, 3])  # both go on as if nothing had happened
    _equal_to_offline({b: tuple(t.clone() for t in dec.finish([b])) for b in (0, 1)}, out)


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["plain", "graph_lm"])
def test_accept_does_not_synchronise(config, monkeypatch):
    """accept_lprobs under torch's sync debug mode: without an LM one step launch for all streams, with one a launch per frame
    index; the finished streams equal the offline search."""
    _need_gpu()
    from espresso_amd import kernels

    d, x, phrases = _inputs()
    opts = _setup(config, d, phrases)
    xd = torch.tensor(x).to(DEV)
    lens = torch.full((4,), 12, dtype=torch.int32, device=DEV)
    out = _offline(d, 6, 4, nbest=2, **opts).search(xd[:4, :12].contiguous(), lens)
    dec = _streaming(d, 4, 12, 6, 4, nbest=2, **opts)
    ids = list(range(4))
    dec.open(ids)
    dec.accept_lprobs(ids, xd[:4, :2].reshape(8, -1), [2] * 4)  # warm-up: state, tables, the reset of the opened slots
    calls = []
    real = kernels.ctc_prefix_beam_stream_step
    monkeypatch.setattr(kernels, "ctc_prefix_beam_stream_step", lambda *a, **k: calls.append(1) or real(*a, **k))
    counts = [10, 0, 3, 10]
    rows = torch.cat([xd[b, 2:2 + n] for b, n in zip(ids, counts)])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        assert dec.accept_lprobs(ids, rows, counts) is None
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(calls) == (1 if config == "plain" else 10)
    assert [dec.streams[b][1] for b in ids] == [12, 2, 5, 12]
    got = dec.finish([0, 3])
    for i, b in enumerate((0, 3)):
        for g_, r_ in zip(got, out):
            assert torch.equal(g_[i], r_[b])


def _write_wav(path, samples):
    import wave

    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(samples, -32768, 32767).astype("<i2").tobytes())


def _tones(rng, seconds):
    """Two tones that change every 0.12 s and every 0.2 s over faint noise: audio whose features, and so the model's best token,
    vary in time (under white noise the random checkpoint says one token throughout)."""
    n = int(16000 * seconds)
    wave = 2.0 * rng.standard_normal(n)
    for segment in (0.12, 0.2):
        seg = int(16000 * segment)
        freq = np.repeat(rng.uniform(200.0, 6000.0, n // seg + 1), seg)[:n]
        wave += 4000.0 * np.sin(2 * np.pi * np.cumsum(freq) / 16000.0)
    return wave


def _cli_fixture(tmp_path, audio=_tones, scale=8.0):
    """A small random chunk-streaming CTC checkpoint (its output layer scaled up, so that the frames have a clear best token as a
    trained model's do), a 30-token dictionary and three synthetic WAV files under tmp_path: (dictionary, utterance ids, the
    command line's --path --dict --wav-scp)."""
    from espresso_amd import registry
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask

    dict_path = str(tmp_path / "dict.txt")
    open(dict_path, "w").write("".join(f"t{i} 1\n" for i in range(30)))
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(dict=dict_path, autoregressive=False,
                                                                                    criterion_name="ctc_loss"))
    enc = {"conv_channels": "[64, 64, 16, 16]", "embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4,
           "normalize_before": True, "relative_positional_embeddings": True, "layer_type": "transformer", "chunk_size": 8,
           "chunk_left_window": 2, "chunk_right_window": 0}
    name = "speech_transformer_encoder_model"
    block = {"_name": name, "encoder": enc, "dropout": 0.0, "attention_dropout": 0.0, "activation_dropout": 0.0,
             "layernorm_embedding": True}
    cls = registry.MODEL_REGISTRY[name]
    torch.manual_seed(0)
    model = cls.build_model(cls.config_class.from_dict(block), task)
    with torch.no_grad():
        model.encoder.fc_out.weight.mul_(scale)
    torch.save({"model": model.state_dict(), "cfg": {"model": block}}, str(tmp_path / "model.pt"))
    rng = np.random.default_rng(0)
    utts = [f"utt{i}" for i in range(3)]
    with open(tmp_path / "wav.scp", "w") as f:
        for i, u in enumerate(utts):
            p = str(tmp_path / f"{u}.wav")
            _write_wav(p, audio(rng, 0.7 + 0.4 * i))
            f.write(f"{u} {p}\n")
    return task.target_dictionary, utts, ["--path", str(tmp_path / "model.pt"), "--dict", dict_path, "--wav-scp", str(tmp_path / "wav.scp")]


@pytest.mark.gpu
@pytest.mark.parametrize("with_lm,with_hotwords", [(False, False), (True, False), (False, True), (True, True)])
def test_cli_round_trip(tmp_path, capsys, monkeypatch, with_lm, with_hotwords):
    """speech_recognize --streaming --search ctc_stream_beam [--lm-path] [--hotwords] on the checkpoint and the WAV files of
    _cli_fixture: the H- lines carry the texts of --search ctc_beam with the same options, and are, texts and scores, those of
    the offline search over the log-probs the streaming encoder produced; the stable part of every P- line is a prefix of the
    final text."""
    _need_gpu()
    from espresso_amd import kernels
    from espresso_amd import speech_recognize as sr
    from espresso_amd.models.lstm_lm import LSTMLanguageModelEspresso
    from espresso_amd.tools.context_graph import load_context_graph
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder
    from espresso_amd.tools.streaming_ctc_prefix_beam_decoder import StreamingCTCPrefixBeamDecoder

    d, utts, base = _cli_fixture(tmp_path)
    opts = ["--beam", "5", "--nbest", "2", "--ctc-beam-size-token", "4", "--ctc-insertion-bonus", "0.1"]
    lm = None
    if with_lm:
        class _LMTask:
            target_dictionary = source_dictionary = d

        torch.manual_seed(1)
        lm = LSTMLanguageModelEspresso.build_model(dict(arch="lstm_lm_wsj", is_wordlm=False), _LMTask)
        torch.save(lm.state_dict(), str(tmp_path / "lm.pt"))
        lm = lm.to(DEV).eval()
        opts += ["--lm-path", str(tmp_path / "lm.pt"), "--lm-arch", "lstm_lm_wsj", "--lm-weight", "0.5"]

    def run(extra):
        capsys.readouterr()
        sr.main(base + extra)
        out = capsys.readouterr().out.splitlines()
        lines = {}
        for l in out:
            if l.startswith("H-"):
                lines.setdefault(l.split("\t")[0][2:], []).append(l.split("\t")[1:])
        return lines, [l.split("\t") for l in out if l.startswith("P-")]

    graph = None
    if with_hotwords:  # the 2-grams of what the model says without them, and one phrase it never says
        plain, _ = run(["--search", "ctc_beam", "--batch-size", "1"] + opts)
        toks = [h[0].split() for hyps in plain.values() for h in hyps]
        grams = sorted({tuple(t[i:i + 2]) for t in toks for i in range(len(t) - 1)})
        grams = [gr for gr in grams if all(d.index(w) != d.unk() for w in gr)][:6]
        hot = tmp_path / "hot.txt"
        hot.write_text("".join(" ".join(gr) + ("\t0.9\n" if k % 2 else "\n") for k, gr in enumerate(grams)) + "t28 t29 t28\n",
                       encoding="utf-8")
        opts += ["--hotwords", str(hot), "--hotword-score", "1.3"]
        graph = load_context_graph(str(hot), d, d.bos(), 1.3)
        assert len(grams) >= 3 and graph.num_nodes > 6

    offline, _ = run(["--search", "ctc_beam", "--batch-size", "1"] + opts)
    fed = {}  # utterance index -> the logits the CLI's streaming encoder gave the decoder
    real_accept = StreamingCTCPrefixBeamDecoder.accept

    def recording_accept(self, ids, logits, counts):
        r = 0
        for i, c in zip(ids, counts):
            fed.setdefault(i, []).append(logits[r:r + c].clone())
            r += c
        return real_accept(self, ids, logits, counts)

    monkeypatch.setattr(StreamingCTCPrefixBeamDecoder, "accept", recording_accept)
    streamed, partial_lines = run(["--streaming", "--search", "ctc_stream_beam", "--stream-chunk-ms", "170", "--streams", "2",
                                   "--stream-partials"] + opts)
    monkeypatch.setattr(StreamingCTCPrefixBeamDecoder, "accept", real_accept)
    assert set(offline) == set(streamed) == set(utts)

    # the offline search over the streamed log-probs: texts and scores
    gen = CTCPrefixBeamSearchDecoder([None], d, beam_size=5, nbest=2, beam_size_token=4, lm_model=lm, lm_weight=0.5 if with_lm else 0.0,
                                     insertion_bonus=0.1, context_graph=graph)
    V = len(d)
    for i, u in enumerate(utts):
        logits = torch.cat(fed[i])
        lp = kernels.log_softmax(logits, logits.shape[0], V, logits.stride(0))
        tokens, lengths, scores, nhyp = (t.cpu() for t in gen.search(lp[None], torch.tensor([lp.shape[0]], dtype=torch.int32, device=DEV)))
        assert len(streamed[u]) == int(nhyp[0]) == 2
        for j, (text, score) in enumerate(streamed[u]):
            assert text == d.string(tokens[0, j, :int(lengths[0, j])].long()), (u, j, text)
            assert float(score) == float(scores[0, j]) / math.log(2), (u, j, score, float(scores[0, j]))
    # the offline command line with the same options: the same texts
    for u in utts:
        with capsys.disabled():
            print(f"{u}: streamed {streamed[u]} offline {offline[u]}")
        assert [h[0] for h in streamed[u]] == [h[0] for h in offline[u]], (u, streamed[u], offline[u])
    assert any(h[0][0] for h in streamed.values())  # the texts are not all empty

    # partial lines: the stable column is a prefix of the utterance's final text
    assert partial_lines and {l[0][2:] for l in partial_lines} <= set(utts)
    for l in partial_lines:
        assert len(l) == 4 and float(l[1]) > 0
        final = streamed[l[0][2:]][0][0]
        assert final == l[2] or final.startswith(l[2] + " ") or l[2] == "", (l, final)
    with capsys.disabled():
        print(f"{len(partial_lines)} partial lines, {sum(bool(l[2]) for l in partial_lines)} with a stable text")
