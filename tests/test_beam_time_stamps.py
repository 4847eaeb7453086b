"""Time stamps of the four device-resident beam searches (csrc/ctc_beam.hip and csrc/rnnt_beam.hip, the kTimes kernels; the
`token_times` argument of the four decoders; `speech_recognize --ctm`).

tests/beam_times_ref.py states the contract in float64.  The CPU tests hold those oracles equal to the oracles they restate (tokens
and scores) and their times and Viterbi scores to brute force over every alignment; the GPU tests hold the kernels to the
oracles, the searches with times to the searches without (bit for bit), the streamed kernels to the offline ones (bit for bit),
the CTC times to the forced aligner, and the decoders and the command line to each other.

Bounds.  vscores against the float64 oracle: SCORE_TOL for CTC, SCORE_TOL + 8 * TERM_TOL * terms for the transducer (what the
existing tests allow for scores; a Viterbi score is a sum of the same fp32 terms without the log-add-exp).  Times are compared
exactly, which needs every pruning margin and every gap a max rested on clear of the fp32 error: each case's seed was chosen on
the CPU so that both exceed twice the bound (the first seed from 0 that does), and every test asserts it before it compares."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests.beam_times_ref import (PrefixBeamTimesOracle, ctc_best_alignments, ctc_times_words, frame_beam_times_oracle,
                                  prefix_beam_times_oracle, rnnt_times_words, transducer_best_alignments)
from tests.hotword_ref import bias_lm_fn, biased_oracle, grid_phrases
from tests.streaming_beam_ref import StepwiseBeamOracle
from tests.test_ctc_prefix_beam import LM_TOL, SCORE_TOL, _cpu_lm_fn, _dictionary, _peaked, _tiny_lm, prefix_beam_oracle
from tests.test_transducer_frame_beam import BLANK, EOS, TERM_TOL
from tests.test_transducer_hotword_beam import _Case, _Family, _offline, _streamed
from tests.transducer_frame_beam_ref import TableLM, TableModel, frame_beam_oracle
from tests.transducer_hotword_ref import biased_frame_beam_oracle

DEV = "cuda:0"
PAD = 1
LENS = np.array([14, 0, 1, 9, 12], dtype=np.int32)
B, T = len(LENS), int(LENS.max())
pytestmark = [pytest.mark.filterwarnings("ignore:invalid value encountered in scalar subtract:RuntimeWarning"),
              pytest.mark.filterwarnings("ignore:invalid value encountered in subtract:RuntimeWarning")]


def _graph(phrases, V):
    from espresso_amd.tools.context_graph import ContextGraph

    return ContextGraph(phrases, V)


# =============================================================================================================== CPU: the oracles
@pytest.mark.parametrize("beam,K", [(1, 1), (4, 4), (16, 4)])
@pytest.mark.parametrize("mode", ["plain", "bonus", "graph"])
def test_ctc_oracle_equals_the_oracles_it_restates(beam, K, mode):
    """Tokens, scores and margins are those of prefix_beam_oracle and of StepwiseBeamOracle fed in pieces, as float64."""
    V = 20
    x = _peaked(np.random.default_rng(3), T, V, sharp=4.0, scale=2.0)
    kw = dict(bonus=0.3) if mode == "bonus" else {}
    if mode == "graph":
        g = _graph(grid_phrases(x[None], [T], 0), V)
        kw = dict(lm_fn=bias_lm_fn(g, V), lm_weight=1.0, eos=V, bonus=0.1)
    nbest = min(beam, 3)
    got, margin, vgap = prefix_beam_times_oracle(x, T, beam, K, 0, nbest=nbest, **kw)
    ref, ref_margin = prefix_beam_oracle(x, T, beam, K, 0, nbest=nbest, **kw)
    assert [(y, s) for y, s, _, _ in got] == ref and margin == ref_margin and vgap > 0
    a, b = PrefixBeamTimesOracle(beam, K, 0, **kw), StepwiseBeamOracle(beam, K, 0, kw.get("lm_fn"), kw.get("lm_weight", 1.0),
                                                                        kw.get("bonus", 0.0), kw.get("eos"))
    for lo, hi in ((0, 3), (3, 4), (4, 4), (4, 11), (11, T)):
        a.feed(x[lo:hi])
        b.feed(x[lo:hi])
        assert [(y, s) for y, s, _, _ in a.finish(nbest)[0]] == b.finish(nbest)[0] and a.finish(nbest)[1] == b.finish(nbest)[1]
    assert a.finish(nbest)[0] == got


@pytest.mark.parametrize("beam,K", [(1, 1), (4, 4), (16, 4)])
@pytest.mark.parametrize("mode", ["plain", "lm", "no_blank_eos", "graph"])
def test_transducer_oracle_equals_the_oracles_it_restates(beam, K, mode):
    V = 20
    table = TableModel(V, 2, blank=BLANK)
    kw = {}
    if mode == "lm":
        kw = dict(lm_fn=TableLM(V, 9), lm_weight=0.6)
    if mode == "no_blank_eos":
        kw = dict(lm_fn=TableLM(V - 1, 9), lm_weight=0.6, eos=EOS, predicts_eos=True, temperature=1.3, normalize=False)
    nbest = min(beam, 3)
    fn = table.logits_fn(0)
    if mode == "graph":
        y = frame_beam_oracle(fn, T, 16, 4, BLANK, nbest=2)[0][1][0]
        g = _graph([(list(y[i:i + 2]), 0.73 + 0.64 * (i % 2)) for i in range(len(y) - 1)], V)
        got = frame_beam_times_oracle(fn, T, beam, K, BLANK, graph=g, nbest=nbest)
        ref = biased_frame_beam_oracle(fn, T, beam, K, BLANK, g, nbest=nbest)
    else:
        got = frame_beam_times_oracle(fn, T, beam, K, BLANK, nbest=nbest, **kw)
        ref = frame_beam_oracle(fn, T, beam, K, BLANK, nbest=nbest, **kw)
    assert [(y, s) for y, s, _, _ in got[0]] == ref[0] and got[1] == ref[1] and got[2] == ref[2] and got[3] > 0


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("T_", [1, 3, 5])
def test_ctc_oracle_against_brute_force_without_pruning(seed, T_):
    """V 3, beam 64 (63 label sequences of at most 5 tokens exist), K 2: every finite hypothesis' times and Viterbi score are
    those of the best of all its alignments, found by enumerating the 3^T frame labellings."""
    V = 3
    x = np.random.default_rng(seed).standard_normal((T_, V)) * 1.5
    x -= np.logaddexp.reduce(x, axis=1, keepdims=True)
    hyps, _, _ = prefix_beam_times_oracle(x, T_, 64, 2, 0, nbest=64)
    brute = ctc_best_alignments(x, 0)
    finite = [h for h in hyps if h[1] > -math.inf]
    assert {h[0] for h in finite} == set(brute)
    for y, s, times, v in finite:
        best, starts, lead = brute[y]
        assert lead > 1e-9, (y, lead)  # the best alignment is unique
        assert abs(v - best) < 1e-9 and times == starts, (y, v, best, times, starts)
    for y, s, times, v in hyps:
        if s == -math.inf:
            assert v == -math.inf and len(times) == len(y)


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("T_", [1, 3, 5])
def test_transducer_oracle_against_brute_force_without_pruning(seed, T_, with_lm):
    """The TableModel with two non-blank tokens: every hypothesis' times and Viterbi score are those of the best of all choices of
    the frames that emit."""
    V = 3
    table = TableModel(V, seed, blank=BLANK, sharp=1.0)
    lm = TableLM(V, seed + 50) if with_lm else None
    hyps = frame_beam_times_oracle(table.logits_fn(0), T_, 10 ** 6, V - 1, BLANK, lm_fn=lm, lm_weight=0.7, normalize=False,
                                   nbest=10 ** 6)[0]
    brute = transducer_best_alignments(table.logits_fn(0), T_, V, BLANK, lm, 0.7)
    assert {h[0] for h in hyps} == set(brute) and len(hyps) == len(brute)
    for y, s, times, v in hyps:
        best, emit, lead = brute[y]
        assert lead > 1e-9, (y, lead)
        assert abs(v - best) < 1e-9 and times == emit, (y, v, best, times, emit)


def _check_invariants(hyps, frames):
    for y, s, times, v in hyps:
        assert (v > -math.inf) == (s > -math.inf), (y, s, v)
        assert v <= s + 1e-12, (y, s, v)
        assert len(times) == len(y) and all(a < b for a, b in zip(times, times[1:])), (y, times)
        assert all(u <= f < frames for u, f in enumerate(times)), (y, times)


@pytest.mark.parametrize("beam", [4, 16])
@pytest.mark.parametrize("seed", range(5))
def test_invariants_hold_on_pruned_searches(beam, seed):
    """V 20, T 14: v is finite iff the sum is, v <= the sum, one strictly increasing frame per token, u <= times[u] < frames."""
    V = 20
    x = _peaked(np.random.default_rng(seed), T, V, sharp=4.0, scale=2.0)
    _check_invariants(prefix_beam_times_oracle(x, T, beam, 4, 0, nbest=beam)[0], T)
    table = TableModel(V, seed, blank=BLANK)
    _check_invariants(frame_beam_times_oracle(table.logits_fn(0), T, beam, 4, BLANK, normalize=False, nbest=beam)[0], T)


def test_times_state_sizes_match_the_header():
    from espresso_amd import _lib

    assert all(name in _lib.parse_header() for name in (
        "ea_ctc_prefix_beam_times_workspace_bytes", "ea_ctc_prefix_beam_times_step", "ea_ctc_prefix_beam_times_finish",
        "ea_ctc_prefix_beam_stream_times_state_bytes", "ea_ctc_prefix_beam_stream_times_reset", "ea_ctc_prefix_beam_stream_times_step",
        "ea_ctc_prefix_beam_stream_times_finish", "ea_rnnt_frame_beam_times_workspace_bytes", "ea_rnnt_frame_beam_times_step",
        "ea_rnnt_frame_beam_times_finish", "ea_rnnt_frame_beam_stream_times_state_bytes", "ea_rnnt_frame_beam_stream_times_reset",
        "ea_rnnt_frame_beam_stream_times_step", "ea_rnnt_frame_beam_stream_times_finish"))
    header = open(_lib.HEADER_PATH).read()
    assert "times words = 4 * beam + 2 + 2 * cap" in header and "times words = 2 * beam + 2 + 2 * cap" in header
    try:
        lib = _lib.lib()
    except _lib.EspressoAmdLibraryError:
        pytest.skip("the library is not built")
    for mf, beam in [(1, 1), (7, 3), (100, 5), (250, 10), (1000, 64), (33, 16)]:
        assert lib.ea_ctc_prefix_beam_stream_times_state_bytes(mf, beam) == 4 * ctc_times_words(mf, beam)
        assert lib.ea_rnnt_frame_beam_stream_times_state_bytes(mf, beam) == 4 * rnnt_times_words(mf, beam)
        for nb in (1, 5):
            assert lib.ea_ctc_prefix_beam_times_workspace_bytes(nb, mf, beam) == 4 * nb * ctc_times_words(mf, beam)
            assert lib.ea_rnnt_frame_beam_times_workspace_bytes(nb, mf, beam) == 4 * nb * rnnt_times_words(mf, beam)
    assert lib.ea_ctc_prefix_beam_times_workspace_bytes(2, 0, 4) == 4 * 2 * ctc_times_words(0, 4)  # T = 0: node 0 alone
    for fn in (lib.ea_ctc_prefix_beam_stream_times_state_bytes, lib.ea_rnnt_frame_beam_stream_times_state_bytes):
        assert fn(10, 65) == 0 and fn(0, 4) == 0 and fn(10, 0) == 0
    for fn in (lib.ea_ctc_prefix_beam_times_workspace_bytes, lib.ea_rnnt_frame_beam_times_workspace_bytes):
        assert fn(1, 4, 65) == 0 and fn(0, 4, 4) == 0 and fn(1, -1, 4) == 0


# =============================================================================================================== CPU: CLI and CTM
def _main(argv):
    from espresso_amd import speech_recognize as sr

    return sr.main(["--path", "/nonexistent.pt", "--dict", "/nonexistent.txt", "--wav-scp", "/nonexistent.scp", *argv])


@pytest.mark.parametrize("extra", [["--search", "beam"], ["--search", "ctc"], ["--search", "transducer_greedy"], ["--search", "transducer_beam"],
                                   ["--search", "ctc_beam", "--ngram-lm", "lm.arpa"], [],
                                   ["--search", "ctc", "--streaming"], ["--search", "ctc_beam", "--ngram-lm", "lm.arpa", "--streaming"]])
def test_cli_refuses_ctm_elsewhere(extra, tmp_path):
    """Every search without time stamps refuses --ctm by name before anything is loaded (no file exists) or written."""
    out = tmp_path / "out.ctm"
    with pytest.raises(NotImplementedError, match="--ctm"):
        _main(["--ctm", str(out), *extra])
    assert not out.exists()


def test_cli_ctm_options_reach_the_decoders():
    from espresso_amd import speech_align, speech_recognize as sr

    def args(*extra):
        return sr.get_parser().parse_args(["--path", "m.pt", "--dict", "d.txt", "--wav-scp", "w.scp", *extra])

    a = args("--search", "ctc_beam")
    assert (a.ctm, a.ctm_unit) == (None, "token")
    unit = next(x for x in speech_align.get_parser()._actions if x.dest == "unit")
    ctm_unit = next(x for x in sr.get_parser()._actions if x.dest == "ctm_unit")
    assert (ctm_unit.choices, ctm_unit.default) == (unit.choices, unit.default)
    d = _dictionary(8)
    for search in ("ctc_beam", "transducer_frame_beam"):
        assert sr.build_generator(args("--search", search), None, d).token_times is False
        assert sr.build_generator(args("--search", search, "--ctm", "o.ctm", "--ctm-unit", "word"), None, d).token_times is True
    on, off = args("--search", "ctc_stream_beam", "--streaming", "--ctm", "o.ctm"), args("--search", "ctc_stream_beam", "--streaming")
    assert sr.ctc_stream_beam_options(on)["token_times"] is True and "token_times" not in sr.ctc_stream_beam_options(off)
    assert sr.stream_beam_options(on)["token_times"] is True and "token_times" not in sr.stream_beam_options(off)
    for search, extra in (("ctc_beam", []), ("ctc_stream_beam", ["--streaming"]), ("transducer_frame_beam", []),
                          ("transducer_stream_beam", ["--streaming"])):
        sr.check_ctm_args(args("--search", search, "--ctm", "o.ctm", *extra))  # accepted
    from espresso_amd.tools.streaming_ctc_prefix_beam_decoder import StreamingCTCPrefixBeamDecoder

    assert StreamingCTCPrefixBeamDecoder(d, 2, 8, token_times=True).token_times is True
    assert StreamingCTCPrefixBeamDecoder(d, 2, 8).token_times is False


def test_ctm_lines_of_a_hand_made_hypothesis():
    """Tokens span [start, start + 1) frames; a word runs from its first token's start to its last token's start + 1; stripped
    symbols carry no line; the confidence column stays 1.00."""
    from espresso_amd import speech_recognize as sr
    from espresso_amd.data.asr_dictionary import AsrDictionary
    from espresso_amd.tools.beam_common import hyps_from_tensors

    d = AsrDictionary.from_symbols(["a", "b", "<space>", "c"], enable_bos=True)
    ia, ib, isp, ic = (d.index(s) for s in ("a", "b", "<space>", "c"))
    toks = [ia, ib, isp, ic, d.eos()]
    tokens = torch.full((1, 2, 7), d.pad(), dtype=torch.int32)
    tokens[0, 0, :5] = torch.tensor(toks)
    times = torch.full((1, 2, 7), -1, dtype=torch.int32)
    times[0, 0, :5] = torch.tensor([2, 3, 7, 9, 12])
    hyps = hyps_from_tensors(tokens, torch.tensor([[5, 0]]), torch.tensor([[-3.5, -math.inf]]), torch.tensor([1]), times,
                             torch.tensor([[-4.25, -math.inf]]))
    assert len(hyps) == 1 and len(hyps[0]) == 1
    h = hyps[0][0]
    assert h["times"].dtype == torch.int64 and h["times"].tolist() == [2, 3, 7, 9, 12] and float(h["viterbi_score"]) == -4.25
    assert h["tokens"].tolist() == toks and float(h["score"]) == -3.5
    assert "times" not in hyps_from_tensors(tokens, torch.tensor([[5, 0]]), torch.tensor([[-3.5, -math.inf]]), torch.tensor([1]))[0][0]
    strip = {d.eos(), d.pad()}
    assert sr.hypothesis_ctm_lines("u1", h, d, strip, "token", 0.04) == [
        "u1 1 0.080 0.040 a 1.00", "u1 1 0.120 0.040 b 1.00", "u1 1 0.280 0.040 <space> 1.00", "u1 1 0.360 0.040 c 1.00"]
    assert sr.hypothesis_ctm_lines("u1", h, d, strip, "word", 0.04) == ["u1 1 0.080 0.080 ab 1.00", "u1 1 0.360 0.040 c 1.00"]


# =============================================================================================================== GPU
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


# --------------------------------------------------------------------------------------------------------------- CTC: the cases
LM_WEIGHT, BONUS = 0.4, 0.2


def _ctc_case(V, beam, K, seed, dtype="fp32", config="plain", lens=LENS):
    return dict(V=V, beam=beam, K=K, seed=seed, dtype=dtype, config=config, lens=lens)


# V 20, B 5, T 14, lengths [14, 0, 1, 9, 12]; (beam, K) over {(1, 1), (4, 4), (16, 4), (64, 4)} in fp32, one bf16 case, one V 5200
# case (beyond the columns staged in LDS), the tiny LM, a context graph, both
CTC_CASES = [
    _ctc_case(20, 1, 1, 0), _ctc_case(20, 4, 4, 0), _ctc_case(20, 16, 4, 0), _ctc_case(20, 64, 4, 0),
    _ctc_case(20, 4, 4, 0, dtype="bf16"),
    _ctc_case(5200, 4, 4, 0, lens=np.array([3, 2], dtype=np.int32)),
    _ctc_case(20, 4, 4, 0, config="lm"), _ctc_case(20, 16, 4, 0, config="graph"), _ctc_case(20, 4, 4, 11, config="graph_lm"),
]


def _ctc_id(c):
    return "V{V}-b{beam}-K{K}-{dtype}-{config}".format(**c)


def _ctc_bound(c):
    """(what the pruning margin must exceed, what every Viterbi gap must exceed, the bound of the scores): twice the bounds; the
    LM terms of a score carry LM_TOL each (bf16 LM on the device against the fp32 oracle LM), a Viterbi score has none."""
    lm = LM_WEIGHT * LM_TOL * (int(c["lens"].max()) + 1) if "lm" in c["config"] else 0.0
    return 2 * (SCORE_TOL + lm), 2 * SCORE_TOL, SCORE_TOL + lm


class _CtcCase:
    """Inputs (as the kernel sees them: bf16-rounded for bf16), dictionary, options and the oracle of every utterance."""

    def __init__(self, c):
        self.c = c
        V, lens = c["V"], c["lens"]
        self.d = _dictionary(V - 5)
        assert len(self.d) == V
        nb, nt = len(lens), int(lens.max())
        rng = np.random.default_rng(c["seed"])
        if V > 5120:  # the frames' best tokens lie beyond the staged columns
            z = rng.standard_normal((nb * nt, V))
            for boost in (6.0, 5.0, 4.5, 4.0):
                z[np.arange(nb * nt), rng.integers(5120, V, nb * nt)] += boost
            z[rng.random(nb * nt) < 0.4, 0] += 6.5
            x = (z - np.logaddexp.reduce(z, axis=1, keepdims=True)).reshape(nb, nt, V)
        else:
            x = _peaked(rng, nb * nt, V, sharp=4.0, scale=2.0).reshape(nb, nt, V)
        self.dtype = torch.bfloat16 if c["dtype"] == "bf16" else torch.float32
        self.x32 = torch.from_numpy(x).to(torch.float32)
        self.x_seen = self.x32.to(self.dtype).to(torch.float32).numpy().astype(np.float64)
        self.lens, self.nbest = lens, min(c["beam"], 3)
        self.phrases = grid_phrases(self.x_seen, lens, self.d.bos()) if "graph" in c["config"] else None
        self.graph = _graph(self.phrases, V) if self.phrases is not None else None
        self.lm_seed = 3

    @functools.cached_property
    def lm_fn(self):
        return _cpu_lm_fn(_tiny_lm(self.d, seed=self.lm_seed), self.d) if "lm" in self.c["config"] else None

    def oracle(self, b):
        c, d, V = self.c, self.d, self.c["V"]
        lm_fn, has_lm = self.lm_fn, "lm" in self.c["config"]
        kw = dict(lm_fn=lm_fn, lm_weight=LM_WEIGHT, bonus=BONUS, eos=d.eos()) if has_lm else {}
        if self.graph is not None:
            kw = dict(lm_fn=bias_lm_fn(self.graph, V, lm_fn, LM_WEIGHT if has_lm else 0.0, d.eos()), lm_weight=1.0, eos=V,
                      bonus=BONUS if has_lm else 0.0)
        return prefix_beam_times_oracle(self.x_seen[b], int(self.lens[b]), c["beam"], c["K"], d.bos(), nbest=self.nbest, **kw)

    @functools.cached_property
    def refs(self):
        return [self.oracle(b) for b in range(len(self.lens))]

    def decoder(self, token_times=True, nbest=None):
        from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder

        has_lm = "lm" in self.c["config"]
        lm = _tiny_lm(self.d, seed=self.lm_seed).to(DEV) if has_lm else None
        return CTCPrefixBeamSearchDecoder([None], self.d, beam_size=self.c["beam"], nbest=self.nbest if nbest is None else nbest,
                                          beam_size_token=self.c["K"], lm_model=lm, lm_weight=LM_WEIGHT if has_lm else 0.0,
                                          insertion_bonus=BONUS if has_lm else 0.0, context_graph=self.graph, token_times=token_times)

    def device_inputs(self):
        return self.x32.to(DEV, self.dtype), torch.from_numpy(self.lens).to(DEV)


@functools.lru_cache(maxsize=None)
def _ctc_built(i):
    return _CtcCase(CTC_CASES[i])


def test_ctc_case_margins_are_clear():
    """Every case without the LSTM LM on the CPU (the LM cases take the oracle LM a while: the GPU test asserts theirs)."""
    for i, c in enumerate(CTC_CASES):
        if "lm" not in c["config"] and c["V"] <= 100:
            need_margin, need_gap, _ = _ctc_bound(c)
            r = _ctc_built(i)
            assert min(m for _, m, _ in r.refs) > need_margin and min(g for _, _, g in r.refs) > need_gap, _ctc_id(c)


def _times_hyps(out, b):
    tokens, lengths, scores, nhyp, times, vscores = (t.cpu() for t in out)
    res = []
    for i in range(int(nhyp[b])):
        n = int(lengths[b, i])
        assert bool((times[b, i, n:] == -1).all()), (b, i, times[b, i])
        res.append((tuple(tokens[b, i, :n].tolist()), float(scores[b, i]), tuple(times[b, i, :n].tolist()), float(vscores[b, i])))
    for i in range(int(nhyp[b]), tokens.shape[1]):
        assert bool((times[b, i] == -1).all()) and float(vscores[b, i]) == -math.inf and int(lengths[b, i]) == 0
    return res


def _compare_with_oracle(got, ref, score_bound, v_bound, where):
    """Tokens, n-best order and times equal; scores and Viterbi scores within their bounds.  Returns the worst differences."""
    assert [h[0] for h in got] == [h[0] for h in ref], (where, got, ref)
    ws = wv = 0.0
    for (y, s, times, v), (_, rs, rtimes, rv) in zip(got, ref):
        assert times == rtimes, (where, y, times, rtimes)
        if rs == -math.inf:
            assert s == -math.inf and v == -math.inf and rv == -math.inf, (where, y, s, v)
            continue
        ws, wv = max(ws, abs(s - rs)), max(wv, abs(v - rv))
        assert abs(s - rs) < score_bound and abs(v - rv) < v_bound, (where, y, s, rs, v, rv)
    return ws, wv


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CTC_CASES)), ids=[_ctc_id(c) for c in CTC_CASES])
def test_ctc_step_kernels_vs_oracle(i):
    """The times kernels through CTCPrefixBeamSearchDecoder(token_times=True).search: tokens, n-best order and times equal the
    oracle's, scores within the existing bound, vscores within SCORE_TOL; every utterance of every case."""
    _need_gpu()
    r = _ctc_built(i)
    need_margin, need_gap, score_bound = _ctc_bound(r.c)
    margin, vgap = min(m for _, m, _ in r.refs), min(g for _, _, g in r.refs)
    assert margin > need_margin and vgap > need_gap, (margin, vgap)
    out = r.decoder().search(*r.device_inputs())
    ws = wv = 0.0
    n_tok = 0
    for b in range(len(r.lens)):
        got = _times_hyps(out, b)
        a, b_ = _compare_with_oracle(got, r.refs[b][0], score_bound, SCORE_TOL, (_ctc_id(r.c), b))
        ws, wv = max(ws, a), max(wv, b_)
        n_tok += sum(len(h[0]) for h in got)
        for y, s, times, v in got:
            assert all(a_ < c_ for a_, c_ in zip(times, times[1:])) and all(u <= f < int(r.lens[b]) for u, f in enumerate(times))
    assert n_tok > 0
    print(f"{_ctc_id(r.c)}: margin {margin:.3g}, Viterbi gap {vgap:.3g}, max |score - oracle| {ws:.2e}, max |vscore - oracle| {wv:.2e}")
    if len(r.lens) == B:  # in_len 0: the empty hypothesis, no tokens, Viterbi score 0 (its score: the LM's end-of-sentence term)
        empty = _times_hyps(out, 1)
        assert len(empty) == 1 and (empty[0][0], empty[0][2], empty[0][3]) == ((), (), 0.0)
        assert empty[0][1] == 0.0 or "lm" in r.c["config"]


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CTC_CASES)), ids=[_ctc_id(c) for c in CTC_CASES])
def test_ctc_times_on_equals_times_off(i):
    """The decoder with and without token_times: tokens, lengths, scores and nhyp are torch.equal."""
    _need_gpu()
    r = _ctc_built(i)
    xd, lens = r.device_inputs()
    on, off = r.decoder(True).search(xd, lens), r.decoder(False).search(xd, lens)
    assert len(on) == 6 and len(off) == 4
    for a, b in zip(on, off):
        assert torch.equal(a, b)


def _synthetic_lm_rows(rows, parent, token, keep, emb):
    """A stand-in for an LM update on the device: a function of the triple alone, so two searches that write equal triples get
    equal rows."""
    new = torch.log_softmax(0.5 * rows[parent.long()] + emb[token.long()], dim=1)
    return torch.where(keep.bool()[:, None], rows[parent.long()], new)


@pytest.mark.gpu
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("beam,K", [(4, 4), (16, 4)])
def test_ctc_triples_with_an_lm_are_those_of_the_search_without_times(beam, K, biased):
    """The offline kernels frame by frame with LM rows, with and without times, each on the rows its own triples give: every
    frame's (parent, token, keep) and the finish are torch.equal; then the same through the streamed kernels."""
    _need_gpu()
    from espresso_amd import kernels as Kn

    r = _CtcCase(_ctc_case(20, beam, K, 1, config="graph" if biased else "plain"))
    V, d = 20, r.d
    xd, lens = r.device_inputs()
    x2 = xd.view(B * T, V)
    g = r.graph.cuda(DEV) if biased else None
    N = B * beam
    gen = torch.Generator().manual_seed(5)
    emb = torch.randn(V, V, generator=gen).to(DEV)
    rows0 = torch.log_softmax(torch.randn(1, V, generator=gen), dim=1).to(DEV).expand(N, V).contiguous()
    kw = dict(B=B, T=T, V=V, beam=beam, K=K, blank=d.bos(), lm_weight=LM_WEIGHT, ins_bonus=BONUS)

    def run(times):
        ws = (Kn.ctc_prefix_beam_bias_workspace if biased else Kn.ctc_prefix_beam_workspace)(B, T, beam, DEV)
        tws = Kn.ctc_prefix_beam_times_workspace(B, T, beam, DEV).fill_(0xA5) if times else None
        rows, triples = rows0, []
        out = (torch.empty(N, dtype=torch.int32, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV),
               torch.empty(N, dtype=torch.uint8, device=DEV))
        for t in range(T):
            if times:
                Kn.ctc_prefix_beam_times_step(x2, lens, ws, tws, t0=t, t1=t + 1, graph=g, lm_rows=rows, lm_out=out, **kw)
            elif biased:
                Kn.ctc_prefix_beam_bias_step(x2, lens, ws, g, t0=t, t1=t + 1, lm_rows=rows, lm_out=out, **kw)
            else:
                Kn.ctc_prefix_beam_step(x2, lens, ws, t0=t, t1=t + 1, lm_rows=rows, lm_out=out, **kw)
            triples.append(tuple(o.clone() for o in out))
            rows = _synthetic_lm_rows(rows, *out, emb)
        fkw = dict(lm_rows=rows, lm_weight=LM_WEIGHT, ins_bonus=BONUS, eos=d.eos())
        if times:
            fin = Kn.ctc_prefix_beam_times_finish(ws, tws, B, T, beam, 3, PAD, graph=g, **fkw)
        elif biased:
            fin = Kn.ctc_prefix_beam_bias_finish(ws, g, B, T, beam, 3, PAD, **fkw)
        else:
            fin = Kn.ctc_prefix_beam_finish(ws, B, T, beam, 3, PAD, **fkw)
        return triples, fin

    (tr_on, fin_on), (tr_off, fin_off) = run(True), run(False)
    for t in range(T):
        for a, b in zip(tr_on[t], tr_off[t]):
            assert torch.equal(a, b), t
    for a, b in zip(fin_on, fin_off):
        assert torch.equal(a, b)
    assert int((tr_on[5][2] == 0).sum()) > 0  # some rows appended a token

    # streamed: every stream fed one frame per call in its own slot, with and without times
    def run_streamed(times):
        state, _ = Kn.ctc_prefix_beam_stream_state(B, T, beam, DEV)
        slots = torch.arange(B, dtype=torch.int32, device=DEV)
        tstate = None
        if times:
            tstate, _ = Kn.ctc_prefix_beam_stream_times_state(B, T, beam, DEV)
            tstate.fill_(0xA5)
            Kn.ctc_prefix_beam_stream_times_reset(state, tstate, slots, T, beam)
        else:
            Kn.ctc_prefix_beam_stream_reset(state, slots, T, beam)
        rows, triples = rows0, []
        out = (torch.empty(N, dtype=torch.int32, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV),
               torch.empty(N, dtype=torch.uint8, device=DEV))
        packed = torch.cat([xd[b, : int(r.lens[b])] for b in range(B)])
        off = np.concatenate([[0], np.cumsum(r.lens)[:-1]])
        meta = torch.tensor([list(range(B)), r.lens.tolist(), off.tolist()], dtype=torch.int32, device=DEV)
        skw = dict(max_frames=T, V=V, beam=beam, K=K, blank=d.bos(), graph=g, lm_weight=LM_WEIGHT, ins_bonus=BONUS)
        for j in range(T):
            if times:
                Kn.ctc_prefix_beam_stream_times_step(packed, meta, state, tstate, j0=j, j1=j + 1, lm_rows=rows, lm_out=out, **skw)
            else:
                Kn.ctc_prefix_beam_stream_step(packed, meta, state, j0=j, j1=j + 1, lm_rows=rows, lm_out=out, **skw)
            triples.append(tuple(o.clone() for o in out))
            rows = _synthetic_lm_rows(rows, *out, emb)
        fkw = dict(graph=g, lm_rows=rows, lm_weight=LM_WEIGHT, ins_bonus=BONUS, eos=d.eos())
        if times:
            return triples, Kn.ctc_prefix_beam_stream_times_finish(state, tstate, slots, T, beam, 3, PAD, T, **fkw)
        return triples, Kn.ctc_prefix_beam_stream_finish(state, slots, T, beam, 3, PAD, T, **fkw)

    (st_on, sfin_on), (st_off, sfin_off) = run_streamed(True), run_streamed(False)
    for t in range(T):
        for a, b, c in zip(st_on[t], st_off[t], tr_off[t]):
            assert torch.equal(a, b) and torch.equal(a, c), t
    for a, b in zip(sfin_on, sfin_off):
        assert torch.equal(a, b)
    for a, b in zip(sfin_on, fin_on):  # times and vscores included: streamed = offline
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------------- CTC: streamed
def _ctc_offline_prefixes(r, g, nbest):
    """The offline times search of the first L frames of every utterance, for every L in 0 .. T: fins[L] = the six finish tensors
    (tokens and times [B][nbest][T])."""
    from espresso_amd import kernels as Kn

    c, d = r.c, r.d
    V, beam, K = c["V"], c["beam"], c["K"]
    xd, lens = r.device_inputs()
    fins = []
    for L in range(T + 1):
        ws = (Kn.ctc_prefix_beam_workspace if g is None else Kn.ctc_prefix_beam_bias_workspace)(B, T, beam, DEV)
        tws = Kn.ctc_prefix_beam_times_workspace(B, T, beam, DEV).fill_(0x5A)
        Kn.ctc_prefix_beam_times_step(xd.view(B * T, V), torch.clamp(lens, max=L), ws, tws, B, T, V, beam, K, d.bos(), 0, T, graph=g)
        fins.append(Kn.ctc_prefix_beam_times_finish(ws, tws, B, T, beam, nbest, PAD, graph=g))
    return fins


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("beam,K,biased", [(4, 4, False), (16, 4, True), (64, 4, False)])
def test_ctc_streamed_times_equal_offline_bit_for_bit(beam, K, biased, dtype):
    """The streamed times kernels over uneven pieces, idle entries and shuffled slots of a larger buffer, for two values of
    max_frames: after every piece the finish of every listed stream (tokens, lengths, scores, nhyp, times, vscores) is torch.equal
    to the offline times search over the frames consumed so far; an idle entry leaves its slot and its times slot untouched, and
    the finish leaves both states untouched."""
    _need_gpu()
    from espresso_amd import kernels as Kn

    r = _CtcCase(_ctc_case(20, beam, K, 2, dtype=dtype, config="graph" if biased else "plain"))
    V, d, nbest = 20, r.d, min(beam, 3)
    g = r.graph.cuda(DEV) if biased else None
    xd, _ = r.device_inputs()
    fins = _ctc_offline_prefixes(r, g, nbest)
    lens = r.lens.tolist()
    for max_frames, max_streams, seed in ((T, 8, 0), (40, 6, 1)):
        rng = np.random.default_rng(seed)
        slot_of = rng.permutation(max_streams)[:B].tolist()
        state, _ = Kn.ctc_prefix_beam_stream_state(max_streams, max_frames, beam, DEV)
        tstate, nbytes = Kn.ctc_prefix_beam_stream_times_state(max_streams, max_frames, beam, DEV)
        assert nbytes == 4 * ctc_times_words(max_frames, beam)
        state.fill_(0xA5)
        tstate.fill_(0xA5)
        Kn.ctc_prefix_beam_stream_times_reset(state, tstate, torch.tensor(slot_of, dtype=torch.int32, device=DEV), max_frames, beam)
        pos, pieces, rounds = [0] * B, [1, 3, 2, 5, 1, 4], 0

        def readouts(entries):
            slots = torch.tensor([slot_of[b] for b in entries], dtype=torch.int32, device=DEV)
            before, tbefore = state.clone(), tstate.clone()
            fin = Kn.ctc_prefix_beam_stream_times_finish(state, tstate, slots, max_frames, beam, nbest, PAD, T, graph=g)
            assert torch.equal(state, before) and torch.equal(tstate, tbefore)
            for e, b in enumerate(entries):
                for got, want in zip(fin, fins[pos[b]]):
                    assert torch.equal(got[e], want[b]), (b, pos[b], got[e], want[b])

        readouts(list(range(B)))
        while any(pos[b] < lens[b] for b in range(B)):
            entries = [b for b in rng.permutation(B).tolist() if rng.random() < 0.8]
            if not entries:
                continue
            n_new = [min(pieces[(rounds + 2 * b) % len(pieces)], lens[b] - pos[b]) if rng.random() < 0.85 else 0 for b in entries]
            rounds += 1
            rows = [xd[b, pos[b]:pos[b] + c] for b, c in zip(entries, n_new)]
            off = np.concatenate([[0], np.cumsum(n_new)[:-1]]).astype(int).tolist()
            meta = torch.tensor([[slot_of[b] for b in entries], n_new, off], dtype=torch.int32, device=DEV)
            packed = torch.cat(rows) if sum(n_new) else xd[0, :1]  # (an all-idle call still gets a valid pointer)
            idle = {b: (state[slot_of[b]].clone(), tstate[slot_of[b]].clone()) for b, c in zip(entries, n_new) if c == 0}
            Kn.ctc_prefix_beam_stream_times_step(packed, meta, state, tstate, max_frames, V, beam, K, d.bos(), j0=0, j1=max(n_new + [0]),
                                                 graph=g)
            for b, c in zip(entries, n_new):
                pos[b] += c
            for b, (s0, t0) in idle.items():
                assert torch.equal(state[slot_of[b]], s0) and torch.equal(tstate[slot_of[b]], t0), b
            readouts(entries)
        assert pos == lens
        readouts(list(range(B)))
    # and the last offline finish is the search the oracle describes
    tokens, lengths, _, nhyp, times, _ = (t.cpu() for t in fins[T])
    assert int(nhyp.min()) >= 1 and int(lengths[1, 0]) == 0
    for b in range(B):
        n = int(lengths[b, 0])
        tm = times[b, 0, :n].tolist()
        assert all(a < c for a, c in zip(tm, tm[1:])) and all(u <= f < lens[b] for u, f in enumerate(tm)), (b, tm)


@pytest.mark.gpu
def test_ctc_times_entries_refuse_bad_arguments():
    _need_gpu()
    from espresso_amd import kernels as Kn

    nb, nt, V, beam = 1, 2, 8, 2
    ws, tws = Kn.ctc_prefix_beam_workspace(nb, nt, beam, DEV), Kn.ctc_prefix_beam_times_workspace(nb, nt, beam, DEV)
    x = torch.zeros(nb * nt, V, device=DEV)
    in_len = torch.ones(nb, dtype=torch.int32, device=DEV)
    for kw in (dict(K=8), dict(t1=3), dict(blank=8), dict(beam=65)):
        a = dict(beam=beam, K=2, blank=0, t0=0, t1=2)
        a.update(kw)
        with pytest.raises((RuntimeError, AssertionError)):
            Kn.ctc_prefix_beam_times_step(x, in_len, ws, tws, nb, nt, V, a["beam"], a["K"], a["blank"], a["t0"], a["t1"])
    lib = Kn._lib.lib()
    out = Kn._finish_outputs(nb, 1, nt, DEV) + Kn._times_outputs(nb, 1, nt, DEV)
    ptr = [Kn._p(t) for t in out]
    assert lib.ea_ctc_prefix_beam_times_finish(Kn._p(ws), None, None, 0, 0.0, 0.0, -1, None, 0, nb, nt, beam, 1, PAD, *ptr, Kn._stream()) == -2
    assert lib.ea_ctc_prefix_beam_times_finish(Kn._p(ws), Kn._p(tws), None, 0, 0.0, 0.0, -1, None, 0, nb, nt, beam, 1, PAD, *ptr[:4], None,
                                               ptr[5], Kn._stream()) == -2
    assert lib.ea_ctc_prefix_beam_times_step(Kn._p(x), V, 0, Kn._p(in_len), Kn._p(ws), None, None, 0, None, None, None, None, None, None,
                                             0, 0, nb, nt, V, beam, 2, 0, 0.0, 0.0, 0, nt, Kn._stream()) == -2


# --------------------------------------------------------------------------------------------------------------- CTC: exhaustive
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
def test_ctc_times_equal_the_forced_aligner_on_every_hypothesis(seed):
    """V 3, T 5, beam 64, K 2, nbest 64: no pruning, so every finite hypothesis' times are the token starts and its vscore the
    score of K.ctc_viterbi_align on the same rows and tokens: the aligner predates the time stamps and shares no code with them."""
    _need_gpu()
    from espresso_amd import kernels as Kn

    V, Tn, beam, blank = 3, 5, 64, 0  # (no dictionary is this small: the kernels are called directly)
    x = np.random.default_rng(seed).standard_normal((Tn, V)) * 1.5
    x = (x - np.logaddexp.reduce(x, axis=1, keepdims=True)).astype(np.float32)
    brute = ctc_best_alignments(x.astype(np.float64), blank)
    assert min(lead for _, _, lead in brute.values()) > 2 * SCORE_TOL  # every best alignment is clear of the fp32 error
    xd = torch.from_numpy(x).to(DEV)[None].contiguous()
    ws, tws = Kn.ctc_prefix_beam_workspace(1, Tn, beam, DEV), Kn.ctc_prefix_beam_times_workspace(1, Tn, beam, DEV)
    Kn.ctc_prefix_beam_times_step(xd.view(Tn, V), torch.tensor([Tn], dtype=torch.int32, device=DEV), ws, tws, 1, Tn, V, beam, 2, blank, 0, Tn)
    hyps = _times_hyps(Kn.ctc_prefix_beam_times_finish(ws, tws, 1, Tn, beam, beam, PAD), 0)
    finite = [h for h in hyps if h[1] > -math.inf]
    assert {h[0] for h in finite} == set(brute)
    n = len(finite)
    targets = torch.zeros(n, Tn, dtype=torch.int32)
    for k, h in enumerate(finite):
        targets[k, : len(h[0])] = torch.tensor(h[0], dtype=torch.int32)
    tgt_len = torch.tensor([len(h[0]) for h in finite], dtype=torch.int32, device=DEV)
    start, _, _, score = Kn.ctc_viterbi_align(xd.expand(n, Tn, V).contiguous().view(n * Tn, V), targets.to(DEV),
                                              torch.full((n,), Tn, dtype=torch.int32, device=DEV), tgt_len, n, Tn, V, blank)
    start, score = start.cpu(), score.cpu()
    for k, (y, s, times, v) in enumerate(finite):
        assert list(times) == start[k, : len(y)].tolist() == list(brute[y][1]), (y, times, start[k], brute[y])
        assert abs(v - float(score[k])) < SCORE_TOL and abs(v - brute[y][0]) < SCORE_TOL, (y, v, float(score[k]), brute[y][0])


# --------------------------------------------------------------------------------------------------------------- transducer
def _rnnt_case(V, beam, K, seed, biased=False, **opts):
    return dict(V=V, beam=beam, K=K, seed=seed, biased=biased, opts=opts)


# V 20, B 5, T 14, lengths [14, 0, 1, 9, 12]; (beam, K) over {(1, 1), (4, 4), (16, 4), (64, 4)}, one V 5200 case, both LM layouts,
# model_predicts_eos, a context graph, graph + LM
RNNT_CASES = [
    _rnnt_case(20, 1, 1, 0), _rnnt_case(20, 4, 4, 0), _rnnt_case(20, 16, 4, 17), _rnnt_case(20, 64, 4, 2),
    _rnnt_case(5200, 4, 4, 0),
    _rnnt_case(20, 4, 4, 1, lm="blank", lm_weight=0.6), _rnnt_case(20, 4, 4, 0, lm="no_blank", lm_weight=0.6),
    _rnnt_case(20, 4, 4, 1, predicts_eos=True),
    _rnnt_case(20, 16, 4, 1, biased=True), _rnnt_case(20, 4, 4, 1, biased=True, lm="blank", lm_weight=0.6, normalize=False),
]


def _rnnt_id(c):
    return "V{V}-b{beam}-K{K}".format(**c) + ("-graph" if c["biased"] else "") + "".join(f"-{k}={v}" for k, v in c["opts"].items())


def _rnnt_bound(terms):
    return SCORE_TOL + 8 * TERM_TOL * terms


RNNT_MARGIN = 2 * _rnnt_bound(2 * T)  # twice the largest bound: T frame terms, and as many bias terms at most


class _RnntCase(_Case):
    """tests.test_transducer_hotword_beam._Case (models, rows fed to the kernels, biased oracle; an empty graph for an unbiased
    case, whose oracle is then the unbiased one) with the times oracle of every utterance."""

    def __init__(self, c):
        super().__init__(dict(V=c["V"], beam=c["beam"], K=c["K"], seed=c["seed"], opts=c["opts"]), phrases=None if c["biased"] else [])
        self.biased = c["biased"]
        self.trefs = [frame_beam_times_oracle(self.table.logits_fn(b), self.lens[b], self.beam, self.K, BLANK,
                                              graph=self.graph if self.biased else None, normalize=self.normalize, nbest=self.nbest,
                                              **self.kw) for b in range(self.B)]
        for tr, ref in zip(self.trefs, self.refs):  # the two oracles agree on tokens, scores, triples
            assert [(y, s) for y, s, _, _ in tr[0]] == [(y, s) for y, s in ref[0]] or not self.biased
            assert tr[1] == ref[1]
        self.tmargin, self.vgap, self.pmargin = (min(r[k] for r in self.trefs) for k in (2, 3, 4))
        self.own_slots = self.beam >= 64  # see _drive_from_own_triples


@functools.lru_cache(maxsize=None)
def _rnnt_built(i):
    return _RnntCase(RNNT_CASES[i])


class _TimesFamily:
    """The calls of tests.test_transducer_hotword_beam._Family for the times entry points (graph None: on the unbiased workspace
    and state); the times workspace / state is made with the beam's and rides along."""

    def __init__(self, graph):
        from espresso_amd import kernels as Kn

        g = self.g = None if graph is None else graph.cuda(DEV)
        self.plain = _Family(graph)
        self.partial = self.plain.partial

        def workspace(nb, nt, beam, dev):
            self.tws = Kn.rnnt_frame_beam_times_workspace(nb, nt, beam, dev).fill_(0x5A)
            return self.plain.workspace(nb, nt, beam, dev)

        def state(max_streams, max_frames, beam, dev):
            self.tstate, nbytes = Kn.rnnt_frame_beam_stream_times_state(max_streams, max_frames, beam, dev)
            assert nbytes == 4 * rnnt_times_words(max_frames, beam)
            self.tstate.fill_(0x5A)
            return self.plain.state(max_streams, max_frames, beam, dev)

        def sstep(x, si, nn, j, st, out, *a, **k):
            idle = [(int(s), self.tstate[int(s)].clone()) for s, c in zip(si.tolist(), nn.tolist()) if j >= c]
            Kn.rnnt_frame_beam_stream_times_step(x, si, nn, j, st, self.tstate, out, *a, graph=g, **k)
            for s, before in idle:
                assert torch.equal(self.tstate[s], before), s  # an entry that is not due leaves its times slot untouched

        def sfinish(st, slots, *a, **k):
            before = self.tstate.clone()
            out = Kn.rnnt_frame_beam_stream_times_finish(st, self.tstate, slots, *a, graph=g, **k)
            assert torch.equal(self.tstate, before)
            return out

        self.workspace, self.state, self.sstep, self.sfinish = workspace, state, sstep, sfinish
        self.step = lambda x, in_len, ws, out, *a, **k: Kn.rnnt_frame_beam_times_step(x, in_len, ws, self.tws, out, *a, graph=g, **k)
        self.finish = lambda ws, *a, **k: Kn.rnnt_frame_beam_times_finish(ws, self.tws, *a, graph=g, **k)
        self.reset = lambda st, slots, mf, beam: Kn.rnnt_frame_beam_stream_times_reset(st, self.tstate, slots, mf, beam, biased=g is not None)


def _rnnt_margins_clear(r):
    """Beam 64 keeps sixty-four neighbouring scores per frame and utterance in order: no seed keeps all of those apart over 14
    frames, so that case is driven from the kernels' own triples (the order of the slots is then the kernels') and needs only the
    margins that decide which hypotheses exist and which are returned; every other case needs the whole margin."""
    return (r.pmargin if r.own_slots else r.tmargin) > RNNT_MARGIN and r.vgap > RNNT_MARGIN


def test_transducer_case_margins_are_clear():
    for i, c in enumerate(RNNT_CASES):
        if c["V"] <= 100:
            r = _rnnt_built(i)
            assert _rnnt_margins_clear(r), (_rnnt_id(c), r.tmargin, r.pmargin, r.vgap)


def _drive_from_own_triples(r, fam):
    """The offline kernels of a family frame by frame, the rows of every frame built from the sequences the kernels' own triples
    give (the number of live slots after a frame is the oracle's; rows of dead slots and finished utterances are NaN).  After every
    frame the live sequences are the oracle's as a set.  Returns (the triples of every frame, the finish)."""
    nb, nt, V, beam = r.B, r.T, r.V, r.beam
    ws = fam.workspace(nb, nt, beam, DEV)
    in_len = torch.tensor(r.lens, dtype=torch.int32, device=DEV)
    out = (torch.empty(nb * beam, dtype=torch.int32, device=DEV), torch.empty(nb * beam, dtype=torch.int32, device=DEV),
           torch.empty(nb * beam, dtype=torch.uint8, device=DEV))
    seqs, want = [[()] for _ in range(nb)], [[()] for _ in range(nb)]
    triples = []
    for t in range(nt):
        x = np.full((nb * beam, V + 3), np.nan, dtype=np.float32)
        m = np.full((nb * beam, r.nlm), np.nan, dtype=np.float32)
        for b in range(nb):
            if t < r.lens[b]:
                for j, y in enumerate(seqs[b]):
                    x[b * beam + j, :V] = r.table.row(b, t, y)
                    if r.lm is not None:
                        m[b * beam + j] = r.lm.row(y)
        fam.step(torch.from_numpy(x).to(DEV)[:, :V], in_len, ws, out, nb, nt, V, beam, r.K, BLANK, t,
                 lm_rows=torch.from_numpy(m).to(DEV) if r.lm is not None else None, **r.step_kw)
        triples.append(tuple(o.clone() for o in out))
        parent, token, keep = (o.cpu().tolist() for o in out)
        for b in range(nb):
            if t < r.lens[b]:
                ref = r.trefs[b][1][t]
                want[b] = [want[b][p] + (() if k else (v,)) for p, v, k in ref]
                rows = range(b * beam, b * beam + len(ref))
                seqs[b] = [seqs[b][parent[n] - b * beam] + (() if keep[n] else (token[n],)) for n in rows]
                assert sorted(seqs[b]) == sorted(want[b]), (b, t)
    return triples, fam.finish(ws, nb, nt, beam, r.nbest, PAD, normalize=r.normalize)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(RNNT_CASES)), ids=[_rnnt_id(c) for c in RNNT_CASES])
def test_transducer_step_kernels_vs_oracle(i):
    """The offline times kernels frame by frame on table logits: the triples of every frame, tokens, n-best order and times equal
    the oracle's; scores and vscores within 1e-4 + 8 * 2^-20 * terms (frames, plus tokens with a graph).  Then the search
    without times on the same rows: every frame's triples and the finish after every frame are torch.equal."""
    _need_gpu()
    r = _rnnt_built(i)
    assert _rnnt_margins_clear(r), (r.tmargin, r.pmargin, r.vgap)
    graph = r.graph if r.biased else None
    if r.own_slots:
        triples, fin = _drive_from_own_triples(r, _TimesFamily(graph))
        off_triples, off_fin = _drive_from_own_triples(r, _Family(graph))
        fins, off_fins = [None, fin], [None, off_fin]
    else:
        triples, fins, _ = _offline(r, _TimesFamily(graph))
    for t, tr in enumerate(triples if not r.own_slots else []):
        tr = tr.cpu().tolist()
        for b in range(r.B):
            got = [tuple(x) for x in tr[b]]
            if t >= r.lens[b]:
                assert got == [(j, BLANK, 1) for j in range(r.beam)], (b, t, got)
                continue
            want = r.trefs[b][1][t]
            assert got[: len(want)] == want and got[len(want):] == [(0, BLANK, 1)] * (r.beam - len(want)), (b, t, got, want)
    ws = wv = 0.0
    for b in range(r.B):
        got = _times_hyps(fins[-1], b)
        bound = _rnnt_bound(r.lens[b] + (max([len(h[0]) for h in got] + [0]) if r.biased else 0))
        a, b_ = _compare_with_oracle(got, r.trefs[b][0], bound, _rnnt_bound(r.lens[b]), (_rnnt_id(RNNT_CASES[i]), b))
        ws, wv = max(ws, a), max(wv, b_)
        for y, s, times, v in got:
            assert all(a_ < c_ for a_, c_ in zip(times, times[1:])) and all(u <= f < r.lens[b] for u, f in enumerate(times))
    assert _times_hyps(fins[-1], 1) == [((), 0.0, (), 0.0)]
    print(f"{_rnnt_id(RNNT_CASES[i])}: margin {r.tmargin:.3g}, Viterbi gap {r.vgap:.3g}, max |score - oracle| {ws:.2e}, "
          f"max |vscore - oracle| {wv:.2e}")
    if not r.own_slots:
        off_triples, off_fins, _ = _offline(r, _Family(graph))
    for t in range(r.T):
        for a, b in zip(triples[t], off_triples[t]) if r.own_slots else [(triples[t], off_triples[t])]:
            assert torch.equal(a, b), t
    for on, off in zip(fins[1:], off_fins[1:]):
        assert len(on) == 6 and len(off) == 4
        for a, b in zip(on, off):
            assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("i", [1, 2, 5, 8, 9], ids=[_rnnt_id(RNNT_CASES[i]) for i in (1, 2, 5, 8, 9)])
def test_transducer_streamed_times_equal_offline_bit_for_bit(i):
    """The streamed times kernels over uneven pieces, idle entries and shuffled slots of a larger buffer, for two values of
    max_frames: every triple, and after every piece every finish tensor (times and vscores included), torch.equal to the offline
    times kernels after the same number of frames; then the streamed search without times gives the same triples and finishes."""
    _need_gpu()
    r = _rnnt_built(i)
    graph = r.graph if r.biased else None
    offline = _offline(r, _TimesFamily(graph))
    assert all(len(f) == 6 for f in offline[1][1:])
    for max_frames, max_streams, seed in ((r.T, 8, 0), (40, 6, 1)):
        _streamed(r, _TimesFamily(graph), offline, max_frames, max_streams, seed)
    _streamed(r, _Family(graph), offline, r.T, 8, 0)  # (zip stops at the four tensors the search without times returns)


@pytest.mark.gpu
def test_transducer_times_entries_refuse_bad_arguments():
    _need_gpu()
    from espresso_amd import kernels as Kn

    nb, nt, V, beam = 1, 2, 8, 2
    ws, tws = Kn.rnnt_frame_beam_workspace(nb, nt, beam, DEV), Kn.rnnt_frame_beam_times_workspace(nb, nt, beam, DEV)
    in_len = torch.ones(nb, dtype=torch.int32, device=DEV)
    out = (torch.empty(2, dtype=torch.int32, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV), torch.empty(2, dtype=torch.uint8, device=DEV))
    x = torch.zeros(2, V, device=DEV)
    for kw in (dict(K=8), dict(t=2), dict(blank=8), dict(eos=0), dict(temperature=0.0)):
        a = dict(K=2, blank=0, t=0)
        a.update(kw)
        with pytest.raises(RuntimeError, match="ea_rnnt_frame_beam_times_step"):
            Kn.rnnt_frame_beam_times_step(x, in_len, ws, tws, out, nb, nt, V, beam, **a)
    lib = Kn._lib.lib()
    fin = Kn._finish_outputs(nb, 1, nt, DEV) + Kn._times_outputs(nb, 1, nt, DEV)
    ptr = [Kn._p(t) for t in fin]
    assert lib.ea_rnnt_frame_beam_times_finish(Kn._p(ws), None, None, 0, nb, nt, beam, 1, PAD, 0, *ptr, Kn._stream()) == -2
    assert lib.ea_rnnt_frame_beam_times_finish(Kn._p(ws), Kn._p(tws), None, 0, nb, nt, beam, 3, PAD, 0, *ptr, Kn._stream()) == -2
    # T = 0: no step has run; the finish reads neither workspace
    ws0, tws0 = Kn.rnnt_frame_beam_workspace(2, 0, 3, DEV).fill_(0xFF), Kn.rnnt_frame_beam_times_workspace(2, 0, 3, DEV).fill_(0xFF)
    one = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    lengths, scores = torch.full((2, 2), 77, dtype=torch.int32, device=DEV), torch.full((2, 2), 77.0, device=DEV)
    nhyp, vs = torch.full((2,), 77, dtype=torch.int32, device=DEV), torch.full((2, 2), 77.0, device=DEV)
    Kn.check(lib.ea_rnnt_frame_beam_times_finish(Kn._p(ws0), Kn._p(tws0), None, 0, 2, 0, 3, 2, PAD, 1, Kn._p(one), Kn._p(lengths),
                                                 Kn._p(scores), Kn._p(nhyp), Kn._p(one), Kn._p(vs), Kn._stream()), "times_finish")
    assert nhyp.tolist() == [1, 1] and scores.tolist() == [[0.0, -math.inf]] * 2 and vs.tolist() == [[0.0, -math.inf]] * 2


# --------------------------------------------------------------------------------------------------------------- decoders
def _close_times(hyps):
    return [(tuple(h["tokens"].tolist()), tuple(h["times"].tolist()), float(h["viterbi_score"])) for h in hyps]


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["plain", "graph_lm"])
def test_ctc_decoders_with_token_times(config):
    """The streaming decoder with token_times closes every stream with the tokens, scores, times and Viterbi scores of the
    offline decoder with token_times (bit for bit), and neither its accept nor the offline search synchronises with the host."""
    _need_gpu()
    from espresso_amd.tools.streaming_ctc_prefix_beam_decoder import StreamingCTCPrefixBeamDecoder
    from tests.test_streaming_lexicon_beam import _session

    r = _CtcCase(_ctc_case(20, 6, 4, 4, config=config))
    xd, lens = r.device_inputs()
    off = r.decoder(True, nbest=2)
    ref = [t.clone() for t in off.search(xd, lens)]  # warm-up (cached bf16 weights, graph tables)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = off.search(xd, lens)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(out, ref):
        assert torch.equal(a, b)
    dec = StreamingCTCPrefixBeamDecoder(r.d, 3, T, beam_size=6, nbest=2, beam_size_token=4, lm_model=off.lm_model, lm_weight=off.lm_weight,
                                        insertion_bonus=off.insertion_bonus, context_graph=r.graph, token_times=True)
    res = _session(dec, xd, r.lens, np.random.default_rng(11), 3, whole=(3,), finish=lambda b: tuple(t.clone() for t in dec.finish([b])))
    assert sorted(res) == list(range(B)) and dec.times_state is not None
    tokens, lengths, scores, nhyp, times, vscores = out
    for b, (tk, ln, sc, nh, tm, vs) in res.items():
        assert torch.equal(nh[0], nhyp[b]) and torch.equal(ln[0], lengths[b]) and torch.equal(sc[0], scores[b]) and torch.equal(vs[0], vscores[b])
        U = tk.shape[2]
        assert torch.equal(tk[0], tokens[b, :, :U]) and torch.equal(tm[0], times[b, :, :U]) and bool((times[b, :, U:] == -1).all())
    # accept under the sync debug mode, and close() carries the times into the hypotheses
    dec.open(["a", "b"])
    dec.accept_lprobs(["a", "b"], torch.cat([xd[0, :2], xd[3, :2]]), [2, 2])  # warm-up: the reset of the opened slots
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        dec.accept_lprobs(["a", "b"], torch.cat([xd[0, 2:14], xd[3, 2:5]]), [12, 3])
        dec.accept_lprobs(["a", "b"], xd[3, 5:9], [0, 4])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    from espresso_amd.tools.beam_common import hyps_from_tensors

    want = hyps_from_tensors(*(t.cpu() for t in out))
    assert _close_times(dec.close("a")) == _close_times(want[0]) and _close_times(dec.close("b")) == _close_times(want[3])
    assert sum(len(h[0]) for h in _close_times(want[0])) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("lm_weight,lm_seed", [(0.0, None), (0.3, 1)])
def test_transducer_decoders_with_token_times(lm_weight, lm_seed):
    """On the chunk transducer of the streaming decoder tests: the offline decoder with token_times returns the tokens and scores of
    the one without (bit for bit) plus times that satisfy the invariants; the streaming decoder with token_times, fed the same
    rows in pieces, returns the same tokens and times (an utterance whose oracle margin is below twice the score bound is compared
    on its 1-best score only, as the existing decoder test does; at most one may be); no synchronisation inside search / accept."""
    _need_gpu()
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder
    from tests.test_streaming_transducer_beam import _chunk_transducer
    from tests.test_transducer_frame_beam import _OneRowModel

    model, d, rows = _chunk_transducer()
    lm = _tiny_lm(d, seed=lm_seed).to(DEV) if lm_weight else None
    kw = dict(nbest=3, normalize_scores=False, lm_model=lm, lm_weight=lm_weight)
    beam = 4
    on = TransducerFrameBeamDecoder([model], d, beam_size=beam, token_times=True, **kw)
    off = TransducerFrameBeamDecoder([model], d, beam_size=beam, **kw)
    want, margins, bounds = [], [], []
    for x in rows:
        E = model.joint_encoder_branch(x).view(1, x.shape[0], -1)
        n = torch.tensor([x.shape[0]], device=DEV)
        a = [t.clone() for t in on.search(E, n)]
        b = off.search(E, n)
        assert len(a) == 6 and len(b) == 4
        for p, q in zip(a, b):
            assert torch.equal(p, q)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            again = on.search(E, n)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        for p, q in zip(a, again):
            assert torch.equal(p, q)
        hyps = _times_hyps(a, 0)
        for y, s, times, v in hyps:
            assert all(p < q for p, q in zip(times, times[1:])) and all(u <= f < x.shape[0] for u, f in enumerate(times))
            assert v <= s + _rnnt_bound(x.shape[0])
        want.append(hyps)
        one = _OneRowModel(off, E)
        margins.append(frame_beam_times_oracle(one.logits_fn(0), x.shape[0], beam, off.beam_size_token, off.blank,
                                               lm_fn=one.lm_fn if lm else None, lm_weight=lm_weight, normalize=False, nbest=off.nbest)[2:4])
        bounds.append(_rnnt_bound(x.shape[0] * (2 if lm else 1)))
    assert sum(len(w[0][0]) for w in want) > 0
    on_scores_only = set()
    for pieces in ([3, 5, 1], [2, 7]):
        dec = StreamingTransducerFrameBeamDecoder(model, d, beam, max_streams=2, max_frames=max(x.shape[0] for x in rows) + 1,
                                                  token_times=True, **kw)
        pos, live, pending, got, k = {}, [], list(range(len(rows))), {}, 0
        warm = False
        while pending or live:
            if pending and len(live) < 2:
                b = pending.pop(0)
                dec.open([b])
                live.append(b)
                pos[b] = 0
                warm = False  # the next accept resets the opened slot from a pinned upload: not under the debug mode
            counts = [min(pieces[(k + b) % len(pieces)], rows[b].shape[0] - pos[b]) for b in live]
            fed = torch.cat([rows[b][pos[b]:pos[b] + c] for b, c in zip(live, counts)])
            if warm:
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")
            try:
                dec.accept(list(live), fed, counts)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            warm = True
            for b, c in zip(list(live), counts):
                pos[b] += c
                if pos[b] >= rows[b].shape[0]:
                    mid = dec.finish(b)
                    h = dec.close(b)
                    assert _close_times(mid) == _close_times(h)
                    got[b] = [(tuple(x_["tokens"].tolist()), float(x_["score"]), tuple(x_["times"].tolist()), float(x_["viterbi_score"]))
                              for x_ in h]
                    live.remove(b)
            k += 1
        assert not dec.streams
        for b in range(len(rows)):
            if min(margins[b]) < 2 * bounds[b]:
                on_scores_only.add(b)
                near = [h for h in want[b] if h[0] == got[b][0][0]]
                assert near and abs(near[0][1] - got[b][0][1]) < bounds[b], (b, got[b], want[b])
                continue
            assert [h[0] for h in got[b]] == [h[0] for h in want[b]], (b, pieces, got[b], want[b])
            assert [h[2] for h in got[b]] == [h[2] for h in want[b]], (b, pieces, got[b], want[b])
            assert all(abs(g_[1] - w_[1]) < bounds[b] and abs(g_[3] - w_[3]) < bounds[b] for g_, w_ in zip(got[b], want[b]))
    print(f"lm {lm_weight}: oracle (margin, Viterbi gap) {[(f'{m:.3g}', f'{g_:.3g}') for m, g_ in margins]}")
    assert len(on_scores_only) <= 1, on_scores_only


# --------------------------------------------------------------------------------------------------------------- the command line
def _run_cli(capsys, argv):
    from espresso_amd import speech_recognize as sr

    capsys.readouterr()
    sr.main(argv)
    return [l for l in capsys.readouterr().out.splitlines() if l.startswith("H-")]


def _check_ctm(path, utts, h_lines, unit_count):
    lines = open(path, encoding="utf-8").read().splitlines()
    assert lines, "the CTM is empty"
    by_utt = {}
    for l in lines:
        f = l.split(" ")
        assert len(f) == 6 and f[1] == "1" and f[5] == "1.00" and float(f[3]) > 0, l
        by_utt.setdefault(f[0], []).append((float(f[2]), float(f[3]), f[4]))
    assert [u for u in utts if u in by_utt] == list(dict.fromkeys(l.split(" ")[0] for l in lines))  # wav.scp order
    best = {}
    for l in h_lines:
        best.setdefault(l.split("\t")[0][2:], l.split("\t")[1])
    for u, rows in by_utt.items():
        assert all(a[0] < b[0] for a, b in zip(rows, rows[1:])), (u, rows)
        assert unit_count(best[u]) == len(rows), (u, best[u], rows)
    return lines


@pytest.mark.gpu
@pytest.mark.parametrize("unit", ["token", "word"])
def test_cli_ctm_ctc_offline_equals_streaming(tmp_path, capsys, unit):
    """speech_recognize --ctm on the chunk-streaming CTC checkpoint of the streamed decoder's CLI test: --search ctc_beam and
    --streaming --search ctc_stream_beam write identical files; the H- lines are those of the runs without --ctm; every
    1-best token (word) has its line, in time order."""
    _need_gpu()
    from tests.test_streaming_ctc_prefix_beam import _cli_fixture

    d, utts, base = _cli_fixture(tmp_path)
    opts = ["--beam", "5", "--nbest", "2", "--ctc-beam-size-token", "4", "--ctc-insertion-bonus", "0.1"]
    off_args = base + opts + ["--search", "ctc_beam", "--batch-size", "1"]
    st_args = base + opts + ["--streaming", "--search", "ctc_stream_beam", "--stream-chunk-ms", "170", "--streams", "2"]
    ctm = ["--ctm-unit", unit] if unit != "token" else []
    plain_off, plain_st = _run_cli(capsys, off_args), _run_cli(capsys, st_args)
    h_off = _run_cli(capsys, off_args + ["--ctm", str(tmp_path / "off.ctm")] + ctm)
    h_st = _run_cli(capsys, st_args + ["--ctm", str(tmp_path / "st.ctm"), "--stream-partials"] + ctm)
    assert h_off == plain_off and h_st == plain_st and len(h_off) == 2 * len(utts)
    from espresso_amd.tools.forced_aligner import word_spans

    def count(text):
        syms = text.split()
        return len(syms) if unit == "token" else len(word_spans(syms, range(len(syms)), range(1, len(syms) + 1)))

    lines = _check_ctm(str(tmp_path / "off.ctm"), utts, h_off, count)
    assert lines == open(tmp_path / "st.ctm", encoding="utf-8").read().splitlines()


@pytest.mark.gpu
def test_cli_ctm_transducer_offline_equals_streaming(tmp_path, capsys):
    """The same for --search transducer_frame_beam and --streaming --search transducer_stream_beam, on a small random
    chunk-streaming transducer checkpoint (the one of the streamed decoder's CLI test) with --transducer-hotwords."""
    _need_gpu()
    from espresso_amd import registry
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
    utts = [f"utt{i}" for i in range(3)]
    with open(tmp_path / "wav.scp", "w") as f:
        for i, u in enumerate(utts):
            p = str(tmp_path / f"{u}.wav")
            _write_wav(p, _tones(rng, 0.9 + 0.7 * i))
            f.write(f"{u} {p}\n")
    hot = tmp_path / "hot.txt"
    hot.write_text("t3 t4\nt5 t6 t7\t0.9\n", encoding="utf-8")
    base = ["--path", str(tmp_path / "model.pt"), "--dict", dict_path, "--wav-scp", str(tmp_path / "wav.scp"), "--beam", "4", "--nbest", "2",
            "--transducer-beam-size-token", "3", "--transducer-hotwords", str(hot)]
    off_args = base + ["--search", "transducer_frame_beam", "--batch-size", "1"]
    st_args = base + ["--search", "transducer_stream_beam", "--streaming", "--stream-chunk-ms", "170", "--streams", "2"]
    plain_off, plain_st = _run_cli(capsys, off_args), _run_cli(capsys, st_args)
    h_off = _run_cli(capsys, off_args + ["--ctm", str(tmp_path / "off.ctm")])
    h_st = _run_cli(capsys, st_args + ["--ctm", str(tmp_path / "st.ctm")])
    assert h_off == plain_off and h_st == plain_st and len(h_off) == 2 * len(utts)
    lines = _check_ctm(str(tmp_path / "off.ctm"), utts, h_off, lambda text: len(text.split()))
    assert lines == open(tmp_path / "st.ctm", encoding="utf-8").read().splitlines()
