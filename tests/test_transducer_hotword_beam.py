"""Hotword (contextual phrase) biasing of the frame-synchronous transducer beam search, offline and streamed (the kBias kernels
of csrc/rnnt_beam.hip, ea_rnnt_frame_beam_bias_* / ea_rnnt_frame_beam_stream_bias_*, the `context_graph` option of the two
decoders, speech_recognize --transducer-hotwords).

Truth is float64: tests.transducer_hotword_ref.biased_frame_beam_oracle (frame_beam_oracle with (q, b) through ContextGraph.step),
held on the CPU to brute force without pruning through tests.hotword_ref.locked_bonus, which knows no automaton.  The GPU tests
hold the offline bias kernels to the oracle, the streamed bias kernels to the offline ones bit for bit, and the bias entry points
with an empty graph to the unbiased entry points bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.hotword_ref import BOOSTS, locked_bonus
from tests.test_transducer_frame_beam import BLANK, EOS, SCORE_TOL, TERM_TOL, _args, _dictionary
from tests.transducer_frame_beam_ref import TableLM, TableModel, frame_beam_oracle
from tests.transducer_hotword_ref import biased_beam, biased_frame_beam_oracle, biased_partial_oracle, cut_phrases

DEV = "cuda:0"
PAD = 1
LENS = [14, 0, 1, 9, 12]


def bound(n_tokens):
    """|fp32 search - float64 oracle| allowed for a hypothesis of n_tokens tokens: the project's fp32-vs-float64 allowance of
    the device-resident searches plus one fp32 ulp of a value below 16 per term of the fp32 bias sum, with the usual factor 8."""
    return SCORE_TOL + 8 * TERM_TOL * n_tokens


MARGIN = 2 * bound(max(LENS))  # every case's oracle margin is at least twice its largest bound


def _graph(phrases, V):
    from espresso_amd.tools.context_graph import ContextGraph

    return ContextGraph(phrases, V)


# ---------------------------------------------------------------------------------------------------------------- cases
def _case(V, beam, K, seed, **opts):
    return dict(V=V, beam=beam, K=K, seed=seed, opts=opts)


# (beam, K) over {(1, 1), (4, 4), (16, 4), (16, 16)} for V = 20 and V = 5004, then one case per option.  The seed of a case is the
# first one, counting from 0, at which the biased oracle's margin is at least MARGIN (found on the CPU, before any run of the
# kernels; test_case_margins_are_clear asserts the V = 20 ones, the GPU test every one)
CASES = [
    _case(20, 1, 1, 0), _case(20, 4, 4, 0), _case(20, 16, 4, 0), _case(20, 16, 16, 3),
    _case(5004, 1, 1, 0), _case(5004, 4, 4, 0), _case(5004, 16, 4, 11), _case(5004, 16, 16, 16),
    _case(20, 16, 4, 1, lm="blank", lm_weight=0.6), _case(20, 16, 4, 1, lm="no_blank", lm_weight=0.6),
    _case(20, 4, 4, 0, temperature=1.7), _case(20, 4, 4, 0, predicts_eos=True), _case(20, 4, 4, 0, normalize=False),
]


def _case_id(c):
    return "V{V}-b{beam}-K{K}".format(**c) + "".join(f"-{k}={v}" for k, v in c["opts"].items())


class _Case:
    """Models, phrases (the recipe's, or those given), graph and the biased oracle of every utterance of a case, computed once."""

    def __init__(self, c, phrases=None):
        self.c, o = c, c["opts"]
        self.V, self.beam, self.K = c["V"], c["beam"], c["K"]
        self.lens, self.B, self.T = LENS, len(LENS), max(LENS)
        self.table = TableModel(self.V, c["seed"], blank=BLANK)
        self.lm = TableLM(self.V - (o["lm"] == "no_blank"), c["seed"] + 1000) if o.get("lm") else None
        self.nlm = self.lm.n if self.lm is not None else 0
        self.kw = dict(lm_fn=self.lm, lm_weight=o.get("lm_weight", 0.0), eos=EOS, predicts_eos=o.get("predicts_eos", False),
                       temperature=o.get("temperature", 1.0))
        self.step_kw = dict(eos=EOS if o.get("predicts_eos") else -1, temperature=o.get("temperature", 1.0),
                            lm_weight=o.get("lm_weight", 0.0), lm_no_blank=o.get("lm") == "no_blank")
        self.normalize = o.get("normalize", True)
        self.nbest = min(self.beam, 3)
        fns = [self.table.logits_fn(b) for b in range(self.B)]
        self.phrases = cut_phrases(fns, self.lens, BLANK, self.V, **self.kw) if phrases is None else phrases
        self.graph = _graph(self.phrases, self.V)
        self.refs = [biased_frame_beam_oracle(fns[b], self.lens[b], self.beam, self.K, BLANK, self.graph, normalize=self.normalize,
                                              nbest=self.nbest, **self.kw) for b in range(self.B)]
        self.margin = min(r[2] for r in self.refs)
        self.plain = [frame_beam_oracle(fns[b], self.lens[b], self.beam, self.K, BLANK, normalize=self.normalize, nbest=self.nbest,
                                        **self.kw)[0] for b in range(self.B)]
        # the rows the kernels are fed: those of the oracle's live hypotheses, NaN for dead beam slots, a row stride above V
        self.logits, self.lm_rows = {}, {}
        for b, L in enumerate(self.lens):
            seqs = [()]
            for t in range(L):
                x = np.full((self.beam, self.V + 3), np.nan, dtype=np.float32)
                m = np.full((self.beam, self.nlm), np.nan, dtype=np.float32)
                for j, y in enumerate(seqs):
                    x[j, : self.V] = self.table.row(b, t, y)
                    if self.lm is not None:
                        m[j] = self.lm.row(y)
                self.logits[b, t], self.lm_rows[b, t] = x, m
                seqs = [seqs[p] + (() if k else (v,)) for p, v, k in self.refs[b][1][t]]
        self._live = {}

    def rows(self, frames):
        """Device (logits [n*beam][V] view of a wider tensor, lm_rows or None) of the listed (utterance, frame or None) pairs."""
        nan_x = np.full((self.beam, self.V + 3), np.nan, dtype=np.float32)
        nan_m = np.full((self.beam, self.nlm), np.nan, dtype=np.float32)
        x = np.concatenate([self.logits.get(f, nan_x) if f[1] is not None else nan_x for f in frames])
        m = np.concatenate([self.lm_rows.get(f, nan_m) if f[1] is not None else nan_m for f in frames])
        return torch.from_numpy(x).to(DEV)[:, : self.V], (torch.from_numpy(m).to(DEV) if self.lm is not None else None)

    def live(self, b, t):
        """The oracle's live beam [(tokens, s, q, b)] of utterance b after its first t frames, the triples, the margin."""
        if (b, t) not in self._live:
            self._live[b, t] = biased_beam(self.table.logits_fn(b), t, self.beam, self.K, BLANK, self.graph, **self.kw)
        return self._live[b, t]


@functools.lru_cache(maxsize=None)
def _built(i):
    return _Case(CASES[i])


# ---------------------------------------------------------------------------------------------------------------- CPU
def _unbiased_all(logits_fn, T, V):
    hyps, _, _ = frame_beam_oracle(logits_fn, T, beam=10 ** 6, K=V - 1, blank=BLANK, normalize=False, nbest=10 ** 6)
    return dict(hyps)


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("T", [1, 2, 4])
def test_oracle_is_exact_without_pruning(seed, T):
    """beam and K exhaustive (the shapes of test_transducer_frame_beam.test_oracle_is_exact_without_pruning, which holds the
    unbiased oracle to brute force over every alignment): the biased oracle returns every sequence, and its final minus the
    unbiased final of the same tokens is B(y) as locked_bonus states it, without an automaton."""
    V = 4
    table = TableModel(V, seed, blank=BLANK, sharp=1.0)
    phrases = [([1, 2], BOOSTS[0]), ([1, 2, 3], BOOSTS[1]), ([2], 0.41), ([3, 3, 1], 0.9), ([2, 3], 0.55)]
    g = _graph(phrases, V)
    hyps, triples, _ = biased_frame_beam_oracle(table.logits_fn(0), T, 10 ** 6, V - 1, BLANK, g, normalize=False, nbest=10 ** 6)
    plain = _unbiased_all(table.logits_fn(0), T, V)
    assert {y for y, _ in hyps} == set(plain) and len(hyps) == len(plain)
    for y, s in hyps:
        assert abs(s - plain[y] - locked_bonus(g.phrases, y)) < 1e-9, (y, s, plain[y])
    assert hyps[0][0] == max(plain, key=lambda y: plain[y] + locked_bonus(g.phrases, y))
    assert any(locked_bonus(g.phrases, y) > 0 for y in plain) or T == 1
    assert len(triples) == T


def test_oracle_with_an_empty_graph_is_the_unbiased_oracle():
    table = TableModel(12, 3, blank=BLANK)
    for beam, K in [(1, 1), (4, 3)]:
        a = biased_frame_beam_oracle(table.logits_fn(0), 8, beam, K, BLANK, _graph([], 12), nbest=beam)
        b = frame_beam_oracle(table.logits_fn(0), 8, beam, K, BLANK, nbest=beam)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]


def test_case_margins_are_clear():
    """Every V = 20 case: the biased oracle's margin is at least twice the bound (the V = 5004 ones take longer on the CPU: the
    GPU test asserts theirs); the phrase list holds a proper prefix, a phrase inside a longer one and the 64-token phrase; and
    over the cases the bias does change 1-best results and credits phrases."""
    flipped = credited = 0
    for i, c in enumerate(CASES):
        if c["V"] > 100:
            continue
        r = _built(i)
        assert r.margin >= MARGIN, (_case_id(c), r.margin)
        toks = [tuple(p) for p, _ in r.phrases]
        assert any(len(p) == 64 for p in toks)
        assert any(a != b and b[: len(a)] == a for a in toks for b in toks if len(b) <= 3)
        assert any(len(a) == 1 and len(b) == 3 and b[1] == a[0] for a in toks for b in toks)
        for b in range(r.B):
            flipped += r.refs[b][0][0][0] != r.plain[b][0][0]
            credited += locked_bonus(r.graph.phrases, r.refs[b][0][0][0]) > 0
    print(f"1-best changed by the bias in {flipped} utterances, carries a completed phrase in {credited}")
    assert flipped >= 9 and credited >= 18  # (on the CPU: 22 and 27 of 45)


_HOT = ["--transducer-hotwords", "missing_hot.txt"]
_MISSING = ["--path", "missing.pt", "--dict", "missing.txt", "--wav-scp", "missing.scp"]


def test_cli_option_reaches_the_decoders():
    from espresso_amd import speech_recognize as sr
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder
    from tests.test_ctc_prefix_beam import _tiny_lm

    d = _dictionary(8)
    g = _graph([([5, 6], 1.0)], len(d))
    checks = (sr.check_frame_beam_args, sr.check_stream_beam_args, sr.check_hotword_args, sr.check_ngram_args, sr.check_streaming_args)
    for extra in ([], ["--lm-path", "lm.pt", "--lm-weight", "0.3"], ["--nbest", "2", "--hotword-score", "2"]):
        a = _args("--search", "transducer_frame_beam", *_HOT, *extra)
        assert a.transducer_hotwords == "missing_hot.txt" and a.hotwords is None
        for check in checks:
            check(a)
        gen = sr.build_generator(a, None, d, lm=_tiny_lm(d) if "--lm-path" in extra else None, context_graph=g)
        assert type(gen) is TransducerFrameBeamDecoder and gen.context_graph is g
        a = _args("--streaming", "--search", "transducer_stream_beam", "--stream-partials", *_HOT, *extra)
        for check in checks:
            check(a)
        dec = StreamingTransducerFrameBeamDecoder(None, d, max_streams=2, max_frames=10, **sr.stream_beam_options(a, None, g))
        assert dec.context_graph is g and dec.offline.context_graph is g
    assert sr.build_generator(_args("--search", "transducer_frame_beam"), None, d).context_graph is None
    assert "context_graph" not in sr.stream_beam_options(_args("--streaming", "--search", "transducer_stream_beam"))
    assert StreamingTransducerFrameBeamDecoder(None, d, 4, max_streams=2, max_frames=10).context_graph is None
    help_text = " ".join(sr.get_parser().format_help().split())
    assert "--transducer-hotwords" in help_text and "global top" in help_text
    with pytest.raises(FileNotFoundError):  # every argument check passed: the failure is the missing checkpoint
        sr.main(_MISSING + ["--device", "cpu", "--search", "transducer_frame_beam"] + _HOT)
    with pytest.raises(ValueError, match="context graph"):
        TransducerFrameBeamDecoder([None], d, context_graph=_graph([], len(d) + 1))
    with pytest.raises(ValueError, match="context graph"):
        StreamingTransducerFrameBeamDecoder(None, d, 4, max_streams=2, max_frames=10, context_graph=_graph([], len(d) + 1))


@pytest.mark.parametrize("extra", [[], ["--search", "beam"], ["--search", "ctc"], ["--search", "transducer_greedy"],
                                   ["--search", "transducer_beam"], ["--search", "ctc_beam", "--ngram-lm", "lm.arpa"],
                                   ["--search", "ctc_beam", "--streaming"], ["--search", "ctc", "--streaming"],
                                   ["--search", "ctc_beam", "--ngram-lm", "lm.arpa", "--streaming"], ["--search", "ctc_beam"]])
def test_cli_refuses_the_option_elsewhere(extra):
    """The searches of test_ctc_hotword_beam.test_cli_refuses_hotwords_elsewhere, and the CTC prefix beam itself: refused by
    name before any file is opened."""
    from espresso_amd import speech_recognize as sr

    with pytest.raises(NotImplementedError, match="--transducer-hotwords"):
        sr.main(_MISSING + _HOT + extra)


def test_cli_refuses_both_options_and_keeps_the_pinned_messages():
    from espresso_amd import speech_recognize as sr

    for search in (["--search", "ctc_beam"], ["--search", "transducer_frame_beam"], ["--streaming", "--search", "transducer_stream_beam"]):
        with pytest.raises(NotImplementedError, match="--transducer-hotwords"):
            sr.main(_MISSING + _HOT + ["--hotwords", "h.txt"] + search)
    for search in (["--search", "transducer_frame_beam"], ["--streaming", "--search", "transducer_stream_beam"]):
        with pytest.raises(NotImplementedError, match=r"(^|\s)--hotwords\s.*--transducer-hotwords"):
            sr.main(_MISSING + ["--hotwords", "h.txt"] + search)
    for opt in (["--hotword-score", "2"], ["--bpe", "characters_asr"], ["--sentencepiece-model", "m.model"]):
        with pytest.raises(ValueError, match=opt[0]):
            sr.main(_MISSING + ["--search", "transducer_frame_beam"] + opt)
    with pytest.raises(ValueError, match="positive"):
        sr.main(_MISSING + ["--search", "transducer_frame_beam", "--hotword-score", "0"] + _HOT)


def bias_state_words(max_frames, beam):
    """The documented formula (include/espresso_amd.h): the unbiased slot followed by q [beam] and b [beam]."""
    cap = 1 + max_frames * beam
    tsize = 64
    while tsize < 2 * cap:
        tsize *= 2
    w = 3 * tsize + 5 * beam + 2 + 2 * cap + 2 * beam + 2 * beam * 64
    return 2 + w + (w & 1) + 2 * beam


def test_bias_state_bytes_formula():
    from espresso_amd import _lib

    try:
        lib = _lib.lib()
    except _lib.EspressoAmdLibraryError:
        pytest.skip("the library is not built")
    for mf, beam in [(1, 1), (7, 3), (100, 5), (250, 10), (1000, 64), (33, 16)]:
        assert lib.ea_rnnt_frame_beam_stream_bias_state_bytes(mf, beam) == 4 * bias_state_words(mf, beam)
        assert lib.ea_rnnt_frame_beam_stream_bias_state_bytes(mf, beam) == lib.ea_rnnt_frame_beam_stream_state_bytes(mf, beam) + 8 * beam
        for B in (1, 5):
            assert lib.ea_rnnt_frame_beam_bias_workspace_bytes(B, mf, beam) == lib.ea_rnnt_frame_beam_workspace_bytes(B, mf, beam) + 8 * beam * B
    assert lib.ea_rnnt_frame_beam_stream_bias_state_bytes(10, 65) == 0 and lib.ea_rnnt_frame_beam_bias_workspace_bytes(1, 4, 65) == 0
    assert lib.ea_rnnt_frame_beam_stream_bias_state_bytes(0, 4) == 0 and lib.ea_rnnt_frame_beam_stream_bias_state_bytes(10, 0) == 0


# ---------------------------------------------------------------------------------------------------------------- GPU
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


def _triples_out(N):
    return (torch.empty(N, dtype=torch.int32, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV),
            torch.empty(N, dtype=torch.uint8, device=DEV))


def _hyps(out, b):
    tokens, lengths, scores, nhyp = (t.cpu() for t in out)
    return [(tuple(tokens[b, i, : int(lengths[b, i])].tolist()), float(scores[b, i])) for i in range(int(nhyp[b]))]


class _Family:
    """The eight calls of one search family with the graph bound: graph None = the unbiased entry points."""

    def __init__(self, graph):
        from espresso_amd import kernels as Kn

        g = self.g = None if graph is None else graph.cuda(DEV)
        if g is None:
            self.workspace, self.finish = Kn.rnnt_frame_beam_workspace, Kn.rnnt_frame_beam_finish
            self.step = lambda x, in_len, ws, out, *a, **k: Kn.rnnt_frame_beam_step(x, in_len, ws, out, *a, **k)
            self.state, self.reset, self.partial = Kn.rnnt_frame_beam_stream_state, Kn.rnnt_frame_beam_stream_reset, Kn.rnnt_frame_beam_stream_partial
            self.sstep = lambda x, si, nn, j, st, out, *a, **k: Kn.rnnt_frame_beam_stream_step(x, si, nn, j, st, out, *a, **k)
            self.sfinish = Kn.rnnt_frame_beam_stream_finish
        else:
            self.workspace = Kn.rnnt_frame_beam_bias_workspace
            self.finish = lambda ws, *a, **k: Kn.rnnt_frame_beam_bias_finish(ws, g, *a, **k)
            self.step = lambda x, in_len, ws, out, *a, **k: Kn.rnnt_frame_beam_bias_step(x, in_len, ws, g, out, *a, **k)
            self.state, self.reset = Kn.rnnt_frame_beam_stream_bias_state, Kn.rnnt_frame_beam_stream_bias_reset
            self.partial = Kn.rnnt_frame_beam_stream_bias_partial
            self.sstep = lambda x, si, nn, j, st, out, *a, **k: Kn.rnnt_frame_beam_stream_bias_step(x, si, nn, j, st, g, out, *a, **k)
            self.sfinish = lambda st, slots, *a, **k: Kn.rnnt_frame_beam_stream_bias_finish(st, slots, g, *a, **k)


def _offline(r, fam):
    """The offline kernels of a family over the case: per frame the triples [B][beam][3] (parent as a beam slot), and after every
    frame count 0 .. T the finish tensors (the finish only reads: after step t it is the search over t + 1 frames)."""
    B, T, V, beam = r.B, r.T, r.V, r.beam
    ws = fam.workspace(B, T, beam, DEV)
    ws.fill_(0xA5)  # any contents: frame 0 initialises
    in_len = torch.tensor(r.lens, dtype=torch.int32, device=DEV)
    out = _triples_out(B * beam)
    row0 = (torch.arange(B, device=DEV, dtype=torch.int32) * beam).repeat_interleave(beam)
    scores0 = torch.full((B, r.nbest), -math.inf, device=DEV)
    scores0[:, 0] = 0.0
    triples = []
    fins = [(torch.full((B, r.nbest, T), PAD, dtype=torch.int32, device=DEV), torch.zeros(B, r.nbest, dtype=torch.int32, device=DEV),
             scores0, torch.ones(B, dtype=torch.int32, device=DEV))]
    for t in range(T):
        x, m = r.rows([(b, t if t < r.lens[b] else None) for b in range(B)])
        fam.step(x, in_len, ws, out, B, T, V, beam, r.K, BLANK, t, lm_rows=m, **r.step_kw)
        triples.append(torch.stack([out[0] - row0, out[1], out[2].to(torch.int32)], 1).view(B, beam, 3).clone())
        fins.append(tuple(a.clone() for a in fam.finish(ws, B, T, beam, r.nbest, PAD, normalize=r.normalize)))
    return triples, fins, ws


def _streamed(r, fam, offline, max_frames, max_streams, seed, check_partials=False):
    """The streamed kernels of a family over the case in uneven pieces, streams in shuffled slots of a larger buffer, some entries
    idle: every triple and the finish after every piece torch.equal to `offline`; with check_partials the partial against the
    oracle's live beam.  Returns (partial checkpoints compared, worst |partial score - oracle|, every partial of utterance 0)."""
    triples, fins = offline[:2]
    B, T, V, beam = r.B, r.T, r.V, r.beam
    rng = np.random.default_rng(seed)
    slot_of = rng.permutation(max_streams)[:B].tolist()
    state, _ = fam.state(max_streams, max_frames, beam, DEV)
    state.fill_(0xA5)
    fam.reset(state, torch.tensor(slot_of, dtype=torch.int32, device=DEV), max_frames, beam)
    pos, pieces, rounds = [0] * B, [1, 3, 2, 5, 1, 4], 0
    compared, worst, stable_log = 0, 0.0, []

    def readouts(entries):
        nonlocal compared, worst
        slots = torch.tensor([slot_of[b] for b in entries], dtype=torch.int32, device=DEV)
        before = state.clone()
        fin = fam.sfinish(state, slots, max_frames, beam, r.nbest, PAD, T, normalize=r.normalize)
        par = fam.partial(state, slots, max_frames, beam, PAD, T)
        assert torch.equal(state, before)  # both readouts leave the state alone
        for e, b in enumerate(entries):
            for got, w in zip(fin, fins[pos[b]]):
                assert torch.equal(got[e], w[b]), (b, pos[b], got[e], w[b])
        if check_partials:
            toks, lens_, scores, stable = (t.cpu() for t in par)
            for e, b in enumerate(entries):
                hyps, _, margin = r.live(b, pos[b])
                y, k, s = biased_partial_oracle(hyps)
                got = tuple(toks[e, : int(lens_[e])].tolist())
                assert got == y and int(stable[e]) == k, (b, pos[b], got, int(stable[e]), y, k)
                assert bool((toks[e, int(lens_[e]):] == PAD).all())
                if b == 0:
                    stable_log.append(got[:k])
                if margin >= MARGIN:
                    compared += 1
                    worst = max(worst, abs(float(scores[e]) - s))
                    assert abs(float(scores[e]) - s) <= bound(len(y)), (b, pos[b], float(scores[e]), s)

    readouts(list(range(B)))
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
            fam.sstep(x, slot_idx, nn, j, state, out, max_frames, V, beam, r.K, BLANK, lm_rows=m, **r.step_kw)
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
    heads = state.view(torch.int32).view(max_streams, -1)[:, 0].cpu().tolist()
    assert [heads[slot_of[b]] for b in range(B)] == r.lens
    return compared, worst, stable_log


def _check_vs_oracle(r, triples, fin):
    """Triples of every frame (live slots the oracle's, the rest the dead-slot triple, finished utterances the identity),
    sequences, n-best order and scores of the last finish against the biased oracle.  Returns the worst score difference."""
    for t, tr in enumerate(triples):
        tr = tr.cpu().tolist()
        for b in range(r.B):
            got = [tuple(x) for x in tr[b]]
            if t >= r.lens[b]:
                assert got == [(j, BLANK, 1) for j in range(r.beam)], (b, t, got)
                continue
            want = r.refs[b][1][t]
            assert got[: len(want)] == want, (b, t, got, want)
            assert got[len(want):] == [(0, BLANK, 1)] * (r.beam - len(want)), (b, t, got)
    worst = 0.0
    for b, (ref, _, _) in enumerate(r.refs):
        got = _hyps(fin, b)
        assert [y for y, _ in got] == [y for y, _ in ref], (b, got, ref)
        for (y, s), (_, q) in zip(got, ref):
            worst = max(worst, abs(s - q))
            assert abs(s - q) <= bound(len(y)), (b, y, s, q)
    assert _hyps(fin, 1) == [((), 0.0)]  # in_len 0: the empty hypothesis
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_bias_step_kernels_vs_oracle(i):
    """The offline bias kernels frame by frame on table logits: triples of every frame, sequences and n-best order equal the
    biased oracle's, scores within 1e-4 + 8 * 2^-20 * |y|."""
    _need_gpu()
    r = _built(i)
    assert r.margin >= MARGIN, r.margin
    triples, fins, _ = _offline(r, _Family(r.graph))
    worst = _check_vs_oracle(r, triples, fins[-1])
    flips = sum(r.refs[b][0][0][0] != r.plain[b][0][0] for b in range(r.B))
    print(f"{_case_id(r.c)}: {r.graph.num_nodes} nodes, oracle margin {r.margin:.3g}, 1-best changed in {flips} utterances, "
          f"max |score - oracle| {worst:.2e}")


EMPTY_CASES = [1, 6, 9]  # V20-b4-K4, V5004-b16-K4, V20-b16-K4 with the LM without a blank column


@pytest.mark.gpu
@pytest.mark.parametrize("i", EMPTY_CASES, ids=[_case_id(CASES[i]) for i in EMPTY_CASES])
def test_empty_graph_equals_no_graph_bit_for_bit(i):
    """The bias entry points with the root-only graph (cg_edges NULL) against the unbiased entry points on the same rows (those
    of the unbiased oracle): triples of every frame and tokens, lengths, scores, nhyp after every frame torch.equal, offline and
    streamed."""
    _need_gpu()
    plain = _Case(CASES[i], phrases=[])  # the oracle with the root-only graph is the unbiased oracle (a CPU test): its rows serve both
    assert plain.graph.num_nodes == 1 and plain.graph.edges.shape == (0, 4)
    unbiased = _offline(plain, _Family(None))
    empty = _offline(plain, _Family(plain.graph))
    for a, b_ in zip(unbiased[0], empty[0]):
        assert torch.equal(a, b_)
    for fa, fb in zip(unbiased[1], empty[1]):
        assert all(torch.equal(a, b_) for a, b_ in zip(fa, fb))
    assert float(unbiased[1][-1][2][0, 0]) != 0.0  # (something was scored)
    # streamed, both families, against the unbiased offline results
    _streamed(plain, _Family(None), unbiased, plain.T, plain.B + 2, 3)
    _streamed(plain, _Family(plain.graph), unbiased, plain.T + 5, plain.B + 1, 4)


def _near_tied_input(T=5, a=5, b_=6, V=10):
    """Blank ahead on odd frames; on even frames token b_ ahead of token a by about 0.2, everything else far behind."""
    x = -8.0 - 0.5 * np.arange(V, dtype=np.float64)[None].repeat(T, 0)
    for t in range(T):
        if t % 2 == 0:
            x[t, b_], x[t, a], x[t, 0] = -0.6 - 0.07 * t, -0.8 - 0.03 * t, -3.0
        else:
            x[t, 0] = -0.05
    return x.astype(np.float32)


def _run_single(x, fam, beam, K, nbest, normalize=False):
    """One utterance whose logits row of frame t is x[t] for every hypothesis, through the offline kernels of a family."""
    T, V = x.shape
    ws = fam.workspace(1, T, beam, DEV)
    out = _triples_out(beam)
    in_len = torch.tensor([T], dtype=torch.int32, device=DEV)
    triples = []
    for t in range(T):
        fam.step(torch.from_numpy(x[t])[None].repeat(beam, 1).to(DEV), in_len, ws, out, 1, T, V, beam, K, BLANK, t)
        triples.append(list(zip(*(o.cpu().tolist() for o in out))))
    return _hyps(fam.finish(ws, 1, T, beam, nbest, PAD, normalize=normalize), 0), triples, ws


@pytest.mark.gpu
def test_biasing_changes_the_answer():
    """Two near-tied tokens on three emitting frames, one phrase on the loser: the biased best is the phrase, the unbiased best
    is not, and its score is the unbiased score of those tokens plus the boost.  Then beam 1 and a two-token phrase whose first
    token loses acoustically: the hypothesis survives frame 0 only through its pending phi and is completed at frame 2."""
    _need_gpu()
    a, b_, V, beam, K = 5, 6, 10, 3, 2
    x = _near_tied_input()
    fn = lambda t, y: x[t].astype(np.float64)  # noqa: E731
    g = _graph([([a, a, a], 0.5)], V)
    ref, triples, margin = biased_frame_beam_oracle(fn, 5, beam, K, BLANK, g, normalize=False, nbest=beam)
    assert margin >= 2 * bound(3)
    plain, ptriples, _ = _run_single(x, _Family(None), beam, K, beam)
    got, gtriples, _ = _run_single(x, _Family(g), beam, K, beam)
    assert plain[0][0] == (b_, b_, b_) and got[0][0] == (a, a, a) == ref[0][0], (plain, got, ref)
    for t in range(5):
        assert gtriples[t][: len(triples[t])] == triples[t], (t, gtriples[t], triples[t])
    # the unbiased score of (a, a, a) under the same pruning is the s the oracle carries for it; the pruned alignments (a token on a
    # blank frame, 8 nats down) are within 2e-3 of nothing
    s_aaa = next(s for y, s, _, _ in biased_beam(fn, 5, beam, K, BLANK, g)[0] if y == (a, a, a))
    every = dict(frame_beam_oracle(fn, 5, 10 ** 6, V - 1, BLANK, normalize=False, nbest=10 ** 6)[0])
    assert abs(ref[0][1] - (s_aaa + 1.5)) < 1e-12 and abs(s_aaa - every[(a, a, a)]) < 2e-3 and locked_bonus(g.phrases, (a, a, a)) == 1.5
    assert abs(got[0][1] - ref[0][1]) <= bound(3), (got, ref)
    assert [y for y, _ in got] == [y for y, _ in ref]

    c2 = 7  # frame 2: token c2 ahead, so the phrase (a, c2) completes if (a) is still there
    x2 = x.copy()
    x2[2, c2], x2[4, 0] = 0.5, 2.0
    fn2 = lambda t, y: x2[t].astype(np.float64)  # noqa: E731
    g2 = _graph([([a, c2], 0.3)], V)
    ref2, _, margin2 = biased_frame_beam_oracle(fn2, 5, 1, K, BLANK, g2, normalize=False)
    assert margin2 >= 2 * bound(2)
    plain2, _, _ = _run_single(x2, _Family(None), 1, K, 1)
    got2, _, _ = _run_single(x2, _Family(g2), 1, K, 1)
    assert plain2[0][0] == (b_, c2) and got2[0][0] == (a, c2) == ref2[0][0], (plain2, got2, ref2)
    live = [biased_beam(fn2, t, 1, K, BLANK, g2)[0][0] for t in range(6)]
    assert live[1][0] == (a,) and abs(live[1][3] - 0.3) < 1e-12 and live[3][0] == (a, c2) and abs(live[3][3] - 0.6) < 1e-12
    assert live[1][1] < biased_beam(fn2, 1, 1, K, BLANK, _graph([], V))[0][0][1]  # (a) is behind (b_) on s alone
    assert abs(ref2[0][1] - (live[5][1] + 0.6)) < 1e-12 and abs(got2[0][1] - ref2[0][1]) <= bound(2), (got2, ref2)
    # a phrase that is never completed gives its pending bonus back
    g3 = _graph([([a, 9], 0.3)], V)
    got3, _, _ = _run_single(x2, _Family(g3), 1, K, 1)
    ref3, _, _ = biased_frame_beam_oracle(fn2, 5, 1, K, BLANK, g3, normalize=False)
    assert got3[0][0] == ref3[0][0] == (a, c2) and abs(got3[0][1] - ref3[0][1]) <= bound(2)
    assert abs(got3[0][1] - (got2[0][1] - 0.6)) <= 2 * bound(2)


@pytest.mark.gpu
def test_merge_keeps_one_state():
    """() and (1) are in the beam and () + 1 meets the stay of (1) (test_oracle_extension_meets_stay): one hypothesis (1) is
    left, its final is the oracle's, and ea_context_graph_score of every hypothesis' tokens gives the (q, b) the workspace
    holds and the b - phi(q) that the finish added to the unbiased score, bit for bit."""
    _need_gpu()
    from espresso_amd import kernels as Kn

    p = {(): [0.5, 0.4, 0.1], (1,): [0.6, 0.2, 0.2], (2,): [0.8, 0.1, 0.1]}
    V, beam, K, T = 3, 3, 2, 2
    g = _graph([([1, 2], 0.7), ([2], 0.3)], V)
    fn = lambda t, y: np.log(p[y])  # noqa: E731
    ref, triples, margin = biased_frame_beam_oracle(fn, T, beam, K, BLANK, g, normalize=False, nbest=beam)
    assert margin >= 2 * bound(2)
    _, ptriples, _ = frame_beam_oracle(fn, T, beam, K, BLANK, normalize=False, nbest=beam)
    assert triples[1][0] == (0, BLANK, 1) and [y for y, _ in ref].count((1,)) == 1  # () + 1 met the stay of (1), the best slot
    outs = {}
    for name, fam, want in (("plain", _Family(None), ptriples), ("bias", _Family(g), triples)):
        ws = fam.workspace(1, T, beam, DEV)
        out = _triples_out(beam)
        in_len = torch.tensor([T], dtype=torch.int32, device=DEV)
        seqs = [()]
        for t in range(T):
            x = np.full((beam, V), np.nan, dtype=np.float32)
            for j, y in enumerate(seqs):
                x[j] = np.log(p[y])
            fam.step(torch.from_numpy(x).to(DEV), in_len, ws, out, 1, T, V, beam, K, BLANK, t)
            got = list(zip(*(o.cpu().tolist() for o in out)))
            assert got[: len(want[t])] == want[t], (name, t, got, want[t])
            seqs = [seqs[pp] + (() if k else (v,)) for pp, v, k in want[t]]
        outs[name] = (_hyps(fam.finish(ws, 1, T, beam, beam, PAD, normalize=False), 0), ws)
    got, ws = outs["bias"]
    assert [y for y, _ in got] == [y for y, _ in ref] and sum(y == (1,) for y, _ in got) == 1, (got, ref)
    for (y, s), (_, q) in zip(got, ref):
        assert abs(s - q) <= bound(len(y)), (y, s, q)
    L = max(1, max(len(y) for y, _ in got))
    tokens = torch.tensor([list(y) + [0] * (L - len(y)) for y, _ in got], dtype=torch.int32, device=DEV)
    lens = torch.tensor([len(y) for y, _ in got], dtype=torch.int32, device=DEV)
    running, final, qn = (t.cpu() for t in Kn.context_graph_score(g.cuda(DEV), tokens, lens))
    tail = ws.view(torch.int32)[-2 * beam:].cpu()
    ws_q, ws_b = tail[:beam].tolist(), tail[beam:].view(torch.float32).tolist()
    replay = sorted((int(qn[i]), float(running[i, len(y) - 1]) if y else 0.0) for i, (y, _) in enumerate(got))
    assert sorted(zip(ws_q[: len(got)], ws_b[: len(got)])) == replay, (ws_q, ws_b, replay)
    tsize = 64  # the hash table of 1 + T * beam = 7 nodes: `score` [beam] follows its 3 * tsize words (csrc/rnnt_beam.hip, RnntWs)
    ws_s = ws.view(torch.float32)[3 * tsize: 3 * tsize + beam].cpu().tolist()
    plain = dict(outs["plain"][0])
    for i, (y, s) in enumerate(got):
        j = list(zip(ws_q, ws_b)).index((int(qn[i]), float(running[i, len(y) - 1]) if y else 0.0))
        assert np.float32(s) == np.float32(ws_s[j]) + np.float32(final[i]), (y, s, ws_s[j], float(final[i]))
        assert y not in plain or np.float32(plain[y]) == np.float32(ws_s[j]), (y, plain[y], ws_s[j])  # the merge added s alone
        assert abs(float(final[i]) - locked_bonus(g.phrases, y)) < 1e-6
    assert (1,) in plain and () in plain


STREAM_CASES = list(range(len(CASES)))  # the cases of test_bias_step_kernels_vs_oracle, every one


@pytest.mark.gpu
@pytest.mark.parametrize("i", STREAM_CASES, ids=[_case_id(CASES[i]) for i in STREAM_CASES])
def test_streamed_bias_kernels_equal_offline_bit_for_bit(i):
    """With a graph: per-frame triples and the finish after every piece torch.equal to the offline bias calls, for a state
    sized for exactly the longest utterance and for a larger one; the partial = the oracle's best live hypothesis by s + b and
    the common-prefix length at every checkpoint; on one case (V20-b4-K4) every later partial and the final results start with the
    tokens reported as stable."""
    _need_gpu()
    r = _built(i)
    assert r.margin >= MARGIN, r.margin
    fam = _Family(r.graph)
    offline = _offline(r, fam)
    _check_vs_oracle(r, offline[0], offline[1][-1])
    _streamed(r, fam, offline, r.T, r.B + 3, 1)
    compared, worst, stable_log = _streamed(r, fam, offline, r.T + 9, r.B + 1, 2, check_partials=True)
    print(f"{_case_id(r.c)}: {compared} partial checkpoints compared on scores, max |partial score - oracle| {worst:.2e}")
    assert compared > 0
    if i == STREAM_CASES[1]:
        final = [y for y, _ in _hyps(offline[1][-1], 0)]
        for n, st in enumerate(stable_log):
            for later in stable_log[n:]:
                assert later[: len(st)] == st, (st, later)
            assert all(y[: len(st)] == st for y in final), (st, final)
        assert any(stable_log)


@pytest.mark.gpu
def test_untouched_slots_and_bad_arguments():
    """Slots not listed, idle, out of range or full are byte-identical after a bias step; malformed graph arguments and beam, K,
    V out of range return -2 (a RuntimeError naming the entry point).  The first half launches reset, steps and a partial on valid
    arguments; the refusals are checks of return codes only and launch nothing."""
    _need_gpu()
    from espresso_amd import kernels as Kn

    V, beam, K, mf, S = 20, 4, 3, 2, 3
    lib = Kn._lib.lib()
    table = TableModel(V, 0, blank=BLANK)
    g = _graph([([3, 4], 1.0), ([5], 0.5)], V)
    gd = g.cuda(DEV)
    state, nbytes = Kn.rnnt_frame_beam_stream_bias_state(S, mf, beam, DEV)
    assert nbytes == 4 * bias_state_words(mf, beam) == state.shape[1]
    Kn.rnnt_frame_beam_stream_bias_reset(state, torch.tensor([0, 1, 2, 7, -1], dtype=torch.int32, device=DEV), mf, beam)
    x = torch.from_numpy(np.stack([table.row(0, 0, ())] * (3 * beam))).to(DEV)
    out = _triples_out(3 * beam)
    ident = lambda e: [(e * beam + s, BLANK, 1) for s in range(beam)]  # noqa: E731
    trip = lambda: list(zip(*(o.cpu().tolist() for o in out)))  # noqa: E731

    def step(slots, n_new, j):
        Kn.rnnt_frame_beam_stream_bias_step(x, torch.tensor(slots, dtype=torch.int32, device=DEV),
                                            torch.tensor(n_new, dtype=torch.int32, device=DEV), j, state, gd, out, mf, V, beam, K, BLANK)

    before = state.clone()
    step([0, 5, 2], [0, 1, 1], 0)  # idle, out of range, active
    got = trip()
    assert got[:beam] == ident(0) and got[beam:2 * beam] == ident(1) and got[2 * beam:] != ident(2)
    assert torch.equal(state[:2], before[:2]) and not torch.equal(state[2], before[2])
    step([2, 0, 1], [2, 0, 1], 1)  # j = 1: only the first entry is due
    assert torch.equal(state[:2], before[:2])
    full = state.clone()
    step([2, -3, 1], [1, 1, 0], 0)  # slot 2 is full (2 of 2 frames), a negative slot, idle
    assert trip() == ident(0) + ident(1) + ident(2) and torch.equal(state, full)

    slots = torch.tensor([0], dtype=torch.int32, device=DEV)
    o1 = _triples_out(beam)
    for kw in (dict(K=V), dict(blank=V), dict(eos=BLANK), dict(temperature=0.0), dict(K=65), dict(K=0)):
        a = dict(K=K, blank=BLANK)
        a.update(kw)
        with pytest.raises(RuntimeError, match="ea_rnnt_frame_beam_stream_bias_step"):
            Kn.rnnt_frame_beam_stream_bias_step(x[:beam], slots, slots, 0, state, gd, o1, mf, V, beam, **a)
    in_len = torch.ones(1, dtype=torch.int32, device=DEV)
    ws = Kn.rnnt_frame_beam_bias_workspace(1, mf, beam, DEV)
    for kw in (dict(K=V), dict(t=mf), dict(blank=V), dict(eos=BLANK), dict(temperature=0.0)):
        a = dict(K=K, blank=BLANK, t=0)
        a.update(kw)
        with pytest.raises(RuntimeError, match="ea_rnnt_frame_beam_bias_step"):
            Kn.rnnt_frame_beam_bias_step(x[:beam], in_len, ws, gd, o1, 1, mf, V, beam, **a)
    # the graph arguments and the ranges, on the C entry points themselves
    p, st = Kn._p, Kn._stream()
    nodes, edges, root = (p(t) for t in gd)
    N = g.num_nodes

    def off(nodes_, edges_, root_, n_nodes, n_edges, V_=V, beam_=beam, K_=K):
        return lib.ea_rnnt_frame_beam_bias_step(p(x), x.stride(0), None, 0, 0, p(in_len), p(ws), p(o1[0]), p(o1[1]), p(o1[2]), nodes_, edges_,
                                                root_, n_nodes, n_edges, 1, mf, V_, beam_, K_, BLANK, -1, 1.0, 0.0, 0, st)

    def strm(nodes_, edges_, root_, n_nodes, n_edges, V_=V, beam_=beam, K_=K):
        return lib.ea_rnnt_frame_beam_stream_bias_step(p(x), x.stride(0), None, 0, 0, p(slots), p(slots), 0, 1, p(state), p(o1[0]), p(o1[1]),
                                                       p(o1[2]), nodes_, edges_, root_, n_nodes, n_edges, S, mf, V_, beam_, K_, BLANK, -1,
                                                       1.0, 0.0, st)

    for call in (off, strm):
        assert call(None, edges, root, N, N - 1) == -2 and call(nodes, None, root, N, N - 1) == -2
        assert call(nodes, edges, None, N, N - 1) == -2
        assert call(nodes, edges, root, N, N) == -2 and call(nodes, edges, root, N, N - 2) == -2 and call(nodes, edges, root, 0, -1) == -2
        assert call(nodes, edges, root, N, N - 1, beam_=65) == -2 and call(nodes, edges, root, N, N - 1, beam_=0) == -2
        assert call(nodes, edges, root, N, N - 1, K_=65) == -2 and call(nodes, edges, root, N, N - 1, K_=V) == -2
        assert call(nodes, edges, root, N, N - 1, V_=1) == -2 and call(nodes, edges, root, N, N - 1, V_=65536) == -2
    assert torch.equal(state, full)
    tk, ln, sc, nh = (torch.empty(4, dtype=torch.int32, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV),
                      torch.empty(2, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV))
    assert lib.ea_rnnt_frame_beam_bias_finish(p(ws), None, N, 1, mf, beam, 2, PAD, 1, p(tk), p(ln), p(sc), p(nh), st) == -2
    assert lib.ea_rnnt_frame_beam_bias_finish(p(ws), nodes, 0, 1, mf, beam, 2, PAD, 1, p(tk), p(ln), p(sc), p(nh), st) == -2
    assert lib.ea_rnnt_frame_beam_bias_finish(p(ws), nodes, N, 1, mf, beam, beam + 1, PAD, 1, p(tk), p(ln), p(sc), p(nh), st) == -2
    assert lib.ea_rnnt_frame_beam_stream_bias_finish(p(state), p(slots), 1, S, mf, beam, None, N, 2, PAD, 1, 2, p(tk), p(ln), p(sc), p(nh), st) == -2
    assert lib.ea_rnnt_frame_beam_stream_bias_finish(p(state), p(slots), 1, S, mf, 65, nodes, N, 2, PAD, 1, 2, p(tk), p(ln), p(sc), p(nh), st) == -2
    assert lib.ea_rnnt_frame_beam_stream_bias_partial(p(state), p(slots), 1, S, mf, 0, PAD, 2, p(tk), p(ln), p(sc), p(nh), st) == -2
    assert lib.ea_rnnt_frame_beam_stream_bias_reset(p(state), p(slots), 1, S, mf, 65, st) == -2
    par = Kn.rnnt_frame_beam_stream_bias_partial(state, torch.tensor([9, 0], dtype=torch.int32, device=DEV), mf, beam, PAD, 3)
    assert par[1].tolist() == [0, 0] and par[3].tolist() == [0, 0] and par[2].tolist() == [-math.inf, 0.0]
    assert torch.equal(state, full)


# ------------------------------------------------------------------------------------------ the decoders
def _second_best_phrase(hyps_per_utt):
    """A phrase (2 or 3 tokens) cut from the second-best unbiased hypothesis of the first utterance that has one long enough."""
    for hyps in hyps_per_utt:
        if len(hyps) > 1 and len(hyps[1][0]) >= 2:
            return list(hyps[1][0][:3])
    raise AssertionError(("no second-best hypothesis of two tokens", hyps_per_utt))


@pytest.mark.gpu
@pytest.mark.parametrize("lm_weight,lm_seed", [(0.0, None), (0.3, 1)])
def test_offline_decoder_vs_oracle(lm_weight, lm_seed):
    """TransducerFrameBeamDecoder(context_graph=...) on the reference-pinned tiny transducer, beam 4: hypotheses, order and scores
    equal the biased oracle's whose rows come from the same GPU modules one hypothesis at a time.  Bound = 1e-4 + 8 x 2^-20 x
    terms (one term per frame, two with an LM: the formula of DESIGN section 3.5 as it stands); as in test_transducer_frame_beam, an utterance whose
    oracle margin is below twice the bound is compared on scores only, and at most one may be.  The search runs under
    set_sync_debug_mode("error")."""
    _need_gpu()
    from tests.test_ctc_prefix_beam import _tiny_lm
    from tests.test_transducer_frame_beam import _decoder, _OneRowModel, _tiny_transducer

    model, d, sample = _tiny_transducer()
    lm = _tiny_lm(d, seed=lm_seed).to(DEV) if lm_weight else None
    kw = dict(nbest=3, lm_model=lm, lm_weight=lm_weight, normalize_scores=False)
    plain = _decoder(model, d, 4, **kw)
    E, enc_len = plain.encode(sample)
    out0 = plain.search(E, enc_len)
    phrase = _second_best_phrase([_hyps(out0, b) for b in range(E.shape[0])])
    g = _graph([(phrase, 1.5)], len(d))
    dec = _decoder(model, d, 4, context_graph=g, **kw)
    dec.search(E, enc_len)  # warm-up: the tables are uploaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = dec.search(E, enc_len)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    one = _OneRowModel(dec, E)
    on_scores_only, worst, changed = 0, 0.0, 0
    for b, L in enumerate(enc_len.cpu().tolist()):
        ref, _, margin = biased_frame_beam_oracle(one.logits_fn(b), int(L), 4, dec.beam_size_token, dec.blank, g,
                                                  lm_fn=one.lm_fn if lm else None, lm_weight=lm_weight, normalize=False, nbest=dec.nbest)
        got = _hyps(out, b)
        bd = SCORE_TOL + 8 * TERM_TOL * int(L) * (2 if lm else 1)
        changed += [y for y, _ in got] != [y for y, _ in _hyps(out0, b)]
        print(f"lm {lm_weight} utterance {b}: {int(L)} frames, phrase {phrase}, oracle margin {margin:.3g}, bound {bd:.2e}, 1-best {got[0]}")
        if margin < 2 * bd:
            on_scores_only += 1
            near = [r_ for y, r_ in ref if y == got[0][0]]
            assert near and abs(near[0] - got[0][1]) < bd, (b, got, ref)
            continue
        assert [y for y, _ in got] == [y for y, _ in ref], (b, got, ref)
        worst = max([worst] + [abs(s - r_) for (_, s), (_, r_) in zip(got, ref)])
        assert worst < bd, (b, worst, bd)
    print(f"lm {lm_weight}: max |score - oracle| {worst:.2e}, n-best lists changed by the phrase: {changed}")
    assert on_scores_only <= 1 and changed >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("lm_weight,lm_seed", [(0.0, None), (0.3, 1)])
def test_streaming_decoder_equals_offline_decoder(lm_weight, lm_seed):
    """StreamingTransducerFrameBeamDecoder(context_graph=...) on the chunk-streaming tiny transducer, beam 4, fed in pieces with
    streams interleaved: sequences and n-best order equal TransducerFrameBeamDecoder.search with the same graph on the same rows
    (the two run the same device code: the score difference is printed and held to the decoder bound); accept runs under
    set_sync_debug_mode("error")."""
    _need_gpu()
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder
    from tests.test_ctc_prefix_beam import _tiny_lm
    from tests.test_streaming_transducer_beam import _chunk_transducer, _hyp_list, _stream_rows

    model, d, rows = _chunk_transducer()
    lm = _tiny_lm(d, seed=lm_seed).to(DEV) if lm_weight else None
    kw = dict(nbest=3, normalize_scores=False, lm_model=lm, lm_weight=lm_weight)

    def offline(dec):
        return [_hyp_list(dec.search(model.joint_encoder_branch(x).view(1, x.shape[0], -1), torch.tensor([x.shape[0]], device=DEV))) for x in rows]

    plain = offline(TransducerFrameBeamDecoder([model], d, beam_size=4, **kw))
    g = _graph([(_second_best_phrase(plain), 1.5)], len(d))
    want = offline(TransducerFrameBeamDecoder([model], d, beam_size=4, context_graph=g, **kw))
    assert want != plain  # (the phrase changes a list or a score)
    mf = max(x.shape[0] for x in rows) + 1
    worst = 0.0
    for pieces in ([3, 5, 1], [2, 7]):
        dec = StreamingTransducerFrameBeamDecoder(model, d, 4, max_streams=2, max_frames=mf, context_graph=g, **kw)
        assert dec.state_bytes_per_stream() == dec.state.shape[1] == 4 * bias_state_words(mf, 4)
        got = _stream_rows(dec, rows, pieces, max_live=2)
        for b in range(len(rows)):
            assert [y for y, _ in got[b]] == [y for y, _ in want[b]], (b, pieces, got[b], want[b])
            bd = SCORE_TOL + 8 * TERM_TOL * rows[b].shape[0] * (2 if lm else 1)
            worst = max([worst] + [abs(s - q) for (_, s), (_, q) in zip(got[b], want[b])])
            assert worst < bd, (b, worst, bd)
    print(f"lm {lm_weight}: max |streamed - offline score| with a graph {worst:.2e}")
    dec = StreamingTransducerFrameBeamDecoder(model, d, 4, max_streams=2, max_frames=mf, context_graph=g, **kw)
    dec.open([0, 1])
    dec.accept([0, 1], torch.cat([rows[0][:2], rows[1][:2]]), [2, 2])  # warm-up: the reset of the opened slots
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        dec.accept([0, 1], torch.cat([rows[0][2:], rows[1][2:5]]), [rows[0].shape[0] - 2, 3])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    toks, k, _ = dec.partial([0])[0]
    h = [(tuple(x["tokens"].tolist()), float(x["score"])) for x in dec.close(0)]
    assert [y for y, _ in h] == [y for y, _ in want[0]] and all(tuple(toks[:k]) == y[:k] for y, _ in h)


@pytest.mark.gpu
def test_cli_round_trip_with_transducer_hotwords(tmp_path, capsys):
    """speech_recognize on synthetic WAVs with a small random chunk-streaming transducer checkpoint: --search
    transducer_frame_beam --transducer-hotwords F prints H- lines that differ from the run without F in text or score, and
    --streaming --search transducer_stream_beam --transducer-hotwords F gives the same texts."""
    _need_gpu()
    from espresso_amd import registry
    from espresso_amd import speech_recognize as sr
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from tests.test_transducer_frame_beam import _write_wav

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
            _write_wav(p, rng.standard_normal(int(16000 * (0.9 + 0.7 * i))) * 3000)
            f.write(f"{u} {p}\n")
    base = ["--path", str(tmp_path / "model.pt"), "--dict", dict_path, "--wav-scp", str(tmp_path / "wav.scp"), "--beam", "4", "--nbest", "2",
            "--transducer-beam-size-token", "3"]

    def run(extra):
        capsys.readouterr()
        sr.main(base + extra)
        lines = {}
        for l in capsys.readouterr().out.splitlines():
            if l.startswith("H-"):
                lines.setdefault(l.split("\t")[0][2:], []).append(l.split("\t")[1:])
        return lines

    plain = run(["--search", "transducer_frame_beam", "--batch-size", "1"])
    second = next((h[1][0].split() for h in plain.values() if len(h) > 1 and len(h[1][0].split()) >= 2), None)
    assert second is not None, plain
    hot = tmp_path / "hot.txt"
    hot.write_text("# cut from a second-best hypothesis\n" + " ".join(second[:3]) + "\t2.0\nt3 t4\n", encoding="utf-8")
    offline = run(["--search", "transducer_frame_beam", "--batch-size", "1", "--transducer-hotwords", str(hot)])
    streamed = run(["--search", "transducer_stream_beam", "--streaming", "--stream-chunk-ms", "170", "--streams", "2",
                    "--transducer-hotwords", str(hot)])
    assert set(offline) == set(streamed) == set(utts) and offline != plain
    worst = 0.0
    for u in utts:
        assert [t for t, _ in offline[u]] == [t for t, _ in streamed[u]], (u, offline[u], streamed[u])
        worst = max([worst] + [abs(float(s) - float(q)) for (_, s), (_, q) in zip(offline[u], streamed[u])])
    print(f"max |offline - streamed score| (base 2) {worst:.2e}")
    assert worst < (SCORE_TOL + 8 * TERM_TOL * 2 * 64) / math.log(2)  # the decoder bound at 64 frames: no utterance here has more
    print(f"H- texts with the phrase file: {[offline[u][0][0] for u in utts]}; without: {[plain[u][0][0] for u in utts]}")
