"""Frame-synchronous transducer beam search (tools/transducer_frame_beam_decoder.py, csrc/rnnt_beam.hip).

tests/transducer_frame_beam_ref.frame_beam_oracle is a float64 numpy statement of the contract.  The CPU
tests hold the oracle to brute force over every alignment; the GPU tests hold the HIP search to the oracle: the step kernels
alone on a table model, then the whole decoder on the reference-pinned tiny transducer."""
import itertools
import math
import os
import wave

import numpy as np
import pytest
import torch

from tests.transducer_frame_beam_ref import TableLM, TableModel, _lae, frame_beam_oracle, fused_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# fp32 search (log-softmax, fusion and score sums in fp32) vs the float64 oracle on the same logits: the project's bound for its
# device-resident searches (tests/test_ctc_prefix_beam.py).  Measured on an MI355X over every case below: 2.1e-6 at worst
SCORE_TOL = 1e-4
# |log-prob of a row of a batched B * beam-row joint_step + step call - the same row computed alone|, per frame term, on the tiny
# transducer below (bf16 GEMM operands, fp32 accumulation; the rows of a GEMM do not interact).  Measured on an MI355X
# (_term_diff, 96 rows): 0.0.  The bound of the whole-decoder comparisons is SCORE_TOL (fp32 search
# vs float64 oracle, as above) + 8 x this x number of terms; with a measured 0 the per-term allowance is one fp32 ulp of a
# log-prob of magnitude < 16
TERM_TOL = 2.0 ** -20
BLANK, EOS = 0, 2


# ---------------------------------------------------------------------------------------------------------------- cases
LENS = [14, 0, 1, 9, 12]  # ragged, with an empty and a one-frame utterance
LENS_WIDE = [7, 0, 1, 4, 6]  # beam 16: sixteen neighbouring scores per frame and utterance leave few seeds with clear margins over 14 frames


def _case(V, beam, K, seed, **opts):
    return dict(V=V, beam=beam, K=K, seed=seed, opts=opts)


# (beam, K) over {1, 4, 16} x {1, 4, beam} for V = 20 and V = 5004, then the options on two of them.  The seeds were chosen on the
# CPU so that the oracle's smallest margin exceeds 10 x SCORE_TOL (test_case_margins_are_clear asserts it, the GPU test again)
CASES = [
    _case(20, 1, 1, 0), _case(20, 1, 4, 0), _case(20, 4, 1, 0), _case(20, 4, 4, 0), _case(20, 16, 1, 1), _case(20, 16, 4, 12),
    _case(20, 16, 16, 2),
    _case(5004, 1, 1, 0), _case(5004, 1, 4, 0), _case(5004, 4, 1, 0), _case(5004, 4, 4, 0), _case(5004, 16, 1, 1),
    _case(5004, 16, 4, 144), _case(5004, 16, 16, 1),
    _case(20, 4, 4, 2, temperature=1.7), _case(20, 4, 4, 1, predicts_eos=True), _case(20, 16, 4, 5, lm="blank", lm_weight=0.6),
    _case(20, 16, 4, 3, lm="no_blank", lm_weight=0.6), _case(20, 4, 4, 0, normalize=False),
    _case(5004, 4, 4, 0, lm="no_blank", lm_weight=0.4, predicts_eos=True, temperature=0.8, normalize=False),
    # V beyond the 5120 columns the row phase stages in LDS: the rest of the row is recomputed from global memory
    _case(6000, 4, 4, 1), _case(6000, 4, 4, 7, lm="blank", lm_weight=0.5),
    # beam 16 over the long utterances (14 frames): the merge and the prefix table at their busiest
    _case(20, 16, 4, 66, long=True),
]


def _lens(c):
    return LENS_WIDE if c["beam"] >= 16 and not c["opts"].get("long") else LENS


def _case_id(c):
    return "V{V}-b{beam}-K{K}".format(**c) + "".join(f"-{k}={v}" for k, v in c["opts"].items())


def _case_models(c):
    o = c["opts"]
    table = TableModel(c["V"], c["seed"], blank=BLANK)
    lm = None
    if o.get("lm"):
        lm = TableLM(c["V"] - (o["lm"] == "no_blank"), c["seed"] + 1000)
    return table, lm


def _case_oracle(c, table, lm, b, nbest):
    o = c["opts"]
    return frame_beam_oracle(table.logits_fn(b), _lens(c)[b], c["beam"], c["K"], BLANK, lm_fn=lm, lm_weight=o.get("lm_weight", 0.0), eos=EOS,
                             predicts_eos=o.get("predicts_eos", False), temperature=o.get("temperature", 1.0),
                             normalize=o.get("normalize", True), nbest=nbest)


def case_margin(c):
    table, lm = _case_models(c)
    return min(_case_oracle(c, table, lm, b, min(c["beam"], 3))[2] for b in range(len(_lens(c))))


# ---------------------------------------------------------------------------------------------------------------- CPU
def _brute_force(logits_fn, T, V, blank, lm_fn=None, lm_weight=0.0):
    """log of the summed probability of ALL alignments (one of `blank` or a token per frame) of every token sequence."""
    tot = {}
    for path in itertools.product(range(V), repeat=T):
        y, lp = (), 0.0
        for t, v in enumerate(path):
            r = fused_row(logits_fn(t, y), blank, 1.0, lm_fn(y) if lm_fn is not None else None, lm_weight)
            lp += r[v]
            if v != blank:
                y = y + (v,)
        tot[y] = _lae(tot.get(y, -math.inf), lp)
    return tot


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("T", [1, 2, 4])
def test_oracle_is_exact_without_pruning(seed, T, with_lm):
    """beam and K exhaustive: every score is the log of the sum over all alignments with at most one symbol per frame, and the
    1-best is the arg-max; with an LM the same with the fused rows."""
    V = 4
    table = TableModel(V, seed, blank=BLANK, sharp=1.0)
    lm = TableLM(V, seed + 50) if with_lm else None
    hyps, triples, _ = frame_beam_oracle(table.logits_fn(0), T, beam=10 ** 6, K=V - 1, blank=BLANK, lm_fn=lm, lm_weight=0.7,
                                         normalize=False, nbest=10 ** 6)
    brute = _brute_force(table.logits_fn(0), T, V, BLANK, lm, 0.7)
    assert {y for y, _ in hyps} == set(brute) and len(hyps) == len(brute)
    for y, s in hyps:
        assert abs(s - brute[y]) < 1e-9, (y, s, brute[y])
    assert hyps[0][0] == max(brute, key=brute.get)
    assert len(triples) == T and all(len(tr) == min(10 ** 6, sum(3 ** n for n in range(t + 2))) for t, tr in enumerate(triples))


def test_oracle_extension_meets_stay():
    """() and (1) are in the beam; () + 1 meets the stay of (1): the scores add, the triple is the stay's."""
    p = {(): [0.5, 0.4, 0.1], (1,): [0.6, 0.2, 0.2], (2,): [0.8, 0.1, 0.1]}
    hyps, triples, _ = frame_beam_oracle(lambda t, y: np.log(p[y]), 2, beam=3, K=2, blank=0, normalize=False, nbest=3)
    assert triples[0] == [(0, 0, 1), (0, 1, 0), (0, 2, 0)]
    got = dict(hyps)
    assert abs(got[(1,)] - math.log(0.4 * 0.6 + 0.5 * 0.4)) < 1e-12
    assert abs(got[()] - math.log(0.25)) < 1e-12
    slot = [y for y, _ in sorted(hyps, key=lambda h: -h[1])].index((1,))
    assert slot == 0 and triples[1][0] == (1, 0, 1)  # continues row 1 (the stay), appends nothing


def test_case_margins_are_clear():
    for c in CASES:
        if c["V"] <= 100:  # (the V = 5004 cases take a minute on the CPU: the GPU test asserts theirs)
            assert case_margin(c) > 10 * SCORE_TOL, _case_id(c)


def _args(*extra):
    from espresso_amd import speech_recognize as sr

    return sr.get_parser().parse_args(["--path", "m.pt", "--dict", "d.txt", "--wav-scp", "wav.scp", *extra])


def _dictionary(n):
    from espresso_amd.data.asr_dictionary import AsrDictionary

    return AsrDictionary.from_symbols([f"t{i}" for i in range(n)], enable_bos=True)


def test_cli_options_and_build_generator():
    from espresso_amd import speech_recognize as sr
    from espresso_amd.tools.transducer_beam_search_decoder import TransducerBeamSearchDecoder
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder
    from tests.test_ctc_prefix_beam import _tiny_lm

    a = _args("--search", "transducer_frame_beam")
    assert (a.search, a.beam, a.nbest, a.transducer_beam_size_token, a.ctc_beam_size_token) == ("transducer_frame_beam", 10, 1, None, None)
    d = _dictionary(8)
    g = sr.build_generator(a, None, d)
    assert type(g) is TransducerFrameBeamDecoder
    assert (g.beam_size, g.nbest, g.beam_size_token, g.temperature, g.normalize_scores, g.lm_model) == (10, 1, 10, 1.0, True, None)
    assert (g.blank, g.bos, g.eos, g.pad) == (d.bos(), d.eos(), d.eos(), d.pad())
    lm = _tiny_lm(d)
    a = _args("--search", "transducer_frame_beam", "--beam", "6", "--nbest", "2", "--transducer-beam-size-token", "3", "--lm-path", "lm.pt",
              "--lm-weight", "0.3", "--temperature", "1.5", "--unnormalized", "--ctc-beam-size-token", "7")
    g = sr.build_generator(a, None, d, lm=lm)
    assert (g.beam_size, g.nbest, g.beam_size_token, g.temperature, g.normalize_scores, g.lm_model, g.lm_weight, g.no_blank_in_lm) == \
        (6, 2, 3, 1.5, False, lm, 0.3, False)
    assert sr.build_generator(_args("--search", "transducer_frame_beam", "--beam", "64"), None, d).beam_size_token == len(d) - 1
    stub = type("M", (), {"eval": lambda self: self})()
    assert type(sr.build_generator(_args("--search", "transducer_beam", "--beam", "3"), stub, d)) is TransducerBeamSearchDecoder
    with pytest.raises(ValueError, match="dictionary"):
        TransducerFrameBeamDecoder([None], _dictionary(10), lm_model=lm)
    with pytest.raises(ValueError):
        TransducerFrameBeamDecoder([None], d, beam_size=65)
    with pytest.raises(ValueError):
        TransducerFrameBeamDecoder([None], d, beam_size=4, nbest=5)
    with pytest.raises(NotImplementedError, match="ensembles"):
        TransducerFrameBeamDecoder([None, None], d)
    with pytest.raises(NotImplementedError, match="print_alignment"):
        TransducerFrameBeamDecoder([None], d, print_alignment=True)
    with pytest.raises(ValueError, match="transducer-beam-size-token"):
        sr.main(["--path", "missing.pt", "--dict", "missing.txt", "--wav-scp", "missing.scp", "--transducer-beam-size-token", "3"])


@pytest.mark.parametrize("extra,named", [
    (["--streaming"], "--streaming"), (["--hotwords", "h.txt"], "--hotwords"), (["--ngram-lm", "lm.arpa"], "--ngram-lm"),
    (["--lm-path", "lm.pt", "--word-dict", "w.txt"], "--word-dict"), (["--word-dict", "w.txt"], "--word-dict"),
    (["--lm-path", os.pathsep.join(["sub.pt", "word.pt"])], "--lm-path"),
    (["--print-alignment", "--results-path", "res"], "--print-alignment"), (["--path", os.pathsep.join(["a.pt", "b.pt"])], "ensembles")])
def test_cli_refusals(extra, named):
    """Every combination the search does not implement raises before a checkpoint is opened (the files do not exist)."""
    from espresso_amd import speech_recognize as sr

    with pytest.raises(NotImplementedError, match=named):
        sr.main(["--path", "missing.pt", "--dict", "missing.txt", "--wav-scp", "missing.scp", "--search", "transducer_frame_beam", *extra])


# ---------------------------------------------------------------------------------------------------------------- GPU
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


def _hyps(out, b):
    tokens, lengths, scores, nhyp = (t.cpu() for t in out)
    return [(tuple(tokens[b, i, : int(lengths[b, i])].tolist()), float(scores[b, i])) for i in range(int(nhyp[b]))]


def _drive_step_kernels(c, table, lm, refs, nbest):
    """The step kernels frame by frame on table logits; the sequences are kept on the host from the triples read back.  The
    number of live slots after a frame is the oracle's (the step does not report it); the slots beyond must carry the
    dead-slot triple.  Rows of dead slots and of finished utterances are NaN: a kernel that read one would not match."""
    from espresso_amd import kernels as Kn

    o, V, beam, K = c["opts"], c["V"], c["beam"], c["K"]
    LENS = _lens(c)
    B, T = len(LENS), max(LENS)
    N = B * beam
    ws = Kn.rnnt_frame_beam_workspace(B, T, beam, DEV)
    in_len = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    out = (torch.empty(N, dtype=torch.int32, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV),
           torch.empty(N, dtype=torch.uint8, device=DEV))
    seqs = [[()] for _ in range(B)]
    nlm = lm.n if lm is not None else 0
    for t in range(T):
        logits = np.full((N, V + 3), np.nan, dtype=np.float32)  # (a row stride larger than V, as a padded output layer gives)
        lm_rows = np.full((N, nlm), np.nan, dtype=np.float32) if lm is not None else None
        for b in range(B):
            if t < LENS[b]:
                for j, y in enumerate(seqs[b]):
                    logits[b * beam + j, :V] = table.row(b, t, y)
                    if lm is not None:
                        lm_rows[b * beam + j] = lm.row(y)
        Kn.rnnt_frame_beam_step(torch.from_numpy(logits).to(DEV)[:, :V], in_len, ws, out, B, T, V, beam, K, BLANK, t,
                                eos=EOS if o.get("predicts_eos") else -1, temperature=o.get("temperature", 1.0),
                                lm_rows=None if lm is None else torch.from_numpy(lm_rows).to(DEV), lm_weight=o.get("lm_weight", 0.0),
                                lm_no_blank=o.get("lm") == "no_blank")
        parent, token, keep = (x.cpu().tolist() for x in out)
        for b in range(B):
            rows = range(b * beam, (b + 1) * beam)
            got = [(parent[n] - b * beam, token[n], keep[n]) for n in rows]
            if t >= LENS[b]:
                assert got == [(j, BLANK, 1) for j in range(beam)], (b, t, got)
                continue
            want = refs[b][1][t]
            assert got[: len(want)] == want, (b, t, got, want)
            assert got[len(want):] == [(0, BLANK, 1)] * (beam - len(want)), (b, t, got)
            seqs[b] = [seqs[b][p] + (() if k else (v,)) for p, v, k in want]
    return Kn.rnnt_frame_beam_finish(ws, B, T, beam, nbest, 1, normalize=o.get("normalize", True))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_step_kernels_vs_oracle(c):
    _need_gpu()
    table, lm = _case_models(c)
    nbest = min(c["beam"], 3)
    refs = [_case_oracle(c, table, lm, b, nbest) for b in range(len(_lens(c)))]
    margin = min(r[2] for r in refs)
    assert margin > 10 * SCORE_TOL, margin
    out = _drive_step_kernels(c, table, lm, refs, nbest)
    worst = 0.0
    for b, (ref, _, _) in enumerate(refs):
        got = _hyps(out, b)
        assert [y for y, _ in got] == [y for y, _ in ref], (b, got, ref)
        worst = max([worst] + [abs(s - r) for (_, s), (_, r) in zip(got, ref)])
    print(f"{_case_id(c)}: oracle margin {margin:.3g}, max |score - oracle| {worst:.2e}")
    assert worst < SCORE_TOL, worst
    assert _hyps(out, 1) == [((), 0.0)]  # in_len 0: the empty hypothesis
    assert float(out[2][1, 1:].max()) == -math.inf if nbest > 1 else True


@pytest.mark.gpu
def test_step_kernels_refuse_bad_arguments():
    _need_gpu()
    from espresso_amd import kernels as Kn

    B, T, V, beam = 1, 2, 8, 2
    ws = Kn.rnnt_frame_beam_workspace(B, T, beam, DEV)
    in_len = torch.ones(B, dtype=torch.int32, device=DEV)
    out = (torch.empty(2, dtype=torch.int32, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV), torch.empty(2, dtype=torch.uint8, device=DEV))
    x = torch.zeros(2, V, device=DEV)
    for kw in (dict(K=8), dict(t=2), dict(blank=8), dict(eos=0), dict(temperature=0.0)):
        a = dict(K=2, blank=0, t=0)
        a.update(kw)
        with pytest.raises(RuntimeError, match="ea_rnnt_frame_beam_step"):
            Kn.rnnt_frame_beam_step(x, in_len, ws, out, B, T, V, beam, **a)
    with pytest.raises(RuntimeError, match="device tensors"):
        Kn.rnnt_frame_beam_step(x.cpu(), in_len, ws, out, B, T, V, beam, 2, 0, 0)
    with pytest.raises(RuntimeError, match="ea_rnnt_frame_beam_finish"):
        Kn.rnnt_frame_beam_finish(ws, B, T, beam, 3, 1)
    assert Kn._lib.lib().ea_rnnt_frame_beam_workspace_bytes(1, 4, 65) == 0


@pytest.mark.gpu
def test_finish_without_frames():
    """T = 0: no step has run, so the finish must not read the workspace (all bits set here: a count read from it would be
    -1 and a score NaN).  Every utterance ends as the oracle's search over no frames does, with the empty hypothesis at score
    0, and the other n-best entries are empty.  tokens is [B][nbest][0]; the entry point still wants a pointer."""
    _need_gpu()
    from espresso_amd import kernels as Kn

    B, beam, nbest = 2, 3, 2
    ref, _, _ = frame_beam_oracle(lambda t, y: None, 0, beam, beam, BLANK, nbest=nbest)
    assert ref == [((), 0.0)]
    ws = Kn.rnnt_frame_beam_workspace(B, 0, beam, DEV).fill_(0xFF)
    tokens = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    lengths = torch.full((B, nbest), 77, dtype=torch.int32, device=DEV)
    scores = torch.full((B, nbest), 77.0, device=DEV)
    nhyp = torch.full((B,), 77, dtype=torch.int32, device=DEV)
    for normalize in (0, 1):
        Kn.check(Kn._lib.lib().ea_rnnt_frame_beam_finish(Kn._p(ws), B, 0, beam, nbest, 1, normalize, Kn._p(tokens), Kn._p(lengths),
                                                         Kn._p(scores), Kn._p(nhyp), Kn._stream()), "ea_rnnt_frame_beam_finish")
        assert nhyp.tolist() == [1] * B and lengths.tolist() == [[0, 0]] * B and tokens.tolist() == [77]
        assert scores.tolist() == [[ref[0][1], -math.inf]] * B


@pytest.mark.gpu
def test_fusion_changes_the_answer():
    """Two tokens nearly tied acoustically at every emitting frame; the LM prefers one strongly: lambda = 0 picks the acoustic
    winner, lambda > 0 the LM's choice, and both equal the oracle."""
    _need_gpu()
    from espresso_amd import kernels as Kn

    V, beam, K, T = 10, 3, 2, 5
    a, b_ = 5, 6  # the LM prefers a over b_; acoustically b_ is ahead by about 0.2 per emitting frame
    x = -8.0 - 0.5 * np.arange(V, dtype=np.float64)[None].repeat(T, 0)
    for t in range(T):
        if t % 2 == 0:
            x[t, b_], x[t, a], x[t, 0] = -0.6 - 0.07 * t, -0.8 - 0.03 * t, -3.0
        else:
            x[t, 0] = -0.05
    x = x.astype(np.float32)
    m = np.full(V, -6.0)
    m[a], m[b_] = -0.1, -5.0
    m = (m - math.log(np.exp(m).sum())).astype(np.float32)
    best = {}
    for lam in (0.0, 0.5):
        ref, triples, margin = frame_beam_oracle(lambda t, y: x[t].astype(np.float64), T, beam, K, BLANK, lm_fn=lambda y: m.astype(np.float64),
                                                 lm_weight=lam, normalize=False)
        assert margin > 10 * SCORE_TOL
        ws = Kn.rnnt_frame_beam_workspace(1, T, beam, DEV)
        out = (torch.empty(beam, dtype=torch.int32, device=DEV), torch.empty(beam, dtype=torch.int32, device=DEV),
               torch.empty(beam, dtype=torch.uint8, device=DEV))
        in_len = torch.tensor([T], dtype=torch.int32, device=DEV)
        lm_rows = torch.from_numpy(m)[None].repeat(beam, 1).to(DEV)
        for t in range(T):
            Kn.rnnt_frame_beam_step(torch.from_numpy(x[t])[None].repeat(beam, 1).to(DEV), in_len, ws, out, 1, T, V, beam, K, BLANK, t,
                                    lm_rows=lm_rows, lm_weight=lam)
            got = list(zip(*(o.cpu().tolist() for o in out)))[: len(triples[t])]
            assert got == triples[t], (lam, t, got, triples[t])
        got = _hyps(Kn.rnnt_frame_beam_finish(ws, 1, T, beam, 1, 1, normalize=False), 0)
        assert got[0][0] == ref[0][0] and abs(got[0][1] - ref[0][1]) < SCORE_TOL, (got, ref)
        best[lam] = got[0][0]
    assert best[0.0] == (b_, b_, b_) and best[0.5] == (a, a, a), best


# ------------------------------------------------------------------------------------------ the whole decoder, tiny transducer
def _tiny_transducer():
    from tests.gpu_checks import GOLD, _Task, build_tiny_transducer

    g = np.load(os.path.join(GOLD, "ref_conformer_transducer_tiny.npz"))
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}
    model = build_tiny_transducer().to(DEV)
    model.load_state_dict(model.upgrade_state_dict_named(dict(sd), ""), strict=False)
    model.eval()
    d = _Task(40).target_dictionary
    sample = {"net_input": {"src_tokens": torch.from_numpy(g["feats"]).to(DEV), "src_lengths": torch.from_numpy(g["lengths"]).to(DEV)}}
    return model, d, sample


def _decoder(model, d, beam, **kw):
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder

    return TransducerFrameBeamDecoder([model], d, beam_size=beam, **kw)


class _OneRowModel:
    """logits_fn / lm_fn of the oracle from the same GPU modules, one hypothesis at a time: the predictor (and the LM) advanced
    from the zero state along bos + y, joint_step on one row."""

    def __init__(self, dec, E):
        self.dec, self.E = dec, E  # E fp32 [B][T'][J]
        self._pred, self._lm = {}, {}

    def _walk(self, cache, module, first, y, tok_map):
        if y not in cache:
            if not y:
                state = module.init_state(1, DEV)
                tok = first
            else:
                state = self._walk(cache, module, first, y[:-1], tok_map)[1]
                tok = y[-1]
            cache[y] = module.advance(tok_map(torch.tensor([tok], dtype=torch.int32, device=DEV)), state)
        return cache[y]

    def logits_fn(self, b):
        model = self.dec.model

        def fn(t, y):
            out = self._walk(self._pred, model.decoder, self.dec.bos, y, lambda x: x)[0]
            return model.joint_step(self.E[b, t:t + 1].contiguous(), out)[0, : self.dec.vocab_size].double().cpu().numpy()

        return fn

    def lm_fn(self, y):
        feat = self._walk(self._lm, self.dec.lm_model.decoder, self.dec.eos, y, self.dec._lm_tokens)[0]
        return self.dec._lm_rows(feat)[0].double().cpu().numpy()


def _term_diff(dec, E, n_rows=96):
    """max |log-softmax of a row of a batched joint_step call - the same row computed alone| over n_rows (frame, predictor state)
    pairs of the model: the per-term quantity TERM_TOL is derived from."""
    from espresso_amd import kernels as Kn

    model, V = dec.model, dec.vocab_size
    rng = np.random.default_rng(0)
    Ef = E.reshape(-1, E.shape[-1])
    rows = torch.from_numpy(rng.integers(0, Ef.shape[0], n_rows)).to(DEV)
    toks = torch.from_numpy(rng.integers(4, V, n_rows).astype(np.int32)).to(DEV)
    state = model.decoder.init_state(n_rows, DEV)
    _, state = model.decoder.advance(torch.full((n_rows,), dec.bos, dtype=torch.int32, device=DEV), state)
    out, _ = model.decoder.advance(toks, state)
    Er = Ef.index_select(0, rows).contiguous()
    lg = model.joint_step(Er, out)[:, :V]
    batched = Kn.log_softmax(lg, n_rows, V, lg.stride(0))
    worst = 0.0
    for i in range(n_rows):
        l1 = model.joint_step(Er[i:i + 1].contiguous(), out[i:i + 1].contiguous())[:, :V]
        worst = max(worst, float((Kn.log_softmax(l1, 1, V, l1.stride(0))[0] - batched[i]).abs().max()))
    return worst


@pytest.mark.gpu
def test_decoder_beam1_equals_greedy():
    _need_gpu()
    from espresso_amd.tools.transducer_greedy_decoder import TransducerGreedyDecoder

    model, d, sample = _tiny_transducer()
    greedy = TransducerGreedyDecoder([model], d, max_num_expansions_per_step=1)
    toks, _, _ = greedy._generate(sample)
    hyps = _decoder(model, d, 1).generate([model], sample)
    assert len(hyps) == toks.shape[0]
    n_tok = 0
    for b in range(toks.shape[0]):
        want = [int(v) for v in toks[b].tolist() if int(v) != greedy.blank]
        assert hyps[b][0]["tokens"].tolist() == want, (b, hyps[b][0]["tokens"].tolist(), want)
        n_tok += len(want)
    assert n_tok > 0


@pytest.mark.gpu
# LM weight and the seed of the tiny LM per beam: chosen, before any run of the search, for clear margins of the ORACLE on the
# fp32 CPU model (oracle/torch_ref.py: encoder, lstm_predictor, transducer_joint, lstm_lm), as the margins are the oracle's own
@pytest.mark.parametrize("beam,lm_weight,lm_seed", [(3, 0.0, None), (5, 0.0, None), (3, 0.3, 1), (5, 0.2, 1)])
def test_decoder_vs_oracle_on_the_same_modules(beam, lm_weight, lm_seed):
    """Every utterance of the fixture: hypotheses, their order and scores equal the oracle's whose rows come from the same GPU
    modules one hypothesis at a time.  Bound = SCORE_TOL + 8 x TERM_TOL x terms (one term per frame, two with an LM); an
    utterance whose oracle margin is below twice the bound is compared on scores only, and at most one utterance may be.

    Measured on an MI355X: beam 3 without LM: oracle margins 8.5e-4, 4.7e-3, 5.5e-3, worst score difference 5.8e-6."""
    _need_gpu()
    from tests.test_ctc_prefix_beam import _tiny_lm

    model, d, sample = _tiny_transducer()
    lm = _tiny_lm(d, seed=lm_seed).to(DEV) if lm_weight else None
    dec = _decoder(model, d, beam, nbest=min(beam, 3), lm_model=lm, lm_weight=lm_weight, normalize_scores=False)
    E, enc_len = dec.encode(sample)
    print(f"per-term |batched - one row| on this model: {_term_diff(dec, E):.2e}")
    out = dec.search(E, enc_len)
    one = _OneRowModel(dec, E)
    lens = enc_len.cpu().tolist()
    on_scores_only, worst = 0, 0.0
    for b, L in enumerate(lens):
        ref, _, margin = frame_beam_oracle(one.logits_fn(b), int(L), beam, dec.beam_size_token, dec.blank, lm_fn=one.lm_fn if lm else None,
                                           lm_weight=lm_weight, normalize=False, nbest=dec.nbest)
        bound = SCORE_TOL + 8 * TERM_TOL * int(L) * (2 if lm else 1)
        got = _hyps(out, b)
        print(f"beam {beam} lm {lm_weight} utterance {b}: {int(L)} frames, oracle margin {margin:.3g}, bound {bound:.2e}, 1-best {got[0]}")
        if margin < 2 * bound:
            on_scores_only += 1
            near = [r for y, r in ref if y == got[0][0]]
            assert near and abs(near[0] - got[0][1]) < bound, (b, got, ref)
            continue
        assert [y for y, _ in got] == [y for y, _ in ref], (b, got, ref)
        worst = max([worst] + [abs(s - r) for (_, s), (_, r) in zip(got, ref)])
        assert worst < bound, (b, worst, bound)
    print(f"beam {beam} lm {lm_weight}: max |score - oracle| {worst:.2e}")
    assert on_scores_only <= 1, on_scores_only


@pytest.mark.gpu
def test_decoder_batch_equals_single():
    """A batch of 3 gives, per utterance, what that utterance gives alone on the same encoder output."""
    _need_gpu()
    model, d, sample = _tiny_transducer()
    dec = _decoder(model, d, 4, nbest=2)
    E, enc_len = dec.encode(sample)
    assert E.shape[0] >= 3
    out = dec.search(E[:3], enc_len[:3])
    for b in range(3):
        alone = _hyps(dec.search(E[b:b + 1], enc_len[b:b + 1]), 0)
        got = _hyps(out, b)
        bound = SCORE_TOL + 8 * TERM_TOL * int(enc_len[b])
        assert [y for y, _ in got] == [y for y, _ in alone], (b, got, alone)
        assert all(abs(s - r) < bound for (_, s), (_, r) in zip(got, alone)), (b, got, alone)


@pytest.mark.gpu
@pytest.mark.parametrize("with_lm", [False, True])
def test_search_does_not_synchronise(with_lm):
    _need_gpu()
    from tests.test_ctc_prefix_beam import _tiny_lm

    model, d, sample = _tiny_transducer()
    lm = _tiny_lm(d, seed=3).to(DEV) if with_lm else None
    dec = _decoder(model, d, 4, nbest=2, lm_model=lm, lm_weight=0.3)
    E, enc_len = dec.encode(sample)
    ref = [t.clone() for t in dec.search(E, enc_len)]  # warm-up (cached bf16 weights)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = dec.search(E, enc_len)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(out, ref):
        assert torch.equal(a, b)
    assert int(ref[1][:, 0].sum()) > 0  # (something was recognised)


def _write_wav(path, samples):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(samples, -32768, 32767).astype("<i2").tobytes())


@pytest.mark.gpu
def test_cli_end_to_end(tmp_path, capsys):
    """speech_recognize --search transducer_frame_beam on synthetic WAVs: one H- line per utterance equal to what the decoder
    returns directly; --nbest 2 --results-path writes the result files; a CTC model is refused."""
    _need_gpu()
    from espresso_amd import registry
    from espresso_amd import speech_recognize as sr
    from espresso_amd.data.audio_utils import read_wav
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder

    dict_path = str(tmp_path / "dict.txt")
    with open(dict_path, "w") as f:
        f.write("".join(f"t{i} 1\n" for i in range(30)))
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(dict=dict_path, autoregressive=False,
                                                                                    criterion_name="transducer_loss"))
    d = task.target_dictionary
    enc = {"conv_channels": "[64, 64, 16, 16]", "embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4,
           "normalize_before": True, "relative_positional_embeddings": True, "layer_type": "conformer"}
    name = "speech_transformer_transducer_base"
    block = {"_name": name, "encoder": enc, "decoder": {"embed_dim": 48, "hidden_size": 64, "layers": 1}, "joint_dim": 64,
             "dropout": 0.0, "attention_dropout": 0.0, "activation_dropout": 0.0}
    cls = registry.MODEL_REGISTRY[name]
    torch.manual_seed(0)
    model = cls.build_model(cls.config_class.from_dict(block), task)
    torch.save({"model": model.state_dict(), "cfg": {"model": block}}, str(tmp_path / "model.pt"))
    model = model.to(DEV).eval()
    rng = np.random.default_rng(0)
    utts = [f"utt{i}" for i in range(4)]
    with open(tmp_path / "wav.scp", "w") as f:
        for i, u in enumerate(utts):
            p = str(tmp_path / f"{u}.wav")
            _write_wav(p, rng.standard_normal(int(16000 * (0.6 + 0.3 * i))) * 3000)
            f.write(f"{u} {p}\n")
    argv = ["--path", str(tmp_path / "model.pt"), "--dict", dict_path, "--wav-scp", str(tmp_path / "wav.scp"), "--search",
            "transducer_frame_beam", "--beam", "4", "--max-tokens", "500", "--batch-size", "3"]
    capsys.readouterr()
    sr.main(argv)
    lines = [l.split("\t") for l in capsys.readouterr().out.splitlines() if l.startswith("H-")]

    waves = [read_wav(str(tmp_path / f"{u}.wav")) for u in utts]
    task.build_frontend(torch.device(DEV))
    gen = TransducerFrameBeamDecoder([model], d, beam_size=4)
    expect = []
    for bt in sr.make_batches(utts, [len(w) for w in waves], 500, 3):
        sample = sr.collate(bt, utts, waves, torch.device(DEV))
        hyps = gen.generate([model], task.prepare_sample(sample, train=False))
        for i, u in enumerate(sample["utt_ids"]):
            toks = [t for t in hyps[i][0]["tokens"].tolist() if t not in gen.symbols_to_strip_from_output]
            expect.append((f"H-{u}", d.string(torch.tensor(toks)), float(hyps[i][0]["score"]) / math.log(2)))
    assert len(lines) == len(expect) == len(utts)
    assert any(text.strip() for _, text, _ in lines)  # (something was recognised: equal empty lines would show nothing)
    for (hu, text, score), (eu, etext, escore) in zip(lines, expect):
        assert (hu, text) == (eu, etext)
        assert abs(float(score) - escore) < 1e-4, (hu, score, escore)

    res = str(tmp_path / "res")
    capsys.readouterr()
    sr.main(argv + ["--nbest", "2", "--results-path", res])
    log = open(os.path.join(res, "decode.log")).read().splitlines()
    assert sum(l.startswith("H-") for l in log) == 2 * len(utts)
    for f in ("decoded_results.txt", "decoded_char_results.txt"):
        assert os.path.getsize(os.path.join(res, f)) > 0

    ctc_block = {"_name": "speech_transformer_encoder_model", "encoder": enc, "dropout": 0.0, "attention_dropout": 0.0,
                 "activation_dropout": 0.0, "layernorm_embedding": True}
    torch.save({"model": {}, "cfg": {"model": ctc_block}}, str(tmp_path / "ctc.pt"))
    with pytest.raises(NotImplementedError, match="transducer model"):
        sr.main(["--path", str(tmp_path / "ctc.pt")] + argv[2:])
