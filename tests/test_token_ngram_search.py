"""The four token-level beam searches with the sub-word n-gram LM (models/token_ngram_lm.py): the offline CTC prefix beam and
transducer frame beam against the float64 oracles whose `lm_fn` comes from tests.ngram_ref.ArpaRef, the streamed searches
against the offline ones bit for bit, no host synchronisation in the loop, and one command-line round trip.

Margin rule, as in tests/test_ctc_prefix_beam.py with the n-gram rows' error in place of LM_TOL: an utterance whose oracle
margin is below twice the score bound is not compared (its hypotheses count as skipped), and at most 10 % of the compared
hypotheses may be skipped; test_chosen_seeds_keep_the_skipped_share_low checks that share on the CPU with the oracles alone."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_ctc_prefix_beam import SCORE_TOL, _decoder, _dictionary, _hyps, _peaked, prefix_beam_oracle
from tests.token_ngram_ref import ROW_TOL, TokenRowsRef, random_lm_text, write_arpa
from tests.transducer_frame_beam_ref import TableModel, frame_beam_oracle

DEV = "cuda:0"
pytestmark = [pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")]  # (-inf) - (-inf) in oracle margins
MAX_SKIPPED = 0.10

# ---- the CTC cases: the shapes of test_ctc_prefix_beam.test_search_vs_oracle_with_lm --------------------------------------------
CTC_B, CTC_T, CTC_LAM = 4, 6, 0.4
CTC_LENS = np.array([6, 5, 1, 0], dtype=np.int32)
CTC_CASES = [(2, 3), (4, 4), (6, 3), (10, 6)]  # (beam, K)
CTC_LMS = [(3, True, 0), (2, False, 1), (6, True, 2)]  # (order, <unk>, seed of the file)
CTC_BOUND = SCORE_TOL + CTC_LAM * ROW_TOL * (CTC_T + 1)  # one LM term per token and the eos term

# ---- the transducer cases: the shape of test_transducer_frame_beam's V = 20 LM-fusion cases -------------------------------------
RN_V, RN_LENS = 20, [7, 0, 1, 4, 6]
# (beam, K, seed, lm_weight); the seeds were scanned on the CPU for oracle margins above twice the bound (the test below asserts it)
RN_CASES = [(16, 4, 3, 0.6), (4, 4, 1, 0.6)]
RN_BOUND = SCORE_TOL + 0.6 * ROW_TOL * max(RN_LENS)
BLANK, EOS = 0, 2


@functools.lru_cache(maxsize=None)
def _ctc_inputs():
    d = _dictionary(16)
    x = _peaked(np.random.default_rng(0), CTC_B * CTC_T, len(d), sharp=6.0, scale=2.5).reshape(CTC_B, CTC_T, len(d)).astype(np.float32)
    x.setflags(write=False)
    return d, x


@functools.lru_cache(maxsize=None)
def _lm_text(n_symbols, order, unk, seed):
    return random_lm_text(_dictionary(n_symbols), order, unk, seed=100 + seed, per_order=80)


@functools.lru_cache(maxsize=None)
def _ctc_oracle(beam, K, lm_case):
    """Per utterance (hypotheses, margin) of the oracle, computed once per case."""
    d, x = _ctc_inputs()
    ref = TokenRowsRef(_lm_text(16, *lm_case), d)
    return [prefix_beam_oracle(x[b].astype(np.float64), int(CTC_LENS[b]), beam, K, d.bos(), lm_fn=ref.lm_fn, lm_weight=CTC_LAM,
                               eos=d.eos(), nbest=2) for b in range(CTC_B)]


@functools.lru_cache(maxsize=None)
def _rnnt_oracle(beam, K, seed, lam):
    d = _dictionary(RN_V - 5)
    assert len(d) == RN_V and d.bos() == BLANK and d.eos() == EOS
    ref = TokenRowsRef(_lm_text(RN_V - 5, 3, True, seed), d)
    table = TableModel(RN_V, seed, blank=BLANK)
    return table, [frame_beam_oracle(table.logits_fn(b), RN_LENS[b], beam, K, BLANK, lm_fn=ref.lm_fn, lm_weight=lam, eos=EOS,
                                     nbest=min(beam, 3)) for b in range(len(RN_LENS))]


def _skipped_share(results, bound):
    """results: per utterance (hypotheses, ..., margin) -> (share of the hypotheses in utterances below the margin rule, flags)."""
    skip = [r[-1] < 2 * bound for r in results]
    n = sum(len(r[0]) for r in results)
    return sum(len(r[0]) for r, s in zip(results, skip) if s) / max(1, n), skip


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_chosen_seeds_keep_the_skipped_share_low():
    for lm_case in CTC_LMS:
        for beam, K in CTC_CASES:
            share, _ = _skipped_share(_ctc_oracle(beam, K, lm_case), CTC_BOUND)
            assert share <= MAX_SKIPPED, (lm_case, beam, K, share)
    for c in RN_CASES:
        share, _ = _skipped_share(_rnnt_oracle(*c)[1], RN_BOUND)
        assert share <= MAX_SKIPPED, (c, share)


def test_oracle_rows_put_minus_inf_where_the_map_says():
    d, _ = _ctc_inputs()
    ref = TokenRowsRef(_lm_text(16, 2, False, 1), d)
    row = ref.lm_fn((d.index("t3"), d.eos()))
    assert row[d.pad()] == row[d.bos()] == -math.inf and math.isfinite(row[d.eos()]) and row[d.unk()] == -math.inf
    assert row[d.eos()] == ref.ref.logp(["<s>", ref.word(d.index("t3")), "</s>"], "</s>")


# ---------------------------------------------------------------------------------------------------------------- GPU
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


def _token_lm(tmp_path, d, text):
    from espresso_amd.models.token_ngram_lm import TokenNGramLM

    return TokenNGramLM(write_arpa(tmp_path, "lm.arpa", text), d)


@pytest.mark.gpu
@pytest.mark.parametrize("lm_case", CTC_LMS)
@pytest.mark.parametrize("beam,K", CTC_CASES)
def test_ctc_search_vs_oracle(tmp_path, beam, K, lm_case):
    _need_gpu()
    d, x = _ctc_inputs()
    lm = _token_lm(tmp_path, d, _lm_text(16, *lm_case))
    dec = _decoder(d, beam, K, nbest=2, lm=lm, lm_weight=CTC_LAM)
    out = dec.search(torch.from_numpy(np.array(x)).to(DEV), torch.from_numpy(CTC_LENS).to(DEV))
    refs = _ctc_oracle(beam, K, lm_case)
    share, skip = _skipped_share(refs, CTC_BOUND)
    assert share <= MAX_SKIPPED
    worst = 0.0
    for b, ((ref, margin), s) in enumerate(zip(refs, skip)):
        got = _hyps(out, b)
        print(f"utterance {b}: oracle margin {margin:.3g}, got {got}, oracle {ref}")
        if s:
            continue
        finite = [(y, r) for y, r in ref if r > -math.inf]
        assert [y for y, _ in got] == [y for y, _ in finite], (b, got, ref)
        worst = max([worst] + [abs(g - r) for (_, g), (_, r) in zip(got, finite)])
    print(f"beam {beam} K {K} n-gram {lm_case}: max |score - oracle| {worst:.2e} (bound {CTC_BOUND:.2e})")
    assert worst < CTC_BOUND, worst


@pytest.mark.gpu
@pytest.mark.parametrize("beam,K,seed,lam", RN_CASES)
def test_transducer_steps_vs_oracle(tmp_path, beam, K, seed, lam):
    """The loop of TransducerFrameBeamDecoder.search (step, then lm_update with the step's triple) on table logits: the triples
    of every frame and the final hypotheses equal the oracle's."""
    _need_gpu()
    from espresso_amd import kernels as Kn
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder

    table, refs = _rnnt_oracle(beam, K, seed, lam)
    share, skip = _skipped_share(refs, RN_BOUND)
    assert share <= MAX_SKIPPED and not any(skip)  # (the triples below are checked for every utterance)
    d = _dictionary(RN_V - 5)
    lm = _token_lm(tmp_path, d, _lm_text(RN_V - 5, 3, True, seed))
    dec = TransducerFrameBeamDecoder(None, d, beam_size=beam, beam_size_token=K, nbest=min(beam, 3), lm_model=lm, lm_weight=lam)
    B, T, N = len(RN_LENS), max(RN_LENS), len(RN_LENS) * beam
    ws = Kn.rnnt_frame_beam_workspace(B, T, beam, DEV)
    in_len = torch.tensor(RN_LENS, dtype=torch.int32, device=DEV)
    out = (torch.empty(N, dtype=torch.int32, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV),
           torch.empty(N, dtype=torch.uint8, device=DEV))
    state, lm_rows = dec.lm_start(N, torch.device(DEV))
    seqs = [[()] for _ in range(B)]
    for t in range(T):
        logits = np.zeros((N, RN_V), dtype=np.float32)
        for b in range(B):
            if t < RN_LENS[b]:
                for j, y in enumerate(seqs[b]):
                    logits[b * beam + j] = table.row(b, t, y)
        Kn.rnnt_frame_beam_step(torch.from_numpy(logits).to(DEV), in_len, ws, out, B, T, RN_V, beam, K, BLANK, t, lm_rows=lm_rows,
                                lm_weight=lam, lm_no_blank=dec.no_blank_in_lm)
        state, lm_rows = dec.lm_update(state, *out)
        parent, token, keep = (x.cpu().tolist() for x in out)
        for b in range(B):
            if t < RN_LENS[b]:
                want = refs[b][1][t]
                got = [(parent[n] - b * beam, token[n], keep[n]) for n in range(b * beam, b * beam + len(want))]
                assert got == want, (b, t, got, want)
                seqs[b] = [seqs[b][p] + (() if k else (v,)) for p, v, k in want]
    res = Kn.rnnt_frame_beam_finish(ws, B, T, beam, dec.nbest, 1, normalize=True)
    worst = 0.0
    for b, (ref, _, margin) in enumerate(refs):
        got = _hyps(res, b)
        assert [y for y, _ in got] == [y for y, _ in ref], (b, got, ref)
        worst = max([worst] + [abs(g - r) for (_, g), (_, r) in zip(got, ref)])
    print(f"beam {beam} K {K}: max |score - oracle| {worst:.2e} (bound {RN_BOUND:.2e})")
    assert worst < RN_BOUND


def _prefer_text(d, a, b_):
    """A bigram file over d's symbols that prefers `a` strongly over `b_` in every context."""
    syms = [s for i, s in enumerate(d.symbols) if i not in (d.bos(), d.pad(), d.eos(), d.unk())]
    uni = [("<s>", -99.0), ("</s>", -1.0), ("<unk>", -3.0)] + [(s, -0.05 if s == a else -3.0 if s == b_ else -2.5) for s in syms]
    bi = [(a, a, -0.02), (b_, b_, -2.9), ("<s>", a, -0.03)]
    lines = ["\\data\\", f"ngram 1={len(uni)}", f"ngram 2={len(bi)}", "", "\\1-grams:"] + [f"{p}\t{w}\t-0.1" for w, p in uni]
    return "\n".join(lines + ["", "\\2-grams:"] + [f"{p}\t{u} {w}" for u, w, p in bi] + ["", "\\end\\"]) + "\n"


def _tied_lprobs(V, a, b_, T=5):
    """test_ctc_prefix_beam.test_fusion_changes_the_answer's input: b_ ahead of a by about 0.2 per emitting frame."""
    x = -8.0 - 0.5 * np.arange(V, dtype=np.float64)[None].repeat(T, 0)
    for t in range(T):
        if t % 2 == 0:
            x[t, b_], x[t, a], x[t, 0] = -0.6 - 0.07 * t, -0.8 - 0.03 * t, -3.0
        else:
            x[t, 0] = -0.05
    return (x - np.logaddexp.reduce(x, axis=1, keepdims=True))[None].astype(np.float32)


@pytest.mark.gpu
def test_fusion_changes_the_answer(tmp_path):
    _need_gpu()
    d = _dictionary(10)
    a, b_ = 5, 6
    x = _tied_lprobs(len(d), a, b_)
    lens = np.array([x.shape[1]], dtype=np.int32)
    text = _prefer_text(d, d.symbols[a], d.symbols[b_])
    lm, ref = _token_lm(tmp_path, d, text), TokenRowsRef(text, d)
    args = (torch.from_numpy(x).to(DEV), torch.from_numpy(lens).to(DEV))
    plain = _hyps(_decoder(d, 3, 2).search(*args), 0)[0][0]
    dec = _decoder(d, 3, 2, lm=lm, lm_weight=0.5)
    fused = _hyps(dec.search(*args), 0)[0]
    want, margin = prefix_beam_oracle(x[0].astype(np.float64), 5, 3, 2, d.bos(), lm_fn=ref.lm_fn, lm_weight=0.5, eos=d.eos())
    assert margin > 2 * (SCORE_TOL + 0.5 * ROW_TOL * 6)
    assert plain == (b_, b_, b_) and fused[0] == (a, a, a) == want[0][0], (plain, fused, want)
    assert abs(fused[1] - want[0][1]) < SCORE_TOL + 0.5 * ROW_TOL * 6


def _graph(d, x, lens):
    from espresso_amd.tools.context_graph import ContextGraph
    from tests.hotword_ref import grid_phrases

    return ContextGraph(grid_phrases(x.astype(np.float64), lens, d.bos()), len(d))


@pytest.mark.gpu
@pytest.mark.parametrize("with_graph", [False, True])
def test_ctc_streamed_equals_offline(tmp_path, with_graph):
    """Pieces of 1, 3 and all frames: nhyp, lengths, scores and tokens of every stream are torch.equal to the offline search's."""
    _need_gpu()
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder
    from espresso_amd.tools.streaming_ctc_prefix_beam_decoder import StreamingCTCPrefixBeamDecoder

    d = _dictionary(20)
    V, B, T = len(d), 4, 12
    x = _peaked(np.random.default_rng(0), B * T, V, sharp=4.0, scale=2.0).reshape(B, T, V).astype(np.float32)
    lens = np.array([12, 7, 0, 10], dtype=np.int32)
    lm = _token_lm(tmp_path, d, random_lm_text(d, 3, True, seed=5, per_order=80))
    graph = _graph(d, x, lens) if with_graph else None
    kw = dict(beam_size=6, nbest=3, beam_size_token=4, lm_model=lm, lm_weight=0.5, insertion_bonus=0.3, context_graph=graph)
    xd = torch.from_numpy(x).to(DEV)
    tokens, lengths, scores, nhyp = CTCPrefixBeamSearchDecoder([None], d, **kw).search(xd, torch.from_numpy(lens).to(DEV))
    assert int(lengths[:, 0].sum()) > 0
    for piece in (1, 3, T):
        dec = StreamingCTCPrefixBeamDecoder(d, B, T, **kw)
        ids = list(range(B))
        dec.open(ids)
        for t0 in range(0, T, piece):
            counts = [max(0, min(piece, int(lens[b]) - t0)) for b in ids]
            dec.accept_lprobs(ids, torch.cat([xd[b, t0:t0 + c] for b, c in zip(ids, counts)]), counts)
        for b in ids:
            tk, ln, sc, nh = dec.finish([b], max_u=T)
            assert torch.equal(nh[0], nhyp[b]) and torch.equal(ln[0], lengths[b]) and torch.equal(sc[0], scores[b]), (piece, b)
            for i in range(int(nhyp[b])):
                n = int(lengths[b, i])
                assert torch.equal(tk[0, i, :n], tokens[b, i, :n]), (piece, b, i)
            dec.close(b)


def _chunk_transducer():
    from tests.test_streaming_transducer_beam import _chunk_transducer as make

    return make()


@pytest.mark.gpu
@pytest.mark.parametrize("with_graph", [False, True])
def test_transducer_streamed_equals_offline(tmp_path, with_graph):
    """The chunk transducer's encoder rows through TransducerFrameBeamDecoder.search, one utterance at a time, and through the
    streaming decoder in pieces of 1, 3 and all frames: torch.equal."""
    _need_gpu()
    from espresso_amd.tools.context_graph import ContextGraph
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder

    model, d, rows = _chunk_transducer()
    lm = _token_lm(tmp_path, d, random_lm_text(d, 3, True, seed=9, per_order=150, absent=0.1))
    plain = TransducerFrameBeamDecoder([model], d, beam_size=4, nbest=3, normalize_scores=False)
    want_plain = [plain.search(model.joint_encoder_branch(x).view(1, x.shape[0], -1), torch.tensor([x.shape[0]], device=DEV)) for x in rows]
    graph = None
    if with_graph:  # phrases from what the unbiased search recognises, so that the bias is live
        best = [tuple(w[0][0, 0, : int(w[1][0, 0])].tolist()) for w in want_plain]
        graph = ContextGraph([(list(y[:2]), 1.5) for y in best if len(y) >= 2] or [([5, 6], 1.5)], len(d))
    kw = dict(nbest=3, normalize_scores=False, lm_model=lm, lm_weight=0.6, context_graph=graph)
    off = TransducerFrameBeamDecoder([model], d, beam_size=4, **kw)
    want = [off.search(model.joint_encoder_branch(x).view(1, x.shape[0], -1), torch.tensor([x.shape[0]], device=DEV)) for x in rows]
    T = max(x.shape[0] for x in rows)
    for piece in (1, 3, T):
        dec = StreamingTransducerFrameBeamDecoder(model, d, 4, max_streams=len(rows), max_frames=T, **kw)
        ids = list(range(len(rows)))
        dec.open(ids)
        for t0 in range(0, T, piece):
            counts = [max(0, min(piece, rows[b].shape[0] - t0)) for b in ids]
            dec.accept(ids, torch.cat([rows[b][t0:t0 + c] for b, c in zip(ids, counts)]), counts)
        for b in ids:
            tk, ln, sc, nh = dec.finish_tensors([b], max_u=rows[b].shape[0])
            wt, wl, wsc, wn = want[b]
            assert torch.equal(nh, wn) and torch.equal(ln, wl) and torch.equal(sc, wsc), (piece, b, sc, wsc)
            for i in range(int(wn[0])):
                n = int(wl[0, i])
                assert torch.equal(tk[0, i, :n], wt[0, i, :n]), (piece, b, i)


@pytest.mark.gpu
@pytest.mark.parametrize("search", ["ctc", "transducer"])
def test_search_with_the_ngram_lm_does_not_synchronise(tmp_path, search):
    _need_gpu()
    if search == "ctc":
        d = _dictionary(16)
        x = torch.from_numpy(_peaked(np.random.default_rng(3), 3 * 12, len(d)).reshape(3, 12, len(d)).astype(np.float32)).to(DEV)
        lens = torch.tensor([12, 5, 0], dtype=torch.int32, device=DEV)
        dec = _decoder(d, 6, 4, nbest=2, lm=_token_lm(tmp_path, d, _lm_text(16, 3, True, 0)), lm_weight=0.5)
        run = lambda: dec.search(x, lens)  # noqa: E731
    else:
        from tests.test_transducer_frame_beam import _decoder as rnnt_decoder
        from tests.test_transducer_frame_beam import _tiny_transducer

        model, d, sample = _tiny_transducer()
        lm = _token_lm(tmp_path, d, random_lm_text(d, 3, True, seed=9, per_order=150, absent=0.1))
        dec = rnnt_decoder(model, d, 4, nbest=2, lm_model=lm, lm_weight=0.3)
        E, enc_len = dec.encode(sample)
        run = lambda: dec.search(E, enc_len)  # noqa: E731
    ref = [t.clone() for t in run()]  # warm-up: the upload of the tables and the map
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(out, ref):
        assert torch.equal(a, b)
    assert int(ref[1][:, 0].sum()) > 0


@pytest.mark.gpu
def test_cli_round_trip(tmp_path, capsys):
    """speech_recognize --search ctc_beam --token-ngram-lm prints, for every utterance, what the decoder returns directly."""
    _need_gpu()
    from espresso_amd import registry
    from espresso_amd import speech_recognize as sr
    from espresso_amd.data.audio_utils import read_wav
    from espresso_amd.models.token_ngram_lm import TokenNGramLM
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder
    from tests.test_ctc_prefix_beam import _write_wav

    dict_path = str(tmp_path / "dict.txt")
    with open(dict_path, "w") as f:
        f.write("".join(f"t{i} 1\n" for i in range(30)))
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(dict=dict_path, autoregressive=False,
                                                                                    criterion_name="ctc_loss"))
    d = task.target_dictionary
    block = {"_name": "speech_transformer_encoder_model", "encoder": {"conv_channels": "[64, 64, 16, 16]", "embed_dim": 64,
             "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4, "normalize_before": True, "relative_positional_embeddings": True,
             "layer_type": "conformer"}, "dropout": 0.0, "attention_dropout": 0.0, "activation_dropout": 0.0, "layernorm_embedding": True}
    cls = registry.MODEL_REGISTRY["speech_transformer_encoder_model"]
    torch.manual_seed(0)
    model = cls.build_model(cls.config_class.from_dict(block), task)
    torch.save({"model": model.state_dict(), "cfg": {"model": block}}, str(tmp_path / "model.pt"))
    model = model.to(DEV).eval()
    arpa = write_arpa(tmp_path, "tok.arpa", random_lm_text(d, 3, True, seed=2, per_order=100))
    rng = np.random.default_rng(0)
    utts = [f"utt{i}" for i in range(3)]
    with open(tmp_path / "wav.scp", "w") as f:
        for i, u in enumerate(utts):
            p = str(tmp_path / f"{u}.wav")
            _write_wav(p, rng.standard_normal(int(16000 * (0.6 + 0.3 * i))) * 3000)
            f.write(f"{u} {p}\n")
    capsys.readouterr()
    sr.main(["--path", str(tmp_path / "model.pt"), "--dict", dict_path, "--wav-scp", str(tmp_path / "wav.scp"), "--search", "ctc_beam",
             "--beam", "5", "--nbest", "2", "--max-tokens", "500", "--batch-size", "3", "--token-ngram-lm", arpa, "--lm-weight", "0.5"])
    lines = [l.split("\t") for l in capsys.readouterr().out.splitlines() if l.startswith("H-")]
    waves = [read_wav(str(tmp_path / f"{u}.wav")) for u in utts]
    task.build_frontend(torch.device(DEV))
    gen = CTCPrefixBeamSearchDecoder([model], d, beam_size=5, nbest=2, lm_model=TokenNGramLM(arpa, d), lm_weight=0.5)
    expect = []
    for bt in sr.make_batches(utts, [len(w) for w in waves], 500, 3):
        sample = sr.collate(bt, utts, waves, torch.device(DEV))
        hyps = gen.generate([model], task.prepare_sample(sample, train=False))
        for i, u in enumerate(sample["utt_ids"]):
            for h in hyps[i][:2]:
                expect.append((f"H-{u}", d.string(h["tokens"]), float(h["score"]) / math.log(2)))
    assert len(lines) == len(expect) and len(lines) >= len(utts)
    for (hu, text, score), (eu, etext, escore) in zip(lines, expect):
        assert (hu, text) == (eu, etext)
        assert abs(float(score) - escore) < 1e-4, (hu, score, escore)
