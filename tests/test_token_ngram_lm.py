"""The sub-word n-gram LM of the token-level beam searches (models/token_ngram_lm.py, csrc/ngram_rows.hip): the host rows
against the float64 ArpaRef and against NGramLanguageModel.score_host, the map rules of TokenNGramLM, the command line, and
on the GPU the row kernel against the host rows, bit for bit."""
import math

import numpy as np
import pytest
import torch

from tests.token_ngram_ref import (ROW_TOL, TokenRowsRef, dense_arpa, dictionary, plain_symbols, random_lm_text, random_triples,
                                   walk_triples, wide_tail_arpa, write_arpa)

DEV = "cuda:0"


def _lm(tmp_path, d, text, name="lm.arpa", **kw):
    from espresso_amd.models.token_ngram_lm import TokenNGramLM

    return TokenNGramLM(write_arpa(tmp_path, name, text), d, **kw)


def _walk(lm, ref, rng, N, steps):
    """The host rows over `steps` random triples from the start state, each step held to the reference; yields
    (ctx int32 [N][W], rows fp32 [N][V], the rows' word histories)."""
    d = lm.dictionary
    W = lm.order - 1
    ctx, rows = lm.start_host(N)
    hist = [["<s>"] for _ in range(N)]
    yield ctx, rows, hist
    for parent, token, keep in walk_triples(lm, rng, N, steps):
        ctx, rows = lm.rows_host(ctx, parent, token, keep)
        hist = [hist[p] if k else hist[p] + [ref.word(int(t))] for p, t, k in zip(parent, token, keep)]
        yield ctx, rows, hist
    assert ctx.shape == (N, W)


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("unk", [True, False])
@pytest.mark.parametrize("order", [1, 2, 3, 6])
def test_host_rows_vs_arpa_ref(tmp_path, order, unk):
    d = dictionary(24)
    text = random_lm_text(d, order, unk, seed=order)
    lm, ref = _lm(tmp_path, d, text), TokenRowsRef(text, d)
    assert 1 < (lm.tok2word == -1).sum() <= len(plain_symbols(d)) // 2  # some symbols are absent from the file
    rng = np.random.default_rng(10 + order)
    worst, n_backoff, n_inf = 0.0, 0, 0
    for ctx, rows, hist in _walk(lm, ref, rng, N=9, steps=12):
        for i, h in enumerate(hist):
            want = ref.row(h)
            inf = np.isinf(want)
            assert np.array_equal(np.isneginf(rows[i]), inf), (h, rows[i], want)
            worst = max(worst, float(np.abs(rows[i][~inf] - want[~inf]).max()))
            n_inf += int(inf.sum())
            tail = tuple(h[len(h) - (order - 1):]) if order > 1 else ()
            n_backoff += len(tail) >= 2 and tail not in ref.ref.prob and tail[1:] in ref.ref.prob
    print(f"order {order} unk {unk}: max |host - ArpaRef| {worst:.2e}, {n_backoff} contexts whose longest suffix is absent")
    assert worst < ROW_TOL, worst
    assert n_inf >= 2 * 9  # pad and blank at least
    if order >= 3:
        assert n_backoff > 0


@pytest.mark.parametrize("order,unk", [(1, True), (2, False), (3, True), (6, False), (6, True)])
def test_host_rows_equal_score_host(tmp_path, order, unk):
    """Bit for bit what the single-query entry point returns, for every column with an ARPA id and for the <unk> columns."""
    d = dictionary(24)
    text = random_lm_text(d, order, unk, seed=20 + order)
    lm, ref = _lm(tmp_path, d, text), TokenRowsRef(text, d)
    cols = np.flatnonzero(lm.tok2word >= -1)
    assert (lm.tok2word[cols] == -1).any() and len(cols) == len(d) - 2
    n = 0
    for ctx, rows, _ in _walk(lm, ref, np.random.default_rng(order), N=7, steps=8):
        for i in range(ctx.shape[0]):
            single = lm.ngram.score_host(np.repeat(ctx[i:i + 1], len(cols), 0), lm.tok2word[cols])
            assert np.array_equal(single.view(np.int32), rows[i, cols].view(np.int32)), (i, ctx[i])
            n += len(cols)
        assert np.isneginf(rows[:, [d.pad(), d.bos()]]).all()
    assert n > 1000


def test_host_rows_on_the_dense_file(tmp_path):
    """A unigram context with every word as a child, and contexts where a trigram and a bigram land on one column."""
    d = dictionary(12)
    text = dense_arpa(plain_symbols(d)[:10])
    lm, ref = _lm(tmp_path, d, text), TokenRowsRef(text, d)
    a, b, c = (d.index(f"t{i}") for i in range(3))
    ctx, rows = lm.start_host(1)
    keep0 = np.zeros(1, dtype=np.uint8)
    hist = ["<s>"]
    for t in (a, a, b, a, c, a):
        ctx, rows = lm.rows_host(ctx, np.zeros(1, dtype=np.int32), np.array([t], dtype=np.int32), keep0)
        hist.append(d.symbols[t])
        want = ref.row(hist)
        inf = np.isinf(want)
        assert np.array_equal(np.isneginf(rows[0]), inf)
        assert np.abs(rows[0][~inf] - want[~inf]).max() < ROW_TOL, hist


def test_token_map_rules(tmp_path):
    from espresso_amd.data.asr_dictionary import AsrDictionary

    d = dictionary(8)
    syms = plain_symbols(d)
    rng = np.random.default_rng(0)
    from tests.ngram_ref import random_arpa

    text = random_arpa(rng, syms[:6], 2, 20, unk=True)
    lm = _lm(tmp_path, d, text)
    w = lm.ngram.word2id
    assert lm.tok2word[d.eos()] == w["</s>"] and lm.tok2word[d.unk()] == w["<unk>"]
    assert lm.tok2word[d.pad()] == -2 and lm.tok2word[d.bos()] == -2 and lm.blank == d.bos()
    for s in syms:
        assert lm.tok2word[d.index(s)] == w.get(s, -1)
    assert sorted(d.symbols[i] for i in np.flatnonzero(lm.tok2word == -1)) == sorted(syms[6:])
    # without <unk> the dictionary's <unk> has no entry; a blank given by hand
    lm2 = _lm(tmp_path, d, random_arpa(rng, syms, 3, 20, unk=False), name="nounk.arpa", blank=d.index("t3"))
    assert lm2.tok2word[d.unk()] == -1 and lm2.tok2word[d.index("t3")] == -2 and lm2.tok2word[d.bos()] == -1
    # a dictionary without a blank of its own: bos() is eos(), which stays </s>
    d3 = AsrDictionary.from_symbols(syms[:-1], enable_bos=False)
    lm3 = _lm(tmp_path, d3, text, name="again.arpa")
    assert lm3.blank is None and lm3.tok2word[d3.eos()] == w["</s>"] and (lm3.tok2word == -2).sum() == 1
    # more than half of the symbols unknown to the file: the wrong file, named symbols
    with pytest.raises(ValueError, match="'t3'.*unigram|unigram.*'t3'"):
        _lm(tmp_path, d, random_arpa(rng, syms[:3], 2, 5, unk=True), name="few.arpa")
    exactly_half = _lm(tmp_path, d, random_arpa(rng, syms[: (len(syms) + 1) // 2], 2, 5, unk=True), name="half.arpa")
    assert (exactly_half.tok2word == -1).sum() == len(syms) // 2
    # no <s> (or no </s>): refused as a ValueError
    bad = "\\data\\\nngram 1=2\n\n\\1-grams:\n-1.0\t</s>\n-1.0\tt0\n\n\\end\\\n"
    with pytest.raises(ValueError, match="<s>"):
        _lm(tmp_path, d, bad, name="nobos.arpa")


def test_decoders_accept_the_ngram_lm_and_refuse_a_zero_weight(tmp_path):
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder
    from espresso_amd.tools.streaming_ctc_prefix_beam_decoder import StreamingCTCPrefixBeamDecoder
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder

    d = dictionary(8)
    lm = _lm(tmp_path, d, random_lm_text(d, 3, True, seed=1, absent=0.0))
    assert CTCPrefixBeamSearchDecoder([None], d, lm_model=lm, lm_weight=0.5).lm_model is lm
    dec = TransducerFrameBeamDecoder(None, d, lm_model=lm, lm_weight=0.5)
    assert dec.lm_model is lm and dec.no_blank_in_lm is False
    assert StreamingCTCPrefixBeamDecoder(d, 2, 8, lm_model=lm, lm_weight=0.5).lm_model is lm
    assert StreamingTransducerFrameBeamDecoder(None, d, 4, 2, 8, lm_model=lm, lm_weight=0.5)._step["lm_no_blank"] is False
    for make in (lambda **kw: CTCPrefixBeamSearchDecoder([None], d, **kw), lambda **kw: TransducerFrameBeamDecoder(None, d, **kw),
                 lambda **kw: StreamingCTCPrefixBeamDecoder(d, 2, 8, **kw),
                 lambda **kw: StreamingTransducerFrameBeamDecoder(None, d, 4, 2, 8, **kw)):
        for w in (0.0, -0.5):
            with pytest.raises(ValueError, match="lm_weight"):
                make(lm_model=lm, lm_weight=w)
    with pytest.raises(ValueError, match="dictionary"):
        CTCPrefixBeamSearchDecoder([None], dictionary(9), lm_model=lm, lm_weight=0.5)
    for make in (lambda **kw: CTCPrefixBeamSearchDecoder([None], d, **kw), lambda **kw: TransducerFrameBeamDecoder(None, d, **kw)):
        with pytest.raises(ValueError, match="blank"):  # the LM holds another column at -inf than the search's blank
            make(lm_model=lm, lm_weight=0.5, blank=d.index("t1"))


def test_staging_capacity_constant_matches_the_kernel():
    """kernels.NGRAM_ROW_LDS, which the wide-row tests size themselves by, is the kernel's kNgRowLds."""
    import os
    import re

    from espresso_amd import kernels as K

    src = open(os.path.join(os.path.dirname(K.__file__), "csrc", "ngram_rows.hip")).read()
    assert int(re.search(r"constexpr int kNgRowLds = (\d+);", src).group(1)) == K.NGRAM_ROW_LDS


def _main(*extra):
    from espresso_amd import speech_recognize as sr

    return sr.main(["--path", "missing.pt", "--dict", "missing.txt", "--wav-scp", "missing.scp", *extra])


def test_cli_option_parses():
    from espresso_amd import speech_recognize as sr

    a = sr.get_parser().parse_args(["--path", "m.pt", "--dict", "d.txt", "--wav-scp", "w.scp", "--search", "ctc_beam",
                                    "--token-ngram-lm", "lm.arpa", "--lm-weight", "0.7"])
    assert (a.token_ngram_lm, a.lm_weight, a.ngram_lm) == ("lm.arpa", 0.7, None)
    assert sr.get_parser().parse_args(["--path", "m.pt", "--dict", "d.txt", "--wav-scp", "w.scp"]).token_ngram_lm is None
    for search in sr.TOKEN_NGRAM_SEARCHES:
        a.search, a.streaming = search, search.endswith("stream_beam")
        sr.check_token_ngram_args(a)  # accepted


@pytest.mark.parametrize("search", ["beam", "ctc", "transducer_greedy", "transducer_beam"])
def test_cli_other_searches_refuse_the_option(search):
    with pytest.raises(NotImplementedError, match="--token-ngram-lm"):
        _main("--search", search, "--token-ngram-lm", "lm.arpa", "--lm-weight", "0.5")


@pytest.mark.parametrize("extra,exc", [(["--search", "ctc_beam", "--ngram-lm", "w.arpa"], NotImplementedError),
                                       (["--search", "ctc_beam", "--lm-path", "lm.pt"], NotImplementedError),
                                       (["--search", "transducer_frame_beam", "--lm-path", "lm.pt"], NotImplementedError),
                                       (["--search", "transducer_frame_beam", "--word-dict", "w.txt"], NotImplementedError),
                                       (["--search", "ctc_stream_beam", "--streaming", "--lm-path", "lm.pt"], NotImplementedError),
                                       (["--search", "ctc_beam"], ValueError),  # --lm-weight defaults to 0
                                       (["--search", "transducer_stream_beam", "--streaming", "--lm-weight", "-1"], ValueError)])
def test_cli_refusals_name_the_option(extra, exc):
    with pytest.raises(exc, match="--token-ngram-lm"):
        _main("--token-ngram-lm", "lm.arpa", *([] if exc is ValueError else ["--lm-weight", "0.5"]), *extra)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


def _kernel_vs_host(lm, rng, N, steps, ld, triples=None, observe=None):
    """Twenty steps of random triples (or the given ones): rows and contexts of the kernel equal the host's bits.
    observe(ctx_h) sees the host contexts of every step."""
    from espresso_amd import kernels as K

    d, W, V = lm.dictionary, lm.order - 1, len(lm.dictionary)
    lm.to(DEV)
    ctx_h, rows_h = lm.start_host(N)
    ctx_d, rows_d = K.ngram_token_rows_start(lm.ngram.handle, lm._map, N, W, ld=ld)
    assert rows_d.stride(0) == ld and rows_d.shape == (N, V)
    bufs = [torch.empty_like(ctx_d), ctx_d]
    n_inf = n_dup = 0
    for step, triple in enumerate([None] + (walk_triples(lm, rng, N, steps) if triples is None else triples)):  # 0: the start rows
        if step:
            parent, token, keep = triple
            ctx_h, rows_h = lm.rows_host(ctx_h, parent, token, keep)
            out = bufs[step % 2 == 0]
            full = torch.full((N, ld), float("nan"), dtype=torch.float32, device=DEV)
            rows_d = K.ngram_token_rows_step(lm.ngram.handle, lm._map, ctx_d, *(torch.from_numpy(a).to(DEV) for a in (parent, token, keep)),
                                             out, rows=full)
            ctx_d = out
            assert torch.isnan(full[:, V:]).all()  # nothing written past V
            n_dup += N - len(set(parent.tolist()))
        assert torch.equal(ctx_d[:, :W].cpu(), torch.from_numpy(ctx_h)), step
        if observe is not None:
            observe(ctx_h)
        got = rows_d.cpu().contiguous()
        assert torch.equal(got.view(torch.int32), torch.from_numpy(rows_h).contiguous().view(torch.int32)), step
        n_inf += int(torch.isinf(got).sum())
    assert n_inf > 0 and n_dup > 0  # -inf columns, and parents that duplicate and drop rows
    return rows_h


@pytest.mark.gpu
@pytest.mark.parametrize("unk", [True, False])
@pytest.mark.parametrize("order", [1, 2, 3, 6])
def test_kernel_equals_host_small(tmp_path, order, unk):
    _need_gpu()
    d = dictionary(6)
    assert len(d) == 11
    lm = _lm(tmp_path, d, random_lm_text(d, order, unk, seed=30 + order, per_order=25))
    _kernel_vs_host(lm, np.random.default_rng(order), N=7, steps=20, ld=13 if unk else 16)  # 4-byte and 16-byte stores


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 2, 3, 6])
def test_kernel_equals_host_past_the_lds_stage(tmp_path, order):
    _need_gpu()
    from espresso_amd import kernels as K

    V = K.NGRAM_ROW_LDS + 7
    d = dictionary(V - 5)
    assert len(d) == V
    from tests.ngram_ref import random_arpa

    words = [s for i, s in enumerate(plain_symbols(d)) if i % 4 != 3]  # every fourth symbol is absent, also past the stage
    lm = _lm(tmp_path, d, random_arpa(np.random.default_rng(40 + order), words, order, 4000, unk=order != 3))
    assert (lm.tok2word[K.NGRAM_ROW_LDS:] >= 0).any() and (lm.tok2word[K.NGRAM_ROW_LDS:] == -1).any()
    _kernel_vs_host(lm, np.random.default_rng(order), N=7, steps=20, ld=V + 5)


@pytest.mark.gpu
def test_scatter_past_the_lds_stage(tmp_path):
    """The per-order scatters into columns the LDS stage does not hold: a file whose bigram and trigram children sit in the
    dictionary's last columns, rows steered through the contexts that have them, then random triples.  The test counts the
    (row, step) pairs whose bigram context, whose trigram context, and whose both have a child at or beyond the stage."""
    _need_gpu()
    from espresso_amd import kernels as K

    V = K.NGRAM_ROW_LDS + 7
    d = dictionary(V - 5)
    syms = plain_symbols(d)
    tail = syms[-6:-1]  # five of the last six symbols; the very last one stays out of the file (a -1 column past the stage)
    lm = _lm(tmp_path, d, wide_tail_arpa(syms[:-1], tail))
    assert min(d.index(s) for s in tail) >= K.NGRAM_ROW_LDS and lm.tok2word[V - 1] == -1
    far = {w for v, w in enumerate(lm.tok2word.tolist()) if v >= K.NGRAM_ROW_LDS and w >= 0}
    with_far_child = [{tuple(g[:-1]) for g in lm.ngram.records(k)[0].tolist() if g[-1] in far} for k in (2, 3)]
    hits = {"bigram": 0, "trigram": 0, "both": 0}

    def observe(ctx_h):
        for c in ctx_h.tolist():
            bi, tri = tuple(c[1:]) in with_far_child[0], tuple(c) in with_far_child[1]
            hits["bigram"] += bi
            hits["trigram"] += tri
            hits["both"] += bi and tri

    a, b = d.index(syms[0]), d.index(syms[1])
    N = 5
    ident, zeros = np.arange(N, dtype=np.int32), np.zeros(N, dtype=np.uint8)
    steered = [(ident, np.array(t, dtype=np.int32), zeros) for t in ([a, b, a, d.eos(), d.index(tail[0])], [a, a, b, a, a],
                                                                    [a, a, a, a, b], [b, a, a, a, a], [a, b, a, b, a])]
    triples = steered + list(random_triples(np.random.default_rng(0), N, V, 15, d.bos(), d.pad()))
    _kernel_vs_host(lm, None, N, len(triples), ld=V + 1, triples=triples, observe=observe)
    print(hits)
    assert hits["bigram"] >= 5 and hits["trigram"] >= 3 and hits["both"] >= 3, hits


@pytest.mark.gpu
def test_kernel_equals_host_on_the_dense_file(tmp_path):
    """Every word a child of one context (a full-width scatter), and a bigram and a trigram on one column: the trigram's value
    is the one that stays.  The walk is steered through those contexts."""
    _need_gpu()
    from espresso_amd import kernels as K

    d = dictionary(12)
    lm = _lm(tmp_path, d, dense_arpa(plain_symbols(d)[:10])).to(DEV)
    a, b = d.index("t0"), d.index("t1")
    N, W = 5, 2
    seqs = np.array([[a, a, a, b, a], [b, a, a, a, a], [a, b, b, a, a], [d.eos(), a, a, a, b]], dtype=np.int32)
    ctx_h, rows_h = lm.start_host(N)
    ctx_d, rows_d = K.ngram_token_rows_start(lm.ngram.handle, lm._map, N, W)
    bufs = [torch.empty_like(ctx_d), ctx_d]
    ident = np.arange(N, dtype=np.int32)
    for step, token in enumerate(seqs, 1):
        keep = np.zeros(N, dtype=np.uint8)
        ctx_h, rows_h = lm.rows_host(ctx_h, ident, token, keep)
        out = bufs[step % 2 == 0]
        rows_d = K.ngram_token_rows_step(lm.ngram.handle, lm._map, ctx_d, *(torch.from_numpy(x).to(DEV) for x in (ident, token, keep)), out)
        ctx_d = out
        assert torch.equal(ctx_d.cpu(), torch.from_numpy(ctx_h))
        assert torch.equal(rows_d.cpu().view(torch.int32), torch.from_numpy(rows_h).view(torch.int32)), step
    # the context (t0, t0): the trigram (t0, t0, t2) beats the bigram (t0, t2) in the column of t2
    ng3, lp3, _ = lm.ngram.records(3)
    w = lm.ngram.word2id
    hit = [i for i, g in enumerate(ng3) if tuple(g) == (w["t0"], w["t0"], w["t2"])]
    ctx, rows = lm.rows_host(np.array([[w["t0"], w["t0"]]], dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32),
                             np.ones(1, dtype=np.uint8))
    assert len(hit) == 1 and rows[0, d.index("t2")] == lp3[hit[0]]


@pytest.mark.gpu
def test_update_alternates_two_context_buffers(tmp_path):
    _need_gpu()
    d = dictionary(8)
    lm = _lm(tmp_path, d, random_lm_text(d, 3, True, seed=3, absent=0.0)).to(DEV)
    N = 6
    ctx, rows = lm.start(N, torch.device(DEV))
    parent = torch.arange(N, dtype=torch.int32, device=DEV)
    token = torch.full((N,), d.index("t1"), dtype=torch.int32, device=DEV)
    keep = torch.zeros(N, dtype=torch.uint8, device=DEV)
    seen = []
    for _ in range(4):
        new, rows = lm.update(ctx, parent, token, keep)
        assert new.data_ptr() != ctx.data_ptr()
        seen.append(new.data_ptr())
        ctx = new
    assert seen[0] == seen[2] and seen[1] == seen[3] and seen[0] != seen[1]
    assert math.isfinite(float(rows[0, d.eos()])) and torch.isneginf(rows[:, d.pad()]).all()
