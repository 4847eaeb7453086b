"""Hotword (contextual phrase) biasing of the CTC prefix beam search (tools/context_graph.py, the BIAS kernels of
csrc/ctc_beam.hip, speech_recognize --hotwords).

Truth is float64: `ContextGraph.score` (a dict-of-nodes replay), tests.hotword_ref.locked_bonus (B(y) without an automaton) and
tests.test_ctc_prefix_beam.prefix_beam_oracle with the bias passed through its `lm_fn` hook.  The CPU tests hold those to known
answers and to brute force over every alignment; the GPU tests hold the HIP search to them."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

from tests.hotword_ref import BOOSTS, GRID, GRID_LENS, bias_lm_fn, biased_oracle, grid_inputs, grid_phrases, locked_bonus
from tests.test_ctc_prefix_beam import (DEV, LM_TOL, SCORE_TOL, _decoder, _dictionary, _hyps, _lm_setup, _need_gpu, _peaked, _write_wav,
                                        prefix_beam_oracle)

KNOWN = [([1, 2, 3], [1, 2, 3], 3), ([1, 2, 4], [1, 2, 0], 0), ([5, 2], [0, 1], 1), ([1, 1, 2, 3], [1, 1, 2, 3], 3), ([1, 2], [1, 2], 0)]


def _graph(phrases, V):
    from espresso_amd.tools.context_graph import ContextGraph

    return ContextGraph(phrases, V)


def _random_phrases(rng, V, n, dyadic):
    """Shared prefixes, prefixes and suffixes of other phrases, single tokens, per-phrase boosts; tokens from a small alphabet so
    that they collide."""
    def boost():
        return float(rng.integers(8, 128)) / 64.0 if dyadic else float(rng.uniform(0.1, 0.39))

    A = min(V, 6)
    out = [([int(t) for t in rng.integers(1, A, int(rng.integers(1, 4)))], boost()) for _ in range(n)]
    long = [p for p, _ in out if len(p) >= 2]
    for p in long[:3]:
        out.append((p[:-1], boost()))  # a prefix of another phrase
        out.append((p[1:], boost()))   # a suffix of another phrase
        out.append((p[:1] + [int(rng.integers(1, A))], boost()))  # a shared first edge
    out.append(([int(rng.integers(1, A))], boost()))
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_known_answers():
    g = _graph([([1, 2, 3], 1.0), ([2], 1.0)], 8)
    running, final, q = g.score_host([y for y, _, _ in KNOWN])
    for i, (y, run, fin) in enumerate(KNOWN):
        r, f = g.score(y)
        assert r == run and f == fin, (y, r, f)
        assert running[i, : len(y)].tolist() == run and final[i] == fin, (y, running[i], final[i])
        assert q[i] == g.state(y)
        assert locked_bonus(g.phrases, y) == fin
    # a phrase of n tokens and boost s is worth n * s; e is a max over the phrases that share an edge
    g = _graph([([4, 5, 6], 0.5), ([4, 5], 2.0)], 8)
    assert g.score([4, 5, 6])[1] == 2.0 + 2.0 + 0.5 and g.score([4, 5])[1] == 4.0 and g.score([7, 4, 5, 7])[1] == 4.0
    assert g.score([4, 5, 6])[0] == [2.0, 4.0, 4.5]  # nothing pending at an end node, so [4, 5] stays locked
    # the documented limit: [2] inside the pending [1, 2, 3] is reached by a failure link only and is not credited
    g = _graph([([1, 2, 3], 1.0), ([2], 1.0)], 8)
    assert g.score([1, 2, 5])[1] == 0.0 and g.score([2, 5])[1] == 1.0


def test_empty_graph_and_limits():
    g = _graph([], 8)
    assert g.num_nodes == 1 and g.edges.shape == (0, 4) and g.score([1, 2, 3]) == ([0.0] * 3, 0.0)
    running, final, q = g.score_host([[1, 2, 3], []])
    assert not running.any() and not final.any() and not q.any()
    for bad in ([([], 1.0)], [([1], 0.0)], [([1], -1.0)], [([8], 1.0)], [([1] * 65, 1.0)]):
        with pytest.raises(ValueError):
            _graph(bad, 8)
    assert _graph([([1, 2], 0.5), ([1, 2], 2.0), ([1, 2], 1.0)], 8).phrases == [((1, 2), 2.0)]  # duplicates: the larger boost


@pytest.mark.parametrize("dyadic", [True, False])
@pytest.mark.parametrize("seed", range(6))
def test_packed_tables_vs_dict_replay(seed, dyadic):
    """fp32 packed walk (ea_context_graph_score_host) against the float64 dict replay to 1e-6, nodes exactly.  Dyadic boosts
    (k / 64, at most 2) make every fp32 sum exact whatever the row length.  The others are drawn from [0.1, 0.39) with phrases
    of at most 3 tokens and rows of 5 tokens: every intermediate value stays below 2, so one fp32 rounding is at most 2^-24 = 6e-8,
    a token costs at most three of them (phi + e, - phi, b +), and five tokens stay under 9e-7."""
    rng = np.random.default_rng(seed)
    V = 9
    g = _graph(_random_phrases(rng, V, 12, dyadic), V)
    L = 24 if dyadic else 5
    rows = [[int(t) for t in rng.integers(0, 7, int(rng.integers(0, L + 1)))] for _ in range(200)]
    rows += [list(p) * 2 for p, _ in g.phrases][: 40 if dyadic else 0]
    running, final, q = g.score_host(rows)
    worst = 0.0
    for i, y in enumerate(rows):
        r, f = g.score(y)
        assert abs(f - locked_bonus(g.phrases, y)) < 1e-12, y  # the telescoping claim, against the automaton-free statement
        assert f >= -1e-12
        assert q[i] == g.state(y), y
        worst = max([worst, abs(final[i] - f)] + [abs(running[i, u] - r[u]) for u in range(len(y))])
    print(f"seed {seed} dyadic {dyadic}: {g.num_nodes} nodes, max |fp32 packed - float64 dict| {worst:.2e}")
    assert worst < 1e-6


def test_csr_tables():
    g = _graph([([3, 1], 1.0), ([3, 2, 1], 0.5), ([2, 1], 0.25), ([2], 2.0)], 6)
    for n in range(g.num_nodes):
        toks = g.tok[g.off[n] : g.off[n + 1]].tolist()
        assert toks == sorted(toks) and len(set(toks)) == len(toks)
        assert g.fail[n] < max(n, 1)
    assert g.off[-1] == g.num_nodes - 1 and g.phi[0] == 0 and g.fail[0] == 0
    n32 = g.state([3, 2])
    assert g.fail[n32] == g.state([2]) and g.phi[n32] == 1.5 and g.edge_boost[n32] == 0.5 and g.edge_boost[g.state([3])] == 1.0
    assert g.phi[g.state([2])] == 0.0 and g.phi[g.state([3, 2, 1])] == 0.0  # end nodes hold nothing on credit
    assert g.root[3].tolist() == [g.state([3]), np.float32(1.0).view(np.int32)] and g.root[1, 0] == -1


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("T", [1, 3, 5])
def test_biased_oracle_is_exact_without_pruning(seed, T):
    """beam and K exhaustive: the biased search returns every label sequence with score = its exact CTC log-probability (every
    alignment summed) + B(y), so the bias telescopes to B(y) whatever path the beam took."""
    from oracle.torch_ref import ctc_nll_numpy

    rng = np.random.default_rng(seed)
    V, blank = 4, 0
    x = rng.standard_normal((T, V)) * 1.5
    x -= np.logaddexp.reduce(x, axis=1, keepdims=True)
    g = _graph([([1, 2], BOOSTS[0]), ([1, 2, 3], BOOSTS[1]), ([2], 0.41), ([3, 3, 1], 0.9), ([2, 3], 0.55)], V)
    hyps, _ = biased_oracle(x, T, 10 ** 6, V - 1, blank, g, nbest=10 ** 6)
    hyps = [(y, s) for y, s in hyps if s > -math.inf]
    brute = {}
    for n in range(T + 1):
        for y in itertools.product(range(1, V), repeat=n):
            nll = ctc_nll_numpy(x, list(y), blank=blank)
            if np.isfinite(nll):
                brute[y] = -nll + locked_bonus(g.phrases, y)
    assert {y for y, _ in hyps} == set(brute)
    for y, s in hyps:
        assert abs(s - brute[y]) < 1e-9, (y, s, brute[y])
    assert hyps[0][0] == max(brute, key=brute.get)
    assert any(locked_bonus(g.phrases, y) > 0 for y in brute) or T == 1


def test_phrase_file(tmp_path):
    from espresso_amd.tools.context_graph import load_context_graph, read_hotwords

    d = _dictionary(8)
    p = tmp_path / "hot.txt"
    p.write_text("# names\nt1 t2\t2.5\n\nt3\n  # indented comment\nt1 t2\t0.5\nt1 t2 t4\n", encoding="utf-8")
    t = [d.index(f"t{i}") for i in range(8)]
    assert read_hotwords(str(p), d, d.bos(), 1.25) == [([t[1], t[2]], 2.5), ([t[3]], 1.25), ([t[1], t[2]], 0.5), ([t[1], t[2], t[4]], 1.25)]
    g = load_context_graph(str(p), d, d.bos(), 1.25)
    assert g.phrases == sorted([((t[1], t[2]), 2.5), ((t[3],), 1.25), ((t[1], t[2], t[4]), 1.25)]) and g.vocab_size == len(d)
    p.write_text("t1 t2\nt1 zebra t2\n", encoding="utf-8")
    with pytest.raises(ValueError, match=r"hot\.txt:2: .*<unk>"):
        read_hotwords(str(p), d, d.bos(), 1.0)
    p.write_text("t1\tlots\n", encoding="utf-8")
    with pytest.raises(ValueError, match=r"hot\.txt:1: "):
        read_hotwords(str(p), d, d.bos(), 1.0)
    p.write_text("t1\t-1\n", encoding="utf-8")
    with pytest.raises(ValueError, match=r"hot\.txt:1: "):
        read_hotwords(str(p), d, d.bos(), 1.0)


_BASE = ["--path", "missing.pt", "--dict", "missing.txt", "--wav-scp", "missing.scp", "--hotwords", "missing_hot.txt"]


@pytest.mark.parametrize("extra", [[], ["--search", "beam"], ["--search", "ctc"], ["--search", "transducer_greedy"],
                                   ["--search", "transducer_beam"], ["--search", "ctc_beam", "--ngram-lm", "lm.arpa"],
                                   ["--search", "ctc_beam", "--streaming"], ["--search", "ctc", "--streaming"],
                                   ["--search", "ctc_beam", "--ngram-lm", "lm.arpa", "--streaming"]])
def test_cli_refuses_hotwords_elsewhere(extra):
    """Every combination but --search ctc_beam without --ngram-lm / --streaming is refused by name before any file is opened."""
    from espresso_amd import speech_recognize as sr

    with pytest.raises(NotImplementedError, match="--hotwords"):
        sr.main(_BASE + extra)


def test_cli_hotword_options():
    from espresso_amd import speech_recognize as sr
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder

    parse = sr.get_parser().parse_args
    a = parse(_BASE + ["--search", "ctc_beam", "--lm-path", "lm.pt"])
    assert (a.hotwords, a.hotword_score) == ("missing_hot.txt", None)
    sr.check_hotword_args(a)  # accepted, with an LSTM LM too
    assert "acoustic" in sr.get_parser().format_help()
    with pytest.raises(ValueError, match="--hotword-score"):
        sr.main(_BASE[:6] + ["--search", "ctc_beam", "--hotword-score", "2"])
    with pytest.raises(ValueError, match="positive"):
        sr.main(_BASE + ["--search", "ctc_beam", "--hotword-score", "0"])
    sr.check_hotword_args(parse(_BASE + ["--search", "ctc_beam", "--hotword-score", "2"]))
    d = _dictionary(8)
    g = _graph([([5, 6], 1.0)], len(d))
    gen = sr.build_generator(parse(_BASE + ["--search", "ctc_beam"]), None, d, context_graph=g)
    assert isinstance(gen, CTCPrefixBeamSearchDecoder) and gen.context_graph is g
    assert sr.build_generator(parse(_BASE[:6] + ["--search", "ctc_beam"]), None, d).context_graph is None
    with pytest.raises(ValueError, match="context graph"):
        CTCPrefixBeamSearchDecoder([None], d, context_graph=_graph([], len(d) + 1))


def _grid_cases():
    """(beam, K, seed, dtype, x as the kernel reads it, phrases) for the grid of test_search_vs_oracle_no_lm, both dtypes."""
    V = len(_dictionary(20))
    for beam, K, seed in GRID:
        x = grid_inputs(seed, V)
        phrases = grid_phrases(x, GRID_LENS, 0)
        for dtype in (torch.float32, torch.bfloat16):
            yield beam, K, seed, dtype, torch.from_numpy(x).to(dtype).float().numpy(), phrases


def test_grid_margins_of_the_float64_oracle():
    """The condition of test_biased_search_vs_oracle_no_lm, checked on the oracle alone: at most 1 in 10 of the (utterance,
    configuration) cases has a pruning / ranking margin within SCORE_TOL; and the boosts do flip rankings."""
    V = len(_dictionary(20))
    n = tight = flipped = credited = 0
    for beam, K, seed, dtype, x, phrases in _grid_cases():
        g = _graph(phrases, V)
        for b in range(x.shape[0]):
            nb = min(beam, 3)
            ref, margin = biased_oracle(x[b].astype(np.float64), int(GRID_LENS[b]), beam, K, 0, g, nbest=nb)
            plain, _ = prefix_beam_oracle(x[b].astype(np.float64), int(GRID_LENS[b]), beam, K, 0, nbest=nb)
            n += 1
            tight += margin <= SCORE_TOL
            flipped += ref[0][0] != plain[0][0]
            credited += locked_bonus(g.phrases, ref[0][0]) > 0
    print(f"{n} cases: {tight} within the margin rule, 1-best changed by the bias in {flipped}, carries a phrase in {credited}")
    assert n == 60 and tight * 10 <= n
    assert flipped >= 6 and credited >= 12


# ---------------------------------------------------------------------------------------------------------------- GPU
def _biased_decoder(d, graph, beam, K=None, nbest=1, lm=None, lm_weight=0.0, bonus=0.0):
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder

    return CTCPrefixBeamSearchDecoder([None], d, beam_size=beam, nbest=nbest, beam_size_token=K, lm_model=lm, lm_weight=lm_weight,
                                      insertion_bonus=bonus, context_graph=graph)


@pytest.mark.gpu
def test_context_graph_score_kernel_vs_host():
    _need_gpu()
    from espresso_amd import kernels as Kn

    rng = np.random.default_rng(0)
    V = 9
    g = _graph(_random_phrases(rng, V, 12, True), V)
    N, L = 700, 12
    tokens = rng.integers(0, 7, (N, L)).astype(np.int32)
    lens = rng.integers(0, L + 1, N).astype(np.int32)
    rows = [tokens[i, : lens[i]].tolist() for i in range(N)]
    running, final, q = g.score_host(rows)
    d_run, d_fin, d_q = Kn.context_graph_score(g.cuda(DEV), torch.from_numpy(tokens).to(DEV), torch.from_numpy(lens).to(DEV))
    assert torch.equal(d_q.cpu(), torch.from_numpy(q)) and torch.equal(d_fin.cpu(), torch.from_numpy(final))
    for i in range(N):
        assert d_run[i, : lens[i]].cpu().tolist() == running[i, : lens[i]].tolist()


@pytest.mark.gpu
def test_biased_search_vs_oracle_no_lm():
    """The whole-utterance launch against the float64 oracle on the grid and both dtypes of test_search_vs_oracle_no_lm.
    Hypotheses must be identical wherever the oracle's own pruning / ranking margin exceeds SCORE_TOL; at most 1 in 10 of the
    (utterance, configuration) cases may be left out under that rule."""
    _need_gpu()
    d = _dictionary(20)
    V = len(d)
    n = skipped = 0
    worst = 0.0
    for beam, K, seed, dtype, x_seen, phrases in _grid_cases():
        g = _graph(phrases, V)
        xd = torch.from_numpy(grid_inputs(seed, V)).to(DEV, dtype)
        assert np.array_equal(xd.float().cpu().numpy(), x_seen)
        dec = _biased_decoder(d, g, beam, K, nbest=min(beam, 3))
        out = dec.search(xd, torch.from_numpy(GRID_LENS).to(DEV))
        cfg_worst = 0.0
        for b in range(x_seen.shape[0]):
            ref, margin = biased_oracle(x_seen[b].astype(np.float64), int(GRID_LENS[b]), beam, K, dec.blank, g, nbest=dec.nbest)
            got = _hyps(out, b)
            n += 1
            if margin <= SCORE_TOL:
                skipped += 1
                continue
            assert [y for y, _ in got] == [y for y, _ in ref], (beam, K, seed, dtype, b, got, ref)
            cfg_worst = max([cfg_worst] + [abs(s - r) for (_, s), (_, r) in zip(got, ref)])
        print(f"beam {beam} K {K} seed {seed} {dtype}: {g.num_nodes} nodes, max |score - oracle| {cfg_worst:.2e}")
        worst = max(worst, cfg_worst)
        assert _hyps(out, 1) == [((), 0.0)]  # in_len 0: the empty hypothesis
    print(f"{n} cases, {skipped} left out by the margin rule, max |score - oracle| {worst:.2e}")
    assert n == 60 and skipped * 10 <= n
    assert worst < SCORE_TOL


@pytest.mark.gpu
def test_every_biased_score_is_right_with_lm():
    """The frame-by-frame path with the LSTM LM: every returned score against an independent computation,
    -ctc_nll(y) + lambda * (LM_cpu(y) + log P(eos | y)) + beta * |y| + B(y).  Pruning only ever drops CTC paths of a prefix, so
    that value bounds a returned score from above whatever the beam; it is an equality where the beam keeps the paths of the
    hypothesis.  With nbest 1 the returned hypothesis is the 1-best, which keeps them on these peaked inputs (the float64 oracle
    itself stays within a tenth of SCORE_TOL of the independent value, test_lm_case_oracle_is_exact): equality is asserted for
    every hypothesis returned there.  With nbest 3 the 3-best of the float64 oracle already lose up to 7e-4 to pruning at beam 64,
    so the lower hypotheses are held to the upper bound and to the oracle with the same beam instead."""
    from oracle.torch_ref import ctc_nll_numpy

    _need_gpu()
    d, x, lens, lam, beta, phrases = _lm_case()
    g = _graph(phrases, len(d))
    lm, fn = _lm_setup(d, lam)
    xd, ld = torch.from_numpy(x).to(DEV), torch.from_numpy(lens).to(DEV)
    dec = _biased_decoder(d, g, 64, len(d) - 1, nbest=3, lm=lm, lm_weight=lam, bonus=beta)
    out = dec.search(xd, ld)
    out1 = _biased_decoder(d, g, 64, len(d) - 1, nbest=1, lm=lm, lm_weight=lam, bonus=beta).search(xd, ld)
    worst, n, credited = 0.0, 0, 0
    for b in range(x.shape[0]):
        assert _hyps(out1, b) == _hyps(out, b)[:1]
        oracle, margin = biased_oracle(x[b, : lens[b]].astype(np.float64), int(lens[b]), 64, len(d) - 1, d.bos(), g, lm_fn=fn,
                                       lm_weight=lam, bonus=beta, eos=d.eos(), nbest=3)
        for i, (y, s) in enumerate(_hyps(out, b)):
            lm_y = sum(fn(y[:u])[y[u]] for u in range(len(y))) + fn(y)[d.eos()]
            By = locked_bonus(g.phrases, y)
            ref = -ctc_nll_numpy(x[b, : lens[b]].astype(np.float64), list(y), blank=d.bos()) + lam * lm_y + beta * len(y) + By
            tol = SCORE_TOL + lam * LM_TOL * (len(y) + 1)
            print(f"utterance {b} {y}: score {s:.6f} independent {ref:.6f} B(y) {By:.2f} |diff| {abs(s - ref):.2e} (bound {tol:.1e})")
            assert s < ref + tol, (b, y, s, ref)
            if i == 0:  # every hypothesis of the nbest 1 search
                assert abs(s - ref) < tol, (b, y, s, ref)
                worst = max(worst, abs(s - ref))
            if margin > 2 * tol:
                assert y == oracle[i][0] and abs(s - oracle[i][1]) < tol, (b, i, y, s, oracle)
            credited += By > 0
            n += 1
    assert n == 3 * x.shape[0] and credited >= x.shape[0]
    print(f"max |score - independent| {worst:.2e}")


def _lm_case():
    d = _dictionary(12)
    V = len(d)
    rng = np.random.default_rng(5)
    B, T = 3, 10
    x = _peaked(rng, B * T, V, sharp=6.0).reshape(B, T, V).astype(np.float32)
    lens = np.array([10, 7, 4], dtype=np.int32)
    phrases = []
    for b in range(B):  # the 2-grams of each utterance's unbiased 1-best and 2-best
        hyps, _ = prefix_beam_oracle(x[b].astype(np.float64), int(lens[b]), 16, V - 1, d.bos(), nbest=2)
        for k, (y, _) in enumerate(hyps):
            phrases += [(list(y[i : i + 2]), BOOSTS[k]) for i in range(len(y) - 1)]
    return d, x, lens, 0.5, 0.3, phrases


def test_lm_case_oracle_is_exact():
    """The inputs of test_every_biased_score_is_right_with_lm, float64 oracle alone (a seeded stand-in LM: any function of the
    prefix): beam 64 with every token a candidate loses less than a tenth of SCORE_TOL of the 1-best to pruning, which leaves the
    fp32 search the rest of its tolerance."""
    from oracle.torch_ref import ctc_nll_numpy

    d, x, lens, lam, beta, phrases = _lm_case()
    V = len(d)
    g = _graph(phrases, V)
    table = {}

    def fn(y):
        if y not in table:
            z = np.random.default_rng(abs(hash(y)) % (2 ** 32)).standard_normal(V)
            table[y] = z - np.logaddexp.reduce(z)
        return table[y]

    for b in range(x.shape[0]):
        hyps, _ = biased_oracle(x[b].astype(np.float64), int(lens[b]), 64, V - 1, d.bos(), g, lm_fn=fn, lm_weight=lam, bonus=beta,
                                eos=d.eos(), nbest=3)
        assert len(hyps) == 3
        for y, s in hyps[:1]:
            lm_y = sum(fn(y[:u])[y[u]] for u in range(len(y))) + fn(y)[d.eos()]
            ref = -ctc_nll_numpy(x[b, : lens[b]].astype(np.float64), list(y), blank=d.bos()) + lam * lm_y + beta * len(y) + \
                locked_bonus(g.phrases, y)
            assert abs(s - ref) < SCORE_TOL / 10, (b, y, s, ref)


def _two_token_input(T=5, a=5, b_=6, V=None):
    """Blank on the odd frames; on the even ones token b_ is ahead of token a by about 0.2."""
    x = -8.0 - 0.5 * np.arange(V, dtype=np.float64)[None].repeat(T, 0)
    for t in range(T):
        if t % 2 == 0:
            x[t, b_], x[t, a], x[t, 0] = -0.6 - 0.07 * t, -0.8 - 0.03 * t, -3.0
        else:
            x[t, 0] = -0.05
    return (x - np.logaddexp.reduce(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.gpu
def test_biasing_changes_the_answer():
    """The unbiased 1-best (b, b, b) beats (a, a, a) by delta (exact CTC log-probabilities).  The phrase [a, a, a] with
    3 * boost = delta + 0.2 turns the 1-best into (a, a, a); with delta - 0.2 it does not.  No other sequence of three emitting
    frames holds the phrase."""
    from oracle.torch_ref import ctc_nll_numpy

    _need_gpu()
    d = _dictionary(10)
    V, a, b_ = len(d), 5, 6
    x = _two_token_input(V=V)
    T = x.shape[0]
    delta = ctc_nll_numpy(x.astype(np.float64), [a, a, a], blank=0) - ctc_nll_numpy(x.astype(np.float64), [b_, b_, b_], blank=0)
    assert delta > 0.3
    xd, lens = torch.from_numpy(x).to(DEV)[None].contiguous(), torch.tensor([T], dtype=torch.int32, device=DEV)
    assert _hyps(_decoder(d, 3, 2).search(xd, lens), 0)[0][0] == (b_, b_, b_)
    for total, want in ((delta + 0.2, (a, a, a)), (delta - 0.2, (b_, b_, b_))):
        g = _graph([([a, a, a], total / 3)], V)
        dec = _biased_decoder(d, g, 3, 2, nbest=2)  # (beam 3: the pending bonus is what keeps (a, a) in so narrow a beam)
        got = _hyps(dec.search(xd, lens), 0)
        ref, margin = biased_oracle(x.astype(np.float64), T, 3, 2, 0, g, nbest=2)
        print(f"delta {delta:.4f}, 3 * boost {total:.4f}: {got}; oracle {ref} (margin {margin:.3g})")
        assert margin > SCORE_TOL
        assert got[0][0] == want and [y for y, _ in got] == [y for y, _ in ref]
        assert all(abs(s - r) < SCORE_TOL for (_, s), (_, r) in zip(got, ref))


@pytest.mark.gpu
def test_empty_graph_and_no_graph_are_bit_identical():
    """context_graph=None, an empty graph and the existing entry points called directly: the same bits, on the grid of
    test_search_vs_oracle_no_lm and with the LSTM LM."""
    _need_gpu()
    from espresso_amd import kernels as Kn

    d = _dictionary(20)
    V = len(d)
    lens = torch.from_numpy(GRID_LENS).to(DEV)
    B, T = len(GRID_LENS), int(GRID_LENS.max())
    for beam, K, seed in GRID:
        for dtype in (torch.float32, torch.bfloat16):
            xd = torch.from_numpy(grid_inputs(seed, V)).to(DEV, dtype)
            nb = min(beam, 3)
            plain = _decoder(d, beam, K, nbest=nb).search(xd, lens)
            none = _biased_decoder(d, None, beam, K, nbest=nb).search(xd, lens)
            empty = _biased_decoder(d, _graph([], V), beam, K, nbest=nb).search(xd, lens)
            ws = Kn.ctc_prefix_beam_workspace(B, T, beam, DEV)
            Kn.ctc_prefix_beam_step(xd.view(B * T, V), lens, ws, B, T, V, beam, K, d.bos(), 0, T)
            direct = Kn.ctc_prefix_beam_finish(ws, B, T, beam, nb, d.pad())
            for other in (none, empty, direct):
                for p, o in zip(plain, other):
                    assert torch.equal(p, o), (beam, K, seed, dtype)
    lm, _ = _lm_setup(d, 0.4)
    xd = torch.from_numpy(grid_inputs(1, V)[:, :8]).to(DEV, torch.float32).contiguous()
    lens8 = torch.clamp(lens, max=8)
    plain = _decoder(d, 4, 4, nbest=2, lm=lm, lm_weight=0.4, bonus=0.2).search(xd, lens8)
    empty = _biased_decoder(d, _graph([], V), 4, 4, nbest=2, lm=lm, lm_weight=0.4, bonus=0.2).search(xd, lens8)
    for p, o in zip(plain, empty):
        assert torch.equal(p, o)


@pytest.mark.gpu
@pytest.mark.parametrize("with_lm", [False, True])
def test_merged_hypothesis_keeps_one_state(with_lm):
    """Phrase [a, b, c].  Frame 1 leaves both (a) and (a, b) in the beam; at frame 2 token b extends (a) into (a, b) while
    (a, b) stays by repeating b: the two slot histories merge mid-phrase, and the merged hypothesis carries one (q, b) on to c."""
    from oracle.torch_ref import ctc_nll_numpy

    _need_gpu()
    d = _dictionary(8)
    V, a, b_, c = len(d), 4, 5, 6
    T = 5
    x = np.full((T, V), -9.0)
    x[0, a], x[0, 0] = -0.2, -2.0
    x[1, a], x[1, b_], x[1, 0] = -1.0, -1.1, -1.2   # (a) by repeat or blank, (a, b) by extension: both survive
    x[2, b_], x[2, 0] = -0.3, -1.6                  # (a) + b merges into the stay of (a, b)
    x[3, 0], x[3, c] = -0.4, -1.3
    x[4, c], x[4, 0] = -0.3, -1.7
    x = (x - np.logaddexp.reduce(x, axis=1, keepdims=True)).astype(np.float32)
    g = _graph([([a, b_, c], BOOSTS[1])], V)
    lam = 0.4 if with_lm else 0.0
    lm, fn = _lm_setup(d, lam) if with_lm else (None, None)
    dec = _biased_decoder(d, g, 6, 3, nbest=2, lm=lm, lm_weight=lam)
    got = _hyps(dec.search(torch.from_numpy(x).to(DEV)[None].contiguous(), torch.tensor([T], dtype=torch.int32, device=DEV)), 0)
    # the oracle's trace shows the merge this input is built for
    hyps2, _ = biased_oracle(x[:2].astype(np.float64), 2, 6, 3, 0, g, nbest=6)
    assert {(a,), (a, b_)} <= {y for y, _ in hyps2}
    ref, margin = biased_oracle(x.astype(np.float64), T, 6, 3, 0, g, lm_fn=fn, lm_weight=lam, eos=d.eos(), nbest=2)
    tol = SCORE_TOL + lam * LM_TOL * (T + 1)
    assert margin > 2 * tol
    print(f"with_lm {with_lm}: {got}; oracle {ref}")
    assert [y for y, _ in got] == [y for y, _ in ref] and got[0][0] == (a, b_, c)
    assert all(abs(s - r) < tol for (_, s), (_, r) in zip(got, ref))
    if not with_lm:  # all alignments of (a, b, c), both histories included, plus the whole phrase once
        exact = -ctc_nll_numpy(x.astype(np.float64), [a, b_, c], blank=0) + 3 * BOOSTS[1]
        assert abs(got[0][1] - exact) < 1e-3, (got[0][1], exact)  # (pruned alignments through other prefixes: < 1e-3 here)


@pytest.mark.gpu
@pytest.mark.parametrize("with_lm", [False, True])
def test_biased_search_does_not_synchronise(with_lm):
    _need_gpu()
    d = _dictionary(16)
    V = len(d)
    rng = np.random.default_rng(3)
    B, T = 3, 12
    x = _peaked(rng, B * T, V).reshape(B, T, V).astype(np.float32)
    lens = np.array([12, 5, 0], dtype=np.int32)
    g = _graph(grid_phrases(x.astype(np.float64), lens, 0), V)
    assert g.num_nodes > 4
    lm = _lm_setup(d, 0.5)[0] if with_lm else None
    dec = _biased_decoder(d, g, 6, 4, nbest=2, lm=lm, lm_weight=0.5)
    xd, ld = torch.from_numpy(x).to(DEV), torch.from_numpy(lens).to(DEV)
    ref = [t.clone() for t in dec.search(xd, ld)]  # warm-up (graph upload, cached bf16 weights)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = dec.search(xd, ld)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for p, o in zip(out, ref):
        assert torch.equal(p, o)


@pytest.mark.gpu
def test_cli_round_trip_with_hotwords(tmp_path, capsys):
    """speech_recognize --search ctc_beam --hotwords prints what the decoder with the same graph returns; the H- scores are the
    biased ones."""
    _need_gpu()
    from espresso_amd import registry
    from espresso_amd import speech_recognize as sr
    from espresso_amd.data.audio_utils import read_wav
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from espresso_amd.tools.context_graph import load_context_graph
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder

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
    rng = np.random.default_rng(0)
    utts = [f"utt{i}" for i in range(4)]
    with open(tmp_path / "wav.scp", "w") as f:
        for i, u in enumerate(utts):
            p = str(tmp_path / f"{u}.wav")
            _write_wav(p, rng.standard_normal(int(16000 * (0.6 + 0.3 * i))) * 3000)
            f.write(f"{u} {p}\n")
    waves = [read_wav(str(tmp_path / f"{u}.wav")) for u in utts]
    task.build_frontend(torch.device(DEV))

    def decode(gen):
        res = []
        for bt in sr.make_batches(utts, [len(w) for w in waves], 500, 3):
            sample = sr.collate(bt, utts, waves, torch.device(DEV))
            hyps = gen.generate([model], task.prepare_sample(sample, train=False))
            for i, u in enumerate(sample["utt_ids"]):
                res += [(f"H-{u}", h["tokens"].tolist(), float(h["score"])) for h in hyps[i][:2]]
        return res

    # hotwords: the 2-grams of what the untrained model says without them, and one phrase it never says
    plain = decode(CTCPrefixBeamSearchDecoder([model], d, beam_size=5, nbest=2))
    grams = sorted({tuple(t[i : i + 2]) for _, t, _ in plain for i in range(len(t) - 1)})[:6]
    hot = tmp_path / "hot.txt"
    hot.write_text("# phrases\n" + "".join(" ".join(d[t] for t in gr) + ("\t0.9\n" if k % 2 else "\n") for k, gr in enumerate(grams)) +
                   "t28 t29 t28\n", encoding="utf-8")
    capsys.readouterr()
    sr.main(["--path", str(tmp_path / "model.pt"), "--dict", dict_path, "--wav-scp", str(tmp_path / "wav.scp"), "--search", "ctc_beam",
             "--beam", "5", "--nbest", "2", "--max-tokens", "500", "--batch-size", "3", "--hotwords", str(hot), "--hotword-score", "1.3"])
    lines = [l.split("\t") for l in capsys.readouterr().out.splitlines() if l.startswith("H-")]
    g = load_context_graph(str(hot), d, d.bos(), 1.3)
    expect = decode(CTCPrefixBeamSearchDecoder([model], d, beam_size=5, nbest=2, context_graph=g))
    assert len(lines) == len(expect) == 2 * len(utts)
    for (hu, text, score), (eu, etoks, escore) in zip(lines, expect):
        assert (hu, text) == (eu, d.string(torch.tensor(etoks)))
        assert abs(float(score) - escore / math.log(2)) < 1e-4, (hu, score, escore)
    if grams:  # the printed scores carry B(y)
        assert any(locked_bonus(g.phrases, t) > 0 for _, t, _ in expect)
