"""CTC prefix beam search with LSTM-LM shallow fusion (tools/ctc_prefix_beam_search.py, csrc/ctc_beam.hip).

`prefix_beam_oracle` below is a float64 numpy statement of the search contract; the GPU tests hold the HIP search to it, and
the CPU tests hold the oracle itself to brute force over every label sequence (oracle.torch_ref.ctc_nll_numpy)."""
import math
import os
import wave

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SCORE_TOL = 1e-4  # fp32 search vs the float64 oracle on the same log-probs
# |lm_gpu - lm_cpu| per LM term (one token or the final eos) of the tiny LSTM LM below: bf16 weights and bf16 GEMM operands
# on the HIP path against the fp32 oracle LM.  Measured on an MI355X: 1.2e-4 per term on the 1-best hypotheses of
# test_every_hypothesis_score_is_right_with_lm; the bound leaves 8x headroom over that
LM_TOL = 1e-3


# ------------------------------------------------------------------------------------------------------ the oracle
def _lae(a, b):
    m = max(a, b)
    return -math.inf if m == -math.inf else m + math.log1p(math.exp(-abs(a - b)))


def prefix_beam_oracle(x, length, beam, K, blank, lm_fn=None, lm_weight=0.0, bonus=0.0, eos=None, nbest=1):
    """x (T, V) log-probs of one utterance.  lm_fn(prefix tuple) -> float64 [V] log P_lm(. | prefix) (None: no LM).
    Returns ([(tokens, final score)] best first, the smallest pruning / ranking margin met)."""
    x = np.asarray(x, dtype=np.float64)
    lw = lm_weight if lm_fn is not None else 0.0
    hyps = [((), 0.0, -math.inf, 0.0)]  # (prefix, pb, pnb, lm), best first
    margin = math.inf
    for t in range(length):
        row = x[t]
        cands = sorted(sorted((v for v in range(x.shape[1]) if v != blank), key=lambda v: (-row[v], v))[:K])
        nxt = {}  # prefix -> [pb, pnb, lm, order key]

        def add(y, pb, pnb, lm, key, stay):
            if y in nxt:
                e = nxt[y]
                e[0], e[1] = _lae(e[0], pb), _lae(e[1], pnb)
                if stay:
                    e[2], e[3] = lm, key
            else:
                nxt[y] = [pb, pnb, lm, key]

        for j, (y, pb, pnb, lm) in enumerate(hyps):
            sc = _lae(pb, pnb)
            last = y[-1] if y else None
            add(y, sc + row[blank], pnb + row[last] if (y and last in cands) else -math.inf, lm, (j, 0, 0), True)
            lrow = lm_fn(y) if lm_fn is not None else None
            for c in cands:
                add(y + (c,), -math.inf, (pb if c == last else sc) + row[c], lm + (lrow[c] if lrow is not None else 0.0),
                    (j, 1, c), False)
        scored = sorted(((_lae(e[0], e[1]) + lw * e[2] + bonus * len(y), e[3], y, e) for y, e in nxt.items()),
                        key=lambda r: (-r[0], r[1]))
        if len(scored) > beam:
            margin = min(margin, scored[beam - 1][0] - scored[beam][0])
        hyps = [(y, e[0], e[1], e[2]) for _, _, y, e in scored[:beam]]
    fin = []
    for j, (y, pb, pnb, lm) in enumerate(hyps):
        s = _lae(pb, pnb) + lw * lm + bonus * len(y)
        if lm_fn is not None:
            s += lw * lm_fn(y)[eos]
        fin.append((s, j, y))
    fin.sort(key=lambda r: (-r[0], r[1]))
    top = fin[: nbest + 1]
    for a, b in zip(top, top[1:]):
        margin = min(margin, a[0] - b[0])
    return [(y, s) for s, _, y in fin[:nbest]], margin


def _peaked(rng, T, V, sharp=4.0, scale=1.0):
    """Log-softmax rows with one clearly preferred token per frame (blank half of the time), like a trained CTC model."""
    z = scale * rng.standard_normal((T, V))
    z[np.arange(T), np.where(rng.random(T) < 0.5, 0, rng.integers(1, V, T))] += sharp
    return z - np.logaddexp.reduce(z, axis=1, keepdims=True)


def _dictionary(n):
    from espresso_amd.data.asr_dictionary import AsrDictionary

    return AsrDictionary.from_symbols([f"t{i}" for i in range(n)], enable_bos=True)


def _tiny_lm(d, seed=0, prefer=None):
    """A seeded 2-layer LSTM LM over dictionary d (CPU); prefer=(a, b) biases its output strongly towards a over b."""
    from espresso_amd.models.lstm_lm import LSTMLanguageModelEspresso

    class T:
        target_dictionary = source_dictionary = d

    torch.manual_seed(seed)
    lm = LSTMLanguageModelEspresso.build_model(dict(arch="lstm_lm_wsj", decoder_embed_dim=16, decoder_hidden_size=24, decoder_layers=2,
                                                    decoder_out_embed_dim=24, dropout=0.0, share_embed=False), T)
    with torch.no_grad():
        for p in lm.parameters():
            p.uniform_(-0.3, 0.3)
        lm.decoder.embed_tokens.weight[d.pad()] = 0.0  # the padding row stays zero, as in a trained LM
        if prefer is not None:
            lm.decoder.fc_out.bias[prefer[0]] += 3.0
            lm.decoder.fc_out.bias[prefer[1]] -= 3.0
    return lm.eval()


def _cpu_lm_fn(lm, d):
    """prefix -> float64 log P(. | eos + prefix) from oracle.torch_ref.lstm_lm (fp32, CPU), cached."""
    from oracle import torch_ref

    sd = {k: v.detach().float().cpu() for k, v in lm.state_dict().items()}
    cache = {}

    def fn(prefix):
        if prefix not in cache:
            tok = torch.tensor([[d.eos()] + list(prefix)], dtype=torch.long)
            with torch.no_grad():
                lg = torch_ref.lstm_lm(tok, sd, pad_idx=d.pad())[0, -1].double()
            cache[prefix] = torch.log_softmax(lg, -1).numpy()
        return cache[prefix]

    return fn


def _args(*extra):
    from espresso_amd import speech_recognize as sr

    return sr.get_parser().parse_args(["--path", "m.pt", "--dict", "d.txt", "--wav-scp", "wav.scp", *extra])


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_cli_ctc_beam_options():
    a = _args("--search", "ctc_beam")
    assert (a.search, a.beam, a.nbest, a.ctc_beam_size_token, a.ctc_insertion_bonus, a.lm_weight) == ("ctc_beam", 10, 1, None, 0.0, 0.0)
    a = _args("--search", "ctc_beam", "--ctc-beam-size-token", "4", "--ctc-insertion-bonus", "0.5", "--lm-path", "lm.pt")
    assert (a.ctc_beam_size_token, a.ctc_insertion_bonus) == (4, 0.5)
    from espresso_amd import speech_recognize as sr

    assert sr.lm_fusion_mode(a) == "subword"


@pytest.mark.parametrize("extra", [["--lm-path", "lm.pt", "--word-dict", "words.txt"], ["--word-dict", "words.txt"],
                                   ["--lm-path", os.pathsep.join(["sub.pt", "word.pt"])],
                                   ["--lm-path", os.pathsep.join(["sub.pt", "word.pt"]), "--word-dict", "words.txt"]])
def test_cli_ctc_beam_refuses_word_lms(extra):
    from espresso_amd import speech_recognize as sr

    with pytest.raises(NotImplementedError, match="ctc_beam"):
        sr.main(["--path", "missing.pt", "--dict", "missing.txt", "--wav-scp", "missing.scp", "--search", "ctc_beam", *extra])


def test_cli_ctc_beam_refuses_ensembles():
    from espresso_amd import speech_recognize as sr

    with pytest.raises(NotImplementedError, match="ensembles"):
        sr.main(["--path", os.pathsep.join(["a.pt", "b.pt"]), "--dict", "missing.txt", "--wav-scp", "missing.scp", "--search", "ctc_beam"])


def test_build_generator_ctc_searches():
    from espresso_amd import speech_recognize as sr
    from espresso_amd.tools.ctc_decoder import CTCDecoder
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder

    d = _dictionary(8)
    assert type(sr.build_generator(_args("--search", "ctc", "--lm-path", "lm.pt"), None, d, lm=None)) is CTCDecoder
    lm = _tiny_lm(d)
    g = sr.build_generator(_args("--search", "ctc_beam", "--beam", "6", "--nbest", "2", "--lm-weight", "0.3"), None, d, lm=lm)
    assert isinstance(g, CTCPrefixBeamSearchDecoder)
    assert (g.beam_size, g.nbest, g.beam_size_token, g.lm_model, g.lm_weight, g.blank) == (6, 2, 6, lm, 0.3, d.bos())
    g = sr.build_generator(_args("--search", "ctc_beam", "--beam", "64"), None, d)
    assert g.beam_size_token == len(d) - 1 and g.lm_model is None
    with pytest.raises(AssertionError, match="dictionary"):
        CTCPrefixBeamSearchDecoder([None], _dictionary(9), lm_model=lm)
    with pytest.raises(ValueError):
        CTCPrefixBeamSearchDecoder([None], d, beam_size=65)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("T", [1, 3, 5])
def test_oracle_is_exact_without_pruning(seed, T):
    """beam and K exhaustive: the search is the exact CTC posterior of every prefix, so its 1-best is the argmax of
    -ctc_nll over every label sequence of length <= T and its scores are those log-probabilities."""
    import itertools

    from oracle.torch_ref import ctc_nll_numpy

    rng = np.random.default_rng(seed)
    V, blank = 4, 0
    x = rng.standard_normal((T, V)) * 1.5
    x -= np.logaddexp.reduce(x, axis=1, keepdims=True)
    hyps, _ = prefix_beam_oracle(x, T, beam=10 ** 6, K=V - 1, blank=blank, nbest=10 ** 6)
    hyps = [(y, s) for y, s in hyps if s > -math.inf]  # (prefixes too long for T frames stay, at probability 0)
    brute = {}
    for n in range(T + 1):
        for y in itertools.product(range(1, V), repeat=n):
            nll = ctc_nll_numpy(x, list(y), blank=blank)
            if np.isfinite(nll):
                brute[y] = -nll
    assert {y for y, _ in hyps} == set(brute)
    for y, s in hyps:
        assert abs(s - brute[y]) < 1e-9, (y, s, brute[y])
    assert hyps[0][0] == max(brute, key=brute.get)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


def _decoder(d, beam, K=None, nbest=1, lm=None, lm_weight=0.0, bonus=0.0):
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder

    return CTCPrefixBeamSearchDecoder([None], d, beam_size=beam, nbest=nbest, beam_size_token=K, lm_model=lm, lm_weight=lm_weight,
                                      insertion_bonus=bonus)


def _hyps(out, b):
    tokens, lengths, scores, nhyp = (t.cpu() for t in out)
    return [(tuple(tokens[b, i, : int(lengths[b, i])].tolist()), float(scores[b, i])) for i in range(int(nhyp[b]))]


def _compare(out, x, lens, dec, lm_fn=None, min_margin=SCORE_TOL, score_tol=SCORE_TOL):
    worst = 0.0
    for b in range(x.shape[0]):
        ref, margin = prefix_beam_oracle(x[b].astype(np.float64), int(lens[b]), dec.beam_size, dec.beam_size_token, dec.blank,
                                         lm_fn=lm_fn, lm_weight=dec.lm_weight, bonus=dec.insertion_bonus, eos=dec.eos, nbest=dec.nbest)
        got = _hyps(out, b)
        assert margin > min_margin, (b, margin)
        assert [y for y, _ in got] == [y for y, _ in ref], (b, got, ref)
        for (_, s), (_, r) in zip(got, ref):
            worst = max(worst, abs(s - r))
    assert worst < score_tol, worst
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
# every (beam, K) of {1, 4, 16} x {1, 4}, K > beam included; seeds: oracle margins > 1e-3 for fp32 and bf16
@pytest.mark.parametrize("beam,K,seed", [(1, 1, 0), (1, 4, 0), (4, 1, 0), (4, 4, 1), (16, 1, 0), (16, 4, 11)])
def test_search_vs_oracle_no_lm(beam, K, seed, dtype):
    _need_gpu()
    d = _dictionary(20)
    V = len(d)
    rng = np.random.default_rng(seed)
    B, T = 5, 14
    x = _peaked(rng, B * T, V, sharp=4.0, scale=2.0).reshape(B, T, V)
    lens = np.array([T, 0, 1, 9, 12], dtype=np.int32)
    xd = torch.from_numpy(x).to(DEV, dtype)
    x_seen = xd.float().cpu().numpy()  # what the kernel reads (bf16-rounded for bf16)
    dec = _decoder(d, beam, K, nbest=min(beam, 3))
    out = dec.search(xd, torch.from_numpy(lens).to(DEV))
    worst = _compare(out, x_seen, lens, dec)
    print(f"beam {beam} K {K} {dtype}: max |score - oracle| {worst:.2e}")
    assert _hyps(out, 1) == [((), 0.0)]  # in_len 0: the empty hypothesis


def _lm_setup(d, lm_weight, prefer=None, seed=0):
    lm_cpu = _tiny_lm(d, seed=seed, prefer=prefer)
    fn = _cpu_lm_fn(lm_cpu, d)
    lm_gpu = _tiny_lm(d, seed=seed, prefer=prefer).to(DEV)
    return lm_gpu, fn


@pytest.mark.gpu
def test_every_hypothesis_score_is_right_with_lm():
    """Scores against an independent computation, -ctc_nll(y) + lambda * (LM_cpu(y) + log P(eos | y)) + beta * |y|.
    Pruning only ever drops CTC paths of a prefix, so that value bounds every returned score from above; the 1-best keeps all
    of its paths on these inputs (the oracle's own 1-best is within 6e-6 of it), so there it is an equality."""
    from oracle.torch_ref import ctc_nll_numpy

    _need_gpu()
    d = _dictionary(12)
    V = len(d)
    rng = np.random.default_rng(5)
    B, T = 3, 10
    x = _peaked(rng, B * T, V, sharp=6.0).reshape(B, T, V).astype(np.float32)
    lens = np.array([10, 7, 4], dtype=np.int32)
    lam, beta = 0.5, 0.3
    lm, fn = _lm_setup(d, lam)
    dec = _decoder(d, 16, V - 1, nbest=3, lm=lm, lm_weight=lam, bonus=beta)
    out = dec.search(torch.from_numpy(x).to(DEV), torch.from_numpy(lens).to(DEV))
    worst, n = 0.0, 0
    for b in range(B):
        for i, (y, s) in enumerate(_hyps(out, b)):
            lm_y = sum(fn(y[:u])[y[u]] for u in range(len(y))) + fn(y)[d.eos()]
            ref = -ctc_nll_numpy(x[b, : lens[b]].astype(np.float64), list(y), blank=d.bos()) + lam * lm_y + beta * len(y)
            tol = SCORE_TOL + lam * LM_TOL * (len(y) + 1)
            assert s < ref + tol, (b, y, s, ref)
            if i == 0:
                assert abs(s - ref) < tol, (b, y, s, ref)
                worst = max(worst, abs(s - ref) / (lam * (len(y) + 1)))
            n += 1
    assert n == 3 * B
    print(f"1-best: max |score - independent| / (lambda * LM terms) = {worst:.2e}")


@pytest.mark.gpu
def test_fusion_changes_the_answer():
    """Two tokens nearly tied acoustically at every emitting frame; the LM prefers one strongly: lambda = 0 picks the acoustic
    winner, lambda > 0 the LM's choice, and both match the oracle."""
    _need_gpu()
    d = _dictionary(10)
    V = len(d)
    a, b_ = 5, 6  # the LM prefers a over b_; acoustically b_ is ahead by about 0.2 per emitting frame
    T = 5
    x = -8.0 - 0.5 * np.arange(V, dtype=np.float64)[None].repeat(T, 0)
    for t in range(T):
        if t % 2 == 0:
            x[t, b_], x[t, a], x[t, 0] = -0.6 - 0.07 * t, -0.8 - 0.03 * t, -3.0
        else:
            x[t, 0] = -0.05
    x = x - np.logaddexp.reduce(x, axis=1, keepdims=True)
    x = x[None].astype(np.float32)
    lens = np.array([T], dtype=np.int32)
    lm, fn = _lm_setup(d, 0.5, prefer=(a, b_), seed=5)
    best = {}
    for lam in (0.0, 0.5):
        dec = _decoder(d, 3, 2, lm=lm, lm_weight=lam)
        out = dec.search(torch.from_numpy(x).to(DEV), torch.from_numpy(lens).to(DEV))
        _compare(out, x, lens, dec, lm_fn=fn, min_margin=lam * LM_TOL * (T + 1) * 2 + SCORE_TOL,
                 score_tol=SCORE_TOL + lam * LM_TOL * (T + 1))
        best[lam] = _hyps(out, 0)[0][0]
    assert best[0.0] == (b_, b_, b_) and best[0.5] == (a, a, a), best


@pytest.mark.gpu
@pytest.mark.parametrize("beam,K", [(2, 3), (4, 4), (6, 3), (10, 6)])
def test_search_vs_oracle_with_lm(beam, K):
    _need_gpu()
    d = _dictionary(16)
    V = len(d)
    rng = np.random.default_rng(0)
    B, T = 4, 6
    x = _peaked(rng, B * T, V, sharp=6.0, scale=2.5).reshape(B, T, V).astype(np.float32)
    lens = np.array([6, 5, 1, 0], dtype=np.int32)
    lam = 0.4
    lm, fn = _lm_setup(d, lam, seed=3)
    dec = _decoder(d, beam, K, nbest=2, lm=lm, lm_weight=lam)
    out = dec.search(torch.from_numpy(x).to(DEV), torch.from_numpy(lens).to(DEV))
    worst = _compare(out, x, lens, dec, lm_fn=fn, min_margin=2 * lam * LM_TOL * (T + 1) + SCORE_TOL,
                     score_tol=SCORE_TOL + lam * LM_TOL * (T + 1))
    print(f"beam {beam} K {K} with LM: max |score - oracle| {worst:.2e} (bound {SCORE_TOL + lam * LM_TOL * (T + 1):.1e})")


@pytest.mark.gpu
def test_lm_update_keeps_the_rows_of_kept_hypotheses():
    """The host-side LM update after a step: a row that appended nothing recomputes exactly its parent's LM row."""
    _need_gpu()
    from espresso_amd import kernels as Kn

    d = _dictionary(16)
    V = len(d)
    rng = np.random.default_rng(5)
    B, T, beam = 2, 4, 6
    x = torch.from_numpy(_peaked(rng, B * T, V, sharp=1.0).astype(np.float32)).to(DEV)
    lens = torch.tensor([T, T], dtype=torch.int32, device=DEV)
    lm, _ = _lm_setup(d, 0.5)
    dec = _decoder(d, beam, 4, lm=lm, lm_weight=0.5)
    ws = Kn.ctc_prefix_beam_workspace(B, T, beam, DEV)
    state, rows = dec.lm_start(B * beam, DEV)
    lm_out = (torch.empty(B * beam, dtype=torch.int32, device=DEV), torch.empty(B * beam, dtype=torch.int32, device=DEV),
              torch.empty(B * beam, dtype=torch.uint8, device=DEV))
    n_kept = 0
    for t in range(T):
        Kn.ctc_prefix_beam_step(x, lens, ws, B, T, V, beam, 4, dec.blank, t, t + 1, lm_rows=rows, lm_weight=0.5, lm_out=lm_out)
        parent, token, keep = (o.clone() for o in lm_out)
        prev = rows
        state, rows = dec.lm_update(state, parent, token, keep)
        k = keep.bool()
        n_kept += int(k.sum())
        assert torch.equal(rows[k], prev[parent.long()][k]), t
    assert n_kept > 0


@pytest.mark.gpu
def test_real_model_generate_vs_oracle():
    """The ref_conformer_ctc_tiny fixture model's log-probs through `generate`, against the oracle on the same log-probs."""
    _need_gpu()
    from tests.gpu_checks import _Task, build_tiny_model, load_fixture, load_ref_state

    g, sd, _, _ = load_fixture("ref_conformer_ctc_tiny")
    model = build_tiny_model("conformer").to(DEV).eval()
    load_ref_state(model, sd)
    d = _Task(40).target_dictionary
    feats, lengths = torch.from_numpy(g["feats"]).to(DEV), torch.from_numpy(g["lengths"]).to(DEV)
    with torch.no_grad():
        net_out = model(feats, lengths)
        lp = model.get_normalized_probs(net_out, log_probs=True).transpose(0, 1).float().cpu().numpy()
    out_len = net_out["src_lengths"][0].cpu().numpy()
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder

    dec = CTCPrefixBeamSearchDecoder([model], d, beam_size=8, nbest=3)
    hyps = dec.generate([model], {"net_input": {"src_tokens": feats, "src_lengths": lengths}})
    for b in range(lp.shape[0]):
        ref, margin = prefix_beam_oracle(lp[b].astype(np.float64), int(out_len[b]), 8, dec.beam_size_token, dec.blank, nbest=3)
        got = [(tuple(h["tokens"].tolist()), float(h["score"])) for h in hyps[b]]
        assert len(got) == len(ref)
        for (gy, gs), (ry, rs) in zip(got, ref):
            assert abs(gs - rs) < SCORE_TOL, (b, got, ref)
        if margin > SCORE_TOL:
            assert [y for y, _ in got] == [y for y, _ in ref], (b, got, ref)
        print(f"utterance {b}: {int(out_len[b])} frames, oracle margin {margin:.3g}, 1-best {got[0]}")


@pytest.mark.gpu
@pytest.mark.parametrize("with_lm", [False, True])
def test_device_search_does_not_synchronise(with_lm):
    _need_gpu()
    d = _dictionary(16)
    V = len(d)
    rng = np.random.default_rng(3)
    B, T = 3, 12
    x = torch.from_numpy(_peaked(rng, B * T, V).reshape(B, T, V).astype(np.float32)).to(DEV)
    lens = torch.tensor([12, 5, 0], dtype=torch.int32, device=DEV)
    lm = _lm_setup(d, 0.5)[0] if with_lm else None
    dec = _decoder(d, 6, 4, nbest=2, lm=lm, lm_weight=0.5)
    ref = [t.clone() for t in dec.search(x, lens)]  # warm-up (cached bf16 weights, bias sums)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = dec.search(x, lens)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(out, ref):
        assert torch.equal(a, b)


def _write_wav(path, samples):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(samples, -32768, 32767).astype("<i2").tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("with_lm", [False, True])
def test_cli_round_trip(tmp_path, with_lm, capsys):
    """speech_recognize --search ctc_beam prints, for every utterance, the hypothesis the decoder returns directly."""
    _need_gpu()
    from espresso_amd import registry
    from espresso_amd import speech_recognize as sr
    from espresso_amd.data.audio_utils import read_wav
    from espresso_amd.models.lstm_lm import LSTMLanguageModelEspresso
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
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

    class _LMTask:
        target_dictionary = source_dictionary = d

    lm = None
    argv = ["--path", str(tmp_path / "model.pt"), "--dict", dict_path, "--wav-scp", str(tmp_path / "wav.scp"), "--search", "ctc_beam",
            "--beam", "5", "--nbest", "2", "--max-tokens", "500", "--batch-size", "3"]
    if with_lm:
        lm = LSTMLanguageModelEspresso.build_model(dict(arch="lstm_lm_wsj", is_wordlm=False), _LMTask)
        torch.save(lm.state_dict(), str(tmp_path / "lm.pt"))
        lm = lm.to(DEV).eval()
        argv += ["--lm-path", str(tmp_path / "lm.pt"), "--lm-arch", "lstm_lm_wsj", "--lm-weight", "0.5"]
    rng = np.random.default_rng(0)
    utts = [f"utt{i}" for i in range(4)]
    with open(tmp_path / "wav.scp", "w") as f:
        for i, u in enumerate(utts):
            p = str(tmp_path / f"{u}.wav")
            _write_wav(p, rng.standard_normal(int(16000 * (0.6 + 0.3 * i))) * 3000)
            f.write(f"{u} {p}\n")
    capsys.readouterr()
    sr.main(argv)
    lines = [l.split("\t") for l in capsys.readouterr().out.splitlines() if l.startswith("H-")]

    waves = [read_wav(str(tmp_path / f"{u}.wav")) for u in utts]
    task.build_frontend(torch.device(DEV))
    gen = CTCPrefixBeamSearchDecoder([model], d, beam_size=5, nbest=2, lm_model=lm, lm_weight=0.5 if with_lm else 0.0)
    expect = []
    for bt in sr.make_batches(utts, [len(w) for w in waves], 500, 3):
        sample = sr.collate(bt, utts, waves, torch.device(DEV))
        hyps = gen.generate([model], task.prepare_sample(sample, train=False))
        for i, u in enumerate(sample["utt_ids"]):
            for h in hyps[i][:2]:
                expect.append((f"H-{u}", d.string(h["tokens"]), float(h["score"]) / math.log(2)))
    assert len(lines) == len(expect) == 2 * len(utts)
    for (hu, text, score), (eu, etext, escore) in zip(lines, expect):
        assert (hu, text) == (eu, etext)
        assert abs(float(score) - escore) < 1e-4, (hu, score, escore)
