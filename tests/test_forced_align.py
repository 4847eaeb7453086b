"""Forced alignment (csrc/align.hip, tools/forced_aligner.py, speech_align).

CPU: float64 oracles of both Viterbi searches with the header's tie rules, checked against brute-force enumeration of every
alignment on small lattices (with ties), the CTC lattice against the forward-algorithm NLL, word grouping / CTM, seconds per
encoder frame from the model's strides, CLI parsing and the refusal of attention models.
GPU (-m gpu): both kernels against the oracles on random inputs (fp32 / bf16, ragged lengths, repeats, infeasible and empty
targets), the transducer aligner's fused and materialised lattices on the reference fixture, and the CLI end to end."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

DEV = "cuda:0"
MARGIN = 1e-3


# ------------------------------------------------------------------------------------------------ float64 oracles
def ctc_viterbi_oracle(x, L, y, blank):
    """x: (>= L, V) float64 log-probs.  Returns (frame_label [L], tok_start [U], tok_end [U], score, margin): ties prefer stay,
    then +1, then +2; at the end S-1 over S-2.  margin = the smallest gap between the chosen and the best other candidate over
    the decisions on the chosen path (inf where there was no alternative)."""
    U = len(y)
    S = 2 * U + 1
    lab = np.array([blank if s % 2 == 0 else y[s // 2] for s in range(S)])
    allow2 = np.zeros(S, dtype=bool)
    for s in range(3, S, 2):
        allow2[s] = lab[s] != lab[s - 2]
    none = (np.full(0, -1), np.full(U, -1), np.full(U, -1))
    if L == 0:
        return none + ((0.0 if U == 0 else -np.inf), np.inf)
    a = np.full(S, -np.inf)
    a[0] = x[0, blank]
    if S > 1:
        a[1] = x[0, lab[1]]
    bps, gaps = [None], [None]
    ar = np.arange(S)
    for t in range(1, L):
        c1 = np.concatenate([[-np.inf], a])[:S]
        c2 = np.concatenate([[-np.inf, -np.inf], a])[:S]
        c2[~allow2] = -np.inf
        C = np.stack([a, c1, c2])
        k = np.argmax(C, axis=0)  # first maximum: stay, +1, +2
        best = C[k, ar]
        second = np.sort(C, axis=0)[-2]
        with np.errstate(invalid="ignore"):
            gap = np.where(second == -np.inf, np.inf, best - second)
        bps.append(k)
        gaps.append(gap)
        a = best + x[t, lab]
    e1, e2 = a[S - 1], (a[S - 2] if S > 1 else -np.inf)
    score = e1 if e1 >= e2 else e2
    if score == -np.inf:
        return (np.full(L, -2),) + none[1:] + (-np.inf, np.inf)
    s = S - 1 if e1 >= e2 else S - 2
    margin = np.inf if e2 == -np.inf or e1 == -np.inf else abs(e1 - e2)
    states = np.zeros(L, dtype=np.int64)
    for t in range(L - 1, -1, -1):
        states[t] = s
        if t > 0:
            margin = min(margin, gaps[t][s])
            s -= bps[t][s]
    fl = np.where(states % 2 == 1, states // 2, -1)
    ts, te = np.full(U, -1), np.full(U, -1)
    for t in range(L):
        u = fl[t]
        if u >= 0:
            if t == 0 or fl[t - 1] != u:
                ts[u] = t
            if t == L - 1 or fl[t + 1] != u:
                te[u] = t + 1
    return fl, ts, te, float(score), float(margin)


def rnnt_viterbi_oracle(lpb, lpy, Tb, Ub):
    """lpb / lpy: (>= Tb, >= Ub + 1) float64.  Returns (emit_frame [Ub], score, margin); the decision at a node prefers emit
    over blank (the earlier emission).  Swept along anti-diagonals from the end."""
    if Tb <= 0:
        return np.full(Ub, -1), -np.inf, np.inf
    beta = np.full((Tb + 1, Ub + 2), -np.inf)
    emit = np.zeros((Tb, Ub + 1), dtype=bool)
    gap = np.full((Tb, Ub + 1), np.inf)
    for d in range(Tb - 1 + Ub, -1, -1):
        u = np.arange(max(0, d - Tb + 1), min(Ub, d) + 1)
        t = d - u
        blk = np.where(t == Tb - 1, np.where(u == Ub, lpb[t, u], -np.inf), lpb[t, u] + beta[t + 1, u])
        emt = np.where(u < Ub, lpy[t, u] + beta[t, u + 1], -np.inf)
        e = (u < Ub) & ((t == Tb - 1) | (emt >= blk))
        beta[t, u] = np.where(e, emt, blk)
        emit[t, u] = e
        with np.errstate(invalid="ignore"):
            gap[t, u] = np.where((t == Tb - 1) | (u == Ub), np.inf, np.abs(emt - blk))
    score = beta[0, 0]
    if score == -np.inf:
        return np.full(Ub, -1), -np.inf, np.inf
    ef = np.full(Ub, -1)
    t = u = 0
    margin = np.inf
    while not (t == Tb - 1 and u == Ub):
        margin = min(margin, gap[t, u])
        if emit[t, u]:
            ef[u] = t
            u += 1
        else:
            t += 1
    return ef, float(score), float(margin)


# ------------------------------------------------------------------------------------------------ brute force
def _ctc_brute(x, L, y, blank):
    """Best path by enumeration: (frame states, score) or (None, -inf); ties broken by the total order the backtrace realises
    (end state S-1 first, then the move codes from the last frame backwards, smaller = preferred)."""
    U = len(y)
    S = 2 * U + 1
    lab = [blank if s % 2 == 0 else y[s // 2] for s in range(S)]
    best = None
    for start in (0, 1):
        if start >= S:
            continue
        for moves in itertools.product((0, 1, 2), repeat=L - 1):
            st, ok = [start], True
            for m in moves:
                s = st[-1] + m
                if s >= S or (m == 2 and not (s % 2 == 1 and lab[s] != lab[s - 2])):
                    ok = False
                    break
                st.append(s)
            if not ok or st[-1] < S - 2:
                continue
            sc = 0.0
            for t, s in enumerate(st):
                sc += x[t, lab[s]]
            if sc == -np.inf:
                continue
            key = (-sc, st[-1] != S - 1, tuple(reversed(moves)))
            if best is None or key < best[0]:
                best = (key, st, sc)
    return (None, -np.inf) if best is None else (best[1], best[2])


def _rnnt_brute(lpb, lpy, Tb, Ub):
    """(emit frames, score) of the best path; ties: the move sequence read forwards, emit before blank."""
    best = None
    n = Tb - 1 + Ub
    for pos in itertools.combinations(range(n), Ub):  # positions of the emits among the moves before the final blank
        t = u = 0
        sc, ef, key = 0.0, [], []
        ps = set(pos)
        for i in range(n):
            if i in ps:
                sc += lpy[t, u]
                ef.append(t)
                u += 1
                key.append(0)
            else:
                sc += lpb[t, u]
                t += 1
                key.append(1)
        sc += lpb[Tb - 1, Ub]
        k = (-sc, tuple(key))
        if best is None or k < best[0]:
            best = (k, ef, sc)
    return best[1], best[2]


def _quantised(rng, shape):
    return -rng.integers(1, 4, size=shape).astype(np.float64) * 0.5  # few distinct values: many ties


@pytest.mark.parametrize("seed", range(6))
def test_ctc_oracle_vs_brute_force(seed):
    rng = np.random.default_rng(seed)
    blank, n = 0, 0
    for V in (2, 3, 4):
        for T in range(1, 8):
            for U in range(0, 4):
                for trial in range(2):
                    y = list(rng.integers(1, V, size=U))
                    x = _quantised(rng, (T, V)) if trial == 0 else np.log(rng.dirichlet(np.ones(V), size=T))
                    st, sc = _ctc_brute(x, T, y, blank)
                    fl, ts, te, osc, _ = ctc_viterbi_oracle(x, T, y, blank)
                    if st is None:
                        assert osc == -np.inf and (fl == -2).all() and (ts == -1).all()
                        continue
                    n += 1
                    assert osc == sc, (T, y, osc, sc)
                    want = np.where(np.array(st) % 2 == 1, np.array(st) // 2, -1)
                    assert (fl == want).all(), (T, y, fl, want)
                    for u in range(U):
                        frames = np.nonzero(want == u)[0]
                        assert ts[u] == frames[0] and te[u] == frames[-1] + 1
    assert n > 100


def test_ctc_oracle_infeasible_and_empty():
    x = np.log(np.full((3, 4), 0.25))
    assert ctc_viterbi_oracle(x, 3, [1, 1], 0)[3] > -np.inf  # 1 blank 1: 3 frames
    assert ctc_viterbi_oracle(x, 2, [1, 1], 0)[3] == -np.inf  # a repeat needs the blank between
    assert ctc_viterbi_oracle(x, 2, [1, 2, 3], 0)[3] == -np.inf
    assert ctc_viterbi_oracle(x, 0, [1], 0)[3] == -np.inf
    fl, ts, te, sc, _ = ctc_viterbi_oracle(x, 3, [], 0)
    assert (fl == -1).all() and sc == pytest.approx(3 * np.log(0.25))


@pytest.mark.parametrize("seed", range(6))
def test_rnnt_oracle_vs_brute_force(seed):
    rng = np.random.default_rng(100 + seed)
    for T in range(1, 8):
        for U in range(0, 4):
            for trial in range(3):
                if trial == 0:
                    lpb, lpy = _quantised(rng, (T, U + 1)), _quantised(rng, (T, U + 1))
                else:
                    p = rng.uniform(0.05, 0.95, size=(T, U + 1))
                    lpb, lpy = np.log(p), np.log(1 - p) + np.log(rng.uniform(0.1, 1.0, size=(T, U + 1)))
                ef, sc = _rnnt_brute(lpb, lpy, T, U)
                oef, osc, _ = rnnt_viterbi_oracle(lpb, lpy, T, U)
                assert osc == pytest.approx(sc, abs=1e-12), (T, U)
                assert list(oef) == ef, (T, U, oef, ef)


def test_rnnt_tie_rule_is_the_earlier_emission():
    lpb = np.full((3, 2), -1.0)
    lpy = np.full((3, 2), -1.0)
    ef, sc, margin = rnnt_viterbi_oracle(lpb, lpy, 3, 1)
    assert list(ef) == [0] and sc == -4.0 and margin == 0.0


def test_ctc_viterbi_below_forward_nll_and_equal_on_one_path():
    from oracle.torch_ref import ctc_nll_numpy

    rng = np.random.default_rng(7)
    for T, U in [(12, 3), (30, 8), (9, 0)]:
        x = np.log(rng.dirichlet(np.ones(6), size=T))
        y = list(rng.integers(1, 6, size=U))
        assert ctc_viterbi_oracle(x, T, y, 0)[3] <= -ctc_nll_numpy(x, y, blank=0) + 1e-12
    y = [1, 2, 3, 4, 5]  # T == U, no repeats: the only path puts one token on every frame
    x = np.log(rng.dirichlet(np.ones(6), size=5))
    fl, ts, te, sc, _ = ctc_viterbi_oracle(x, 5, y, 0)
    assert list(fl) == [0, 1, 2, 3, 4]
    assert sc == pytest.approx(-ctc_nll_numpy(x, y, blank=0), abs=1e-9)


# ------------------------------------------------------------------------------------------------ words, CTM, frames
def test_word_spans_space_tokens_and_sentencepiece():
    from espresso_amd.tools.forced_aligner import word_spans

    syms = ["h", "i", "<space>", "y", "o", "u"]
    assert word_spans(syms, [0, 2, 4, 5, 7, 8], [1, 3, 5, 6, 8, 10]) == [("hi", 0, 3), ("you", 5, 10)]
    syms = ["▁he", "llo", "▁wor", "ld", "▁", "x"]
    assert word_spans(syms, [1, 3, 6, 8, 11, 12], [2, 4, 7, 10, 12, 13]) == [("hello", 1, 4), ("world", 6, 10), ("x", 11, 13)]


def _dict(tmp_path, symbols):
    from espresso_amd.data.asr_dictionary import AsrDictionary

    p = tmp_path / "dict.txt"
    p.write_text("".join(f"{s} 1\n" for s in symbols))
    return AsrDictionary.load(str(p), enable_bos=True)


def test_ctm_lines_units_and_infeasible(tmp_path):
    from espresso_amd.tools.forced_aligner import ctm_lines, utterance_units

    d = _dict(tmp_path, list("abc") + ["<space>"])
    a, b, c, sp = (d.index(s) for s in ("a", "b", "c", "<space>"))
    r = {"tokens": np.array([a, b, sp, c]), "start": np.array([2, 4, 6, 9]), "end": np.array([3, 6, 7, 11]), "feasible": True}
    assert ctm_lines("u1", utterance_units(r, d, "token"), 0.04) == [
        "u1 1 0.080 0.040 a 1.00", "u1 1 0.160 0.080 b 1.00", "u1 1 0.240 0.040 <space> 1.00", "u1 1 0.360 0.080 c 1.00"]
    assert ctm_lines("u1", utterance_units(r, d, "word"), 0.04) == ["u1 1 0.080 0.160 ab 1.00", "u1 1 0.360 0.080 c 1.00"]


def test_results_unpacking_marks_infeasible():
    from espresso_amd.tools.forced_aligner import _results

    B, L = 2, 2
    score = np.array([-3.5, -np.inf], dtype=np.float32).view(np.int32)
    host = np.concatenate([[4, 5, 6, 0], [0, 3, -1, -1], [2, 4, -1, -1], [2, 1], [5, 0], score]).astype(np.int32)
    r = _results(host, B, L)
    assert r[0]["feasible"] and list(r[0]["tokens"]) == [4, 5] and list(r[0]["end"]) == [2, 4] and r[0]["score"] == -3.5
    assert not r[1]["feasible"] and list(r[1]["start"]) == [-1] and r[1]["frames"] == 0


@pytest.mark.parametrize("strides,factor", [("[(2, 2), (2, 2)]", 4), ("[(1, 1), (1, 1)]", 1), ("[(1, 1), (3, 3)]", 3)])
def test_frame_seconds_from_the_model_strides(tmp_path, strides, factor):
    from espresso_amd import registry
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from espresso_amd.tools.forced_aligner import frame_seconds

    (tmp_path / "dict.txt").write_text("".join(f"t{i} 1\n" for i in range(10)))
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(dict=str(tmp_path / "dict.txt"),
                                                                                    criterion_name="ctc_loss"))
    block = {"encoder": {"embed_dim": 32, "ffn_embed_dim": 64, "layers": 1, "attention_heads": 2, "conv_channels": "[8, 8]",
                         "conv_kernel_sizes": "[(3, 3), (3, 3)]", "conv_strides": strides}}
    cls = registry.MODEL_REGISTRY["speech_transformer_encoder_model"]
    model = cls.build_model(cls.config_class.from_dict(block), task)
    assert frame_seconds(model, 0.01) == pytest.approx(0.01 * factor)


# ------------------------------------------------------------------------------------------------ CLI (host side)
def test_cli_parser_defaults():
    from espresso_amd import speech_align

    a = speech_align.get_parser().parse_args(["--path", "m.pt", "--dict", "d.txt", "--wav-scp", "w.scp", "--text", "t"])
    assert (a.unit, a.output, a.scores, a.max_tokens, a.batch_size, a.bpe) == ("token", "-", None, 15000, 24, None)
    with pytest.raises(SystemExit):
        speech_align.get_parser().parse_args(["--path", "m.pt", "--dict", "d.txt", "--wav-scp", "w.scp"])  # --text required


@pytest.mark.parametrize("name", ["speech_transformer_base", "speech_lstm", "speech_transformer"])
def test_cli_refuses_attention_models_before_loading(tmp_path, name):
    from espresso_amd import speech_align

    with pytest.raises(NotImplementedError, match="print-alignment"):
        speech_align.main(["--path", str(tmp_path / "missing.pt"), "--model", name, "--dict", "d.txt", "--wav-scp", "w.scp",
                           "--text", "t"])


def test_model_kinds():
    from espresso_amd import speech_align

    assert speech_align.model_kind("speech_transformer_encoder_model") == "ctc"
    assert speech_align.model_kind("speech_transformer_transducer_base") == "transducer"


def test_tokenize_like_training_targets(tmp_path):
    from espresso_amd import speech_align

    d = _dict(tmp_path, list("abc") + ["<space>"])
    d.build_bpe("characters_asr")
    # (characters_asr ends a transcript with <space>, as in the training targets)
    assert speech_align.tokenize(d, "ab c", d.bos()) == [d.index(s) for s in ("a", "b", "<space>", "c", "<space>")]
    plain = _dict(tmp_path, ["x", "y"])  # no encoder: the text is the tokens
    assert speech_align.tokenize(plain, "x y x", plain.bos()) == [plain.index(s) for s in ("x", "y", "x")]
    with pytest.raises(ValueError, match="blank"):
        speech_align.tokenize(plain, "x <s> y", plain.bos())


# ------------------------------------------------------------------------------------------------ GPU
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


def _peaked_lprobs(rng, B, T, V, sharp=3.0):
    z = rng.standard_normal((B, T, V)) * sharp
    z -= z.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ctc_kernel_vs_oracle(dtype):
    _need_gpu()
    from espresso_amd import kernels as K

    rng = np.random.default_rng(11 if dtype == torch.float32 else 12)
    B, T, V, blank, Lmax = 24, 1000, 50, 0, 200
    x = torch.from_numpy(_peaked_lprobs(rng, B, T, V).astype(np.float32)).to(dtype)
    in_len = rng.integers(T // 3, T + 1, size=B)
    in_len[0] = T
    tl = [int(min(Lmax, rng.integers(0, max(1, in_len[b] // 3)))) for b in range(B)]
    tl[0], tl[1], tl[2] = Lmax, 0, 150
    in_len[1] = 37
    in_len[2] = 100  # infeasible: 150 tokens in 100 frames
    tg = np.zeros((B, Lmax), dtype=np.int32)
    for b in range(B):
        y = rng.integers(1, V, size=tl[b])
        rep = rng.random(tl[b]) < 0.15  # repeated adjacent tokens
        for u in range(1, tl[b]):
            if rep[u]:
                y[u] = y[u - 1]
        tg[b, : tl[b]] = y
    xd = x.reshape(B * T, V).to(DEV)
    ts, te, fl, sc = K.ctc_viterbi_align(xd, torch.from_numpy(tg).to(DEV), torch.from_numpy(in_len.astype(np.int32)).to(DEV),
                                         torch.tensor(tl, dtype=torch.int32, device=DEV), B, T, V, blank)
    ts, te, fl, sc = ts.cpu().numpy(), te.cpu().numpy(), fl.cpu().numpy(), sc.cpu().numpy()
    x64 = x.float().numpy().astype(np.float64)
    checked = 0
    for b in range(B):
        L, U = int(in_len[b]), tl[b]
        ofl, ots, ote, osc, margin = ctc_viterbi_oracle(x64[b], L, list(tg[b, :U]), blank)
        if osc == -np.inf:
            assert sc[b] == -np.inf and (fl[b] == -2).all() and (ts[b] == -1).all() and (te[b] == -1).all(), b
            continue
        assert abs(sc[b] - osc) <= 1e-4 * max(1.0, abs(osc)), (b, sc[b], osc)
        assert (fl[b, L:] == -2).all() and (ts[b, U:] == -1).all() and (te[b, U:] == -1).all()
        if margin > MARGIN:
            checked += 1
            assert (fl[b, :L] == ofl).all(), (b, np.nonzero(fl[b, :L] != ofl)[0][:10])
            assert (ts[b, :U] == ots).all() and (te[b, :U] == ote).all(), b
    assert sc[2] == -np.inf and sc[1] > -np.inf and (fl[1, :37] == -1).all()
    assert checked >= B // 2, checked


@pytest.mark.gpu
def test_ctc_kernel_padded_rows_and_refusals():
    _need_gpu()
    from espresso_amd import kernels as K

    rng = np.random.default_rng(5)
    B, T, V = 3, 40, 7
    wide = torch.from_numpy(_peaked_lprobs(rng, B, T, 16).astype(np.float32)).reshape(B * T, 16)
    x = wide[:, :V].contiguous().log_softmax(-1)
    padded = torch.full((B * T, 16), float("nan"))
    padded[:, :V] = x
    tg = torch.tensor([[1, 2, 3], [4, 4, 0], [5, 0, 0]], dtype=torch.int32)
    args = (tg.to(DEV), torch.tensor([40, 30, 2], dtype=torch.int32, device=DEV), torch.tensor([3, 2, 1], dtype=torch.int32, device=DEV))
    a = K.ctc_viterbi_align(x.to(DEV), *args, B, T, V, 0)
    p = K.ctc_viterbi_align(padded.to(DEV)[:, :V], *args, B, T, V, 0, ld=16)
    for u, v in zip(a, p):
        assert torch.equal(u, v)
    bad = torch.tensor([[1, 9, 3], [4, 4, 0], [0, 0, 0]], dtype=torch.int32, device=DEV)  # id 9 >= V, then blank as a target
    _, _, fl, sc = K.ctc_viterbi_align(x.to(DEV), bad, args[1], args[2], B, T, V, 0)
    sc = sc.cpu()
    assert torch.isnan(sc[0]) and torch.isnan(sc[2]) and not torch.isnan(sc[1]) and (fl[0] == -2).all()
    with pytest.raises(RuntimeError):
        K.ctc_viterbi_align(x.to(DEV), torch.zeros(B, 1024, dtype=torch.int32, device=DEV), args[1], args[2], B, T, V, 0)


@pytest.mark.gpu
def test_rnnt_kernel_vs_oracle():
    _need_gpu()
    from espresso_amd import kernels as K

    rng = np.random.default_rng(21)
    B, T, U1 = 12, 400, 121
    p = rng.uniform(0.02, 0.98, size=(B, T, U1))
    lpb = np.log(p).astype(np.float32)
    lpy = (np.log1p(-p) + np.log(rng.uniform(0.05, 1.0, size=(B, T, U1)))).astype(np.float32)
    Tl = rng.integers(1, T + 1, size=B).astype(np.int32)
    Ul = rng.integers(0, U1, size=B).astype(np.int32)
    Tl[0], Ul[0], Ul[1], Tl[2] = T, U1 - 1, 0, 1
    ef, sc = K.rnnt_viterbi_align(torch.from_numpy(lpb).to(DEV), torch.from_numpy(lpy).to(DEV), torch.from_numpy(Tl).to(DEV),
                                  torch.from_numpy(Ul).to(DEV))
    ef, sc = ef.cpu().numpy(), sc.cpu().numpy()
    checked = 0
    for b in range(B):
        oef, osc, margin = rnnt_viterbi_oracle(lpb[b].astype(np.float64), lpy[b].astype(np.float64), int(Tl[b]), int(Ul[b]))
        assert abs(sc[b] - osc) <= 1e-4 * max(1.0, abs(osc)), (b, sc[b], osc)
        assert (ef[b, Ul[b]:] == -1).all()
        assert (np.diff(ef[b, : Ul[b]]) >= 0).all() and (ef[b, : Ul[b]] < Tl[b]).all()
        if margin > MARGIN:
            checked += 1
            assert (ef[b, : Ul[b]] == oef).all(), (b, np.nonzero(ef[b, : Ul[b]] != oef)[0][:10])
    assert checked >= B // 2, checked


def _transducer_fixture():
    from tests.gpu_checks import _Task, build_tiny_transducer

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_conformer_transducer_tiny.npz"))
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}
    model = build_tiny_transducer().to(DEV)
    model.load_state_dict(model.upgrade_state_dict_named(dict(sd), ""), strict=False)
    model.eval()
    d = _Task(40).target_dictionary
    prev = g["prev"]
    targets = [[int(t) for t in prev[b, 1:] if int(t) != d.pad()] for b in range(prev.shape[0])]
    sample = {"net_input": {"src_tokens": torch.from_numpy(g["feats"]).to(DEV), "src_lengths": torch.from_numpy(g["lengths"]).to(DEV)}}
    return model, d, sample, targets


@pytest.mark.gpu
def test_transducer_fused_and_materialised_lattices_align_alike():
    _need_gpu()
    from espresso_amd import kernels as K
    from espresso_amd.tools.forced_aligner import TransducerForcedAligner, _pad_targets

    model, d, sample, targets = _transducer_fixture()
    fused, plain = TransducerForcedAligner([model], d), TransducerForcedAligner([model], d, fused=False)
    tg, tl = _pad_targets(targets, None, 0, DEV)
    lb_f, ly_f, enc_len, loss_f = fused.lattice(sample, tg, tl)
    lb_p, ly_p, _, loss_p = plain.lattice(sample, tg, tl)
    B, T, U1 = lb_f.shape
    for b in range(B):  # the two lattices agree on the nodes that exist (the fused one skips bf16 logits)
        Tb, Ub = int(enc_len[b]), int(tl[b])
        assert (lb_f[b, :Tb, : Ub + 1] - lb_p[b, :Tb, : Ub + 1]).abs().max() < 0.05
    ra, rb = fused.align(sample, targets), plain.align(sample, targets)
    _, sc_ref = K.rnnt_viterbi_align(lb_p.contiguous(), ly_p.contiguous(), enc_len, tl)
    for b, (x, y) in enumerate(zip(ra, rb)):
        oef, osc, margin = rnnt_viterbi_oracle(lb_f[b].double().cpu().numpy(), ly_f[b].double().cpu().numpy(), x["frames"],
                                               len(targets[b]))
        assert x["feasible"] and y["feasible"] and list(x["tokens"]) == targets[b]
        assert list(x["start"]) == list(oef) or margin <= MARGIN
        assert list(x["start"]) == list(y["start"]), (b, x["start"], y["start"])
        assert abs(x["score"] - y["score"]) < 0.05
        assert x["score"] <= -float(loss_f[b]) + 1e-4 and y["score"] <= -float(loss_p[b]) + 1e-4
        assert list(x["end"]) == [s + 1 for s in x["start"]]
        print(f"utterance {b}: {x['frames']} frames, emits {list(x['start'])}, viterbi {x['score']:.4f}, -loss {-float(loss_f[b]):.4f}")


@pytest.mark.gpu
def test_ctc_aligner_on_the_fixture_model_matches_the_oracle():
    _need_gpu()
    from espresso_amd.tools.forced_aligner import CTCForcedAligner
    from tests.gpu_checks import _Task, build_tiny_model, load_fixture, load_ref_state

    g, sd, _, _ = load_fixture("ref_conformer_ctc_tiny")
    model = build_tiny_model("conformer").to(DEV).eval()
    load_ref_state(model, sd)
    d = _Task(40).target_dictionary
    feats, lengths = torch.from_numpy(g["feats"]).to(DEV), torch.from_numpy(g["lengths"]).to(DEV)
    with torch.no_grad():
        net_out = model(feats, lengths)
        lp = model.get_normalized_probs(net_out, log_probs=True).transpose(0, 1).float().cpu().numpy().astype(np.float64)
    enc = net_out["src_lengths"][0].cpu().numpy()
    rng = np.random.default_rng(2)
    targets = [list(rng.integers(5, 40, size=max(1, int(enc[b]) // 4))) for b in range(lp.shape[0])]
    res = CTCForcedAligner([model], d).align({"net_input": {"src_tokens": feats, "src_lengths": lengths}}, targets)
    for b, r in enumerate(res):
        fl, ts, te, sc, margin = ctc_viterbi_oracle(lp[b], int(enc[b]), targets[b], d.bos())
        assert r["frames"] == int(enc[b]) and r["feasible"]
        assert abs(r["score"] - sc) <= 1e-4 * max(1.0, abs(sc))
        if margin > MARGIN:
            assert list(r["start"]) == list(ts) and list(r["end"]) == list(te)


@pytest.mark.gpu
def test_cli_end_to_end_ctm(tmp_path):
    _need_gpu()
    from espresso_amd import speech_align
    from espresso_amd.data import audio_utils
    from tests.gpu_checks import load_fixture

    _, sd, _, _ = load_fixture("ref_conformer_ctc_tiny")
    (tmp_path / "dict.txt").write_text("".join(f"t{i} 1\n" for i in range(35)) + "<space> 1\n")
    block = {"_name": "speech_transformer_encoder_model", "dropout": 0.0, "layernorm_embedding": True,
             "encoder": {"embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4, "normalize_before": True,
                         "relative_positional_embeddings": True, "layer_type": "conformer", "conv_channels": "[64, 64, 16, 16]"}}
    (tmp_path / "cfg.json").write_text(json.dumps(block))
    torch.save({"model": {"encoder." + k: v for k, v in sd.items()}}, str(tmp_path / "m.pt"))
    rng = np.random.default_rng(9)
    utts = {"u0": (1.3, "t3 t4 <space> t7 t7 t9"), "u1": (0.8, "t1 t2 t2"), "u2": (0.1, "t1 t2 t3 t4 t5 t6 t7 t8 t9 t10")}
    scp, text = [], []
    for u, (sec, words) in utts.items():
        p = str(tmp_path / f"{u}.wav")
        audio_utils.write_wav(p, np.round(rng.standard_normal(int(16000 * sec)) * 800).astype(np.float32))
        scp.append(f"{u} {p}\n")
        text.append(f"{u} {words}\n")
    (tmp_path / "wav.scp").write_text("".join(scp))
    (tmp_path / "text").write_text("".join(text))
    base = ["--path", str(tmp_path / "m.pt"), "--model-config", str(tmp_path / "cfg.json"), "--dict", str(tmp_path / "dict.txt"),
            "--wav-scp", str(tmp_path / "wav.scp"), "--text", str(tmp_path / "text"), "--batch-size", "2"]
    res = speech_align.main(base + ["--output", str(tmp_path / "tok.ctm"), "--scores", str(tmp_path / "scores")])
    speech_align.main(base + ["--output", str(tmp_path / "word.ctm"), "--unit", "word"])
    assert not res["u2"]["feasible"] and res["u0"]["feasible"] and res["u1"]["feasible"]
    spf = 0.04  # 10 ms frame shift x the fixture's sub-sampling factor 4
    for u in ("u0", "u1"):
        lines = [l.split() for l in (tmp_path / "tok.ctm").read_text().splitlines() if l.startswith(u + " ")]
        assert [l[4] for l in lines] == utts[u][1].split()  # one CTM line per transcript token
        starts = [float(l[2]) for l in lines]
        ends = [float(l[2]) + float(l[3]) for l in lines]
        assert all(l[1] == "1" and float(l[3]) > 0 for l in lines)
        assert starts == sorted(starts) and all(e <= s2 + 1e-9 for e, s2 in zip(ends, starts[1:]))
        assert ends[-1] <= utts[u][0] + 1e-6 and ends[-1] <= res[u]["frames"] * spf + 1e-6
        assert [round(s / spf) for s in starts] == list(res[u]["start"])
    assert not any(l.startswith("u2 ") for l in (tmp_path / "tok.ctm").read_text().splitlines())
    words = [l.split()[4] for l in (tmp_path / "word.ctm").read_text().splitlines() if l.startswith("u0 ")]
    assert words == ["t3t4", "t7t7t9"]
    sc = {l.split()[0]: l.split() for l in (tmp_path / "scores").read_text().splitlines()}
    assert sc["u2"][-1] == "infeasible" and int(sc["u0"][2]) == 6 and int(sc["u0"][1]) == res["u0"]["frames"]
