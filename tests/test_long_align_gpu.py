"""Long-form forced alignment on the device (csrc/align_long.hip, kernels.ctc_viterbi_align_long, tools/forced_aligner.py
`LongFormCTCAligner`, speech_align --long-form): the tiled kernel against the float64 reference of tests/long_align_ref.py on
quantised inputs (exact, ties included), bit for bit against the one-workgroup kernel `kernels.ctc_viterbi_align` wherever that
one takes the problem, the edge cases of the header, and the whole path on the tiny CTC fixture model and the command line.
Every shape is built from `ea_ctc_viterbi_long_tile`, so the tests follow the kernel's tile constants."""
import json

import numpy as np
import pytest
import torch

from tests import long_align_ref as ref

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
BLANK = 0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib
    from espresso_amd import kernels as K

    _lib.lib()
    return K


def _run(K, x, y, V, blank=BLANK, dtype=torch.float32, ld=None):
    """The kernel on host inputs x float64 [T][>= V] and ids y; outputs as numpy (score: a float32 scalar)."""
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV)
    T = xd.shape[0]
    yd = torch.from_numpy(np.asarray(y, dtype=np.int32)).to(DEV)
    ts, te, fl, flp, sc = K.ctc_viterbi_align_long(xd[:, :V], yd, T, V, blank, ld=ld)
    assert ts.shape == te.shape == (len(y),) and fl.shape == flp.shape == (T,) and sc.shape == (1,)
    return ts.cpu().numpy(), te.cpu().numpy(), fl.cpu().numpy(), flp.cpu().numpy(), sc.cpu().numpy()[0]


def _assert_equals_reference(got, x, y, blank=BLANK):
    ts, te, fl, flp, sc = got
    ofl, ots, ote, oflp, osc, _ = ref.align(x, y, blank)
    assert float(sc) == osc, (float(sc), osc)
    assert np.array_equal(fl, ofl), np.nonzero(fl != ofl)[0][:10]
    assert np.array_equal(ts, ots) and np.array_equal(te, ote)
    assert np.array_equal(flp.astype(np.float64), oflp), np.nonzero(flp != oflp)[0][:10]
    return osc


# ------------------------------------------------------------------------------------------------ exact against float64
def _exact_shapes(TB, TS):
    """U: S = 2U + 1 spans three full state tiles and a remainder that is no multiple of 16; T = max(3 TB + 5, U + U // 4), then
    one less than a multiple of TB, a multiple, and one more."""
    U = (3 * TS + TS // 2 + 36) // 2
    S = 2 * U + 1
    assert S // TS == 3 and (S % TS) % 16 != 0
    T = max(3 * TB + 5, U + U // 4)
    Tm = -(-T // TB) * TB
    return U, [T, Tm - 1, Tm, Tm + 1]


@pytest.mark.parametrize("which", range(4), ids=["T", "multiple-1", "multiple", "multiple+1"])
def test_exact_against_float64_on_quantised_inputs(which):
    """Emissions are multiples of 1/64 in [-16, 0]: every fp32 sum is exact (up to 16 384 frames), so the kernel and the float64
    reference see the same ties and must resolve them by the same rule: score, labels, spans and frame log-probs are equal, with
    no margin and no case left out."""
    K = _need_gpu()
    TB, TS = K.ctc_viterbi_long_tile()
    U, Ts = _exact_shapes(TB, TS)
    T, V = Ts[which], 37
    assert T <= 16384
    rng = np.random.default_rng([7, which])
    x = ref.quantised_lprobs(rng, T, V)
    y = ref.targets_with_repeats(rng, U, V, BLANK)
    assert int((y[1:] == y[:-1]).sum()) > U // 10
    sc = _assert_equals_reference(_run(K, x, y, V), x, y)
    assert np.isfinite(sc)
    print(f"T {T} U {U} (tile {TB} x {TS}): score {sc}")


# ------------------------------------------------------------------------------------------------ against the old kernel
def _peaked_lprobs(rng, T, V, sharp=3.0):
    z = rng.standard_normal((T, V)) * sharp
    z -= z.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("U", [0, 1, 7, 511, 512, 1023])  # (511, 512: S one state short of a state tile, one state into the second)
def test_bit_identical_to_the_one_workgroup_kernel(U, dtype):
    """Real-valued log-probs: max-plus in fp32 in the same order gives the same bits, so every common output is `torch.equal`
    to ea_ctc_viterbi_align's at B = 1; also from a padded matrix (ld > V) whose pad columns hold NaN."""
    K = _need_gpu()
    TB, TS = K.ctc_viterbi_long_tile()
    V, ld = 50, 56
    T = int(1.3 * U) + 2 * TB
    rng = np.random.default_rng([11, U])
    y = ref.targets_with_repeats(rng, U, V, BLANK)
    x = torch.from_numpy(_peaked_lprobs(rng, T, V)).to(dtype).to(DEV)
    yd = torch.from_numpy(y).to(DEV)
    old_tg = torch.zeros(1, max(U, 1), dtype=torch.int32, device=DEV)
    old_tg[0, :U] = yd
    ots, ote, ofl, osc = K.ctc_viterbi_align(x, old_tg, torch.tensor([T], dtype=torch.int32, device=DEV),
                                             torch.tensor([U], dtype=torch.int32, device=DEV), 1, T, V, BLANK)
    padded = torch.full((T, ld), float("nan"), dtype=dtype, device=DEV)
    padded[:, :V] = x
    for src, pitch in ((x, None), (padded[:, :V], ld)):
        ts, te, fl, flp, sc = K.ctc_viterbi_align_long(src, yd, T, V, BLANK, ld=pitch)
        assert torch.equal(sc.view(torch.int32), osc.view(torch.int32)) and bool(torch.isfinite(sc).all())
        assert torch.equal(fl, ofl[0]) and torch.equal(ts, ots[0, :U]) and torch.equal(te, ote[0, :U])
        lab = torch.where(fl >= 0, yd[fl.clamp(min=0).long()] if U else torch.zeros_like(fl), torch.full_like(fl, BLANK))
        assert torch.equal(flp.view(torch.int32), x.float()[torch.arange(T, device=DEV), lab.long()].view(torch.int32))


# ------------------------------------------------------------------------------------------------ edge cases
def test_infeasible_transcripts():
    K = _need_gpu()
    TB, TS = K.ctc_viterbi_long_tile()
    rng = np.random.default_rng(3)
    V = 9
    for U in (5, TS // 2 + 3):
        y = (np.arange(U) % (V - 1) + 1).astype(np.int32)  # no equal neighbours
        for T, yy in ((U - 1, y), (U, np.concatenate([y[:2], y[1:U - 1]]).astype(np.int32))):  # too few frames; a repeat in U frames
            x = ref.quantised_lprobs(rng, T, V)
            ts, te, fl, flp, sc = _run(K, x, yy, V)
            assert sc == -np.inf and (fl == -2).all() and (ts == -1).all() and (te == -1).all() and (flp == 0).all()
            _assert_equals_reference((ts, te, fl, flp, sc), x, yy)
        x = ref.quantised_lprobs(rng, U, V)  # U tokens in exactly U frames: the one path
        got = _run(K, x, y, V)
        _assert_equals_reference(got, x, y)
        assert list(got[2]) == list(range(U))


def test_empty_and_tiny_problems():
    K = _need_gpu()
    TB, TS = K.ctc_viterbi_long_tile()
    rng = np.random.default_rng(4)
    V = 6
    none = np.zeros((0, V))
    ts, te, fl, flp, sc = _run(K, none, [], V)  # T = 0, U = 0
    assert sc == 0.0 and fl.size == 0 and ts.size == 0
    ts, te, fl, flp, sc = _run(K, none, [2, 3], V)  # T = 0, U = 2
    assert sc == -np.inf and list(ts) == [-1, -1] and list(te) == [-1, -1]
    for T in (1, 2, TB - 1, TB, TB + 1, 2 * TB + 3):  # (T < TB among them)
        x = ref.quantised_lprobs(rng, T, V)
        for y in ([], [3], [3, 3], [1, 2, 1]):
            got = _run(K, x, y, V)
            _assert_equals_reference(got, x, y)
            if not y:  # U = 0: the all-blank path
                assert (got[2] == -1).all() and float(got[4]) == x[:, BLANK].sum()
    x = ref.quantised_lprobs(rng, 40, V)
    got = _run(K, x, [4, 2], V, blank=V - 1)  # another blank column
    _assert_equals_reference(got, x, [4, 2], blank=V - 1)


def test_bad_targets_give_nan_and_nothing_aligned():
    K = _need_gpu()
    TB, TS = K.ctc_viterbi_long_tile()
    rng = np.random.default_rng(5)
    V = 7
    U = TS // 2 + 40  # the bad id sits in the second state tile
    T = 2 * U
    x = ref.quantised_lprobs(rng, T, V)
    good = (np.arange(U) % (V - 1) + 1).astype(np.int32)
    for bad_id in (V, -1, 10 ** 6, BLANK):
        for pos in (0, U - 1):
            y = good.copy()
            y[pos] = bad_id
            ts, te, fl, flp, sc = _run(K, x, y, V)
            assert np.isnan(sc) and (fl == -2).all() and (ts == -1).all() and (te == -1).all() and (flp == 0).all(), (bad_id, pos)
    assert np.isfinite(_run(K, x, good, V)[4])


def test_argument_refusals(monkeypatch):
    K = _need_gpu()
    from espresso_amd import _lib

    x = torch.zeros(20, 8, dtype=torch.float32, device=DEV)
    y = torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="ea_ctc_viterbi_long_align"):
        K.ctc_viterbi_align_long(x, y, 20, 8, 8)  # blank outside the vocabulary
    with pytest.raises(RuntimeError, match="ea_ctc_viterbi_long_align"):
        K.ctc_viterbi_align_long(x, y, 20, 8, -1)
    with pytest.raises(RuntimeError, match="ea_ctc_viterbi_long_align"):
        K.ctc_viterbi_align_long(x, y, 20, 8, 0, ld=7)  # ld < V
    lib = _lib.lib()
    for T, V, U in ((-1, 8, 2), (20, 8, -1), (20, 0, 2)):
        assert lib.ea_ctc_viterbi_long_align(None, 8, 0, None, None, None, None, None, None, None, T, V, U, 0, None) != 0
    # more workspace than the device has free: refused with the figures, nothing allocated
    need = int(lib.ea_ctc_viterbi_long_workspace_bytes(20, 2))
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (need - 1, 1 << 40))
    with pytest.raises(ValueError) as e:
        K.ctc_viterbi_align_long(x, y, 20, 8, 0)
    msg = str(e.value)
    assert str(need) in msg and str(need - 1) in msg and "T = 20" in msg and "U = 2" in msg
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (need, 1 << 40))
    K.ctc_viterbi_align_long(x, y, 20, 8, 0)


# ------------------------------------------------------------------------------------------------ the tiny model
WINDOW_S, OVERLAP_S = 1.6, 0.32  # 40 and 8 encoder frames of 40 ms
G = 640


def _tiny(tmp_path):
    """(task with its front-end, model, checkpoint options of the command line) for the tiny CTC fixture model."""
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from tests.gpu_checks import build_tiny_model, load_fixture, load_ref_state

    _, sd, _, _ = load_fixture("ref_conformer_ctc_tiny")
    (tmp_path / "dict.txt").write_text("".join(f"t{i} 1\n" for i in range(35)) + "<space> 1\n")  # (the fixture's V = 40)
    block = {"_name": "speech_transformer_encoder_model", "dropout": 0.0, "layernorm_embedding": True,
             "encoder": {"embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4, "normalize_before": True,
                         "relative_positional_embeddings": True, "layer_type": "conformer", "conv_channels": "[64, 64, 16, 16]"}}
    (tmp_path / "cfg.json").write_text(json.dumps(block))
    torch.save({"model": {"encoder." + k: v for k, v in sd.items()}}, str(tmp_path / "m.pt"))
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(
        dict=str(tmp_path / "dict.txt"), autoregressive=False, criterion_name="ctc_loss"))
    task.build_frontend(torch.device(DEV))
    model = build_tiny_model("conformer").to(DEV).eval()
    load_ref_state(model, sd)
    base = ["--path", str(tmp_path / "m.pt"), "--model-config", str(tmp_path / "cfg.json"), "--dict", str(tmp_path / "dict.txt")]
    return task, model, base


def _wave(seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(16000 * seconds)
    env = 0.2 + np.abs(np.sin(np.arange(n) / 2100.0))  # louder and quieter stretches
    return np.round(rng.standard_normal(n) * 800 * env).astype(np.float32)


def _long_form(task, model):
    from espresso_amd.tools import long_form as LF

    plan = LF.LongFormPlan.from_seconds(LF.samples_per_frame(task.frontend, model), 16000, WINDOW_S, OVERLAP_S)
    assert (plan.g, plan.Tw, plan.Of, plan.Hf) == (G, 40, 8, 32)
    return LF, plan


def test_three_windows_through_the_model_equal_the_old_kernel(tmp_path):
    K = _need_gpu()
    from espresso_amd.tools.forced_aligner import LongFormCTCAligner

    task, model, _ = _tiny(tmp_path)
    LF, plan = _long_form(task, model)
    d = task.target_dictionary
    wave = _wave((2 * plan.H + 15000) / 16000.0, 6)
    assert len(plan.windows(len(wave))) == 3
    tokens = np.random.default_rng(8).integers(5, 40, size=40).tolist()
    aligner = LongFormCTCAligner(task, model, plan, d)
    encode, seen = aligner.long_form.encode, []
    aligner.long_form.encode = lambda m, w: seen.append(encode(m, w)) or seen[-1]  # (the matrix the aligner itself saw)
    r = aligner.align(wave, tokens)
    (lprobs, in_len, cuts, scores), = seen
    T, V = lprobs.shape[1], lprobs.shape[2]
    tg = torch.tensor([tokens], dtype=torch.int32, device=DEV)
    ts, te, fl, sc = K.ctc_viterbi_align(lprobs[0], tg, in_len, torch.tensor([40], dtype=torch.int32, device=DEV), 1, T, V, d.bos())
    assert r["feasible"] and r["frames"] == T == int(in_len[0]) and list(r["tokens"]) == tokens
    assert np.float32(r["score"]).view(np.int32) == sc.cpu().numpy().view(np.int32)[0]
    assert list(r["start"]) == ts[0].cpu().tolist() and list(r["end"]) == te[0].cpu().tolist()
    assert list(r["cuts"]) == cuts.cpu().tolist() and len(r["cuts"]) == 2
    assert np.array_equal(r["cut_scores"].view(np.int32), scores.cpu().numpy().view(np.int32))
    lab = [tokens[u] if u >= 0 else d.bos() for u in fl[0].cpu().tolist()]
    want = lprobs[0].cpu().numpy()[np.arange(T), lab]
    assert r["frame_lp"].dtype == np.float32 and np.array_equal(r["frame_lp"].view(np.int32), want.view(np.int32))
    assert max(r["end"]) > plan.Tw  # the recording's own frame axis, beyond one window


def test_one_window_through_the_model_equals_the_utterance_aligner(tmp_path):
    _need_gpu()
    from espresso_amd.speech_recognize import collate
    from espresso_amd.tools.forced_aligner import CTCForcedAligner, LongFormCTCAligner

    task, model, _ = _tiny(tmp_path)
    _, plan = _long_form(task, model)
    d = task.target_dictionary
    wave = _wave(1.1, 5)
    tokens = np.random.default_rng(9).integers(5, 40, size=9).tolist()
    r = LongFormCTCAligner(task, model, plan, d).align(wave, tokens)
    s = task.prepare_sample(collate([0], ["0"], [wave], torch.device(DEV)), train=False)
    want = CTCForcedAligner([model], d).align(s, [tokens])[0]
    assert r["feasible"] and want["feasible"] and len(r["cuts"]) == 0 and len(r["cut_scores"]) == 0
    assert r["frames"] == want["frames"] and np.float32(r["score"]).view(np.int32) == np.float32(want["score"]).view(np.int32)
    for key in ("tokens", "start", "end"):
        assert list(r[key]) == list(want[key]), key
    assert set(want) <= set(r)


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_long_form_ctm_and_segments(tmp_path, capsys):
    _need_gpu()
    from espresso_amd import speech_align
    from espresso_amd.data import audio_utils

    task, model, base = _tiny(tmp_path)
    _, plan = _long_form(task, model)
    rng = np.random.default_rng(10)
    waves = {"long": _wave((2 * plan.H + 15000) / 16000.0, 6), "short": _wave(1.2, 7)}
    texts = {}
    for u, n_words in (("long", 16), ("short", 3)):  # 2 - 3 tokens a word: "long" has 47 - 63 tokens for its ~87 frames
        words = [" ".join(f"t{k}" for k in rng.integers(1, 35, size=int(rng.integers(2, 4)))) for _ in range(n_words)]
        texts[u] = " <space> ".join(words)
    scp = []
    for u, w in waves.items():
        audio_utils.write_wav(str(tmp_path / f"{u}.wav"), w)
        scp.append(f"{u} {tmp_path / (u + '.wav')}\n")
    (tmp_path / "wav.scp").write_text("".join(scp))
    (tmp_path / "text").write_text("".join(f"{u} {t}\n" for u, t in texts.items()))
    seg_dir = tmp_path / "segs"
    max_s, spf = 0.8, 0.04
    capsys.readouterr()
    res = speech_align.main(base + ["--wav-scp", str(tmp_path / "wav.scp"), "--text", str(tmp_path / "text"), "--output",
                                    str(tmp_path / "word.ctm"), "--unit", "word", "--scores", str(tmp_path / "scores"), "--long-form",
                                    "--long-form-window-s", str(WINDOW_S), "--long-form-overlap-s", str(OVERLAP_S), "--segments-dir",
                                    str(seg_dir), "--segment-max-s", str(max_s), "--segment-min-silence-s", "0.04"])
    assert "long-form: 2 junctions" in capsys.readouterr().err
    assert set(res) == {"long", "short"} and all(r["feasible"] for r in res.values())
    want_words = {u: ["".join(w.split()) for w in t.split(" <space> ")] for u, t in texts.items()}
    ctm = [l.split() for l in (tmp_path / "word.ctm").read_text().splitlines()]
    for u in waves:
        lines = [l for l in ctm if l[0] == u]
        assert [l[4] for l in lines] == want_words[u]
        starts, ends = [float(l[2]) for l in lines], [float(l[2]) + float(l[3]) for l in lines]
        assert starts == sorted(starts) and all(e <= s2 + 1e-9 for e, s2 in zip(ends, starts[1:]))
        assert 0.0 <= starts[0] and ends[-1] <= len(waves[u]) / 16000.0 + spf
    assert max(float(l[2]) + float(l[3]) for l in ctm if l[0] == "long") > WINDOW_S  # times on the recording's axis, past one window
    sc = {l.split()[0]: l.split() for l in (tmp_path / "scores").read_text().splitlines()}
    assert int(sc["long"][1]) == res["long"]["frames"] and int(sc["long"][2]) == len(texts["long"].split())
    # the three segment files: same ids in the same order; times, frames, words and text agree
    seg = [l.split() for l in (seg_dir / "segments").read_text().splitlines()]
    txt = [l.split() for l in (seg_dir / "text").read_text().splitlines()]
    scs = [l.split() for l in (seg_dir / "scores").read_text().splitlines()]
    assert [l[0] for l in seg] == [l[0] for l in txt] == [l[0] for l in scs]
    max_frames = round(max_s / spf)
    for u in waves:
        mine = [k for k, l in enumerate(seg) if l[1] == u]
        assert [seg[k][0] for k in mine] == [f"{u}_{n:04d}" for n in range(len(mine))]
        assert sum((txt[k][1:] for k in mine), []) == want_words[u]  # the transcript = its segments' text, in order
        bounds = [(float(seg[k][2]), float(seg[k][3])) for k in mine]
        assert bounds[0][0] >= 0.0 and bounds[-1][1] <= res[u]["frames"] * spf + 1e-9
        assert all(a < b for a, b in bounds) and all(b1 == a2 for (_, b1), (a2, _) in zip(bounds, bounds[1:]))
        for k, (a, b) in zip(mine, bounds):
            frames, n_words, mean = int(scs[k][1]), int(scs[k][2]), float(scs[k][3])
            assert frames == round((b - a) / spf) and n_words == len(txt[k]) - 1 >= 1 and mean <= 0.0
            lo, hi = round(a / spf), round(b / spf)
            assert mean == pytest.approx(float(res[u]["frame_lp"][lo:hi].mean()), abs=1e-4)
            assert (scs[k][4:] == ["overlong"]) == (frames > max_frames)
    assert len([l for l in seg if l[1] == "long"]) >= 2  # ~90 frames against 20 per segment
