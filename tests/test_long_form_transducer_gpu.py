"""Long-form recognition for transducer models on the device (csrc/long_form.hip: ea_longform_feature_cuts,
ea_longform_stitch_rows; tools/long_form.py LongFormTransducer; speech_recognize --long-form-transducer): the feature cut kernel
against the fp64 restatement of tests/long_form_features_ref.py on every path it has, the row stitch bit for bit, and the whole
path on the tiny transducer fixture model and the command line.

The bound.  |d_fp32 - d_fp64| <= bound(D) = 4 (D + 4) 2^-24, derived in tests/long_form_features_ref.py from the header's rule
(each sum within (D + 3) 2^-24 relatively, one rounding for the quotient, d <= 2); it bounds the scores too.  A cut is compared
with the fp64 cut where the fp64 lead of the best score exceeds 2 x bound(D), which tests/test_long_form_transducer.py shows
to be every case."""
import json

import numpy as np
import pytest
import torch

from tests import long_form_features_ref as fref

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


def _cdev(counts):
    return torch.tensor(counts, dtype=torch.int32, device=DEV)


def _on_device(x64, dtype, offset):
    """x64 [Nw][Tw][ld] as a device tensor whose first element lies `offset` elements behind its allocation's start."""
    Nw, Tw, ld = x64.shape
    store = torch.zeros(Nw * Tw * ld + offset, dtype=dtype, device=DEV)
    t = store[offset:].view(Nw, Tw, ld)
    t.copy_(torch.from_numpy(x64))
    assert np.array_equal(t.double().cpu().numpy(), x64)  # (the reference saw exactly these values)
    return t


def _poison(t, counts):
    """NaN in every row >= counts[n]."""
    for n, c in enumerate(counts):
        t[n, c:] = float("nan")
    return t


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("case", fref.GPU_CASES, ids=[c[0] for c in fref.GPU_CASES])
def test_feature_cuts_and_stitched_rows_equal_the_reference(case, dtype):
    """Cuts equal the fp64 cuts, scores lie within bound(D) of the fp64 scores, and the stitched rows are the owners' bits; rows
    past a window's count hold NaN and leave no trace."""
    _need_gpu()
    from espresso_amd import kernels as K

    name, Nw, Tw, Of, D, ld, last, offset, edge, guard = case
    x64, counts, Hf, _ = fref.gpu_case(case, dtype)
    want_c, want_s, margin = fref.cuts(x64, counts, Hf, D, edge, guard)
    assert margin > 2 * fref.bound(D)
    t = _poison(_on_device(x64, DTYPES[dtype], offset), counts)
    cdev = _cdev(counts)
    got_c, got_s = K.longform_feature_cuts(t, cdev, D, Hf, edge, guard)
    assert bool(torch.isfinite(got_s).all()) and bool((got_s <= 0).all())
    err = float(np.abs(got_s.double().cpu().numpy() - np.array(want_s)).max())
    print(f"{name} {dtype}: cuts {got_c.cpu().tolist()} max |score - fp64| {err:.3e} (bound {fref.bound(D):.3e}, margin {margin:.3e})")
    assert got_c.cpu().tolist() == want_c
    assert err <= fref.bound(D)
    T = (Nw - 1) * Hf + last
    own = fref.owners(counts, want_c, Hf)
    assert len(own) == T
    src = t.view(Nw * Tw, ld)[torch.tensor([n * Tw + j for n, j in own], device=DEV)][:, :D]
    bits = torch.int16 if t.element_size() == 2 else torch.int32
    for pad in (0, 3):
        out = torch.full((T, D + pad), -7.0, dtype=t.dtype, device=DEV)
        got = K.longform_stitch_rows(t, cdev, got_c, D, Hf, T, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out[:, :D].contiguous().view(bits), src.contiguous().view(bits))
        assert bool((out[:, D:] == -7.0).all()) and not bool(torch.isnan(out).any())
    fresh = K.longform_stitch_rows(t, cdev, got_c, D, Hf, T)
    assert fresh.shape == (T, D) and torch.equal(fresh.view(bits), src.contiguous().view(bits))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_identical_overlaps_tie_to_the_middle_and_score_zero(dtype):
    _need_gpu()
    from espresso_amd import kernels as K

    rng = np.random.default_rng(5)
    D = 33
    for Tw, ov, Nw in ((16, 5, 3), (16, 4, 3), (8, 1, 2), (16, 7, 4)):
        Hf = Tw - ov
        t = _on_device(torch.from_numpy(rng.standard_normal((Nw, Tw, D + 3))).to(DTYPES[dtype]).double().numpy(), DTYPES[dtype], 0)
        for n in range(Nw - 1):
            t[n + 1, :ov] = t[n, Hf:]
        for guard in (0, 2):
            for edge in (0, 1):
                got_c, got_s = K.longform_feature_cuts(t, _cdev([Tw] * Nw), D, Hf, edge, guard)
                want = []
                for n in range(Nw - 1):
                    lo, hi = (n + 1) * Hf, (n + 1) * Hf + ov
                    cands = list(range(lo + edge, hi - edge + 1))
                    want.append(min(cands, key=lambda c: (abs(2 * c - (lo + hi)), c)) if cands else (lo + hi) // 2)
                assert got_c.cpu().tolist() == want, (Tw, ov, guard, edge)
                assert bool((got_s == 0).all())
    # all-zero rows: den == 0 gives d = 0, not NaN
    z = torch.zeros(2, 8, 16, dtype=DTYPES[dtype], device=DEV)
    got_c, got_s = K.longform_feature_cuts(z, _cdev([8, 8]), 16, 6, 0, 1)
    assert got_c.cpu().tolist() == [7] and got_s.cpu().tolist() == [0.0]


def test_one_window_launches_nothing_and_copies_the_rows():
    _need_gpu()
    from espresso_amd import kernels as K

    t = torch.randn(1, 11, 20, device=DEV).to(torch.bfloat16)
    t[0, 9:] = float("nan")
    c = _cdev([9])
    cuts, scores = K.longform_feature_cuts(t, c, 20, 11, 0, 2)
    assert cuts.numel() == 0 and scores.numel() == 0
    out = K.longform_stitch_rows(t, c, cuts, 20, 11, 9)
    assert torch.equal(out.view(torch.int16), t[0, :9].contiguous().view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32], ids=["2-byte", "4-byte"])
def test_stitch_rows_moves_bytes_under_hand_made_cuts(dtype):
    """Raw integer elements (no float among them), and cuts that no cut kernel would make: a frame whose owner does not hold it is
    left unwritten and nothing is read past a window."""
    _need_gpu()
    from espresso_amd import kernels as K

    g = torch.Generator(device="cpu").manual_seed(3)
    t = torch.randint(-30000, 30000, (3, 8, 10), generator=g, dtype=torch.int64).to(dtype).to(DEV)
    out = torch.full((20, 12), -7, dtype=dtype, device=DEV)
    K.longform_stitch_rows(t, _cdev([8, 2, 99]), torch.tensor([6, 12], dtype=torch.int32, device=DEV), 10, 6, 20, out=out)
    # window 0 owns frames 0..5 (rows 0..5), window 1 frames 6..11 (rows 0..5, holds 2 of them), window 2 frames 12..19 (rows 0..7)
    assert torch.equal(out[:6, :10], t[0, :6]) and torch.equal(out[6:8, :10], t[1, :2]) and torch.equal(out[12:, :10], t[2])
    assert bool((out[8:12] == -7).all()) and bool((out[:, 10:] == -7).all())


def test_bad_arguments_are_refused():
    _need_gpu()
    from espresso_amd import kernels as K

    t = torch.zeros(3, 8, 10, dtype=torch.float32, device=DEV)
    c = _cdev([8, 8, 8])
    with pytest.raises(RuntimeError, match="ea_longform_feature_cuts"):
        K.longform_feature_cuts(t, c, 10, 9, -1, 0)  # a negative edge
    with pytest.raises(RuntimeError, match="ea_longform_feature_cuts"):
        K.longform_feature_cuts(t, c, 10, 8, 0, 0)  # no overlap at all
    with pytest.raises(RuntimeError, match="ea_longform_feature_cuts"):
        K.longform_feature_cuts(t, c, 10, 0, 0, 0)  # no hop
    cuts, _ = K.longform_feature_cuts(t, c, 10, 6, 0, 0)
    with pytest.raises(RuntimeError, match="ea_longform_stitch_rows"):
        K.longform_stitch_rows(t, c, cuts, 10, 3, 14)  # Tw >= 2 Hf: three windows share a frame
    with pytest.raises(RuntimeError, match="ea_longform_stitch_rows"):
        K.longform_stitch_rows(t, c, cuts, 10, 6, 21)  # more frames than the windows hold
    # counts beyond the window, and cuts that give a frame to a window that does not hold it: nothing is read out of bounds
    out = torch.full((20, 10), -7.0, dtype=torch.float32, device=DEV)
    K.longform_stitch_rows(t, _cdev([8, 2, 99]), torch.tensor([6, 12], dtype=torch.int32, device=DEV), 10, 6, 20, out=out)
    assert bool((out[8:12] == -7.0).all()) and bool((out[:8] != -7.0).all()) and bool((out[12:] != -7.0).all())


# ------------------------------------------------------------------------------------------------ the tiny model
WINDOW_S, OVERLAP_S = 1.6, 0.32  # 40 and 8 encoder frames of 40 ms
G = 640
MODEL = "speech_transformer_transducer_base"


def _tiny(tmp_path):
    """(task with its front-end, model, checkpoint options of the command line) for the tiny transducer fixture model."""
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from tests.gpu_checks import build_tiny_transducer, load_fixture

    _, sd, _, _ = load_fixture("ref_conformer_transducer_tiny")
    (tmp_path / "dict.txt").write_text("".join(f"t{i} 1\n" for i in range(35)) + "<space> 1\n")  # (the fixture's V = 40)
    block = {"_name": MODEL, "dropout": 0.0, "attention_dropout": 0.0, "activation_dropout": 0.0, "joint_dim": 64,
             "max_source_positions": 3600, "max_target_positions": 200,
             "encoder": {"embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4, "normalize_before": True,
                         "relative_positional_embeddings": True, "layer_type": "conformer", "conv_channels": "[64, 64, 16, 16]"},
             "decoder": {"embed_dim": 48, "hidden_size": 64, "layers": 2, "residual": True, "dropout_in": 0.0, "dropout_out": 0.0}}
    (tmp_path / "cfg.json").write_text(json.dumps(block))
    torch.save({"model": dict(sd)}, str(tmp_path / "m.pt"))
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(
        dict=str(tmp_path / "dict.txt"), autoregressive=False, criterion_name="transducer_loss"))
    task.build_frontend(torch.device(DEV))
    model = build_tiny_transducer().to(DEV)
    missing, unexpected = model.load_state_dict(model.upgrade_state_dict_named(dict(sd), ""), strict=False)
    assert not missing and not unexpected
    model.eval()
    base = ["--path", str(tmp_path / "m.pt"), "--model", MODEL, "--model-config", str(tmp_path / "cfg.json"), "--dict", str(tmp_path / "dict.txt")]
    return task, model, base


def _wave(seconds, seed, rate=16000):
    rng = np.random.default_rng(seed)
    n = int(rate * seconds)
    env = 0.2 + np.abs(np.sin(np.arange(n) / (2100.0 * rate / 16000)))  # louder and quieter stretches
    return np.round(rng.standard_normal(n) * 800 * env).astype(np.float32)


def _long_form(task, model, **kw):
    from espresso_amd.tools import long_form as LF

    plan = LF.LongFormPlan.from_seconds(LF.samples_per_frame(task.frontend, model.encoder), 16000, WINDOW_S, OVERLAP_S, **kw)
    assert (plan.g, plan.Tw, plan.Of, plan.Hf) == (G, 40, 8, 32)
    return LF, LF.LongFormTransducer(task, plan)


def _normal_pass(task, model, waves):
    """The offline encoder pass of a batch of utterances as speech_recognize runs it: (`_x_bt` [B * T'][D], lengths, sample)."""
    from espresso_amd.speech_recognize import collate

    names = [str(i) for i in range(len(waves))]
    s = task.prepare_sample(collate(list(range(len(waves))), names, waves, torch.device(DEV)), train=False)
    with torch.no_grad():
        enc = model.encoder(s["net_input"]["src_tokens"], s["net_input"]["src_lengths"])
    return enc["_x_bt"][0], enc["src_lengths"][0], s


def _bits(x):
    return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


def _decoders(d):
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder
    from espresso_amd.tools.transducer_greedy_decoder import TransducerGreedyDecoder

    return (lambda m: TransducerGreedyDecoder([m], d), lambda m: TransducerFrameBeamDecoder([m], d, beam_size=4, nbest=2, token_times=True))


def test_one_window_equals_the_normal_pass(tmp_path):
    _need_gpu()
    task, model, _ = _tiny(tmp_path)
    LF, lf = _long_form(task, model)
    d = task.target_dictionary
    for seconds in (1.1, WINDOW_S):
        wave = _wave(seconds, 5)
        X, enc_len, cuts, scores = lf.encode(model, wave)
        x, lens, sample = _normal_pass(task, model, [wave])
        assert cuts.numel() == 0 and scores.numel() == 0 and enc_len.cpu().tolist() == lens.cpu().tolist()
        assert X.shape == x.shape and X.dtype == x.dtype and torch.equal(_bits(X), _bits(x))
        shim = LF.LongFormTransducerModel(model, lf, search=(4, 2, False, True))
        for make in _decoders(d):
            got = make(shim).generate([shim], {"net_input": shim.net_input(wave)})
            want = make(model).generate([model], sample)
            assert len(got) == len(want) == 1 and len(got[0]) == len(want[0]) >= 1
            for a, b in zip(got[0], want[0]):
                assert a["tokens"].tolist() == b["tokens"].tolist()
                assert torch.equal(a["score"].cpu().view(torch.int32), b["score"].cpu().view(torch.int32))
                if "times" in b:
                    assert a["times"].tolist() == b["times"].tolist()
        assert shim.junctions and all(c.numel() == 0 for c, _ in shim.junctions) and shim.worst_score() is None


def test_three_windows_rows_come_from_the_windows_own_passes(tmp_path):
    _need_gpu()
    task, model, _ = _tiny(tmp_path)
    LF, lf = _long_form(task, model)
    plan = lf.plan
    wave = _wave((2 * plan.H + 15000) / 16000.0, 6)
    wins = plan.windows(len(wave))
    assert len(wins) == 3 and plan.O < wins[-1][1] < plan.W
    X, enc_len, cuts, scores = lf.encode(model, wave)
    counts = LF.window_frames(task.frontend, model.encoder, plan, len(wave))
    T = 2 * plan.Hf + counts[-1]
    assert counts[:2] == [plan.Tw] * 2 and enc_len.cpu().tolist() == [T] and X.shape[0] == T
    assert T == int(model.encoder.output_lengths(task.frontend.num_frames(len(wave))))
    # the windows' own normal pass: one batch, longest first, as the planner makes it
    x, lens, _ = _normal_pass(task, model, [wave[a: a + ln] for a, ln in wins])
    assert lens.cpu().tolist() == counts
    Tp = x.shape[0] // 3
    cut_list = cuts.cpu().tolist()
    for n, c in enumerate(cut_list):
        assert (n + 1) * plan.Hf + plan.edge <= c <= min(n * plan.Hf + counts[n], (n + 1) * plan.Hf + counts[n + 1]) - plan.edge
    assert bool((scores <= 0).all()) and bool((scores >= -2).all())
    own = fref.owners(counts, cut_list, plan.Hf)
    src = x[torch.tensor([n * Tp + j for n, j in own], device=DEV)]
    assert torch.equal(_bits(X), _bits(src))
    # the reference rule on the same encoder outputs picks the same cuts where it has a margin, and the same scores within the bound
    D = x.shape[1]
    want_c, want_s, margin = fref.cuts(x.view(3, Tp, D).double().cpu().numpy(), counts, plan.Hf, D, plan.edge, plan.guard)
    err = float(np.abs(scores.double().cpu().numpy() - np.array(want_s)).max())
    print(f"tiny transducer: cuts {cut_list} scores {scores.cpu().tolist()} max |score - fp64| {err:.3e} margin {margin:.3e}")
    assert err <= fref.bound(D)
    if margin > 2 * fref.bound(D):
        assert cut_list == want_c


# ------------------------------------------------------------------------------------------------ the command line
def _write_scp(tmp_path, waves, rate=16000):
    from espresso_amd.data import audio_utils

    lines = []
    for u, w in waves.items():
        p = str(tmp_path / f"{u}.wav")
        audio_utils.write_wav(p, w, rate)
        lines.append(f"{u} {p}\n")
    (tmp_path / "wav.scp").write_text("".join(lines))
    return ["--wav-scp", str(tmp_path / "wav.scp")]


LFT_OPTS = ["--long-form-transducer", "--long-form-window-s", str(WINDOW_S), "--long-form-overlap-s", str(OVERLAP_S)]


def test_cli_recognize_long_form_transducer(tmp_path, capsys):
    _need_gpu()
    from espresso_amd import speech_recognize

    task, model, base = _tiny(tmp_path)
    LF, lf = _long_form(task, model)
    wave = _wave((2 * lf.plan.H + 15000) / 16000.0, 6)
    seconds = len(wave) / 16000.0
    args = base + _write_scp(tmp_path, {"rec": wave})
    capsys.readouterr()
    speech_recognize.main(args + ["--search", "transducer_frame_beam", "--beam", "4", "--ctm", str(tmp_path / "out.ctm")] + LFT_OPTS)
    cap = capsys.readouterr()
    hyp = [l for l in cap.out.splitlines() if l.startswith("H-")]
    assert len(hyp) == 1 and hyp[0].startswith("H-rec\t")
    assert "long-form-transducer: 2 junctions, lowest cut score" in cap.err
    text = hyp[0].split("\t")[1].split()
    ctm = [l.split() for l in (tmp_path / "out.ctm").read_text().splitlines()]
    assert len(ctm) == len(text) >= 3 and all(l[0] == "rec" for l in ctm)
    starts = [float(l[2]) for l in ctm]
    assert starts == sorted(starts) and len(set(starts)) == len(starts)
    assert 0.0 <= starts[0] and starts[-1] + float(ctm[-1][3]) <= seconds + 0.04
    assert starts[-1] > WINDOW_S  # times on the recording's own axis, beyond one window
    # greedy decoding of the same recording: one hypothesis, the tokens of the decoder run through the shim
    speech_recognize.main(args + ["--search", "transducer_greedy"] + LFT_OPTS)
    greedy = [l for l in capsys.readouterr().out.splitlines() if l.startswith("H-")]
    assert len(greedy) == 1
    from espresso_amd.tools.transducer_greedy_decoder import TransducerGreedyDecoder

    d = task.target_dictionary
    shim = LF.LongFormTransducerModel(model, lf)
    dec = TransducerGreedyDecoder([shim], d)
    want = dec.generate([shim], {"net_input": shim.net_input(wave)})[0][0]["tokens"].tolist()
    assert greedy[0].split("\t")[1].split() == [d[k] for k in want if k not in dec.symbols_to_strip_from_output and k != d.pad()]


def test_cli_recognize_long_form_transducer_at_8_khz(tmp_path, capsys):
    """The same duration at 8 kHz: the recording goes through the device resampler once, then the same path."""
    _need_gpu()
    from espresso_amd import speech_recognize

    _, _, base = _tiny(tmp_path)
    wave = _wave((2 * (40 - 8) * G + 15000) / 16000.0, 6, rate=8000)
    args = base + _write_scp(tmp_path, {"rec": wave}, rate=8000)
    capsys.readouterr()
    speech_recognize.main(args + ["--search", "transducer_frame_beam", "--beam", "4"] + LFT_OPTS)
    cap = capsys.readouterr()
    hyp = [l for l in cap.out.splitlines() if l.startswith("H-")]
    assert len(hyp) == 1 and hyp[0].startswith("H-rec\t")
    assert "long-form-transducer: 2 junctions" in cap.err


def test_cli_refuses_a_ctc_checkpoint(tmp_path):
    _need_gpu()
    from espresso_amd import speech_recognize

    _, _, base = _tiny(tmp_path)
    args = base + _write_scp(tmp_path, {"rec": _wave(0.5, 1)})
    i = args.index("--model")
    args[i + 1] = "speech_transformer_encoder_model"
    with pytest.raises(NotImplementedError, match="--long-form-transducer is implemented for transducer models, not for the ctc model"):
        speech_recognize.main(args + ["--search", "transducer_greedy"] + LFT_OPTS)
