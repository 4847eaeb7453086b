"""Long-form recognition on the device (csrc/long_form.hip, tools/long_form.py, speech_recognize / speech_kws --long-form):
the cut kernel against the fp64 reference of tests/long_form_ref.py, exact ties, the stitch bit for bit against
`kernels.log_softmax` and per element against fp64, and the whole path on the tiny CTC fixture model and the command lines.

The log-softmax bound.  `ea_log_softmax_*` itself, on the inputs of these tests (logits ~ 3 N(0, 1), V <= 5003, bf16 and fp32),
differs from fp64 by at most 1.651e-6 (LSM_MEASURED, rounded up; every test that uses the bound prints what it sees: 3.5e-7 at
V = 5 up to 1.65e-6 at V = 257, 1.58e-6 at V ~ 5000); the long-form kernels must do the same arithmetic, so they get twice that,
3.32e-6, and no more.  Seen on the same run: cut scores within 1.34e-6 of fp64, stitched rows within 1.62e-6."""
import json
import math

import numpy as np
import pytest
import torch

from tests import long_form_ref as ref

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
BLANK = 0
LSM_MEASURED = 1.66e-6  # max |ea_log_softmax - fp64| over every input of this file, measured on an MI355X: 1.651e-6 (V 257, fp32)
LSM_TOL = 2 * LSM_MEASURED


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


def _logits(rng, Nw, Tw, V, ld, dtype, scale=3.0, offset=0):
    """Device logits [Nw][Tw][ld] (columns >= V hold large values that must not be read as vocabulary) and their exact fp64
    values.  offset: elements by which the tensor's first element is moved off its allocation's 16-byte boundary."""
    x = rng.standard_normal((Nw, Tw, ld)) * scale
    x[:, :, V:] = 50.0
    store = torch.zeros(Nw * Tw * ld + offset, dtype=dtype, device=DEV)
    t = store[offset:].view(Nw, Tw, ld)
    t.copy_(torch.from_numpy(x))
    return t, t.double().cpu().numpy()


def _counts(Nw, Tw, last):
    return [Tw] * (Nw - 1) + [last]


def _cdev(counts):
    return torch.tensor(counts, dtype=torch.int32, device=DEV)


def _lsm_error(K, t, x64, V):
    """max |ea_log_softmax - fp64| over the rows of t, and the kernel's rows [Nw * Tw][V]."""
    Nw, Tw, ld = t.shape
    rows = K.log_softmax(t.view(Nw * Tw, ld), Nw * Tw, V, ld)
    err = float(np.abs(rows.double().cpu().numpy() - ref.log_softmax64(x64.reshape(Nw * Tw, ld)[:, :V])).max())
    return err, rows


CUT_SHAPES = [(Tw, ov, Nw, short) for Tw in (8, 16) for ov in (1, 2, 5) for Nw in (2, 3, 5) for short in (False, True)]


def _cut_case(V, ld, dtype, Tw, ov, Nw, short):
    """Seeded inputs of one shape such that, for every (guard, edge) of the test, the reference's best score leads the next lower
    one by more than 1e-3 at every junction: the first seed that qualifies, found on the host."""
    Hf = Tw - ov
    counts = _counts(Nw, Tw, ov + 1 if short else Tw)
    for seed in range(64):
        rng = np.random.default_rng([seed, V, ld, Tw, ov, Nw, int(short)])
        x = rng.standard_normal((Nw, Tw, ld)) * 3.0
        x[:, :, V:] = 50.0
        x = torch.from_numpy(x).to(dtype).double().numpy()  # the values the device will hold
        want = {(g, e): ref.cuts(x, counts, Hf, V, BLANK, e, g) for g in (0, 2) for e in (0, 1)}
        if all(m > 1e-3 for _, _, m in want.values()):
            return x, counts, Hf, want
    raise AssertionError("no seed gives every junction a margin above 1e-3")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V,pad", [(5, 0), (5, 3), (33, 0), (33, 3), (257, 0), (257, 3)])
def test_cuts_equal_the_fp64_reference(V, pad, dtype):
    """Candidates whose guard ranges cover the same overlap frames (every candidate, once the overlap is no longer than the
    guard) take their score from the same b(j) and tie exactly; the margin of 1e-3 is asserted between the best score and the
    next lower one, and the tie rule, which the reference restates, decides among equals."""
    _need_gpu()
    from espresso_amd import kernels as K

    ld = V + pad
    worst, lsm = 0.0, 0.0
    for Tw, ov, Nw, short in CUT_SHAPES:
        x, counts, Hf, want = _cut_case(V, ld, dtype, Tw, ov, Nw, short)
        t = torch.from_numpy(x).to(dtype).to(DEV)
        assert np.array_equal(t.double().cpu().numpy(), x)
        lsm = max(lsm, _lsm_error(K, t, x, V)[0])
        for (guard, edge), (cuts, scores, margin) in want.items():
            assert margin > 1e-3
            got_c, got_s = K.longform_cuts(t, _cdev(counts), V, Hf, BLANK, edge, guard)
            assert got_c.cpu().tolist() == cuts, (Tw, ov, Nw, short, guard, edge)
            err = float(np.abs(got_s.double().cpu().numpy() - np.array(scores)).max())
            worst = max(worst, err)
            assert err <= LSM_TOL, (Tw, ov, Nw, short, guard, edge, err)
    print(f"V {V} ld {ld} {dtype}: max |score - fp64| {worst:.3e}; ea_log_softmax itself {lsm:.3e} (bound {LSM_TOL:.1e})")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_ties_go_to_the_middle_then_to_the_smaller_cut(dtype):
    """Every overlap row of both windows holds the same bits, so every b(j) and every score is the same float."""
    _need_gpu()
    from espresso_amd import kernels as K

    rng = np.random.default_rng(3)
    V = 33
    for Tw, ov, Nw in ((16, 5, 3), (16, 4, 3), (8, 2, 2), (8, 1, 2), (16, 7, 4)):
        Hf = Tw - ov
        t, _ = _logits(rng, Nw, Tw, V, V + 3, dtype)
        row = t[0, 0].clone()
        for n in range(Nw - 1):
            t[n, Hf:] = row
            t[n + 1, :ov] = row
        counts = _counts(Nw, Tw, Tw)
        for guard in (0, 2):
            for edge in (0, 1):
                got_c, got_s = K.longform_cuts(t, _cdev(counts), V, Hf, BLANK, edge, guard)
                want = []
                for n in range(Nw - 1):
                    lo, hi = (n + 1) * Hf, (n + 1) * Hf + ov
                    cands = list(range(lo + edge, hi - edge + 1))
                    want.append(min(cands, key=lambda c: (abs(2 * c - (lo + hi)), c)) if cands else (lo + hi) // 2)
                assert got_c.cpu().tolist() == want, (Tw, ov, guard, edge)
                assert len(set(got_s.cpu().numpy().view(np.int32).tolist())) == 1
        if ov == 5:  # lo + hi is odd: two cuts are equally near the middle, the smaller one wins
            got_c, _ = K.longform_cuts(t, _cdev(counts), V, Hf, BLANK, 0, 0)
            assert got_c.cpu().tolist() == [(n + 1) * Hf + 2 for n in range(Nw - 1)]


STITCH_SHAPES = [  # V, ld, Tw, ov, Nw, last, offset (elements off the 16-byte boundary)
    (5, 5, 8, 1, 3, 8, 0), (5, 8, 8, 2, 2, 3, 0), (33, 36, 16, 5, 3, 6, 0), (257, 257, 16, 2, 5, 16, 0), (257, 264, 16, 5, 2, 9, 1),
    (5000, 5000, 16, 5, 3, 7, 0), (4099, 4104, 8, 2, 2, 8, 0), (5003, 5008, 8, 2, 3, 3, 3), (33, 33, 8, 1, 1, 8, 0), (300, 304, 16, 5, 1, 11, 0),
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", STITCH_SHAPES, ids=lambda s: "V{}ld{}Tw{}ov{}Nw{}last{}off{}".format(*s))
def test_stitch_rows_are_the_log_softmax_rows(shape, dtype):
    """Every stitched row has the bits `kernels.log_softmax` gives its source row, and is within LSM_TOL of fp64; columns >= V
    of a padded output stay as they were; rows that the cuts discard, and the rows past a short last window, hold NaN and leave
    no trace.  One window: no junction, a plain copy.  Measured on an MI355X: ea_log_softmax_* itself is within 1.651e-6 of fp64 on
    the inputs of this file (1.62e-6 on this test's), so the bound is 3.32e-6; the stitched rows were within 1.62e-6."""
    _need_gpu()
    from espresso_amd import kernels as K

    V, ld, Tw, ov, Nw, last, offset = shape
    Hf = Tw - ov if Nw > 1 else Tw
    rng = np.random.default_rng([V, ld, Tw, ov, Nw])
    t, x64 = _logits(rng, Nw, Tw, V, ld, dtype, offset=offset)
    counts = _counts(Nw, Tw, last)
    T = (Nw - 1) * Hf + last
    cdev = _cdev(counts)
    cuts, scores = K.longform_cuts(t, cdev, V, Hf, BLANK, 0, 1)
    cut_list = cuts.cpu().tolist()
    if Nw > 1:
        want_c, want_s, margin = ref.cuts(x64, counts, Hf, V, BLANK, 0, 1)
        assert np.abs(scores.double().cpu().numpy() - np.array(want_s)).max() <= LSM_TOL
        if margin > 1e-3:  # (the shapes of this test are not seeded for a margin: equality where the reference has one)
            assert cut_list == want_c
    else:
        assert cuts.numel() == 0 and scores.numel() == 0
    own = ref.owners(counts, cut_list, Hf)
    assert len(own) == T
    lsm, rows = _lsm_error(K, t, x64, V)
    print(f"{shape} {dtype}: ea_log_softmax itself {lsm:.3e}")
    assert lsm <= LSM_MEASURED, f"ea_log_softmax itself is off by {lsm:.3e}: LSM_MEASURED is stale"
    # poison everything the stitch must not use
    used = np.zeros((Nw, Tw), dtype=bool)
    for n, j in own:
        used[n, j] = True
    poisoned = t.clone()
    poisoned[torch.from_numpy(~used).to(DEV)] = float("nan")
    want64 = ref.stitch(x64, counts, cut_list, Hf, V)
    worst = 0.0
    for ldo in (V, V + 5):
        out = torch.full((T, ldo), -7.0, dtype=torch.float32, device=DEV)
        got = K.longform_stitch(poisoned, cdev, cuts, V, Hf, T, out=out)
        assert got.data_ptr() == out.data_ptr()
        src = rows[torch.tensor([n * Tw + j for n, j in own], device=DEV)]
        assert torch.equal(out[:, :V].view(torch.int32), src.view(torch.int32))
        assert bool((out[:, V:] == -7.0).all())
        worst = max(worst, float(np.abs(out[:, :V].double().cpu().numpy() - want64).max()))
    assert worst <= LSM_TOL
    fresh = K.longform_stitch(poisoned, cdev, cuts, V, Hf, T)
    assert fresh.shape == (T, V) and torch.equal(fresh.view(torch.int32), out[:, :V].contiguous().view(torch.int32))
    if Nw == 1:
        assert torch.equal(fresh.view(torch.int32), rows[:T].view(torch.int32))
    print(f"{shape} {dtype}: max |stitched - fp64| {worst:.3e}; ea_log_softmax itself {lsm:.3e} (bound {LSM_TOL:.1e})")


def test_bad_arguments_are_refused():
    _need_gpu()
    from espresso_amd import kernels as K

    t = torch.zeros(3, 8, 10, dtype=torch.float32, device=DEV)
    c = _cdev([8, 8, 8])
    with pytest.raises(RuntimeError, match="ea_longform_cuts"):
        K.longform_cuts(t, c, 10, 9, 10, 0, 0)  # blank outside the vocabulary
    with pytest.raises(RuntimeError, match="ea_longform_cuts"):
        K.longform_cuts(t, c, 10, 8, 0, 0, 0)  # no overlap at all
    cuts, _ = K.longform_cuts(t, c, 10, 6, 0, 0, 0)
    with pytest.raises(RuntimeError, match="ea_longform_stitch"):
        K.longform_stitch(t, c, cuts, 10, 3, 14)  # Tw >= 2 Hf: three windows share a frame
    with pytest.raises(RuntimeError, match="ea_longform_stitch"):
        K.longform_stitch(t, c, cuts, 10, 6, 21)  # more frames than the windows hold
    # counts beyond the window, and cuts that give a frame to a window that does not hold it: nothing is read out of bounds
    out = torch.full((20, 10), -7.0, dtype=torch.float32, device=DEV)
    K.longform_stitch(t, _cdev([8, 2, 99]), torch.tensor([6, 12], dtype=torch.int32, device=DEV), 10, 6, 20, out=out)
    assert bool((out[8:12] == -7.0).all()) and bool((out[:8] != -7.0).all()) and bool((out[12:] != -7.0).all())


# ------------------------------------------------------------------------------------------------ the tiny model
WINDOW_S, OVERLAP_S = 1.6, 0.32  # 40 and 8 encoder frames of 40 ms
G = 640


def _tiny(tmp_path, cmvn=None):
    """(task with its front-end, model, checkpoint options of the command lines) for the tiny CTC fixture model."""
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


def _long_form(task, model, **kw):
    from espresso_amd.tools import long_form as LF

    plan = LF.LongFormPlan.from_seconds(LF.samples_per_frame(task.frontend, model), 16000, WINDOW_S, OVERLAP_S, **kw)
    assert (plan.g, plan.Tw, plan.Of, plan.Hf) == (G, 40, 8, 32)
    return LF, LF.LongFormCTC(task, plan, task.target_dictionary.bos())


def _normal_pass(task, model, waves):
    """The offline forward of a batch of utterances as speech_recognize runs it: (log-probs [B][T][V], lengths, features)."""
    from espresso_amd.speech_recognize import collate

    names = [str(i) for i in range(len(waves))]
    s = task.prepare_sample(collate(list(range(len(waves))), names, waves, torch.device(DEV)), train=False)
    with torch.no_grad():
        out = model(**s["net_input"])
        lp = model.get_normalized_probs(out, log_probs=True).transpose(0, 1)
    return lp, out["src_lengths"][0], s


def test_one_window_equals_the_normal_pass(tmp_path):
    _need_gpu()
    from espresso_amd.tools.ctc_decoder import CTCDecoder
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder

    task, model, _ = _tiny(tmp_path)
    LF, lf = _long_form(task, model)
    d = task.target_dictionary
    for seconds in (1.1, WINDOW_S):
        wave = _wave(seconds, 5)
        lprobs, in_len, cuts, scores = lf.encode(model, wave)
        lp, lens, sample = _normal_pass(task, model, [wave])
        assert cuts.numel() == 0 and scores.numel() == 0 and in_len.cpu().tolist() == lens.cpu().tolist()
        assert lprobs.shape == lp.shape and torch.equal(lprobs.view(torch.int32), lp.contiguous().view(torch.int32))
        shim = LF.LongFormModel(model, lf)
        for make in (lambda m: CTCDecoder([m], d), lambda m: CTCPrefixBeamSearchDecoder([m], d, beam_size=4, nbest=2, token_times=True)):
            got = make(shim).generate([shim], {"net_input": {"wave": wave}})
            want = make(model).generate([model], sample)
            assert len(got) == len(want) == 1 and len(got[0]) == len(want[0])
            for a, b in zip(got[0], want[0]):
                assert a["tokens"].tolist() == b["tokens"].tolist()
                assert torch.equal(a["score"].view(torch.int32), b["score"].view(torch.int32))
                if "times" in b:
                    assert a["times"].tolist() == b["times"].tolist()


def test_three_windows_rows_come_from_the_windows_own_passes(tmp_path):
    _need_gpu()
    task, model, _ = _tiny(tmp_path)
    LF, lf = _long_form(task, model)
    plan = lf.plan
    wave = _wave((2 * plan.H + 15000) / 16000.0, 6)
    wins = plan.windows(len(wave))
    assert len(wins) == 3 and plan.O < wins[-1][1] < plan.W
    lprobs, in_len, cuts, scores = lf.encode(model, wave)
    counts = LF.window_frames(task.frontend, model, plan, len(wave))
    T = 2 * plan.Hf + counts[-1]
    assert counts[:2] == [plan.Tw] * 2 and in_len.cpu().tolist() == [T] and lprobs.shape[:2] == (1, T)
    assert T == int(model.output_lengths(task.frontend.num_frames(len(wave))))
    # the windows' own normal pass: one batch, longest first, as the planner makes it
    lp, lens, sample = _normal_pass(task, model, [wave[a: a + ln] for a, ln in wins])
    assert lens.cpu().tolist() == counts
    cut_list = cuts.cpu().tolist()
    for n, c in enumerate(cut_list):
        assert (n + 1) * plan.Hf + plan.edge <= c <= min(n * plan.Hf + counts[n], (n + 1) * plan.Hf + counts[n + 1]) - plan.edge
    assert bool((scores <= 0).all())
    own = ref.owners(counts, cut_list, plan.Hf)
    src = torch.stack([lp[n, j] for n, j in own])
    assert torch.equal(lprobs[0].view(torch.int32), src.contiguous().view(torch.int32))
    # the reference rule on the same logits picks the same cuts (fp64 on the log-probs: log-softmax of log-probs is itself)
    want_c, want_s, margin = ref.cuts(lp.double().cpu().numpy(), counts, plan.Hf, lp.shape[2], lf.blank, plan.edge, plan.guard)
    if margin > 1e-3:
        assert cut_list == want_c
    # the grid on the device: front-end frame f of window n is the recording's frame n * H / 160 + f, bit for bit
    _, _, whole = _normal_pass(task, model, [wave])
    feats, wfeats = whole["net_input"]["src_tokens"][0], sample["net_input"]["src_tokens"]
    for n, (a, ln) in enumerate(wins):
        nf = task.frontend.num_frames(ln)
        assert torch.equal(wfeats[n, :nf].view(torch.int32), feats[n * plan.H // 160: n * plan.H // 160 + nf].view(torch.int32)), n


# ------------------------------------------------------------------------------------------------ the command lines
def _write_scp(tmp_path, waves):
    from espresso_amd.data import audio_utils

    lines = []
    for u, w in waves.items():
        p = str(tmp_path / f"{u}.wav")
        audio_utils.write_wav(p, w)
        lines.append(f"{u} {p}\n")
    (tmp_path / "wav.scp").write_text("".join(lines))
    return ["--wav-scp", str(tmp_path / "wav.scp")]


LF_OPTS = ["--long-form", "--long-form-window-s", str(WINDOW_S), "--long-form-overlap-s", str(OVERLAP_S)]


def test_cli_recognize_long_form(tmp_path, capsys):
    _need_gpu()
    from espresso_amd import speech_recognize

    task, model, base = _tiny(tmp_path)
    _, lf = _long_form(task, model)
    wave = _wave((2 * lf.plan.H + 15000) / 16000.0, 6)
    seconds = len(wave) / 16000.0
    base = base + _write_scp(tmp_path, {"rec": wave})
    capsys.readouterr()
    speech_recognize.main(base + ["--search", "ctc_beam", "--beam", "4", "--ctm", str(tmp_path / "out.ctm")] + LF_OPTS)
    cap = capsys.readouterr()
    hyp = [l for l in cap.out.splitlines() if l.startswith("H-")]
    assert len(hyp) == 1 and hyp[0].startswith("H-rec\t")
    assert "long-form: 2 junctions" in cap.err
    text = hyp[0].split("\t")[1].split()
    ctm = [l.split() for l in (tmp_path / "out.ctm").read_text().splitlines()]
    assert len(ctm) == len(text) >= 3 and all(l[0] == "rec" for l in ctm)
    starts = [float(l[2]) for l in ctm]
    assert starts == sorted(starts) and len(set(starts)) == len(starts)
    assert 0.0 <= starts[0] and starts[-1] + float(ctm[-1][3]) <= seconds + 0.04
    assert starts[-1] > WINDOW_S  # times on the recording's own axis, beyond one window
    # greedy decoding of the same recording: one hypothesis as well, the text of the stitched log-probs' best path
    speech_recognize.main(base + ["--search", "ctc"] + LF_OPTS)
    greedy = [l for l in capsys.readouterr().out.splitlines() if l.startswith("H-")]
    assert len(greedy) == 1
    lprobs, _, _, _ = lf.encode(model, wave)
    want = ref.greedy(lprobs[0].cpu().numpy(), lf.blank)
    d = task.target_dictionary
    assert greedy[0].split("\t")[1].split() == [d[k] for k in want if k not in (d.eos(), d.pad())]


def test_cli_kws_long_form_reports_global_time(tmp_path, capsys):
    _need_gpu()
    from espresso_amd import speech_kws

    task, model, base = _tiny(tmp_path)
    _, lf = _long_form(task, model)
    wave = _wave((2 * lf.plan.H + 15000) / 16000.0, 6)
    base = base + _write_scp(tmp_path, {"rec": wave})
    lprobs, _, cuts, _ = lf.encode(model, wave)
    d = task.target_dictionary
    # the keyword: on noise the model's greedy path is one token throughout, so the planted keyword is the token that comes
    # nearest to the greedy one at some frame of the third window, past the last cut, with a threshold just below its ratio there:
    # a one-token keyword scores d_t = lp[t][token] - max lp[t] at frame t and nothing else
    last_cut = int(cuts[-1])
    assert last_cut > lf.plan.Tw
    dmat = (lprobs[0] - lprobs[0].max(dim=1, keepdim=True).values).double().cpu().numpy()
    names = [k for k in range(dmat.shape[1]) if d[k].startswith("t") and k != lf.blank]
    sub = dmat[last_cut + 1:, names]
    sub[sub == 0.0] = -np.inf  # not the greedy token itself
    t_rel, k_rel = np.unravel_index(np.argmax(sub), sub.shape)
    t_star, tok, theta = last_cut + 1 + int(t_rel), names[int(k_rel)], float(np.exp(sub[t_rel, k_rel]) * 0.99)
    assert 0.0 < theta < 1.0
    (tmp_path / "kw.txt").write_text(f"{d[tok]}\t{theta!r}\n")
    res = speech_kws.main(base + ["--keywords", str(tmp_path / "kw.txt"), "--hold-ms", "0", "--output", str(tmp_path / "hits.txt")] + LF_OPTS)
    assert set(res) == {"rec"}
    assert any(h["start"] <= t_star <= h["end"] for h in res["rec"]), (t_star, res["rec"])
    lines = [l.split("\t") for l in (tmp_path / "hits.txt").read_text().splitlines()]
    spans = [(round(float(l[1]) / 0.04), round(float(l[2]) / 0.04)) for l in lines]  # 40 ms per encoder frame; end_s = (end + 1) frames
    assert any(a <= t_star < b and a > lf.plan.Tw for a, b in spans), (t_star, spans)  # beyond one window: the recording's own axis


def test_cli_refusals(tmp_path):
    _need_gpu()
    from espresso_amd import speech_recognize

    _, _, base = _tiny(tmp_path)
    base = base + _write_scp(tmp_path, {"rec": _wave(0.5, 1)})
    with pytest.raises(NotImplementedError, match="encoder-only CTC models, not for the transducer model"):
        speech_recognize.main(base + ["--model", "speech_transformer_transducer_base", "--search", "ctc"] + LF_OPTS)
    with pytest.raises(NotImplementedError, match="no --streaming with it"):
        speech_recognize.main(base + ["--search", "ctc", "--streaming"] + LF_OPTS)
