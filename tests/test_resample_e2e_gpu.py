"""Audio at 48 kHz and 44.1 kHz through every entry point, on the tiny CTC fixture model and a small chunk-streaming model: what
each computes from a file at its own rate is, bit for bit, what it computes from `Resampler`'s output handed over as 16 kHz
audio -- the rate is honoured, and honoured once.  Times come out in the recording's seconds.  Audio at 16 kHz never reaches
`kernels.resample_batch`.

Before the resampler the recognizer dropped the rate returned by the WAV reader (a 48 kHz file was decoded as audio three times
as long), so the first group cannot pass there."""
import io

import numpy as np
import pytest
import torch

from tests.test_long_form_gpu import DEV, _long_form, _need_gpu, _tiny

pytestmark = pytest.mark.gpu
FO = 16000


def _audio(seconds, rate, seed):
    """band-limited noise with louder and quieter stretches, int16 values at `rate`"""
    rng = np.random.default_rng(seed)
    n = int(rate * seconds)
    x = rng.standard_normal(n + 8)
    x = np.convolve(x, np.ones(9) / 3.0, mode="valid")[:n]  # most of the energy below fo / 2
    env = 0.2 + np.abs(np.sin(np.arange(n) / (rate / 7.6)))
    return np.round(x * 900 * env).astype(np.float32)


def _files(tmp_path, spec):
    """{name: (seconds, rate)} -> (names, paths): WAV files written with write_wav"""
    from espresso_amd.data.audio_utils import write_wav

    names, paths = [], []
    for k, (u, (sec, rate)) in enumerate(spec.items()):
        p = str(tmp_path / f"{u}.wav")
        write_wav(p, _audio(sec, rate, 20 + k), rate)
        names.append(u)
        paths.append(p)
    return names, paths


def _as_16k(task, waves, rates):
    """every utterance through `Resampler` alone: host fp32 arrays, to be handed over as 16 kHz audio"""
    out = []
    for w, r in zip(waves, rates):
        y, off, n = task.frontend.resampler(torch.from_numpy(w).to(DEV), torch.tensor([0, len(w)], dtype=torch.int64).to(DEV),
                                            [len(w)], [r])
        assert n == [-(-len(w) * FO // r)]
        out.append(y.cpu().numpy())
    return out


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _forward(task, model, sample):
    s = task.prepare_sample(sample, train=False)
    with torch.no_grad():
        out = model(**s["net_input"])
    return s, out["_logits_bt"][0], out["src_lengths"][0]


def _chunk_model(tmp_path):
    """a small random chunk-streaming CTC model and its task (the model of tests/test_streaming.py's command-line test)"""
    from espresso_amd import registry
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask

    dict_path = str(tmp_path / "cdict.txt")
    open(dict_path, "w").write("".join(f"t{i} 1\n" for i in range(20)))
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(dict=dict_path, autoregressive=False,
                                                                                    criterion_name="ctc_loss"))
    enc = {"conv_channels": "[64, 64, 16, 16]", "embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4,
           "normalize_before": True, "relative_positional_embeddings": True, "layer_type": "transformer", "chunk_size": 8,
           "chunk_left_window": 2, "chunk_right_window": 0}
    name = "speech_transformer_encoder_model"
    block = {"_name": name, "encoder": enc, "dropout": 0.0, "attention_dropout": 0.0, "activation_dropout": 0.0,
             "layernorm_embedding": True}
    cls = registry.MODEL_REGISTRY[name]
    torch.manual_seed(0)
    model = cls.build_model(cls.config_class.from_dict(block), task).to(DEV).eval()
    task.build_frontend(torch.device(DEV))
    return task, model


SPEC = {"a48": (1.3, 48000), "b441": (0.9, 44100)}


def test_offline_recognition_alignment_and_keywords(tmp_path, capsys):
    _need_gpu()
    from espresso_amd import speech_recognize as SR
    from espresso_amd.tools.ctc_decoder import CTCDecoder
    from espresso_amd.tools.forced_aligner import CTCForcedAligner, frame_seconds
    from espresso_amd.tools.keyword_spotter import CTCKeywordSpotter, hit_seconds

    task, model, base = _tiny(tmp_path)
    names, paths = _files(tmp_path, SPEC)
    waves, rates = SR.read_waves(paths)
    assert rates == [48000, 44100] and [len(w) for w in waves] == [62400, 39690]
    dev = torch.device(DEV)
    order = SR.make_batches(names, SR.lengths_at(waves, rates, FO), 15000, 8)
    assert order == [[0, 1]]
    s1, logits1, len1 = _forward(task, model, SR.collate([0, 1], names, waves, dev, rates, FO))
    assert s1["wav_rates"] == rates
    w16 = _as_16k(task, waves, rates)
    assert [len(w) for w in w16] == [20800, 14400]
    s2, logits2, len2 = _forward(task, model, SR.collate([0, 1], names, w16, dev))
    assert "wav_rates" not in s2
    f1, f2 = s1["net_input"]["src_tokens"], s2["net_input"]["src_tokens"]
    assert f1.shape == f2.shape == (2, task.frontend.num_frames(20800), 80) and torch.equal(_bits(f1), _bits(f2))
    assert len1.tolist() == len2.tolist() and logits1.shape == logits2.shape and torch.equal(_bits(logits1), _bits(logits2))
    # the command line on the files themselves prints the greedy hypotheses of those logits
    d = task.target_dictionary
    (tmp_path / "wav.scp").write_text("".join(f"{u} {p}\n" for u, p in zip(names, paths)))
    capsys.readouterr()
    SR.main(base + ["--wav-scp", str(tmp_path / "wav.scp"), "--search", "ctc"])
    cap = capsys.readouterr().out.splitlines()
    got = {l.split("\t")[0]: l.split("\t")[1] for l in cap if l.startswith("H-")}
    strip = {d.eos(), d.pad()}
    want = {}
    for u, h in zip(names, CTCDecoder([model], d).generate([model], s2)):
        want["H-" + u] = d.string(torch.tensor([t for t in h[0]["tokens"].tolist() if t not in strip]), bpe_symbol=None)
    assert got == want
    rtf = [l for l in cap if l.startswith("Recognized")]
    assert len(rtf) == 1  # (its RTF divides by 1.3 s + 0.9 s, not by the sample counts over 16 000)
    # forced alignment and keyword spotting: the same results from both, on the recording's own time axis
    spf = frame_seconds(model, task.frontend.frame_shift / task.frontend.sample_rate)
    targets = [[7, 12, 9, 30], [11, 5]]
    al = CTCForcedAligner([model], d)
    r1, r2 = al.align(s1, targets), al.align(s2, targets)
    for a, b, w, r in zip(r1, r2, waves, rates):
        assert a["feasible"] and b["feasible"] and a["start"].tolist() == b["start"].tolist() and a["end"].tolist() == b["end"].tolist()
        assert a["score"] == b["score"] and a["frames"] == b["frames"]
        assert 0 < a["end"][-1] * spf < len(w) / r  # the last token ends before the recording does, in ITS seconds
        assert a["frames"] * spf > 0.8 * len(w) / r  # ... and the frames span it (not a third of it, not three times it)
    kws = CTCKeywordSpotter(d, [([int(t)], 0.02) for t in range(5, 40)], max_streams=1, hold_frames=0, max_hits=64)
    h1, h2 = kws.spot(model, s1), kws.spot(model, s2)
    assert h1 == h2 and sum(len(h) for h in h1) > 0
    for hits, w, r in zip(h1, waves, rates):
        assert all(hit_seconds(h, spf)[1] <= len(w) / r + spf for h in hits)


def test_streaming_pieces_at_the_files_rate(tmp_path):
    _need_gpu()
    from espresso_amd import speech_recognize as SR
    from espresso_amd.models.transformer.streaming_encoder import StreamingEncoder

    task, model = _chunk_model(tmp_path)
    names, paths = _files(tmp_path, SPEC)
    waves, rates = SR.read_waves(paths)
    w16 = _as_16k(task, waves, rates)

    def stream(wave, rate, open_rate):
        se = StreamingEncoder(model, 1, frontend=task.frontend)
        se.open([0], **({} if open_rate is None else {"rates": [open_rate]}))
        piece, outs, a = int(rate * 400 / 1000), [], 0
        while a < len(wave):
            b = min(len(wave), a + piece)
            y, counts = se.accept_waveform([0], [torch.from_numpy(wave[a:b])], b >= len(wave))
            if y is not None:
                outs.append(y)
            a = b
        se.close([0])
        return torch.cat(outs)

    for w, r, y in zip(waves, rates, w16):
        got, want = stream(w, r, r), stream(y, FO, None)
        assert got.shape == want.shape and got.shape[0] > 8 and torch.equal(_bits(got), _bits(want)), r
    # the streamed recognizer: pieces of 400 ms cut at the file's rate give the hypotheses of the resampled audio (one stream in
    # flight, so that both runs compute every chunk alone)
    d = task.target_dictionary

    def run(ws, rs):
        hyps, log = {}, io.StringIO()
        SR.recognize_streaming(task, model, d, names, ws, torch.device(DEV), chunk_ms=400, streams=1, ctm_hyps=hyps, out=log,
                               **({} if rs is None else {"rates": rs}))
        return {u: (h["tokens"].tolist(), float(h["score"])) for u, (h, _) in hyps.items()}, log.getvalue()

    (got, out1), (want, out2) = run(waves, rates), run(w16, None)
    assert got == want and set(got) == set(names)
    assert [l for l in out1.splitlines() if l.startswith("H-")] == [l for l in out2.splitlines() if l.startswith("H-")]


def test_long_form_resamples_the_recording_once(tmp_path, monkeypatch):
    _need_gpu()
    from espresso_amd import kernels as K
    from espresso_amd.tools.forced_aligner import LongFormCTCAligner

    task, model, _ = _tiny(tmp_path)
    LF, lf = _long_form(task, model)
    seconds = (2 * lf.plan.H + 15000) / 16000.0  # three windows
    calls = []
    real = K.resample_batch
    monkeypatch.setattr(K, "resample_batch", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    for rate, seed in ((48000, 1), (44100, 2)):
        wave = _audio(seconds, rate, seed)
        (y16,) = _as_16k(task, [wave], [rate])
        del calls[:]
        got = lf.encode(model, wave, rate)
        assert len(calls) == 1
        want = lf.encode(model, y16)
        assert len(calls) == 1  # (audio at the front-end's rate: no launch)
        assert len(lf.plan.windows(len(y16))) == 3
        for a, b in zip(got, want):
            assert a.shape == b.shape and torch.equal(_bits(a), _bits(b))
        al = LongFormCTCAligner(task, model, lf.plan, task.target_dictionary)
        r1, r2 = al.align(wave, [7, 12, 9, 30, 11], rate), al.align(y16, [7, 12, 9, 30, 11])
        assert r1["feasible"] and r1["start"].tolist() == r2["start"].tolist() and r1["end"].tolist() == r2["end"].tolist()
        assert r1["end"][-1] * 0.04 < len(wave) / rate


def test_audio_at_the_frontend_rate_never_reaches_the_resampler(tmp_path, monkeypatch, capsys):
    _need_gpu()
    from espresso_amd import kernels as K
    from espresso_amd import speech_recognize as SR
    from espresso_amd.models.transformer.streaming_encoder import StreamingEncoder

    calls = []
    real = K.resample_batch
    monkeypatch.setattr(K, "resample_batch", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    task, model, base = _tiny(tmp_path)
    names, paths = _files(tmp_path, {"x16": (1.0, 16000), "y16": (0.7, 16000)})
    (tmp_path / "wav.scp").write_text("".join(f"{u} {p}\n" for u, p in zip(names, paths)))
    SR.main(base + ["--wav-scp", str(tmp_path / "wav.scp"), "--search", "ctc"])
    waves, rates = SR.read_waves(paths)
    s = SR.collate([0, 1], names, waves, torch.device(DEV), rates, FO)
    assert rates == [16000, 16000] and sorted(s) == ["net_input", "num_samples", "utt_ids", "wav", "wav_offsets"]
    _forward(task, model, s)
    _, lf = _long_form(task, model)
    lf.encode(model, waves[0], 16000)
    ctask, cmodel = _chunk_model(tmp_path)
    se = StreamingEncoder(cmodel, 1, frontend=ctask.frontend)
    se.open([0], rates=[16000])
    se.accept_waveform([0], [torch.from_numpy(waves[0])], True)
    assert se.resampler is None and calls == []
    # (the counter counts: the same file's samples declared as 48 kHz audio do reach it)
    _forward(task, model, SR.collate([0], names, waves, torch.device(DEV), [48000, 48000], FO))
    assert calls == [1]
