"""Chunk-by-chunk streaming recognition: CPU restatement vs the reference fixture, host logic, and (gpu) the ring-cache attention
kernel, the streaming encoder and the CLI against the offline masked pass."""
import json
import os
import random

import numpy as np
import pytest
import torch

from espresso_amd.models.transformer.streaming_encoder import check_streamable
from espresso_amd.tools.streaming_ctc_decoder import collapse_step
from espresso_amd.tools.utils import chunk_streaming_mask
from tests import streaming_ref

FIX = "ref_transformer_ctc_postln_chunk"


def _fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, FIX + ".npz"))
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}
    return g, sd, json.loads(str(g["meta"]))


# ---- CPU -----------------------------------------------------------------------------------------------------------------
def test_restatement_matches_reference_fixture(golden_dir):
    """Utterance 0 (unpadded): every frame; utterances 1, 2: every chunk but the last (the reference's batched pass leaks the
    padded tail into the last real frames), and their full output against the oracle run on the utterance alone.  2e-5 is the
    bound tests/test_oracle.py applies to this fixture."""
    from oracle import torch_ref

    g, sd, meta = _fixture(golden_dir)
    feats, lengths = torch.from_numpy(g["feats"]), g["lengths"].tolist()
    ref = torch.from_numpy(g["out::eval_logits"])
    cs, L = meta["chunk_size"], meta["chunk_left_window"]
    for b in range(3):
        y = streaming_ref.run(sd, feats[b, :lengths[b]], [7, 16, 1, 23], 4, cs, L, meta["normalize_before"])
        To = int(g["out::out_lengths"][b])
        assert y.shape[0] == To
        upto = To if b == 0 else (To - 1) // cs * cs
        err = float((y[:upto] - ref[:upto, b]).abs().max())
        print("utt", b, "frames", upto, "err", err)
        assert err < 2e-5
        if b > 0:
            ln = torch.tensor([lengths[b]])
            alone, _ = torch_ref.encoder(feats[b:b + 1, :lengths[b]], ln, sd, H=4, layer_type="transformer", training=False,
                                         **torch_ref.legacy_encoder_kwargs(meta, ln, False))
            err = float((y - alone[:, 0]).abs().max())
            print("utt", b, "alone err", err)
            assert err < 2e-5


def test_restatement_piece_size_independence(golden_dir):
    g, sd, meta = _fixture(golden_dir)
    f = torch.from_numpy(g["feats"])[0]
    a = streaming_ref.run(sd, f, [7, 16, 1, 23], 4, 4, 1, False)
    b = streaming_ref.run(sd, f, [70], 4, 4, 1, False)
    c = streaming_ref.run(sd, f, [3, 3, 29], 4, 4, 1, False)
    assert torch.equal(a, b) and torch.equal(a, c)


def test_cache_contents_equal_mask_rows():
    rng = random.Random(0)
    for _ in range(200):
        T, cs, L = rng.randint(1, 70), rng.randint(1, 9), rng.randint(0, 4)
        vis = chunk_streaming_mask(torch.tensor([T]), cs, left_window=L, right_window=0, always_partial_in_last=True)
        for c in range(-(-T // cs)):
            n = min(cs, T - c * cs)
            keys = streaming_ref.cache_keys(c, n, cs, L)
            for i in range(n):
                assert torch.nonzero(vis[c * cs + i]).view(-1).tolist() == keys, (T, cs, L, c, i)


def test_ring_slot_arithmetic_matches_cache_contents():
    """The kernel's slot -> (chunk, position) rule (csrc/stream_attention.hip RingGeom), restated on the host."""
    for cs, L in [(4, 1), (3, 0), (5, 3)]:
        for c in range(12):
            for n in range(1, cs + 1):
                got = []
                for s in range((L + 1) * cs):
                    g_, off = divmod(s, cs)
                    cp = c - ((c - g_) % (L + 1))
                    if cp >= 0 and not (cp == c and off >= n):
                        got.append(cp * cs + off)
                assert sorted(got) == streaming_ref.cache_keys(c, n, cs, L)


def _cfg(**kw):
    from espresso_amd.models.transformer.speech_transformer_config import SpeechTransformerConfig

    cfg = SpeechTransformerConfig()
    cfg.encoder.layer_type, cfg.encoder.chunk_size = "transformer", 8
    for k, v in kw.items():
        setattr(cfg.encoder, k, v)
    return cfg


def test_unstreamable_configurations_are_refused_by_name():
    check_streamable(_cfg())
    for kw, word in [(dict(layer_type="conformer"), "layer_type"), (dict(chunk_size=0), "chunk_size"),
                     (dict(chunk_right_window=1), "chunk_right_window"), (dict(transformer_context="(4, 0)"), "transformer_context"),
                     (dict(conv_channels=None), "conv_channels")]:
        with pytest.raises(NotImplementedError, match=word):
            check_streamable(_cfg(**kw))


@pytest.mark.parametrize("extra,word", [
    (["--search", "beam"], "--search beam"), (["--search", "ctc_beam"], "--search ctc_beam"),
    (["--search", "transducer_beam"], "--search transducer_beam"), (["--search", "transducer_greedy", "--lm-path", "lm.pt"], "--lm-path"),
    (["--search", "ctc", "--lm-path", "lm.pt"], "--lm-path"), (["--search", "ctc", "--print-alignment", "--results-path", "r"], "--print-alignment"),
])
def test_cli_refuses_streaming_combinations_before_loading(extra, word):
    from espresso_amd import speech_recognize as sr

    with pytest.raises(NotImplementedError, match=word):  # /nonexistent.pt is never opened
        sr.main(["--path", "/nonexistent.pt", "--dict", "d", "--wav-scp", "w", "--streaming"] + extra)
    with pytest.raises(ValueError, match="--streams"):
        sr.main(["--path", "/nonexistent.pt", "--dict", "d", "--wav-scp", "w", "--search", "ctc", "--streams", "4"])


def test_streaming_ctc_collapse_equals_offline_collapse():
    rng = random.Random(1)
    blank = 0
    for trial in range(300):
        ids = [rng.choice([0, 0, 1, 2, 3]) for _ in range(rng.randint(0, 40))]
        if trial % 3 == 0 and len(ids) > 4:  # a repeat straddling a cut
            k = rng.randint(1, len(ids) - 2)
            ids[k - 1] = ids[k] = 2
            cuts = [k]
        else:
            cuts = sorted(rng.sample(range(len(ids) + 1), min(3, len(ids) + 1)))
        offline = [t for i, t in enumerate(ids) if t != blank and (i == 0 or ids[i - 1] != t)]
        prev, got, a = -1, [], 0
        for cpt in cuts + [len(ids)]:
            new, prev = collapse_step(prev, ids[a:cpt], blank)
            got += new
            a = cpt
        assert got == offline


# ---- GPU -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kw", [
    dict(dh=16, H=4, cs=4, L=1, B=3, chunks=5, relpos=False),
    dict(dh=16, H=4, cs=4, L=3, B=9, chunks=9, relpos=True),
    dict(dh=64, H=2, cs=8, L=0, B=5, chunks=4, relpos=True),
    dict(dh=64, H=2, cs=8, L=0, B=5, chunks=4, relpos=False),
    dict(dh=64, H=2, cs=16, L=3, B=64, chunks=7, relpos=True),
    dict(dh=64, H=8, cs=16, L=1, B=16, chunks=5, relpos=False),
    dict(dh=32, H=2, cs=5, L=1, B=4, chunks=6, relpos=True),
])
def test_stream_attention_kernel(kw):
    """vs the float64 restatement; ragged n_new incl. 0 and a short last chunk, ring wrap-around (chunks > L + 1).  Bound:
    started from the flash-attention forward check's 1.5e-2 of the output range (bf16 outputs and probabilities); measured
    on an MI355X over these cases: at most 4.2e-3 of the output range (1.47e-2 absolute at |out| <= 3.6), so 6e-3 here."""
    from tests import streaming_checks as S

    r = S.check_stream_attention(**kw)
    print(kw, r)
    assert r["frames_ok"] and r["untouched_ok"] and r["idle_counters_zero"], r
    assert r["out_abs"] <= 6e-3 * max(1.0, r["out_ref_max"]), r


@pytest.mark.gpu
def test_streaming_encoder_on_reference_fixture():
    """Measured on an MI355X: utterance 0 streamed vs the reference's fp32 logits 2.3e-2 (bound 3.5e-2, the offline pass's own
    bound on this fixture); three ragged streams together vs the offline pass on each utterance alone: 0.0 (bit-identical)."""
    from tests import streaming_checks as S

    r = S.check_fixture_streaming()
    print(r)
    assert r["utt0_frames"] == 18 and r["lengths"] == r["offline_lengths"] == [18, 16, 10], r
    assert r["utt0_vs_reference"] < S.BOUND, r
    assert r["utt0_clear_frames"] >= 6 and r["utt0_greedy_agree_clear"], r
    assert r["together_vs_offline_alone"] < S.BOUND, r
    assert r["together_vs_alone_stream"] < S.BOUND, r


@pytest.mark.gpu
@pytest.mark.parametrize("learned", [False, True])
def test_streaming_relpos_encoder_vs_offline(learned):
    """Sinusoidal and learned relative tables, dh 64, 3 layers, L = 2, 8 chunks.  Measured on an MI355X: streamed vs offline 0.0."""
    from tests import streaming_checks as S

    r = S.check_relpos_streaming(learned)
    print(r)
    assert r["chunks"] >= 6 and r["lengths_equal"], r
    assert r["streamed_vs_offline"] < S.BOUND, r
    assert r["greedy_agree_clear"], r
    assert r["piece_sizes_bit_identical"], r


@pytest.mark.gpu
def test_streaming_transducer_greedy_search():
    """The transducer fixture's predictor / joint with a transformer chunk encoder of random weights.  Fed the offline encoder
    output cut into uneven chunks, the streaming search returns exactly the offline hypotheses (score: fp32 sums in a different
    order, 1e-4); fed by the streaming encoder, the same tokens on every frame up to the first whose joint top-2 margin is within
    the 3.5e-2 bound of the fixture test."""
    from tests import streaming_checks as S

    r = S.check_transducer_streaming()
    print(r)
    assert r["exact_from_offline_rows"] and r["score_abs"] < 1e-4, r
    assert r["nonblank_tokens"] > 0, r
    assert r["stream_fed_clear_frames"] >= 10 and r["stream_fed_agree_clear"], r
    assert r["encoder_rows_abs"] < S.BOUND, r


@pytest.mark.gpu
def test_accept_waveform_equals_accept_features():
    """fbank frames are independent of each other: feeding samples in uneven pieces (down to 100 samples, less than one frame)
    gives the encoder the same feature frames as the whole waveform's features.  Bound: the project's 3.5e-2 for bf16 compute;
    measured on an MI355X: see the printed value."""
    from tests import streaming_checks as S

    r = S.check_waveform_vs_features()
    print(r)
    assert r["frames_equal"] and min(r["frames"]) > 10, r
    assert r["abs"] < S.BOUND, r


def _write_wav(path, samples):
    import wave

    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(samples, -32768, 32767).astype("<i2").tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("search", ["ctc", "transducer_greedy"])
def test_cli_streaming_matches_offline(tmp_path, capsys, golden_dir, search):
    """speech_recognize --streaming on the repository's FLAC file and two WAV files, with a small random chunk-streaming
    checkpoint: the same H- lines (tokens; score within 1e-3 in base 2) as the offline run of that checkpoint, also through
    --results-path.  The offline run decodes one utterance per batch.  An utterance may differ only if a frame of the offline CTC log-probs has a top-2 margin within 3.5e-2."""
    from espresso_amd import registry
    from espresso_amd import speech_recognize as sr
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from tests.gpu_checks import DEV
    from tests.streaming_checks import BOUND

    dict_path = str(tmp_path / "dict.txt")
    open(dict_path, "w").write("".join(f"t{i} 1\n" for i in range(20)))
    ctc = search == "ctc"
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(
        dict=dict_path, autoregressive=False, criterion_name="ctc_loss" if ctc else "transducer_loss"))
    enc = {"conv_channels": "[64, 64, 16, 16]", "embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4,
           "normalize_before": True, "relative_positional_embeddings": True, "layer_type": "transformer", "chunk_size": 8,
           "chunk_left_window": 2, "chunk_right_window": 0}
    if ctc:
        name = "speech_transformer_encoder_model"
        block = {"_name": name, "encoder": enc, "dropout": 0.0, "attention_dropout": 0.0, "activation_dropout": 0.0,
                 "layernorm_embedding": True}
    else:
        name = "speech_transformer_transducer_base"
        block = {"_name": name, "encoder": enc, "decoder": {"embed_dim": 48, "hidden_size": 64, "layers": 1}, "joint_dim": 64,
                 "dropout": 0.0, "attention_dropout": 0.0, "activation_dropout": 0.0}
    cls = registry.MODEL_REGISTRY[name]
    torch.manual_seed(0)
    model = cls.build_model(cls.config_class.from_dict(block), task)
    torch.save({"model": model.state_dict(), "cfg": {"model": block}}, str(tmp_path / "model.pt"))
    rng = np.random.default_rng(0)
    with open(tmp_path / "wav.scp", "w") as f:
        f.write("flac {}\n".format(os.path.join(golden_dir, "6313-76958-0021.flac")))
        for i in range(2):
            p = str(tmp_path / f"utt{i}.wav")
            _write_wav(p, rng.standard_normal(int(16000 * (1.3 + 0.9 * i))) * 3000)
            f.write(f"utt{i} {p}\n")
    base = ["--path", str(tmp_path / "model.pt"), "--dict", dict_path, "--wav-scp", str(tmp_path / "wav.scp"), "--search", search]

    def run(extra):
        capsys.readouterr()
        sr.main(base + extra)
        out = capsys.readouterr().out.splitlines()
        return {l.split("\t")[0]: l.split("\t")[1:] for l in out if l.startswith("H-")}

    # one utterance per offline batch: in a padded batch the padded tail passes conv + BatchNorm bias + ReLU and leaks into the
    # last real frames of the shorter utterances, so a row of a padded batch is not the utterance alone (which a stream is)
    offline = run(["--batch-size", "1"])
    streamed = run(["--streaming", "--stream-chunk-ms", "170", "--streams", "2"])
    assert set(offline) == set(streamed) == {"H-flac", "H-utt0", "H-utt1"}
    compared = 0
    for k in offline:
        if streamed[k][0] != offline[k][0] and ctc:
            # allowed only when a frame of this utterance is within the bound: checked on the offline log-probs
            from espresso_amd.data.audio_utils import read_wav

            scp = sr.read_scp(str(tmp_path / "wav.scp"))
            w = read_wav(scp[k[2:]])
            task.build_frontend(torch.device(DEV))
            m = model.to(DEV).eval()
            s = task.prepare_sample(sr.collate([0], [k[2:]], [w], torch.device(DEV)), train=False)
            with torch.no_grad():
                lp = m.get_normalized_probs(m(**s["net_input"]), log_probs=True)[:, 0].float()
            top = lp.topk(2, -1).values
            assert float((top[:, 0] - top[:, 1]).min()) <= BOUND, (k, offline[k], streamed[k])
            continue
        assert streamed[k][0] == offline[k][0], (k, offline[k], streamed[k])
        assert abs(float(streamed[k][1]) - float(offline[k][1])) < 1e-3 * max(1.0, abs(float(offline[k][1]))), (k, offline[k], streamed[k])
        compared += 1
    assert compared >= 1
    res = str(tmp_path / "res")
    capsys.readouterr()
    sr.main(base + ["--streaming", "--stream-chunk-ms", "400", "--results-path", res])
    log = open(os.path.join(res, "decode.log")).read().splitlines()
    got = {l.split("\t")[0]: l.split("\t")[1] for l in log if l.startswith("H-")}
    assert got == {k: v[0] for k, v in streamed.items()}
    assert os.path.exists(os.path.join(res, "decoded_results.txt"))
