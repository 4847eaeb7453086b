"""Streaming a causal Conformer on the GPU: the streamed convolution-module kernel (csrc/stream_convmodule.hip) against fp64 and
against the offline causal kernels, StreamingEncoder against the offline masked pass, and speech_recognize --streaming against
its offline run.

Kernel bounds (tests/test_convmodule_kernels.py's, derived from the arithmetic):
  Z  vs the fp64 causal convolution of the whole utterance's U     ulp(ref) + KW 2^-23 sum_k |w u|
  H  vs fp64 BatchNorm + SiLU of the kernel's own Z                ulp(ref) + 2^-20 (|z sc| + |sh|)
  carry == the last KW-1 rows of [zeros ; U so far], bit for bit; rows of idle / out-of-range entries, gap rows and the slabs of
  other streams keep what they held."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import causal_conformer_ref as CR
from tests import convmodule_ref as R
from tests import gpu_checks as G
from tests import test_convmodule_kernels as T
from tests.test_convmodule_kernels import BF, F32, inp, out

pytestmark = pytest.mark.gpu
DEV = G.DEV
EPS = 1e-5
SLAB_SENTINEL = 3.0  # what the carry slabs of streams that are not in use hold


@pytest.fixture
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from espresso_amd import _lib

    return _lib.lib()


# ---- G3: the streamed kernel -------------------------------------------------------------------------------------------------
def _offline_causal(lib, Y, bw, brm, brv, bg, bb, n, C, KW):
    """ea_glu_dwconv_causal_fwd + ea_bn_from_running + ea_bn_act_fwd over one whole utterance -> (U, Z, H) bf16 on the host"""
    bY, bU, bZ, bH, bmr = inp(Y), out((n, C), BF), out((n, C), BF), out((n, C), BF), out((2 * C,), F32)
    assert lib.ea_glu_dwconv_causal_fwd(bY.p, bw.p, bU.p, bZ.p, None, 1, n, C, KW, T._st()) == 0
    assert lib.ea_bn_from_running(brm.p, brv.p, bmr.p, C, EPS, T._st()) == 0
    assert lib.ea_bn_act_fwd(bZ.p, bmr.p, bg.p, bb.p, bH.p, n, C, 2, T._st()) == 0
    torch.cuda.synchronize()
    assert bU.intact() and bZ.intact() and bH.intact() and bmr.intact()
    return bU.cpu(), bZ.cpu(), bH.cpu(), bmr.cpu()


def _stream_case(lib, C, KW, cs, streams, chunks, with_z, seed=0):
    """`chunks` calls over `streams` ragged streams.  Returns per stream the concatenated (Z, H), the inputs, and what was
    checked on the way (carry after every call, untouched rows and slabs)."""
    g = T._gen(seed + 1000 * KW + C + cs)
    HALO, max_streams = KW - 1, streams + 3
    lens = [int(torch.randint(1, chunks * cs + 1, (1,), generator=g)) for _ in range(streams)]
    lens[0] = chunks * cs
    lens[1] = (chunks - 2) * cs + max(1, cs // 2)  # a short last chunk in the call before the last, then idle (n_new 0)
    slots = torch.randperm(max_streams, generator=g)[:streams].tolist()
    scale = [0.5 * 4.0 ** ((0.618 * b) % 1.0) for b in range(streams)]
    Ys = [(torch.randn(n, 2 * C, generator=g) * s).to(BF) for n, s in zip(lens, scale)]
    w = (torch.randn(C, KW, generator=g) / KW ** 0.5).float()
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    rm, rv = 0.3 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    bw, bg, bb, brm, brv = inp(w), inp(gamma), inp(beta), inp(rm), inp(rv)
    off = [_offline_causal(lib, Y, bw, brm, brv, bg, bb, n, C, KW) for Y, n in zip(Ys, lens)]
    mr = off[0][3]
    bmr = inp(mr)
    carry0 = torch.full((max_streams, HALO, C), SLAB_SENTINEL)
    carry0[slots] = 0.0
    bcarry = out((max_streams, HALO, C), BF, carry0)
    Zs, Hs = [[] for _ in range(streams)], [[] for _ in range(streams)]
    saw_idle = False
    for c in range(chunks):
        ns = [max(0, min(cs, n - c * cs)) for n in lens]
        saw_idle = saw_idle or 0 in ns
        order = torch.randperm(streams, generator=g).tolist()
        offs, r = [0] * streams, 0
        for b in order:
            offs[b] = r
            r += ns[b] + 1  # one gap row after every stream
        # three more entries that must be skipped: slot out of range, more rows than a chunk, rows past the buffer
        M = r + 2
        meta = torch.tensor([slots + [max_streams + 5, slots[0], slots[0]], ns + [2, cs + 1, 2], offs + [r, 0, M - 1]], dtype=torch.int32)
        Yp = torch.full((M, 2 * C), float("nan")).to(BF)
        for b in range(streams):
            Yp[offs[b]:offs[b] + ns[b]] = Ys[b][c * cs:c * cs + ns[b]]
        bY, bmeta = inp(Yp), meta.to(DEV)
        p = lambda row: ctypes.c_void_p(bmeta[row].data_ptr())
        bH, bZ = out((M, C), BF), out((M, C), BF)
        B = streams + 3
        assert lib.ea_stream_glu_dwconv_bn_act(bY.p, bw.p, bmr.p, bg.p, bb.p, bcarry.p, p(0), p(1), p(2), bH.p, bZ.p if with_z else None,
                                               B, C, KW, cs, max_streams, M, T._st()) == 0
        torch.cuda.synchronize()
        assert bH.intact() and bZ.intact() and bcarry.intact()
        Hc, Zc, carry = bH.cpu(), bZ.cpu(), bcarry.cpu()
        written = torch.zeros(M, dtype=torch.bool)
        for b in range(streams):
            written[offs[b]:offs[b] + ns[b]] = True
            Hs[b].append(Hc[offs[b]:offs[b] + ns[b]])
            Zs[b].append(Zc[offs[b]:offs[b] + ns[b]])
            # the carry: the last KW-1 rows of [zeros ; U so far], exactly (U as the offline kernel stores it)
            done = min(lens[b], (c + 1) * cs)
            want = torch.cat([torch.zeros(HALO, C, dtype=BF), off[b][0][:done]])[-HALO:]
            assert torch.equal(carry[slots[b]].view(torch.int16), want.view(torch.int16)), (c, b, "carry")
        assert bool(torch.isnan(Hc[~written].float()).all()), "H rows of gap / idle / skipped entries were written"
        assert bool(torch.isnan(Zc.float()).all() if not with_z else torch.isnan(Zc[~written].float()).all())
        assert not bool(torch.isnan(Hc[written].float()).any())
        idle = [s for s in range(max_streams) if s not in slots]
        assert bool((carry[idle].float() == SLAB_SENTINEL).all()), "a carry slab of another stream was written"
    assert saw_idle
    cat = lambda xs: [torch.cat(x) for x in xs]
    return dict(Z=cat(Zs), H=cat(Hs), Y=Ys, off=off, lens=lens, w=w, gamma=gamma, beta=beta, mr=mr)


STREAM_CASES = [(64, 31, 4, 3, 10),   # the chunk is shorter than the carry: fully replaced only after 8 chunks
                (128, 31, 32, 5, 3),  # the chunk is longer than the carry
                (64, 7, 8, 4, 4), (72, 15, 16, 2, 3), (64, 3, 1, 2, 5)]


@pytest.mark.parametrize("C,KW,cs,streams,chunks", STREAM_CASES)
def test_stream_convmodule_kernel(lib, C, KW, cs, streams, chunks):
    """Streamed H against the offline causal kernels (ea_glu_dwconv_causal_fwd + ea_bn_from_running + ea_bn_act_fwd over the whole
    utterance): expected 0.0 — the same taps in the same order through the same helpers; measured on an MI355X over these five
    cases: 0.0.  Asserted: within twice the H bound."""
    r = _stream_case(lib, C, KW, cs, streams, chunks, with_z=True)
    r2 = _stream_case(lib, C, KW, cs, streams, chunks, with_z=False)
    worst_off = 0.0
    for b, n in enumerate(r["lens"]):
        U, Zoff, Hoff, _ = r["off"][b]
        T._check_bf16(f"U[{b}] (offline kernel)", U, R.glu(r["Y"][b]))
        Zr, zmag = CR.dwconv(U, r["w"], 1, n, KW)
        T._check_bf16(f"Z[{b}]", r["Z"][b], Zr, KW * 2.0 ** -23 * zmag)
        Hr, hmag = R.bn_act(r["Z"][b], r["mr"][:C], r["mr"][C:], r["gamma"], r["beta"], 2)
        T._check_bf16(f"H[{b}]", r["H"][b], Hr, 2.0 ** -20 * hmag)
        assert torch.equal(r2["H"][b].view(torch.int16), r["H"][b].view(torch.int16)), "Z = NULL changed H"
        d = (r["H"][b].double() - Hoff.double()).abs()
        worst_off = max(worst_off, float(d.max()))
        Hor, homag = R.bn_act(Zoff, r["mr"][:C], r["mr"][C:], r["gamma"], r["beta"], 2)
        assert bool((d <= 2 * (T._ulp(Hor) + 2.0 ** -20 * homag)).all()), (b, float(d.max()))
    print("streamed H vs offline causal kernels, max abs:", worst_off)


def test_stream_convmodule_unsupported_shapes(lib):
    """C % 8 != 0, a filter width without an instantiation and a chunk above 128 rows return -2 and write nothing"""
    assert lib.ea_stream_convmodule_supported(64, 31, 128) == 1 and lib.ea_stream_convmodule_supported(72, 3, 1) == 1
    C, KW, cs = 64, 7, 8
    g = T._gen(1)
    bY, bw, bmr = inp((torch.randn(8, 2 * 72, generator=g)).to(BF)), inp(torch.randn(72, 8, generator=g)), inp(torch.rand(2 * 72, generator=g))
    meta = torch.tensor([[0], [4], [0]], dtype=torch.int32, device=DEV)
    p = lambda row: ctypes.c_void_p(meta[row].data_ptr())
    for (c, kw, s) in ((C + 4, KW, cs), (C + 2, KW, cs), (C, 5, cs), (C, KW, 129), (C, KW, 0)):
        assert lib.ea_stream_convmodule_supported(c, kw, s) == 0
        bH, bZ, bc = out((8, 72), BF), out((8, 72), BF), out((2, 30, 72), BF)
        assert lib.ea_stream_glu_dwconv_bn_act(bY.p, bw.p, bmr.p, bmr.p, bmr.p, bc.p, p(0), p(1), p(2), bH.p, bZ.p, 1, c, kw, s, 2, 8,
                                               T._st()) == -2, (c, kw, s)
        torch.cuda.synchronize()
        assert bH.untouched() and bZ.untouched() and bc.untouched()


# ---- G6: StreamingEncoder against the offline pass ------------------------------------------------------------------------------
def _seed_running_stats(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if getattr(m, "running_mean", None) is not None:
                m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))


def _causal_conformer(KW, cs, L=2, embed_dim=128, heads=2, ffn=256, layers=3, V=40):
    from espresso_amd.models.transformer.speech_transformer_config import SpeechTransformerConfig
    from espresso_amd.models.transformer.speech_transformer_encoder_model import SpeechTransformerEncoderModel

    cfg = SpeechTransformerConfig()
    e = cfg.encoder
    e.embed_dim, e.ffn_embed_dim, e.layers, e.attention_heads = embed_dim, ffn, layers, heads
    e.normalize_before, e.relative_positional_embeddings, e.layer_type = True, True, "conformer"
    e.depthwise_conv_causal, e.depthwise_conv_kernel_size = True, KW
    e.conv_channels = "[64, 64, 16, 16]"
    e.chunk_size, e.chunk_left_window, e.chunk_right_window = cs, L, 0
    cfg.dropout = cfg.attention_dropout = cfg.activation_dropout = 0.0
    cfg.layernorm_embedding = True
    cfg.max_source_positions, cfg.max_target_positions = 3600, 200
    torch.manual_seed(11)
    model = SpeechTransformerEncoderModel.build_model(cfg, G._Task(V))
    with torch.no_grad():  # the reference initialises the positional biases to zero: make them count
        for l in model.encoder.layers:
            l.self_attn.pos_bias_u.normal_(0, 0.1)
            l.self_attn.pos_bias_v.normal_(0, 0.1)
    _seed_running_stats(model, 12)
    return model.to(DEV).eval()


@pytest.mark.parametrize("KW,cs", [(31, 8), (7, 16)])  # the chunk shorter, and longer, than the KW-1 carried rows
def test_streaming_causal_conformer_vs_offline(KW, cs):
    """C 128, 2 heads (dh 64), 3 layers, L 2, sinusoidal relative positions, seeded BatchNorm running statistics; streams of 230
    and 197 feature frames.  Measured on an MI355X: streamed vs offline 0.0 in both configurations (bit-identical logits)."""
    from espresso_amd.models.transformer.streaming_encoder import StreamingEncoder
    from tests.streaming_checks import BOUND, _margin_agree, _offline_alone, _stream_all

    model = _causal_conformer(KW, cs)
    g = torch.Generator().manual_seed(5)
    utts = [torch.randn(n, 80, generator=g).to(DEV) for n in (230, 197)]
    offl = [_offline_alone(model, u) for u in utts]
    clear = [int(((o.topk(2, -1).values[:, 0] - o.topk(2, -1).values[:, 1]) > BOUND).sum()) for o in offl]
    frames = sum(o.shape[0] for o in offl)
    print("offline frames with a top-2 margin above the bound:", sum(clear), "of", frames)
    assert 2 * sum(clear) >= frames  # (a condition on the offline logits alone)
    se = StreamingEncoder(model, 2)
    assert se.cache_bytes_per_stream() == 3 * (3 * cs * 2 * 128 * 2 + (KW - 1) * 128 * 2)
    a = _stream_all(se, utts, [13, 40, 5])
    b = _stream_all(se, utts, [64, 3])
    assert [x.shape[0] for x in a] == [o.shape[0] for o in offl] == [58, 50]
    diff = max(float((x - o).abs().max()) for x, o in zip(a, offl))
    print("streamed vs offline, max abs:", diff)
    assert diff < BOUND
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "the output depends on how the input is cut into pieces"
    cl = [_margin_agree(x, o, BOUND) for x, o in zip(a, offl)]
    assert sum(c[0] for c in cl) == sum(clear) and all(c[1] for c in cl)
    # a stream alone == the same stream beside the other; its slot held another utterance's carry in between (close, open)
    alone1 = _stream_all(se, utts[1:], [13, 40, 5])[0]
    alone0 = _stream_all(se, utts[:1], [13, 40, 5])[0]
    assert torch.equal(alone0, a[0]) and torch.equal(alone1, a[1])
    again = _stream_all(se, utts, [13, 40, 5])
    assert all(torch.equal(x, y) for x, y in zip(a, again)), "a reopened slot does not start from a zeroed carry"


# ---- G7: the command line --------------------------------------------------------------------------------------------------------
def _write_wav(path, samples):
    import wave

    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(samples, -32768, 32767).astype("<i2").tobytes())


def _cli_checkpoint(tmp_path, golden_dir, ctc):
    from espresso_amd import registry
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask

    dict_path = str(tmp_path / "dict.txt")
    open(dict_path, "w").write("".join(f"t{i} 1\n" for i in range(20)))
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(
        dict=dict_path, autoregressive=False, criterion_name="ctc_loss" if ctc else "transducer_loss"))
    enc = {"conv_channels": "[64, 64, 16, 16]", "embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4,
           "normalize_before": True, "relative_positional_embeddings": True, "layer_type": "conformer", "depthwise_conv_causal": True,
           "depthwise_conv_kernel_size": 15, "chunk_size": 8, "chunk_left_window": 2, "chunk_right_window": 0}
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
    _seed_running_stats(model, 1)
    torch.save({"model": model.state_dict(), "cfg": {"model": block}}, str(tmp_path / "model.pt"))
    rng = np.random.default_rng(0)
    with open(tmp_path / "wav.scp", "w") as f:
        f.write("flac {}\n".format(os.path.join(golden_dir, "6313-76958-0021.flac")))
        for i in range(2):
            p = str(tmp_path / f"utt{i}.wav")
            _write_wav(p, rng.standard_normal(int(16000 * (1.3 + 0.9 * i))) * 3000)
            f.write(f"utt{i} {p}\n")
    return task, model, ["--path", str(tmp_path / "model.pt"), "--dict", dict_path, "--wav-scp", str(tmp_path / "wav.scp")]


def _compare_runs(offline, streamed, tmp_path, task, model, ctc):
    """test_streaming.py's rules: the same tokens and the score within 1e-3; an utterance may differ only if a frame of its
    offline CTC log-probs has a top-2 margin within the bound.  Returns how many utterances were compared in full."""
    from espresso_amd import speech_recognize as sr
    from tests.streaming_checks import BOUND

    assert set(offline) == set(streamed) == {"H-flac", "H-utt0", "H-utt1"}
    compared = 0
    for k in offline:
        if streamed[k][0] != offline[k][0] and ctc:
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
    return compared


@pytest.mark.parametrize("search", ["ctc", "transducer_greedy"])
def test_cli_streaming_causal_conformer_matches_offline(tmp_path, capsys, golden_dir, search):
    """speech_recognize --streaming --streams 2 with a causal Conformer checkpoint (KW 15, cs 8, L 2, seeded running statistics)
    gives the H- lines of the offline run with one utterance per batch; for CTC also --search ctc_stream_beam --beam 4 against
    --search ctc_beam --beam 4 on the same checkpoint."""
    from espresso_amd import speech_recognize as sr

    ctc = search == "ctc"
    task, model, base = _cli_checkpoint(tmp_path, golden_dir, ctc)

    def run(extra):
        capsys.readouterr()
        sr.main(base + extra)
        lines = capsys.readouterr().out.splitlines()
        return {l.split("\t")[0]: l.split("\t")[1:] for l in lines if l.startswith("H-")}

    offline = run(["--search", search, "--batch-size", "1"])
    streamed = run(["--search", search, "--streaming", "--stream-chunk-ms", "170", "--streams", "2"])
    assert _compare_runs(offline, streamed, tmp_path, task, model, ctc) >= 1
    if ctc:
        offline = run(["--search", "ctc_beam", "--beam", "4", "--batch-size", "1"])
        streamed = run(["--search", "ctc_stream_beam", "--streaming", "--beam", "4", "--stream-chunk-ms", "170", "--streams", "2"])
        assert _compare_runs(offline, streamed, tmp_path, task, model, True) >= 1
