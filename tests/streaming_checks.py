"""GPU checks of the chunk-streaming path (kernel vs float64 restatement, streamed vs offline encoder); test_streaming.py asserts."""
import json

import numpy as np
import torch

from tests.gpu_checks import DEV, build_tiny_model, load_fixture, load_ref_state

BOUND = 3.5e-2  # the project's eval-logit bound for bf16 compute against the fp32 reference on the encoder fixtures


def stream_attention_ref(qu, qv, Kh, Vh, pp, center, chunk, n, cs, L, H):
    """float64: rows of chunk `chunk` (n of them) over the frames of chunks chunk-L .. chunk of one stream's K / V history."""
    C = qu.shape[1]
    dh = C // H
    lo, q0 = max(0, chunk - L) * cs, chunk * cs
    hi = q0 + n
    out = torch.zeros(n, C, dtype=torch.float64)
    for h in range(H):
        sl = slice(h * dh, (h + 1) * dh)
        s = qu[:, sl].double() @ Kh[lo:hi, sl].double().T
        if pp is not None:
            idx = center + (torch.arange(lo, hi)[None, :] - (q0 + torch.arange(n))[:, None])
            s = s + (qv[:, sl].double()[:, None, :] * pp[:, sl].double()[idx]).sum(-1)
        out[:, sl] = torch.softmax(s, -1) @ Vh[lo:hi, sl].double()
    return out


def check_stream_attention(dh=64, H=2, cs=8, L=1, B=5, chunks=6, relpos=True, seed=0):
    """Ragged streams (different lengths, a short last chunk, idle entries with n_new 0) run `chunks` steps: ring wrap-around
    whenever chunks > L + 1.  The packed rows are laid out in a shuffled stream order with a one-row gap after every stream,
    and one extra batch entry names a stream slot out of range: gap rows, idle rows and that entry's rows must stay as they were."""
    from espresso_amd import kernels as K

    g = torch.Generator().manual_seed(seed)
    C, W = H * dh, (L + 1) * cs
    max_streams = B + 3
    lens = [int(torch.randint(1, chunks * cs + 1, (1,), generator=g)) for _ in range(B)]
    lens[0] = chunks * cs
    if B > 1:
        lens[1] = (chunks - 1) * cs + max(1, cs // 2)
    slots = torch.randperm(max_streams, generator=g)[:B].tolist()
    Kh = [torch.randn(n, C, generator=g).bfloat16() for n in lens]
    Vh = [torch.randn(n, C, generator=g).bfloat16() for n in lens]
    Qu = [(torch.randn(n, C, generator=g) * 0.35).bfloat16() for n in lens]
    Qv = [(torch.randn(n, C, generator=g) * 0.35).bfloat16() for n in lens]
    pp = torch.randn(2 * W - 1, C, generator=g).bfloat16() if relpos else None
    cache = torch.full((max_streams, W, 2 * C), float("nan"), dtype=torch.bfloat16, device=DEV)
    frames = torch.zeros(max_streams, dtype=torch.int32, device=DEV)
    pp_d = pp.to(DEV) if relpos else None
    worst, ref_max, untouched_ok = 0.0, 0.0, True
    for c in range(chunks):
        ns = [max(0, min(cs, n - c * cs)) for n in lens]
        if sum(ns) == 0:
            continue
        order = torch.randperm(B, generator=g).tolist()
        offs, r = [0] * B, 0
        for b in order:
            offs[b] = r
            r += ns[b] + 1  # one gap row after every stream
        bad_off, M = r, r + 2  # rows of the out-of-range entry
        meta = torch.tensor([slots + [max_streams + 5], ns + [2], offs + [bad_off]], dtype=torch.int32, device=DEV)
        pack = lambda xs: torch.zeros(M, xs[0].shape[1], dtype=torch.bfloat16)
        ku, vu, qu, qv = pack(Kh), pack(Vh), pack(Qu), pack(Qv)
        for b in range(B):
            sl, src = slice(offs[b], offs[b] + ns[b]), slice(c * cs, c * cs + ns[b])
            ku[sl], vu[sl], qu[sl], qv[sl] = Kh[b][src], Vh[b][src], Qu[b][src], Qv[b][src]
        kv = torch.cat([ku, vu], 1).to(DEV).contiguous()
        K.stream_kv_append(kv, 2 * C, cache, meta, frames, B + 1, C, cs, L, M)
        out = torch.full((M, C), 7.0, dtype=torch.bfloat16, device=DEV)
        K.stream_attention(qu.to(DEV), qv.to(DEV), cache, pp_d, W - 1, meta, frames, B + 1, H, dh, cs, L, out=out)
        K.stream_advance(frames, meta, B + 1, cs)
        out = out.float().cpu()
        written = torch.zeros(M, dtype=torch.bool)
        for b in range(B):
            if ns[b] == 0:
                continue
            written[offs[b]:offs[b] + ns[b]] = True
            ref = stream_attention_ref(Qu[b][c * cs:c * cs + ns[b]], Qv[b][c * cs:c * cs + ns[b]], Kh[b], Vh[b], pp, W - 1, c, ns[b],
                                       cs, L, H)
            worst = max(worst, float((out[offs[b]:offs[b] + ns[b]].double() - ref).abs().max()))
            ref_max = max(ref_max, float(ref.abs().max()))
        untouched_ok = untouched_ok and bool((out[~written] == 7.0).all())
    torch.cuda.synchronize()
    fr = frames.cpu().tolist()
    idle = [s for s in range(max_streams) if s not in slots]
    return {"out_abs": worst, "out_ref_max": ref_max, "frames_ok": all(fr[s] == n for s, n in zip(slots, lens)),
            "untouched_ok": untouched_ok, "idle_counters_zero": all(fr[s] == 0 for s in idle)}


def _stream_all(se, feats_list, pieces, ids=None):
    """Feed every utterance in pieces of the given sizes (cycled), all streams together; returns per-stream outputs."""
    ids = list(range(len(feats_list))) if ids is None else ids
    se.open(ids)
    pos = [0] * len(ids)
    outs = [[] for _ in ids]
    k = 0
    while any(p < f.shape[0] for p, f in zip(pos, feats_list)):
        live = [i for i in range(len(ids)) if pos[i] < feats_list[i].shape[0]]
        step = pieces[k % len(pieces)]
        k += 1
        n = [min(step, feats_list[i].shape[0] - pos[i]) for i in live]
        Tm = max(n)
        x = torch.zeros(len(live), Tm, feats_list[0].shape[1], device=DEV)
        for j, i in enumerate(live):
            x[j, :n[j]] = feats_list[i][pos[i]:pos[i] + n[j]]
        fin = [pos[i] + n[j] >= feats_list[i].shape[0] for j, i in enumerate(live)]
        y, counts = se.accept_features([ids[i] for i in live], x, n, fin)
        r = 0
        for j, i in enumerate(live):
            if counts[j]:
                outs[i].append(y[r:r + counts[j]].float().cpu())
            r += counts[j]
            pos[i] += n[j]
    se.close(ids)
    return [torch.cat(o) for o in outs]


def _offline_alone(model, feats):
    with torch.no_grad():
        out = model(feats.unsqueeze(0), torch.tensor([feats.shape[0]], device=DEV))
    return out["encoder_out"][0][:, 0].float().cpu()


def _margin_agree(got, ref, bound):
    top2 = ref.topk(2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) > bound
    return int(clear.sum()), bool((got.argmax(-1)[clear] == ref.argmax(-1)[clear]).all())


def check_fixture_streaming():
    from espresso_amd.models.transformer.streaming_encoder import StreamingEncoder

    g, sd, _, _ = load_fixture("ref_transformer_ctc_postln_chunk")
    legacy = json.loads(str(g["meta"]))
    model = build_tiny_model("transformer", embed_dim=64, heads=4, ffn=128, legacy=legacy).to(DEV).eval()
    load_ref_state(model, sd)
    feats = torch.from_numpy(g["feats"]).to(DEV)
    lengths = g["lengths"].tolist()
    utts = [feats[b, :lengths[b]] for b in range(3)]
    ref = torch.from_numpy(g["out::eval_logits"])  # T x B x V
    se = StreamingEncoder(model, 4)
    res = {}
    y0 = _stream_all(se, utts[:1], [7, 16, 1, 23])[0]
    res["utt0_frames"] = y0.shape[0]
    res["utt0_vs_reference"] = float((y0 - ref[:y0.shape[0], 0]).abs().max())
    res["utt0_clear_frames"], res["utt0_greedy_agree_clear"] = _margin_agree(y0, ref[:, 0], BOUND)
    ys = _stream_all(se, utts, [16, 9, 30])
    offl = [_offline_alone(model, u) for u in utts]
    res["lengths"] = [y.shape[0] for y in ys]
    res["offline_lengths"] = [o.shape[0] for o in offl]
    res["together_vs_offline_alone"] = max(float((y - o).abs().max()) for y, o in zip(ys, offl))
    res["together_vs_alone_stream"] = float((ys[0] - y0).abs().max())
    return res


def build_relpos_model(embed_dim=128, heads=2, ffn=256, layers=3, cs=8, L=2, learned=False, V=40):
    from espresso_amd.models.transformer.speech_transformer_config import SpeechTransformerConfig
    from espresso_amd.models.transformer.speech_transformer_encoder_model import SpeechTransformerEncoderModel
    from tests.gpu_checks import _Task

    cfg = SpeechTransformerConfig()
    e = cfg.encoder
    e.embed_dim, e.ffn_embed_dim, e.layers, e.attention_heads = embed_dim, ffn, layers, heads
    e.normalize_before, e.relative_positional_embeddings, e.layer_type = True, True, "transformer"
    e.learned_pos = learned
    e.conv_channels = "[64, 64, 16, 16]"
    e.chunk_size, e.chunk_left_window, e.chunk_right_window = cs, L, 0
    cfg.dropout = cfg.attention_dropout = cfg.activation_dropout = 0.0
    cfg.layernorm_embedding = True
    cfg.max_source_positions, cfg.max_target_positions = 3600, 200
    torch.manual_seed(11)
    return SpeechTransformerEncoderModel.build_model(cfg, _Task(V)).to(DEV).eval()


def check_relpos_streaming(learned=False):
    """dh 64, 3 layers, L = 2, cs 8: 230 feature frames -> 58 encoder frames = 8 chunks (the last short)."""
    from espresso_amd.models.transformer.streaming_encoder import StreamingEncoder

    model = build_relpos_model(learned=learned)
    g = torch.Generator().manual_seed(5)
    utts = [torch.randn(n, 80, generator=g).to(DEV) for n in (230, 197)]
    se = StreamingEncoder(model, 2)
    a = _stream_all(se, utts, [13, 40, 5])
    b = _stream_all(se, utts, [64, 3])
    offl = [_offline_alone(model, u) for u in utts]
    res = {"chunks": -(-a[0].shape[0] // 8), "lengths_equal": [x.shape[0] for x in a] == [o.shape[0] for o in offl]}
    res["streamed_vs_offline"] = max(float((x - o).abs().max()) for x, o in zip(a, offl))
    res["piece_sizes_bit_identical"] = all(bool(torch.equal(x, y)) for x, y in zip(a, b))
    cl = [_margin_agree(x, o, BOUND) for x, o in zip(a, offl)]
    res["clear_frames"] = sum(c[0] for c in cl)
    res["greedy_agree_clear"] = all(c[1] for c in cl)
    return res


# ---- transducer -------------------------------------------------------------------------------------------------------------
def build_chunk_transducer(cs=4, L=1):
    """The transducer fixture's predictor / joint weights around a transformer chunk encoder of random weights."""
    import os

    from espresso_amd.models.transformer.speech_transformer_config import SpeechTransformerTransducerConfig
    from espresso_amd.models.transformer.speech_transformer_transducer_base import SpeechTransformerTransducerModelBase
    from tests.gpu_checks import GOLD, _Task

    cfg = SpeechTransformerTransducerConfig()
    e, d = cfg.encoder, cfg.decoder
    e.embed_dim, e.ffn_embed_dim, e.layers, e.attention_heads = 64, 128, 2, 4
    e.normalize_before, e.relative_positional_embeddings, e.layer_type = True, True, "transformer"
    e.conv_channels = "[64, 64, 16, 16]"
    e.chunk_size, e.chunk_left_window, e.chunk_right_window = cs, L, 0
    d.embed_dim, d.hidden_size, d.layers, d.residual, d.dropout_in, d.dropout_out = 48, 64, 2, True, 0.0, 0.0
    cfg.joint_dim = 64
    cfg.dropout = cfg.attention_dropout = cfg.activation_dropout = 0.0
    cfg.max_source_positions, cfg.max_target_positions = 3600, 200
    torch.manual_seed(3)
    model = SpeechTransformerTransducerModelBase.build_model(cfg, _Task(40))
    g = np.load(os.path.join(GOLD, "ref_conformer_transducer_tiny.npz"))
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}
    sd = {k: v for k, v in model.upgrade_state_dict_named(dict(sd), "").items() if not k.startswith("encoder.")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("encoder.") for k in missing), (missing, unexpected)
    return model.to(DEV).eval(), g


def _greedy_with_margins(model, x, Ex, blank, bos, V):
    """The greedy search on one utterance's encoder rows x [T][C], frame by frame, with the joint's top-2 margin of every
    decision: (token grid [T][Ex+1], min margin per frame)."""
    from espresso_amd import kernels as K

    E = model.joint_encoder_branch(x.contiguous())
    state = model.decoder.init_state(1, x.device)
    prev = torch.full((1,), bos, dtype=torch.long, device=x.device)
    grid, margins = [], []
    for t in range(x.shape[0]):
        row, m = [blank] * (Ex + 1), float("inf")
        for k in range(Ex):
            dec_out, new_state = model.decoder.advance(prev, state)
            lg = model.joint_step(E[t:t + 1].contiguous(), dec_out)[:, :V]
            lp = K.log_softmax(lg, 1, V, lg.stride(0))
            top = lp[0].topk(2).values
            m = min(m, float(top[0] - top[1]))
            tk = int(lp[0].argmax())
            if tk == blank:
                break
            row[k] = tk
            prev = torch.full((1,), tk, dtype=torch.long, device=x.device)
            state = new_state
        grid.append(row)
        margins.append(m)
    return grid, margins


def check_transducer_streaming(Ex=2):
    from espresso_amd.models.transformer.streaming_encoder import StreamingEncoder
    from espresso_amd.tools.streaming_transducer_greedy_decoder import StreamingTransducerGreedyDecoder
    from espresso_amd.tools.transducer_greedy_decoder import TransducerGreedyDecoder
    from tests.gpu_checks import _Task

    model, g = build_chunk_transducer()
    d = _Task(40).target_dictionary
    feats, lengths = torch.from_numpy(g["feats"]).to(DEV), g["lengths"].tolist()
    utts = [feats[b, :lengths[b]] for b in range(feats.shape[0])]
    off = TransducerGreedyDecoder([model], d, max_num_expansions_per_step=Ex)
    res = {"utts": len(utts), "exact_from_offline_rows": True, "score_abs": 0.0, "nonblank_tokens": 0,
           "stream_fed_agree_clear": True, "stream_fed_clear_frames": 0, "encoder_rows_abs": 0.0}
    se = StreamingEncoder(model, len(utts))
    streamed = _stream_all(se, utts, [11, 30, 4])  # rows as float cpu
    with torch.no_grad():
        for b, u in enumerate(utts):
            sample = {"net_input": {"src_tokens": u.unsqueeze(0), "src_lengths": torch.tensor([u.shape[0]], device=DEV)}}
            toks, score, _ = off._generate(sample)
            x = model.encoder(u.unsqueeze(0), torch.tensor([u.shape[0]], device=DEV))["_x_bt"][0]
            # (a) the offline encoder rows cut into chunks of uneven sizes
            dec = StreamingTransducerGreedyDecoder(model, d, max_num_expansions_per_step=Ex)
            dec.open([b])
            pos, k = 0, 0
            while pos < x.shape[0]:
                n = min([3, 5, 1][k % 3], x.shape[0] - pos)
                dec.accept([b], x[pos:pos + n], [n])
                pos, k = pos + n, k + 1
            h = dec.close(b)
            res["exact_from_offline_rows"] &= bool(torch.equal(h["tokens"].cpu(), toks[0].cpu()))
            res["score_abs"] = max(res["score_abs"], abs(float(h["score"]) - float(score[0])))
            res["nonblank_tokens"] += int((toks[0] != off.blank).sum())
            # (b) fed by the streaming encoder: same tokens up to the first frame whose joint margin is within the bound
            xs = streamed[b].to(DEV).to(torch.bfloat16)
            res["encoder_rows_abs"] = max(res["encoder_rows_abs"], float((xs.float() - x.float()).abs().max()))
            ref_grid, margins = _greedy_with_margins(model, x, Ex, off.blank, off.bos, off.vocab_size)
            dec.open([b])
            dec.accept([b], xs, [xs.shape[0]])
            got = dec.close(b)["tokens"].view(-1, Ex + 1).tolist()
            for t, m in enumerate(margins):
                if m <= BOUND:
                    break
                res["stream_fed_clear_frames"] += 1
                res["stream_fed_agree_clear"] &= got[t] == ref_grid[t]
    return res


# ---- waveform input and the CLI -----------------------------------------------------------------------------------------------
def check_waveform_vs_features():
    """accept_waveform in uneven pieces (some shorter than one fbank frame) vs accept_features on the front-end's features of
    the whole waveform."""
    from espresso_amd.data.gpu_frontend import GpuFbankFrontend
    from espresso_amd.models.transformer.streaming_encoder import StreamingEncoder

    model = build_relpos_model(embed_dim=64, heads=4, ffn=128, layers=2, cs=4, L=1)
    fe = GpuFbankFrontend(torch.device(DEV))
    g = torch.Generator().manual_seed(9)
    waves = [(torch.randn(n, generator=g) * 3000).to(DEV) for n in (20000, 13777)]
    se = StreamingEncoder(model, 2, frontend=fe)
    offs = torch.tensor([0, 20000, 33777], dtype=torch.int64, device=DEV)
    feat, _, frames = fe(torch.cat(waves), offs, [20000, 13777], train=False)
    a = _stream_all(se, [feat[b, :frames[b]] for b in range(2)], [50])
    se.open([0, 1])
    pos, outs, k = [0, 0], [[], []], 0
    pieces = [100, 3000, 250, 7001, 399]
    while any(p < w.numel() for p, w in zip(pos, waves)):
        live = [i for i in range(2) if pos[i] < waves[i].numel()]
        n = pieces[k % len(pieces)]
        k += 1
        ws = [waves[i][pos[i]:pos[i] + n] for i in live]
        fin = [pos[i] + n >= waves[i].numel() for i in live]
        y, counts = se.accept_waveform(live, ws, fin)
        r = 0
        for j, i in enumerate(live):
            if counts[j]:
                outs[i].append(y[r:r + counts[j]].float().cpu())
            r += counts[j]
            pos[i] += n
    se.close([0, 1])
    b = [torch.cat(o) for o in outs]
    return {"frames": [x.shape[0] for x in a], "frames_equal": [x.shape[0] for x in a] == [x.shape[0] for x in b],
            "abs": max(float((x - y).abs().max()) for x, y in zip(a, b))}
