"""Cost of the streamed frame-synchronous transducer beam search (StreamingTransducerFrameBeamDecoder over
ea_rnnt_frame_beam_stream_step) next to the streamed greedy decoder (StreamingTransducerGreedyDecoder) on the same encoder rows.

Model: a random-init chunk-streaming transducer of the recipe's size (conv4 + 16 transformer layers of 512, chunk 16 with one
chunk of left context, 2 x 512 LSTM predictor, joint 512, V = 5004).  The encoder runs once, offline, on synthetic features;
its rows are fed to the decoders `--chunk-frames` encoder frames per `accept`, every stream ready in every call.  A random
joint rarely prefers blank; `--emit-rate R` (tools/bench_transducer_decode.py) also measures with the blank logit biased until
the beam-1 search emits R tokens per second of audio, beside the unbiased run.

Per configuration (beam x streams x biased or not), one JSON line:
  accept_ms_median / _p95   wall time of one `accept` ending in a device synchronise (the beam decoder itself never waits);
  frame_us                  the same per frame and stream;
  greedy_ms_median / _p95   StreamingTransducerGreedyDecoder (2 expansions per frame, the CLI's default) on the same rows;
  ea_calls_per_frame        calls into the library's C ABI per frame index of the accept loop: a LOWER BOUND of the launches
                            per frame (the step is one call of two launches, and what torch launches on its own is not
                            counted); the launches themselves are counted from a kernel trace, see DESIGN section 8.1;
  partial_ms, finish_ms     one `partial` / `finish_tensors` + readback for all streams, at the end of the utterance;
  tokens_per_audio_second   of the 1-best hypotheses.
The last line gives the state bytes per stream for 30 s of audio.

`--endpoint`: instead, per configuration the beam decoder's `accept` without times (the baseline), with times, and endpointed
(`accept` + the `endpoint` readback + the segment ends it asks for; rules of the command line's defaults: 0.8 s / 5 s / 20 s),
the three decoders fed the same pieces in the same loop; endpoint_ms is the probe and its readback alone.  Then the bytes of
device state per stream of a slot at the 20 s limit against one sized for 10 minutes."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

VOCAB = 5004
FRAME_S = 0.04  # one encoder frame: 10 ms features, sub-sampling 4


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(ts, name):
    return {f"{name}_median": round(float(np.median(ts)), 3), f"{name}_p95": round(float(np.percentile(ts, 95)), 3)}


def build(dev, chunk):
    from espresso_amd.data.asr_dictionary import AsrDictionary
    from espresso_amd.models.transformer.speech_transformer_config import SpeechTransformerTransducerConfig
    from espresso_amd.models.transformer.speech_transformer_transducer_base import SpeechTransformerTransducerModelBase
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask

    torch.manual_seed(1)
    d = AsrDictionary.from_symbols([f"u{i}" for i in range(VOCAB - 5)], enable_bos=True)
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(criterion_name="transducer_loss", seed=1), tgt_dict=d)
    cfg = SpeechTransformerTransducerConfig()
    e, dc = cfg.encoder, cfg.decoder
    e.embed_dim, e.ffn_embed_dim, e.layers, e.attention_heads = 512, 2048, 16, 8
    e.normalize_before, e.relative_positional_embeddings, e.layer_type = True, True, "transformer"
    e.conv_channels = "[64, 64, 128, 128]"
    e.chunk_size, e.chunk_left_window, e.chunk_right_window = chunk, 1, 0
    dc.embed_dim, dc.hidden_size, dc.layers = 512, 512, 2
    cfg.joint_dim = 512
    cfg.max_source_positions, cfg.max_target_positions = 3600, 200
    return SpeechTransformerTransducerModelBase.build_model(cfg, task).to(dev).eval(), d


def encoder_rows(model, streams, frames, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    feats = torch.randn(streams, frames * 4, 80, device=dev, generator=g)
    with torch.no_grad():
        enc = model.encoder(feats, torch.full((streams,), frames * 4, device=dev))
    x = enc["_x_bt"][0]
    T = x.shape[0] // streams
    return x.view(streams, T, -1), T


def run(model, d, rows, T, beam, streams, cs, args, biased):
    from espresso_amd import kernels
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder
    from espresso_amd.tools.streaming_transducer_greedy_decoder import StreamingTransducerGreedyDecoder

    ids = list(range(streams))
    dec = StreamingTransducerFrameBeamDecoder(model, d, beam, max_streams=streams, max_frames=T)
    greedy = StreamingTransducerGreedyDecoder(model, d)
    pieces = [(a, min(T, a + cs)) for a in range(0, T, cs)]
    acc, base, part, fin, utt, ntok = [], [], [], [], [], 0
    for rnd in range(args.rounds + 1):  # round 0 warms every shape up
        dec.open(ids)
        greedy.open(ids)
        total = 0.0
        for a, b in pieces:
            x = rows[:, a:b].reshape(streams * (b - a), -1)
            counts = [b - a] * streams
            t_beam, _ = _timed(lambda: dec.accept(ids, x, counts))
            t_greedy, _ = _timed(lambda: greedy.accept(ids, x, counts))
            total += t_beam
            if rnd:
                acc.append(t_beam)
                base.append(t_greedy)
        t_part, _ = _timed(lambda: dec.partial(ids))
        t_fin, out = _timed(lambda: [t.cpu() for t in dec.finish_tensors(ids)])
        if rnd:
            part.append(t_part)
            fin.append(t_fin)
            utt.append(total)
            ntok = int(out[1][:, 0].sum())
        for i in ids:
            dec.close(i)
            greedy.close(i)
    # C-ABI calls of one accept of `cs` frames, less those of an accept of one frame: per frame index of the loop
    calls = []
    real = kernels.check
    kernels.check = lambda rc, what: calls.append(what) or real(rc, what)
    try:
        per = []
        for n in (1, min(cs, T - 1) if T > 1 else 1):
            dec.open(ids)
            dec.accept(ids, rows[:, :1].reshape(streams, -1), [1] * streams)
            del calls[:]
            dec.accept(ids, rows[:, 1:1 + n].reshape(streams * n, -1), [n] * streams)
            per.append((n, len(calls)))
            for i in ids:
                dec.close(i)
    finally:
        kernels.check = real
    (n1, c1), (n2, c2) = per
    res = {"beam": beam, "streams": streams, "chunk_frames": cs, "frames": T, "blank_biased": biased, "timed_accepts": len(acc)}
    res.update(_stats(acc, "accept_ms"))
    res.update(_stats(base, "greedy_ms"))
    res["frame_us"] = round(float(np.median(utt)) * 1e3 / (streams * T), 3)
    res["ea_calls_per_frame"] = round((c2 - c1) / (n2 - n1), 2) if n2 > n1 else c1
    res["partial_ms_median"] = round(float(np.median(part)), 3)
    res["finish_ms_median"] = round(float(np.median(fin)), 3)
    res["tokens_per_audio_second"] = round(ntok / (streams * T * FRAME_S), 2)
    return res


def run_endpoint(model, d, rows, T, beam, streams, cs, args):
    from espresso_amd.tools.beam_common import EndpointRules
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder

    ids = list(range(streams))
    rules = EndpointRules(20, 125, 500)  # 0.8 s, 5 s, 20 s in frames of 40 ms
    mk = lambda mf, **kw: StreamingTransducerFrameBeamDecoder(model, d, beam, max_streams=streams, max_frames=mf, **kw)  # noqa: E731
    decs = {"accept_ms": mk(T), "times_accept_ms": mk(T, token_times=True), "endpointed_accept_ms": mk(rules.segment_frames + cs, endpoint=rules)}
    ts = {k: [] for k in decs}
    probe, ended = [], 0

    def endpointed(dec, x, counts):
        n = 0
        for i in dec.room(ids, counts):
            dec.end_segment(i)
            n += 1
        dec.accept(ids, x, counts)
        for i, (rule, _, _, _) in zip(ids, dec.endpoint(ids)):
            if rule:
                dec.end_segment(i)
                n += 1
        return n

    for rnd in range(args.rounds + 1):  # round 0 warms every shape up
        for dec in decs.values():
            dec.open(ids)
        for a in range(0, T, cs):
            b = min(T, a + cs)
            x, counts = rows[:, a:b].reshape(streams * (b - a), -1), [b - a] * streams
            for k, dec in decs.items():
                t, n = _timed((lambda: endpointed(dec, x, counts)) if k == "endpointed_accept_ms" else (lambda: dec.accept(ids, x, counts)))
                if rnd:
                    ts[k].append(t)
                    ended += n or 0
            t, _ = _timed(lambda: decs["endpointed_accept_ms"].endpoint(ids))
            if rnd:
                probe.append(t)
        for dec in decs.values():
            for i in ids:
                dec.close(i)
    res = {"mode": "endpoint", "beam": beam, "streams": streams, "chunk_frames": cs, "frames": T, "timed_accepts": len(probe),
           "segments_ended": ended}
    for k, v in ts.items():
        res.update(_stats(v, k))
    res.update(_stats(probe, "endpoint_ms"))
    return res


def calibrate(model, d, rows, T, rate, blank):
    """Bisection on the blank bias until the beam-1 search emits `rate` tokens per second of audio."""
    from espresso_amd.tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder

    n = min(16, rows.shape[0])
    ids = list(range(n))
    base = float(model.fc_out.bias[blank].detach())
    lo, hi, got = 0.0, 40.0, None
    for _ in range(9):
        mid = 0.5 * (lo + hi)
        with torch.no_grad():
            model.fc_out.bias[blank] = base + mid
        dec = StreamingTransducerFrameBeamDecoder(model, d, 1, max_streams=n, max_frames=T)
        dec.open(ids)
        dec.accept(ids, rows[:n].reshape(n * T, -1), [T] * n)
        got = int(dec.finish_tensors(ids)[1][:, 0].sum()) / (n * T * FRAME_S)
        lo, hi = (mid, hi) if got > rate else (lo, mid)
    return got


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--beams", default="1,5,10")
    p.add_argument("--streams", default="1,16,64")
    p.add_argument("--chunk-frames", type=int, default=16, help="encoder frames per accept (and the encoder's chunk size)")
    p.add_argument("--frames", type=int, default=96, help="encoder frames per utterance (and max_frames of the decoder)")
    p.add_argument("--rounds", type=int, default=2, help="timed utterances per configuration, after one warm-up")
    p.add_argument("--endpoint", action="store_true", help="the beam decoder with and without endpointing instead (see above)")
    p.add_argument("--emit-rate", type=float, default=4.5, help="also measure with the blank bias calibrated to this many tokens per audio second (0: skip)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_streaming_transducer_beam.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    model, d = build(dev, args.chunk_frames)
    blank = d.bos()
    streams = [int(x) for x in args.streams.split(",")]
    rows, T = encoder_rows(model, max(streams), args.frames, dev)
    if args.endpoint:
        from espresso_amd import _lib

        for beam in [int(x) for x in args.beams.split(",")]:
            for s in streams:
                print(json.dumps(run_endpoint(model, d, rows[:s].contiguous(), T, beam, s, args.chunk_frames, args)), flush=True)
        L, cs = _lib.lib(), args.chunk_frames
        print(json.dumps({"endpointed_20s_bytes_per_stream": {f"beam{b}": int(L.ea_rnnt_frame_beam_stream_state_bytes(500 + cs, b) +
                                                                                L.ea_rnnt_frame_beam_stream_times_state_bytes(500 + cs, b))
                                                              for b in (1, 5, 10, 64)},
                          "slot_10min_bytes_per_stream": {f"beam{b}": int(L.ea_rnnt_frame_beam_stream_state_bytes(15000, b))
                                                          for b in (1, 5, 10, 64)}}), flush=True)
        return
    for biased in ([False, True] if args.emit_rate > 0 else [False]):
        if biased:
            got = calibrate(model, d, rows, T, args.emit_rate, blank)
            print(json.dumps({"blank_bias_calibrated_to_tokens_per_s": round(got, 2)}), flush=True)
        for beam in [int(x) for x in args.beams.split(",")]:
            for s in streams:
                print(json.dumps(run(model, d, rows[:s].contiguous(), T, beam, s, args.chunk_frames, args, biased)), flush=True)
    from espresso_amd import _lib

    frames_30s = -(-(1 + (30 * 16000 - 400) // 160) // 4)  # encoder frames of 30 s: 25 ms / 10 ms fbank, sub-sampling 4
    print(json.dumps({"max_frames_30s": frames_30s,
                      "state_bytes_per_stream": {f"beam{b}": int(_lib.lib().ea_rnnt_frame_beam_stream_state_bytes(frames_30s, b))
                                                 for b in (1, 5, 10, 64)}}), flush=True)


if __name__ == "__main__":
    main()
