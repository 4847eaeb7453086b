"""Per-chunk latency and real-time factor of chunk-by-chunk streaming recognition (StreamingEncoder over ea_stream_attention)
next to the offline masked encode of the same utterances.

Model: the encoder shape of transformer_ctc_librispeech.yaml (12 transformer layers, 512 / 8 heads / FFN 2048, sinusoidal
relative positions, conv front-end 64-64-128-128, V = 5004) with `chunk_size` cs, `chunk_left_window` L, random weights.
`--layer-type conformer`: the same shape with Conformer layers whose depthwise convolution (31 taps) is causal
(`encoder.depthwise_conv_causal`), the only Conformer that streams.
Input: seeded random 80-dim features, `--seconds` of audio per utterance (the offline masked path takes at most 1024 encoder
frames = 40.9 s), every stream fed one chunk's worth of feature frames (4 * cs) per call, in lockstep; finished utterances
are followed by new ones until `--chunks` timed calls are made after one warm-up utterance.

Per configuration (streams x cs): median / p95 wall time of one accept_features call ending in a device synchronise (what a
caller waits for a chunk), the aggregate real-time factor (wall time / audio seconds summed over the streams) and the
offline masked encode of the same batch (median of 3 after a warm-up pass) with its real-time factor.  The first chunk of an
utterance is emitted one call late (6 frames of sub-sampler look-ahead), so calls that emit nothing are counted too.

Prints one JSON line per configuration."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


class _Task:
    feat_dim, feat_in_channels = 80, 1

    def __init__(self, V):
        from espresso_amd.data.asr_dictionary import AsrDictionary

        self.target_dictionary = AsrDictionary.from_symbols([f"t{i}" for i in range(V - 5)], enable_bos=True)


def build(cs, L, layers, dev, layer_type="transformer"):
    from espresso_amd.models.transformer.speech_transformer_config import SpeechTransformerConfig
    from espresso_amd.models.transformer.speech_transformer_encoder_model import SpeechTransformerEncoderModel

    cfg = SpeechTransformerConfig()
    e = cfg.encoder
    e.embed_dim, e.ffn_embed_dim, e.layers, e.attention_heads = 512, 2048, layers, 8
    e.normalize_before, e.relative_positional_embeddings, e.learned_pos, e.layer_type = True, True, False, layer_type
    if layer_type == "conformer":
        e.depthwise_conv_causal, e.depthwise_conv_kernel_size = True, 31
    e.conv_channels = "[64, 64, 128, 128]"
    e.chunk_size, e.chunk_left_window, e.chunk_right_window = cs, L, 0
    cfg.dropout = cfg.attention_dropout = cfg.activation_dropout = 0.0
    cfg.layernorm_embedding = True
    cfg.max_source_positions, cfg.max_target_positions = 9600, 200
    torch.manual_seed(0)
    return SpeechTransformerEncoderModel.build_model(cfg, _Task(5004)).to(dev).eval()


def run(streams, cs, args, dev):
    from espresso_amd.models.transformer.streaming_encoder import StreamingEncoder

    model = build(cs, args.left, args.layers, dev, args.layer_type)
    T = int(args.seconds * 100)
    g = torch.Generator(device=dev).manual_seed(1)
    feats = torch.randn(streams, T, 80, device=dev, generator=g)
    se = StreamingEncoder(model, streams)
    piece = 4 * cs
    per_utt = -(-T // piece)
    times, emitted, rounds = [], 0, 0
    with torch.no_grad():
        while len(times) < args.chunks or rounds < 2:
            ids = list(range(streams))
            se.open(ids)
            for k in range(per_utt):
                a, b = k * piece, min(T, (k + 1) * piece)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                y, counts = se.accept_features(ids, feats[:, a:b], [b - a] * streams, b >= T)
                torch.cuda.synchronize()
                if rounds > 0:  # round 0 warms every shape up
                    times.append(time.perf_counter() - t0)
                    emitted += sum(counts)
            se.close(ids)
            rounds += 1
        lens = torch.full((streams,), T, dtype=torch.long, device=dev)
        off = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model(feats, lens)
            torch.cuda.synchronize()
            off.append(time.perf_counter() - t0)
    ts = np.array(times) * 1e3
    audio = (rounds - 1) * streams * args.seconds
    offline = float(np.median(off[1:]))
    return {"streams": streams, "chunk_size": cs, "left_chunks": args.left, "chunk_audio_ms": piece * 10, "layers": args.layers,
            "layer_type": args.layer_type,
            "timed_calls": len(times), "chunk_ms_median": round(float(np.median(ts)), 3), "chunk_ms_p95": round(float(np.percentile(ts, 95)), 3),
            "stream_rtf": round(float(ts.sum() / 1e3 / audio), 5), "encoder_frames": emitted,
            "offline_ms": round(offline * 1e3, 2), "offline_rtf": round(offline / (streams * args.seconds), 5),
            "cache_MiB_per_stream": round(se.cache_bytes_per_stream() / 2 ** 20, 2)}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--streams", default="1,16,64")
    p.add_argument("--chunk-sizes", default="16,32")
    p.add_argument("--left", type=int, default=3)
    p.add_argument("--layers", type=int, default=12)
    p.add_argument("--layer-type", choices=["transformer", "conformer"], default="transformer",
                   help="conformer: causal depthwise convolution, 31 taps")
    p.add_argument("--seconds", type=float, default=30.0)
    p.add_argument("--chunks", type=int, default=200, help="timed accept calls per configuration (at least)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_streaming.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    for cs in [int(x) for x in args.chunk_sizes.split(",")]:
        for s in [int(x) for x in args.streams.split(",")]:
            print(json.dumps(run(s, cs, args, dev)), flush=True)


if __name__ == "__main__":
    main()
