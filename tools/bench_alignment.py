"""Per-step time of beam search with alignment collection off and on (SequenceGenerator(print_alignment=...)), on the enc-dec
shape of bench.py's `decode` block: conv4 + 12-layer Transformer encoder + 6-layer decoder (C 512, 8 heads), character units,
one batch of up to 24 synthetic utterances (<= 15000 frames), max_len 0.08 * frames, no LM, seeded random weights.

With alignment on, every step adds the probabilities written by the last layer's cross-attention, one ea_attn_history_put
launch and one int32 copy of the parent vector; every finalisation adds one ea_attn_backtrace launch.

Prints one JSON line: per beam and mode the median wall time of one generate() call and that time per decoding step."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", default="10,50")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    from espresso_amd.data import synthetic
    from espresso_amd.data.asr_dictionary import AsrDictionary
    from espresso_amd.models.transformer.speech_transformer_base import SpeechTransformerModelBase
    from espresso_amd.models.transformer.speech_transformer_config import SpeechTransformerConfig
    from espresso_amd.sequence_generator import SequenceGenerator
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask

    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    chars = [chr(ord("a") + i) for i in range(26)] + ["'", ".", "-"] + [f"<n{i}>" for i in range(18)]
    d = AsrDictionary.from_symbols(chars, enable_bos=False)
    task = SpeechRecognitionEspressoTask.setup_task(
        SpeechRecognitionEspressoConfig(seed=1, autoregressive=True, criterion_name="label_smoothed_cross_entropy_v2"), tgt_dict=d)
    cfg = SpeechTransformerConfig()
    e, dc = cfg.encoder, cfg.decoder
    e.embed_dim, e.ffn_embed_dim, e.layers, e.attention_heads = 512, 2048, 12, 8
    e.normalize_before, e.relative_positional_embeddings, e.layer_type = True, True, "transformer"
    e.conv_channels = "[64, 64, 128, 128]"
    dc.embed_dim, dc.ffn_embed_dim, dc.layers, dc.attention_heads, dc.normalize_before = 512, 2048, 6, 8, True
    dc.input_dim = dc.output_dim = 512
    cfg.layernorm_embedding = True
    cfg.max_source_positions, cfg.max_target_positions = 3600, 1024
    model = SpeechTransformerModelBase.build_model(cfg, task).to(dev).eval()
    batches, n_samples = synthetic.make_batches(2864, max_tokens=15000, max_sentences=24, seed=3, median_s=5.35, sigma=0.6)
    task.build_frontend(dev)
    sample = task.prepare_sample(synthetic.make_sample(batches[0], n_samples, len(d), d.pad(), dev, seed=3), train=False)
    steps, inner = [0], model.decoder.step

    def counted(*a, **k):
        steps[0] += 1
        return inner(*a, **k)
    model.decoder.step = counted
    res = {"metric": "beam_search_alignment_overhead", "utts": len(batches[0]), "calls": args.calls}
    for beam in [int(b) for b in args.beams.split(",")]:
        for mode in ("off", "on"):
            gen = SequenceGenerator([model], d, beam_size=beam, max_len_a=0.08, max_len_b=0, print_alignment=mode == "on")
            with torch.no_grad():
                for _ in range(args.warmup):
                    gen.generate([model], sample)
                torch.cuda.synchronize()
                times, steps[0] = [], 0
                for _ in range(args.calls):
                    t0 = time.perf_counter()
                    gen.generate([model], sample)
                    torch.cuda.synchronize()
                    times.append(time.perf_counter() - t0)
            n_steps = steps[0] / args.calls
            med = float(np.median(times)) * 1e3
            res[f"beam{beam}_{mode}"] = {"generate_ms_median": round(med, 2), "steps": n_steps, "step_ms_median": round(med / n_steps, 4)}
        off, on = res[f"beam{beam}_off"]["step_ms_median"], res[f"beam{beam}_on"]["step_ms_median"]
        res[f"beam{beam}_overhead_pct"] = round((on / off - 1) * 100, 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
