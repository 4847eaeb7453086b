"""Time the per-token posterior kernels (csrc/prefix_posterior.hip) alone, the way tools/bench_align.py times the aligners, and
what `token_posteriors=True` adds to a decode run.

Kernels: ea_ctc_prefix_posteriors on seeded synthetic log-probs, B utterances of T encoder frames over V tokens with one U-token
hypothesis each (fp32 and bf16 inputs), reported as microseconds per frame of one hypothesis' chain (kernel time / T: the
hypotheses run side by side); ea_rnnt_prefix_posteriors on random lattices at the tiny reference fixture's shape and at a
recipe-size batch.  Kernel time from CUDA events over `--calls` launches after `--warmup`.

`--decode`: the utterances of bench.py's decode workload (the first 200 of the synthetic dev-other-like plan, <= 15 000 frames and
<= 24 utterances per batch, front-end and encoder inside the timed region) through a random-init conv4 + Transformer-12 CTC
encoder and the CTC prefix beam search at beam 10, nbest 1, once without and once with token_posteriors: wall seconds of each.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tools.bench_align import _time  # noqa: E402


def decode_block(dev, n_utts=200, beam=10, seed=3):
    from espresso_amd import registry
    from espresso_amd.data import synthetic
    from espresso_amd.data.asr_dictionary import AsrDictionary
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder

    torch.manual_seed(1)
    chars = [chr(ord("a") + i) for i in range(26)] + ["'", ".", "-"] + [f"<n{i}>" for i in range(18)]
    d = AsrDictionary.from_symbols(chars, enable_bos=True)
    task = SpeechRecognitionEspressoTask.setup_task(
        SpeechRecognitionEspressoConfig(seed=1, autoregressive=False, criterion_name="ctc_loss"), tgt_dict=d)
    name = "speech_transformer_encoder_model"
    block = {"_name": name, "dropout": 0.0, "attention_dropout": 0.0, "activation_dropout": 0.0, "layernorm_embedding": True,
             "encoder": {"conv_channels": "[64, 64, 128, 128]", "embed_dim": 512, "ffn_embed_dim": 2048, "layers": 12,
                         "attention_heads": 8, "normalize_before": True, "relative_positional_embeddings": True,
                         "layer_type": "transformer"}}
    cls = registry.MODEL_REGISTRY[name]
    model = cls.build_model(cls.config_class.from_dict(block), task).to(dev).eval()
    batches, n_samples = synthetic.make_batches(2864, max_tokens=15000, max_sentences=24, seed=seed, median_s=5.35, sigma=0.6)
    picked, n = [], 0
    for b in batches:
        picked.append(b)
        n += len(b)
        if n >= n_utts:
            break
    samples = [synthetic.make_sample(b, n_samples, len(d), d.pad(), dev, seed=seed) for b in [batches[-1]] + picked]
    task.build_frontend(dev)
    out = {"beam": beam, "sentences": sum(s["nsentences"] for s in samples[1:]),
           "audio_seconds": round(sum(s["audio_seconds"] for s in samples[1:]), 1)}
    for tag, post in (("plain", False), ("token_posteriors", True), ("plain_again", False)):
        gen = CTCPrefixBeamSearchDecoder([model], d, beam_size=beam, nbest=1, token_posteriors=post)
        gen.generate([model], task.prepare_sample(samples[0], train=False))  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ntok = 0
        for smp in samples[1:]:
            ntok += sum(len(h[0]["tokens"]) for h in gen.generate([model], task.prepare_sample(smp, train=False)))
        torch.cuda.synchronize()
        out[tag + "_wall_seconds"] = round(time.perf_counter() - t0, 4)
        out[tag + "_tokens"] = ntok
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=24)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--U", type=int, default=200)
    ap.add_argument("--V", type=int, default=5004)
    ap.add_argument("--rnnt-recipe", default="16,400,101", help="B,T',U+1 of the recipe-size transducer batch")
    ap.add_argument("--decode", action="store_true", help="also time a decode run with and without token_posteriors")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    from espresso_amd import kernels as K

    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    B, T, U, V = args.B, args.T, args.U, args.V
    x = torch.log_softmax(torch.randn(B * T, V, generator=g) * 3.0, -1).to(dev)
    tg = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).to(dev)
    in_len = torch.full((B,), T, dtype=torch.int32, device=dev)
    tl = torch.full((B,), U, dtype=torch.int32, device=dev)
    utt = torch.arange(B, dtype=torch.int32, device=dev)
    res = {"ctc": {"B": B, "T": T, "U": U, "V": V}}
    for name, xx in (("fp32", x), ("bf16", x.to(torch.bfloat16))):
        us = _time(lambda: K.ctc_prefix_posteriors(xx, tg, utt, in_len, tl, B, T, V, 0), args.calls, args.warmup)
        res["ctc"][name + "_us"] = round(us, 1)
        res["ctc"][name + "_us_per_frame"] = round(us / T, 3)
    for tag, (b, t, u1) in (("rnnt_tiny", (3, 18, 8)), ("rnnt_recipe", tuple(int(v) for v in args.rnnt_recipe.split(",")))):
        p = torch.rand(b, t, u1, generator=g) * 0.96 + 0.02
        lpb, lpy = p.log().to(dev), (1 - p).log().to(dev)
        Tl = torch.full((b,), t, dtype=torch.int32, device=dev)
        Ul = torch.full((b,), u1 - 1, dtype=torch.int32, device=dev)
        us = _time(lambda: K.rnnt_prefix_posteriors(lpb, lpy, Tl, Ul), args.calls, args.warmup)
        res[tag] = {"B": b, "T": t, "U1": u1, "us": round(us, 1), "us_per_diagonal": round(us / (t + u1 - 1), 3)}
    if args.decode:
        res["decode"] = decode_block(dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
