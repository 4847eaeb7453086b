"""Per-step time of the tiny fusion beam search (beam 3, 3 sentences, 13 steps, the setting of
tests/golden/ref_multilevel_fusion_tiny.npz) with no LM, the look-ahead word LM and the multi-level (sub-word + word) LM.
Evidence only: the tiny models are launch / host bound, the numbers say what one fused step costs on top of the acoustic
decoder, not how a recipe-size decode behaves.

Prints one JSON line: for each mode the median / min wall time of one generate() call over --calls timed calls (after
--warmup), and that time divided by the number of decoding steps."""
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    from espresso_amd.models.tensorized_lookahead_language_model import TensorizedLookaheadLanguageModel
    from espresso_amd.sequence_generator import SequenceGenerator
    from tests import test_multilevel_lm as T
    from tests.gpu_checks import build_tiny_encdec

    dev = T.DEV
    g = T._load("ref_transformer_encdec_tiny")
    gl, d, ml = T._multilevel("ref_multilevel_fusion_tiny", "symbols", subwordlm_weight=0.8, oov_penalty=1.0, open_vocab=True)
    la = TensorizedLookaheadLanguageModel(ml.wordlm, d, oov_penalty=1e-4, open_vocab=True)
    model = build_tiny_encdec().to(dev)
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}
    model.load_state_dict(model.upgrade_state_dict_named(dict(sd), ""), strict=False)
    model.eval()
    sample = {"net_input": {"src_tokens": torch.from_numpy(g["feats"]).to(dev), "src_lengths": torch.from_numpy(g["lengths"]).to(dev)}}
    res = {"metric": "tiny_fusion_beam3_step_ms", "calls": args.calls}
    steps, inner = [0], model.decoder.step

    def counted(*a, **k):  # one acoustic decoder step per decoding step
        steps[0] += 1
        return inner(*a, **k)
    model.decoder.step = counted
    for mode, lm in (("none", None), ("lookahead", la), ("multilevel", ml)):
        gen = SequenceGenerator([model], d, beam_size=3, max_len_a=0.0, max_len_b=12, lm_model=lm, lm_weight=0.5)
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
        res[mode] = {"generate_ms_median": round(med, 3), "generate_ms_min": round(min(times) * 1e3, 3), "steps": n_steps,
                     "step_ms_median": round(med / n_steps, 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
