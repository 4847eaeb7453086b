"""Time the forced-alignment kernels (csrc/align.hip) alone.

CTC: ea_ctc_viterbi_align on seeded synthetic log-probs, B utterances of T encoder frames over V tokens, U targets each (fp32
and bf16 inputs); reported as microseconds per frame of one utterance's chain (kernel time / T: the B utterances run side by
side).  Transducer: ea_rnnt_viterbi_align on random lattices at the tiny reference fixture's shape (B 3, T' 18, U+1 8) and at
a recipe-size batch (default B 16, T' 400, U+1 101).  Kernel time from CUDA events over `--calls` launches after `--warmup`.

Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _time(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=24)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--U", type=int, default=200)
    ap.add_argument("--V", type=int, default=5004)
    ap.add_argument("--rnnt-recipe", default="16,400,101", help="B,T',U+1 of the recipe-size transducer batch")
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
    res = {"ctc": {"B": B, "T": T, "U": U, "V": V}}
    for name, xx in (("fp32", x), ("bf16", x.to(torch.bfloat16))):
        us = _time(lambda: K.ctc_viterbi_align(xx, tg, in_len, tl, B, T, V, 0), args.calls, args.warmup)
        res["ctc"][name + "_us"] = round(us, 1)
        res["ctc"][name + "_us_per_frame"] = round(us / T, 3)
    for tag, (b, t, u1) in (("rnnt_tiny", (3, 18, 8)), ("rnnt_recipe", tuple(int(v) for v in args.rnnt_recipe.split(",")))):
        p = torch.rand(b, t, u1, generator=g) * 0.96 + 0.02
        lpb, lpy = p.log().to(dev), (1 - p).log().to(dev)
        Tl = torch.full((b,), t, dtype=torch.int32, device=dev)
        Ul = torch.full((b,), u1 - 1, dtype=torch.int32, device=dev)
        us = _time(lambda: K.rnnt_viterbi_align(lpb, lpy, Tl, Ul), args.calls, args.warmup)
        res[tag] = {"B": b, "T": t, "U1": u1, "us": round(us, 1), "us_per_diagonal": round(us / (t + u1 - 1), 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
