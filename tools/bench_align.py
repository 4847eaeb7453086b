"""Time the forced-alignment kernels (csrc/align.hip) alone.

CTC: ea_ctc_viterbi_align on seeded synthetic log-probs, B utterances of T encoder frames over V tokens, U targets each (fp32
and bf16 inputs); reported as microseconds per frame of one utterance's chain (kernel time / T: the B utterances run side by
side).  Transducer: ea_rnnt_viterbi_align on random lattices at the tiny reference fixture's shape (B 3, T' 18, U+1 8) and at
a recipe-size batch (default B 16, T' 400, U+1 101).  Kernel time from CUDA events over `--calls` launches after `--warmup`.

`--long T,U[,V]` adds the tiled aligner (csrc/align_long.hip): `kernels.ctc_viterbi_align_long` of one sequence of T frames and U
targets over V symbols (default 64), device events around the call, median (min - max) of `--calls` calls after one warm-up call,
and the same divided by the anti-diagonals of tiles, as tools/bench_long_posteriors.py reports its kernel.

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


def _time_long(K, T, U, V, calls):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.log_softmax(torch.randn(T, V, generator=g, device=dev) * 3.0, -1)
    y = torch.randint(1, V, (U,), generator=g, device=dev, dtype=torch.int32)
    tb, ts = K.ctc_viterbi_long_tile()
    diagonals = -(-T // tb) + -(-(2 * U + 1) // ts) - 1
    ms = []
    for k in range(calls + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        K.ctc_viterbi_align_long(x, y, T, V, 0)
        b.record()
        torch.cuda.synchronize()
        if k:  # (the first call warms up)
            ms.append(a.elapsed_time(b))
    ms.sort()
    med = ms[len(ms) // 2]
    return {"T": T, "U": U, "V": V, "ms": round(med, 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
            "anti_diagonals": diagonals, "us_per_anti_diagonal": round(med * 1000.0 / diagonals, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=24)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--U", type=int, default=200)
    ap.add_argument("--V", type=int, default=5004)
    ap.add_argument("--rnnt-recipe", default="16,400,101", help="B,T',U+1 of the recipe-size transducer batch")
    ap.add_argument("--long", default=None, help="T,U[,V]: also time the tiled aligner on one sequence of this shape")
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
    if args.long:
        shape = [int(v) for v in args.long.split(",")]
        res["ctc_long"] = _time_long(K, shape[0], shape[1], shape[2] if len(shape) > 2 else 64, args.calls)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
