"""Time the hotword-biased frame-synchronous transducer beam search kernels against the unbiased ones.

Protocol of tools/bench_rnnt_frame_beam_kernels.py: the step kernels alone (T calls of the step + the finish) on seeded logits,
B 24, T 200, V 5004, beam 10, K 10, blank mostly ahead; device events around a whole search, the median of 7 searches after one
warm-up.  Arms: the unbiased entry points, and the bias entry points with an empty graph and with random phrase lists of 100 /
1 000 / 5 000 phrases of 2 - 6 tokens (boost 1.5; `--hit-fraction` of them are cut from the 1-best results of the unbiased search
on the same logits, so that phrases do get matched and completed), built as tools/bench_ctc_hotword_beam.py builds them.  The
arms are interleaved: `--rounds` rounds, each timing every arm, so the run-to-run spread of an arm is visible next to the
differences between arms.  `--lm-rows` adds LM rows (weight 0.3) to every arm.

Prints one JSON line: per arm the median microseconds per frame of every round."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--searches", type=int, default=7)
    ap.add_argument("--sizes", default="0,100,1000,5000")
    ap.add_argument("--hit-fraction", type=float, default=0.1)
    ap.add_argument("--lm-rows", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnnt_hotword_beam.py measures on the GPU: no device found")
    from espresso_amd import kernels as K
    from espresso_amd.tools.context_graph import ContextGraph

    dev = "cuda:0"
    B, T, V, beam, Kt = 24, 200, 5004, 10, 10
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(8, B * beam, V, device=dev, generator=g) * 3
    x[:, :, 0] += 6.0  # blank mostly ahead, as with a trained model
    lm = torch.log_softmax(torch.randn(B * beam, V, device=dev, generator=g), -1) if args.lm_rows else None
    in_len = torch.full((B,), T, dtype=torch.int32, device=dev)
    out = (torch.empty(B * beam, dtype=torch.int32, device=dev), torch.empty(B * beam, dtype=torch.int32, device=dev),
           torch.empty(B * beam, dtype=torch.uint8, device=dev))
    step_kw = dict(lm_rows=lm, lm_weight=0.3 if args.lm_rows else 0.0)

    def unbiased():
        ws = unbiased.ws
        for t in range(T):
            K.rnnt_frame_beam_step(x[t % 8], in_len, ws, out, B, T, V, beam, Kt, 0, t, **step_kw)
        return K.rnnt_frame_beam_finish(ws, B, T, beam, 3, 1)

    unbiased.ws = K.rnnt_frame_beam_workspace(B, T, beam, dev)

    def biased(graph):
        tables, ws = graph.cuda(dev), K.rnnt_frame_beam_bias_workspace(B, T, beam, dev)

        def run():
            for t in range(T):
                K.rnnt_frame_beam_bias_step(x[t % 8], in_len, ws, tables, out, B, T, V, beam, Kt, 0, t, **step_kw)
            return K.rnnt_frame_beam_bias_finish(ws, tables, B, T, beam, 3, 1)

        return run

    tokens, lengths, _, _ = (t.cpu() for t in unbiased())
    said = [tokens[b, 0, : int(lengths[b, 0])].tolist() for b in range(B)]
    said = [row for row in said if len(row) > 6]
    rng = np.random.default_rng(0)

    def phrases(n):
        res = []
        for _ in range(n):
            k = int(rng.integers(2, 7))
            if said and rng.random() < args.hit_fraction:
                row = said[int(rng.integers(0, len(said)))]
                s = int(rng.integers(0, len(row) - k))
                res.append((row[s:s + k], 1.5))
            else:
                res.append(([int(t) for t in rng.integers(5, V, k)], 1.5))
        return res

    arms, graphs = {"unbiased": unbiased}, {}
    for n in [int(s) for s in args.sizes.split(",")]:
        graphs[n] = ContextGraph(phrases(n), V)
        arms[f"hotwords{n}"] = biased(graphs[n])
    res = {"metric": "rnnt_hotword_beam_us_per_frame", "B": B, "T": T, "V": V, "beam": beam, "K": Kt, "lm_rows": bool(args.lm_rows),
           "searches": args.searches, "rounds": args.rounds, "graph_nodes": {str(n): gr.num_nodes for n, gr in graphs.items()},
           "arms": {k: [] for k in arms}}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in arms.items():
            ts = []
            for _ in range(args.searches):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) / T * 1e3)
            res["arms"][name].append(round(float(np.median(ts)), 2))
    # what the largest list did to the 1-best results: the boosts they carry, and the checksums of the unbiased and empty-graph arms
    n = max(graphs)
    tk, ln, sc, _ = (t.cpu() for t in arms[f"hotwords{n}"]())
    res["bonus_of_1best_largest_list"] = round(sum(graphs[n].score(tk[b, 0, : int(ln[b, 0])].tolist())[1] for b in range(B)), 2)
    res["check_unbiased"] = [int(unbiased()[1][:, 0].sum()), float(unbiased()[2][:, 0].sum())]
    if 0 in graphs:
        e = arms["hotwords0"]()
        res["check_empty_graph"] = [int(e[1][:, 0].sum()), float(e[2][:, 0].sum())]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
