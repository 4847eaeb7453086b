"""Time the hotword-biased CTC prefix beam search (`--search ctc_beam --hotwords`) against the unbiased one.

Input as tools/bench_ctc_beam.py: seeded, peaked synthetic log-probs, B = 24 utterances of T' = 400 encoder frames over
V = 5004 tokens, beam 10.  Arms: the unbiased search, and the biased search with an empty graph and with random phrase lists
of 100 / 1 000 / 5 000 phrases of 2 - 6 tokens (boost 1.5; `--hit-fraction` of the phrases are cut from the peak-token
sequences of the inputs so that phrases do get matched and completed), each without an LM and with a random LM of
`lstm_lm_librispeech` size.  `--parent-library PATH` adds the unbiased arms run through another build of libespresso_amd.so
(the parent commit's) in the same process.  The arms are interleaved: `--rounds` rounds, each timing every arm `--calls` times,
so the run-to-run spread of an arm is visible next to the differences between arms.

Prints one JSON line: per arm the median ms per batch of every round."""
import argparse
import ctypes
import json
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--B", type=int, default=24)
    ap.add_argument("--T", type=int, default=400)
    ap.add_argument("--V", type=int, default=5004)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--lm-weight", type=float, default=0.4)
    ap.add_argument("--sizes", default="0,100,1000,5000")
    ap.add_argument("--hit-fraction", type=float, default=0.1)
    ap.add_argument("--no-lm-arms", action="store_true", help="skip the arms with the LSTM LM")
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    from espresso_amd import _lib
    from espresso_amd import kernels as K
    from espresso_amd.data.asr_dictionary import AsrDictionary
    from espresso_amd.models.lstm_lm import LSTMLanguageModelEspresso
    from espresso_amd.tools.context_graph import ContextGraph
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder

    dev = torch.device("cuda:0")
    B, T = args.B, args.T
    d = AsrDictionary.from_symbols([f"t{i}" for i in range(args.V - 5)], enable_bos=True)
    V = len(d)
    assert V == args.V, V
    g = torch.Generator(device="cpu").manual_seed(0)
    z = torch.randn(B * T, V, generator=g) * 2.0
    peak = torch.where(torch.rand(B * T, generator=g) < 0.5, torch.zeros(B * T, dtype=torch.long), torch.randint(1, V, (B * T,), generator=g))
    z[torch.arange(B * T), peak] += 8.0
    z = z.to(dev)
    x = K.log_softmax(z, B * T, V, V).view(B, T, V)
    in_len = torch.full((B,), T, dtype=torch.int32, device=dev)
    in_len[B // 2:] = T - T // 4
    said = [[int(t) for t in peak[b * T:(b + 1) * T].tolist() if t != 0] for b in range(B)]  # peak tokens, blanks dropped

    rng = np.random.default_rng(0)

    def phrases(n):
        out = []
        for i in range(n):
            k = int(rng.integers(2, 7))
            if rng.random() < args.hit_fraction:
                row = said[int(rng.integers(0, B))]
                s = int(rng.integers(0, len(row) - k))
                out.append((row[s:s + k], 1.5))
            else:
                out.append(([int(t) for t in rng.integers(5, V, k)], 1.5))
        return out

    lm = None
    if not args.no_lm_arms:
        class _LMTask:
            target_dictionary = source_dictionary = d

        torch.manual_seed(0)
        lm = LSTMLanguageModelEspresso.build_model(SimpleNamespace(arch="lstm_lm_librispeech", is_wordlm=False), _LMTask).to(dev).eval()

    def decoders(graph):
        out = {"no_lm": CTCPrefixBeamSearchDecoder([None], d, beam_size=args.beam, context_graph=graph)}
        if lm is not None:
            out["lm"] = CTCPrefixBeamSearchDecoder([None], d, beam_size=args.beam, lm_model=lm, lm_weight=args.lm_weight, context_graph=graph)
        return out

    arms, graphs = {}, {}
    for kind, dec in decoders(None).items():
        arms[f"unbiased_{kind}"] = lambda dec=dec: dec.search(x, in_len)
    for n in [int(s) for s in args.sizes.split(",")]:
        graphs[n] = ContextGraph(phrases(n), V)
        for kind, dec in decoders(graphs[n]).items():
            arms[f"hotwords{n}_{kind}"] = lambda dec=dec: dec.search(x, in_len)
    if args.parent_library:
        parent = ctypes.CDLL(os.path.abspath(args.parent_library))
        for name, (restype, argtypes) in _lib.parse_header().items():
            fn = getattr(parent, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        mine = _lib.lib()

        def through_parent(dec):
            def run():
                _lib._lib = parent
                try:
                    return dec.search(x, in_len)
                finally:
                    _lib._lib = mine
            return run

        for kind, dec in decoders(None).items():
            arms[f"parent_unbiased_{kind}"] = through_parent(dec)

    res = {"metric": "ctc_hotword_beam_batch_ms", "B": B, "T": T, "V": V, "beam": args.beam, "calls": args.calls, "rounds": args.rounds,
           "graph_nodes": {str(n): gr.num_nodes for n, gr in graphs.items()}, "arms": {k: [] for k in arms}}
    for fn in arms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in arms.items():
            times = []
            for _ in range(args.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            res["arms"][name].append(round(float(np.median(times)), 3))
    # what the biasing did to the 1-best of the largest list: completed phrases per batch
    n = max(graphs)
    out = decoders(graphs[n])["no_lm"].search(x, in_len)
    toks, lens = out[0].cpu(), out[1].cpu()
    res["bonus_of_1best_largest_list"] = round(sum(graphs[n].score(toks[b, 0, : int(lens[b, 0])].tolist())[1] for b in range(B)), 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
