"""Cost of LM fusion in the offline CTC prefix beam search and the offline transducer frame beam search: no LM, the LSTM LM
(`lstm_lm_librispeech` size, random weights) and a sub-word n-gram LM (models/token_ngram_lm.py; a random ARPA file of
`--order` over the V = 5004 dictionary, `--per-order` n-grams per order above 1).  One setting per process (`--lm none | lstm |
ngram`), so that settings can be alternated between fresh processes.

Shapes: B = 24 utterances, beam 10, V = 5004, `--T` frames.  CTC: seeded peaked log-probs (tools/bench_ctc_beam.py).
Transducer: the random-init recipe-size transducer of tools/bench_streaming_transducer_beam.py on random encoder rows.
With `--lm ngram` the row kernel (ea_ngram_token_rows_step, N = B * beam rows) is also timed alone on the contexts of random
walks.  Prints one JSON line: median ms per search, the same per frame, and the row kernel's median us per launch."""
import argparse
import json
import os
import sys
import tempfile
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def _median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lm", choices=["none", "lstm", "ngram"], default="none")
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--per-order", type=int, default=100000)
    ap.add_argument("--search", choices=["ctc", "transducer", "both"], default="both")
    ap.add_argument("--B", type=int, default=24)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--lm-weight", type=float, default=0.4)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    from espresso_amd import kernels as K
    from espresso_amd.models.lstm_lm import LSTMLanguageModelEspresso
    from espresso_amd.models.token_ngram_lm import TokenNGramLM
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder
    from tests.ngram_ref import random_arpa
    from tools.bench_streaming_transducer_beam import VOCAB, build

    dev = torch.device("cuda:0")
    B, T, beam = args.B, args.T, args.beam
    model, d = build(dev, 16)
    V = len(d)
    assert V == VOCAB
    lm, res = None, {"metric": "lm_fusion_search_ms", "lm": args.lm, "B": B, "T": T, "V": V, "beam": beam}
    if args.lm == "lstm":
        class _LMTask:
            target_dictionary = source_dictionary = d

        torch.manual_seed(0)
        lm = LSTMLanguageModelEspresso.build_model(SimpleNamespace(arch="lstm_lm_librispeech", is_wordlm=False), _LMTask).to(dev).eval()
    elif args.lm == "ngram":
        rng = np.random.default_rng(args.order)
        words = [s for i, s in enumerate(d.symbols) if i not in (d.bos(), d.pad(), d.eos(), d.unk())]
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "lm.arpa")
            with open(path, "w") as f:
                f.write(random_arpa(rng, words, args.order, args.per_order, unk=True))
            lm = TokenNGramLM(path, d, device=dev)
        res.update(order=args.order, ngrams=lm.ngram.counts)
    kw = dict(lm_model=lm, lm_weight=args.lm_weight) if lm is not None else {}
    if args.search in ("ctc", "both"):
        g = torch.Generator(device="cpu").manual_seed(0)
        z = torch.randn(B * T, V, generator=g) * 2.0
        peak = torch.where(torch.rand(B * T, generator=g) < 0.5, torch.zeros(B * T, dtype=torch.long), torch.randint(4, V, (B * T,), generator=g))
        z[torch.arange(B * T), peak] += 8.0
        x = K.log_softmax(z.to(dev), B * T, V, V).view(B, T, V)
        in_len = torch.full((B,), T, dtype=torch.int32, device=dev)
        dec = CTCPrefixBeamSearchDecoder([None], d, beam_size=beam, **kw)
        med, lo = _median_ms(lambda: dec.search(x, in_len), args.calls, args.warmup)
        res["ctc_prefix_beam"] = {"ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_per_frame": round(med / T, 4)}
    if args.search in ("transducer", "both"):
        g = torch.Generator(device=dev).manual_seed(1)
        with torch.no_grad():
            E = model.joint_encoder_branch(torch.randn(B * T, 512, device=dev, generator=g).to(torch.bfloat16)).view(B, T, -1)
        enc_len = torch.full((B,), T, dtype=torch.int32, device=dev)
        dec = TransducerFrameBeamDecoder([model], d, beam_size=beam, **kw)
        med, lo = _median_ms(lambda: dec.search(E, enc_len), args.calls, args.warmup)
        res["transducer_frame_beam"] = {"ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_per_frame": round(med / T, 4)}
    if args.lm == "ngram":  # the row kernel alone, on contexts that follow n-grams of the file half of the time
        N = B * beam
        ng = torch.from_numpy(lm.ngram.records(args.order)[0])
        w2t = torch.full((len(lm.ngram.vocab),), d.unk(), dtype=torch.int32)
        w2t[torch.from_numpy(lm.tok2word[lm.tok2word >= 0]).long()] = torch.from_numpy(np.flatnonzero(lm.tok2word >= 0).astype(np.int32))
        walk = w2t[ng[torch.randint(0, ng.shape[0], (N,))].long()].to(dev)  # [N][order] tokens along n-grams
        ctx, _ = lm.start(N, dev)
        parent = torch.arange(N, dtype=torch.int32, device=dev)
        keep = (torch.rand(N, device=dev) < 0.3).to(torch.uint8)
        times = []
        for step in range(40):
            token = walk[:, step % args.order].contiguous() if step % 8 < 4 else torch.randint(4, V, (N,), dtype=torch.int32, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx, _ = lm.update(ctx, parent, token, keep)
            e1.record()
            e1.synchronize()
            if step >= 8:
                times.append(e0.elapsed_time(e1) * 1e3)
        res["row_kernel_us"] = {"median": round(float(np.median(times)), 2), "min": round(min(times), 2), "rows": N}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
