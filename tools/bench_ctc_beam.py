"""Time CTC decoding of one recipe-size batch: greedy (ea_ctc_greedy_decode), the prefix beam search (`--search ctc_beam`)
with beam 10 and no LM, and the same search fused with a random LM of `lstm_lm_librispeech` size (4 x 800 LSTM, tied
embeddings) at lm_weight 0.4.

Input: seeded, peaked synthetic log-probs, B = 24 utterances of T' = 400 encoder frames over V = 5004 tokens (the recipe's
sub-word vocabulary).  A T' frame is 40 ms of audio, so RTF = batch time / (B * T' * 0.04 s).  "C-ABI calls per frame"
counts the library entries the search calls (each launches one kernel or a few), i.e. the launches that scale with T'.
For the no-LM case the float64 Python oracle of tests/test_ctc_prefix_beam.py is also timed on one utterance.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--B", type=int, default=24)
    ap.add_argument("--T", type=int, default=400)
    ap.add_argument("--V", type=int, default=5004)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--lm-weight", type=float, default=0.4)
    ap.add_argument("--oracle-frames", type=int, default=None, help="frames of the oracle utterance (default: T)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    from espresso_amd import _lib
    from espresso_amd import kernels as K
    from espresso_amd.data.asr_dictionary import AsrDictionary
    from espresso_amd.models.lstm_lm import LSTMLanguageModelEspresso
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder
    from tests.test_ctc_prefix_beam import prefix_beam_oracle

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
    in_len[B // 2:] = T - T // 4  # half the batch shorter, as length-sorted batches are

    class _LMTask:
        target_dictionary = source_dictionary = d

    torch.manual_seed(0)
    # (an attribute object: build_model reads `arch` with getattr, so a dict would fall back to lstm_lm_wsj)
    lm = LSTMLanguageModelEspresso.build_model(SimpleNamespace(arch="lstm_lm_librispeech", is_wordlm=False), _LMTask).to(dev).eval()
    lmd = lm.decoder
    assert (len(lmd.layers), lmd.hidden_size, lmd.share_input_output_embed) == (4, 800, True), "not the lstm_lm_librispeech shape"

    calls = [0]
    inner_check = K.check

    def counting_check(rc, what):
        calls[0] += 1
        return inner_check(rc, what)

    dec_nolm = CTCPrefixBeamSearchDecoder([None], d, beam_size=args.beam)
    dec_lm = CTCPrefixBeamSearchDecoder([None], d, beam_size=args.beam, lm_model=lm, lm_weight=args.lm_weight)
    runs = {"greedy": lambda: K.ctc_greedy_decode(x.view(B * T, V), in_len, B, T, V, d.bos(), d.pad()),
            f"beam{args.beam}_no_lm": lambda: dec_nolm.search(x, in_len),
            f"beam{args.beam}_lm{args.lm_weight:g}": lambda: dec_lm.search(x, in_len)}
    audio_s = B * T * 0.04
    res = {"metric": "ctc_decode_batch_ms", "B": B, "T": T, "V": V, "beam": args.beam, "calls": args.calls, "audio_s_per_batch": audio_s,
           "lm": {"layers": len(lmd.layers), "hidden": lmd.hidden_size, "tied": lmd.share_input_output_embed,
                  "params_M": round(sum(p.numel() for p in lm.parameters()) / 1e6, 2)}}
    for name, fn in runs.items():
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        K.check, calls[0] = counting_check, 0
        fn()
        K.check = inner_check
        n_calls = calls[0]
        torch.cuda.synchronize()
        times = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        med = float(np.median(times))
        res[name] = {"ms_median": round(med, 3), "ms_min": round(min(times), 3), "rtf": med / 1e3 / audio_s,
                     "c_abi_calls": n_calls, "c_abi_calls_per_frame": round(n_calls / T, 2)}
    # the same search on one utterance, float64 Python oracle (CPU)
    Tor = args.oracle_frames or T
    x0 = x[0, :Tor].double().cpu().numpy()
    t0 = time.perf_counter()
    ref, _ = prefix_beam_oracle(x0, Tor, args.beam, dec_nolm.beam_size_token, d.bos())
    res["python_oracle_one_utterance_no_lm"] = {"frames": Tor, "s": round(time.perf_counter() - t0, 3)}
    # agreement of the no-LM search with the oracle on that utterance (1-best)
    got = dec_nolm.search(x[:1, :Tor].contiguous(), torch.full((1,), Tor, dtype=torch.int32, device=dev))
    n = int(got[1][0, 0])
    res["oracle_1best_equal"] = tuple(got[0][0, 0, :n].tolist()) == ref[0][0]
    res["library"] = os.path.basename(_lib.LIB_PATH)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
