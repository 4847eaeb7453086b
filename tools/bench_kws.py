"""The keyword spotter's kernels (csrc/kws.hip) on synthetic CTC log-probs with V = 5004, peaked as a trained model's are.

Offline: 16 utterances x 750 frames in one call -- reset, one step (the row maxima, then the scan), the hits with a flush -- for
K = 1, 100 and 1000 keywords of 2 .. 8 tokens.  Streamed: 16 streams x 10 frames per accept, one step and one poll (hits with
clear) per accept, the same keyword counts.  Times are device events around the calls, median of `--calls` after `--warmup`;
the rate is frames x keywords per second of the step.  K = 1 is in effect the row-max launch alone (the scan is one wave per
entry), so the scan's share of a larger K is that row's time less this one.

Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keywords", default="1,100,1000")
    ap.add_argument("--utts", type=int, default=16)
    ap.add_argument("--frames", type=int, default=750)
    ap.add_argument("--stream-frames", type=int, default=10)
    ap.add_argument("--vocab", type=int, default=5004)
    ap.add_argument("--max-hits", type=int, default=64)
    ap.add_argument("--hold", type=int, default=12)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    from espresso_amd import kernels as K

    assert torch.cuda.is_available(), "bench_kws.py measures on the GPU"
    dev = torch.device("cuda:0")
    B, T, V, H = args.utts, args.frames, args.vocab, args.max_hits
    g = torch.Generator(device=dev).manual_seed(1)
    z = torch.randn(B * T, V, device=dev, generator=g) * 2.0
    peak = torch.randint(0, 200, (B * T,), device=dev, generator=g)
    peak = torch.where(torch.rand(B * T, device=dev, generator=g) < 0.5, torch.zeros_like(peak), peak)  # half the frames blank
    z[torch.arange(B * T, device=dev), peak] += 12.0
    x = K.log_softmax(z, B * T, V, V)
    del z
    res = {"metric": "ctc_keyword_spotting", "utts": B, "frames": T, "vocab": V, "max_hits": H, "hold": args.hold,
           "stream_frames": args.stream_frames, "calls": args.calls}
    rng = np.random.default_rng(2)
    slots = torch.arange(B, dtype=torch.int32, device=dev)
    meta_off = torch.stack([slots, torch.full_like(slots, T), slots * T]).contiguous()
    n = args.stream_frames
    xs = x.view(B, T, V)[:, :n].reshape(B * n, V).contiguous()
    meta_st = torch.stack([slots, torch.full_like(slots, n), slots * n]).contiguous()
    for Kk in [int(k) for k in args.keywords.split(",")]:
        lens = rng.integers(2, 9, size=Kk)
        Lmax = int(lens.max())
        tok = np.zeros((Kk, Lmax), dtype=np.int32)
        for k in range(Kk):
            tok[k, : lens[k]] = rng.integers(1, 200, size=lens[k])  # (over the tokens the synthetic frames peak on)
        tau = (lens * np.log(0.5)).astype(np.float32)
        tables = tuple(torch.from_numpy(a).to(dev) for a in (tok, lens.astype(np.int32), tau))
        state, nbytes = K.ctc_kws_state(B, Kk, Lmax, H, dev)
        rowmax = torch.empty(B * T, dtype=torch.float32, device=dev)
        K.ctc_kws_reset(state, slots, tables, H)

        def step_off():
            K.ctc_kws_step(x, meta_off, state, tables, H, V, 0, args.hold, rowmax=rowmax)

        def search_off():
            K.ctc_kws_reset(state, slots, tables, H)
            K.ctc_kws_step(x, meta_off, state, tables, H, V, 0, args.hold, rowmax=rowmax)
            return K.ctc_kws_hits(state, slots, tables, H, flush=True)

        def accept():
            K.ctc_kws_step(xs, meta_st, state, tables, H, V, 0, args.hold, rowmax=rowmax)
            return K.ctc_kws_hits(state, slots, tables, H, clear=True)

        hits = int(search_off()[3].clamp(max=H).sum())
        s_med, s_min, s_max = timed(step_off, args.warmup, args.calls)
        o_med, _, _ = timed(search_off, args.warmup, args.calls)
        K.ctc_kws_reset(state, slots, tables, H)
        a_med, a_min, a_max = timed(accept, args.warmup, args.calls)
        res[f"K{Kk}"] = {
            "Lmax": Lmax, "state_bytes_per_stream": nbytes, "hits_stored": hits,
            "offline_step_ms": round(s_med, 4), "offline_step_ms_min_max": [round(s_min, 4), round(s_max, 4)],
            "offline_search_ms": round(o_med, 4),
            "offline_frames_x_keywords_per_s": round(B * T * Kk / (s_med * 1e-3), 1),
            "stream_accept_ms": round(a_med, 4), "stream_accept_ms_min_max": [round(a_min, 4), round(a_max, 4)],
            "stream_frames_x_keywords_per_s": round(B * n * Kk / (a_med * 1e-3), 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
