"""Long-form recognition (csrc/long_form.hip, espresso_amd/tools/long_form.py) on a synthetic hour of audio at V = 5000.

Kernels: the bf16 logits of the hour's windows (30 s windows, 6 s overlap: 150 windows x 750 frames) go through
`ea_longform_cuts` and `ea_longform_stitch`; the yardstick is `ea_log_softmax_bf16` alone over as many rows as the stitch writes
(the same bytes read and written, without the cuts and the indirection).  Times are device events around the calls, median of
`--calls` after `--warmup`.

Pipeline: the recipe's 12-layer Conformer-CTC (random weights) over an hour of synthetic noise through `LongFormCTC.encode`
(front-end, encoder over batches of windows, cuts, stitch; greedy decoding on top), wall clock with a device synchronisation,
as the real-time factor seconds of compute per second of audio.  `--pipeline-seconds 0` skips it.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--seconds", type=float, default=3600.0, help="audio behind the synthetic window logits")
    ap.add_argument("--pipeline-seconds", type=float, default=3600.0, help="audio of the whole-pipeline run (0: skip it)")
    ap.add_argument("--window-s", type=float, default=30.0)
    ap.add_argument("--overlap-s", type=float, default=6.0)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--max-tokens", type=int, default=15000)
    ap.add_argument("--batch-size", type=int, default=24)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    from espresso_amd import kernels as K
    from espresso_amd.tools import long_form as LF

    assert torch.cuda.is_available(), "bench_long_form.py measures on the GPU"
    dev = torch.device("cuda:0")
    V, G = args.vocab, 640
    plan = LF.LongFormPlan.from_seconds(G, 16000, args.window_s, args.overlap_s)
    N = int(args.seconds * 16000)
    wins = plan.windows(N)
    Nw, Tw, Hf = len(wins), plan.Tw, plan.Hf
    counts = [-(-(1 + (ln - 400) // 160) // 4) for _, ln in wins]
    T = (Nw - 1) * Hf + counts[-1]
    g = torch.Generator(device=dev).manual_seed(1)
    logits = torch.empty(Nw, Tw, V, dtype=torch.bfloat16, device=dev)
    for n in range(Nw):  # peaked as a trained model's are: half the frames on blank, the rest on one of 199 tokens
        z = torch.randn(Tw, V, device=dev, generator=g) * 2.0
        peak = torch.randint(1, 200, (Tw,), device=dev, generator=g)
        peak = torch.where(torch.rand(Tw, device=dev, generator=g) < 0.5, torch.zeros_like(peak), peak)
        z[torch.arange(Tw, device=dev), peak] += 12.0
        logits[n] = z.to(torch.bfloat16)
    cdev = torch.tensor(counts, dtype=torch.int32, device=dev)
    out = torch.empty(T, V, dtype=torch.float32, device=dev)
    cuts, scores = K.longform_cuts(logits, cdev, V, Hf, 0, plan.edge, plan.guard)
    flat = logits.view(Nw * Tw, V)

    c_med, c_min, c_max = timed(lambda: K.longform_cuts(logits, cdev, V, Hf, 0, plan.edge, plan.guard), args.warmup, args.calls)
    s_med, s_min, s_max = timed(lambda: K.longform_stitch(logits, cdev, cuts, V, Hf, T, out=out), args.warmup, args.calls)

    def both():
        c, _ = K.longform_cuts(logits, cdev, V, Hf, 0, plan.edge, plan.guard)
        K.longform_stitch(logits, cdev, c, V, Hf, T, out=out)

    b_med, b_min, b_max = timed(both, args.warmup, args.calls)

    def yard():  # (the entry point itself, writing into the same buffer as the stitch: no allocation in either timing)
        rc = K._lib.lib().ea_log_softmax_bf16(K._p(flat), V, K._p(out), T, V, K._stream())
        assert rc == 0

    y_med, y_min, y_max = timed(yard, args.warmup, args.calls)
    moved = T * V * (2 + 4)
    res = {"metric": "long_form_ctc", "seconds": args.seconds, "window_s": args.window_s, "overlap_s": args.overlap_s, "vocab": V,
           "windows": Nw, "window_frames": Tw, "hop_frames": Hf, "frames": T, "edge": plan.edge, "guard": plan.guard, "calls": args.calls,
           "window_logits_bytes": logits.numel() * 2, "stitched_bytes": out.numel() * 4,
           "cuts_ms": round(c_med, 4), "cuts_ms_min_max": [round(c_min, 4), round(c_max, 4)],
           "stitch_ms": round(s_med, 4), "stitch_ms_min_max": [round(s_min, 4), round(s_max, 4)],
           "cuts_plus_stitch_ms": round(b_med, 4), "cuts_plus_stitch_ms_min_max": [round(b_min, 4), round(b_max, 4)],
           "log_softmax_same_rows_ms": round(y_med, 4), "log_softmax_same_rows_ms_min_max": [round(y_min, 4), round(y_max, 4)],
           "stitch_GBps": round(moved / (s_med * 1e-3) / 1e9, 1), "log_softmax_GBps": round(moved / (y_med * 1e-3) / 1e9, 1),
           "worst_cut_score": round(float(scores.min()), 4)}
    del logits, out, flat

    if args.pipeline_seconds > 0:
        from espresso_amd.data.asr_dictionary import AsrDictionary
        from espresso_amd.models.transformer.speech_transformer_encoder_model import conformer_ctc_librispeech
        from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask

        torch.manual_seed(1)
        d = AsrDictionary.from_symbols([f"u{i}" for i in range(V - 5)], enable_bos=True)
        task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(criterion_name="ctc_loss"), tgt_dict=d)
        model = task.build_model(conformer_ctc_librispeech()).to(dev).eval()
        task.build_frontend(dev)
        lf = LF.LongFormCTC(task, LF.LongFormPlan.from_seconds(LF.samples_per_frame(task.frontend, model), 16000, args.window_s,
                                                               args.overlap_s), d.bos(), args.max_tokens, args.batch_size)
        wave = (np.random.default_rng(2).standard_normal(int(args.pipeline_seconds * 16000)) * 800).astype(np.float32)

        def run():
            lprobs, in_len, _, _ = lf.encode(model, wave)
            Tn = lprobs.shape[1]
            K.ctc_greedy_decode(lprobs.view(Tn, len(d)), in_len, 1, Tn, len(d), d.bos(), d.pad())
            torch.cuda.synchronize()

        run()  # warm-up: allocator, GEMM workspaces
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            run()
            times.append(time.perf_counter() - t0)
        res.update({"pipeline_seconds": args.pipeline_seconds, "pipeline_windows": lf.plan.num_windows(len(wave)),
                    "pipeline_s": round(float(np.median(times)), 4), "pipeline_s_min_max": [round(min(times), 4), round(max(times), 4)],
                    "pipeline_rtf": round(float(np.median(times)) / args.pipeline_seconds, 6),
                    "max_tokens": args.max_tokens, "batch_size": args.batch_size})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
