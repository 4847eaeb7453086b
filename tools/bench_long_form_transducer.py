"""Long-form recognition for transducer models (csrc/long_form.hip: ea_longform_feature_cuts, ea_longform_stitch_rows;
espresso_amd/tools/long_form.py LongFormTransducer) on a synthetic hour of audio at D = 512.

Kernels: the bf16 encoder outputs of the hour's windows (30 s windows, 6 s overlap: 150 windows x 750 frames) go through the two
kernels.  The yardstick of the stitch is a device-to-device copy of exactly the bytes it writes (and reads), timed by this tool
in the same run; the yardstick of the cuts is the bytes they must read -- both windows' rows of every overlap frame -- at that
copy's bandwidth (a copy of B bytes moves 2 B, so its time for the cuts' bytes is copy time x cuts bytes / (2 x copy bytes)).
Times are device events around the calls, median (min, max) of `--calls` after `--warmup`.

Pipeline: the recipe-size Conformer transducer (16 layers, d 512, 2-layer LSTM predictor, joint 512, V 5004, random weights)
over an hour of synthetic noise through `LongFormTransducerModel` and `TransducerFrameBeamDecoder(beam 5)`: wall clock with a
device synchronisation, split into the encoder part (front-end, encoder over batches of windows, cuts, stitch) and the search.
A random joint rarely prefers blank, so nearly every frame emits a token: the longest hypotheses the search can have.
`--pipeline-seconds 0` skips it.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

VOCAB = 5004


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
    ap.add_argument("--seconds", type=float, default=3600.0, help="audio behind the synthetic window features")
    ap.add_argument("--pipeline-seconds", type=float, default=3600.0, help="audio of the whole-pipeline run (0: skip it)")
    ap.add_argument("--pipeline-calls", type=int, default=2)
    ap.add_argument("--window-s", type=float, default=30.0)
    ap.add_argument("--overlap-s", type=float, default=6.0)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--max-tokens", type=int, default=15000)
    ap.add_argument("--batch-size", type=int, default=24)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    from espresso_amd import kernels as K
    from espresso_amd.tools import long_form as LF

    assert torch.cuda.is_available(), "bench_long_form_transducer.py measures on the GPU"
    dev = torch.device("cuda:0")
    D, G = args.dim, 640
    plan = LF.LongFormPlan.from_seconds(G, 16000, args.window_s, args.overlap_s)
    N = int(args.seconds * 16000)
    wins = plan.windows(N)
    Nw, Tw, Hf = len(wins), plan.Tw, plan.Hf
    counts = [-(-(1 + (ln - 400) // 160) // 4) for _, ln in wins]
    T = (Nw - 1) * Hf + counts[-1]
    g = torch.Generator(device=dev).manual_seed(1)
    # a common signal per global frame plus window-own noise that grows towards a window's ends, as an encoder without the
    # context across its border would give
    common = torch.randn((Nw - 1) * Hf + Tw, D, device=dev, generator=g)
    edge_noise = (torch.arange(Tw, device=dev, dtype=torch.float32) - (Tw - 1) / 2).abs() / (Tw / 2)
    x = torch.empty(Nw, Tw, D, dtype=torch.bfloat16, device=dev)
    for n in range(Nw):
        z = common[n * Hf: n * Hf + Tw] + (0.02 + 0.5 * edge_noise ** 4).unsqueeze(1) * torch.randn(Tw, D, device=dev, generator=g)
        x[n] = z.to(torch.bfloat16)
    del common
    cdev = torch.tensor(counts, dtype=torch.int32, device=dev)
    out = torch.empty(T, D, dtype=torch.bfloat16, device=dev)
    cuts, scores = K.longform_feature_cuts(x, cdev, D, Hf, plan.edge, plan.guard)
    src = x.view(Nw * Tw, D)[:T]

    c_med, c_min, c_max = timed(lambda: K.longform_feature_cuts(x, cdev, D, Hf, plan.edge, plan.guard), args.warmup, args.calls)
    s_med, s_min, s_max = timed(lambda: K.longform_stitch_rows(x, cdev, cuts, D, Hf, T, out=out), args.warmup, args.calls)

    def both():
        c, _ = K.longform_feature_cuts(x, cdev, D, Hf, plan.edge, plan.guard)
        K.longform_stitch_rows(x, cdev, c, D, Hf, T, out=out)

    b_med, b_min, b_max = timed(both, args.warmup, args.calls)
    y_med, y_min, y_max = timed(lambda: out.copy_(src), args.warmup, args.calls)  # device to device, the stitch's bytes
    copy_bytes = T * D * 2
    overlap_frames = sum(min(n * Hf + counts[n], (n + 1) * Hf + counts[n + 1]) - (n + 1) * Hf for n in range(Nw - 1))
    cuts_bytes = 2 * overlap_frames * D * 2
    res = {"metric": "long_form_transducer", "seconds": args.seconds, "window_s": args.window_s, "overlap_s": args.overlap_s, "dim": D,
           "windows": Nw, "window_frames": Tw, "hop_frames": Hf, "frames": T, "edge": plan.edge, "guard": plan.guard, "calls": args.calls,
           "window_features_bytes": x.numel() * 2, "stitched_bytes": copy_bytes, "cuts_read_bytes": cuts_bytes,
           "feature_cuts_ms": round(c_med, 4), "feature_cuts_ms_min_max": [round(c_min, 4), round(c_max, 4)],
           "stitch_rows_ms": round(s_med, 4), "stitch_rows_ms_min_max": [round(s_min, 4), round(s_max, 4)],
           "cuts_plus_stitch_ms": round(b_med, 4), "cuts_plus_stitch_ms_min_max": [round(b_min, 4), round(b_max, 4)],
           "copy_same_bytes_ms": round(y_med, 4), "copy_same_bytes_ms_min_max": [round(y_min, 4), round(y_max, 4)],
           "stitch_rows_GBps": round(2 * copy_bytes / (s_med * 1e-3) / 1e9, 1), "copy_GBps": round(2 * copy_bytes / (y_med * 1e-3) / 1e9, 1),
           "feature_cuts_read_GBps": round(cuts_bytes / (c_med * 1e-3) / 1e9, 1),
           "feature_cuts_bytes_at_copy_bandwidth_ms": round(y_med * cuts_bytes / (2 * copy_bytes), 4),
           "worst_cut_score": round(float(scores.min()), 6)}
    del x, out, src

    if args.pipeline_seconds > 0:
        from espresso_amd.data.asr_dictionary import AsrDictionary
        from espresso_amd.models.transformer.speech_transformer_config import SpeechTransformerTransducerConfig
        from espresso_amd.models.transformer.speech_transformer_transducer_base import SpeechTransformerTransducerModelBase
        from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
        from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder

        torch.manual_seed(1)
        d = AsrDictionary.from_symbols([f"u{i}" for i in range(VOCAB - 5)], enable_bos=True)
        task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(criterion_name="transducer_loss", seed=1), tgt_dict=d)
        cfg = SpeechTransformerTransducerConfig()
        e, dc = cfg.encoder, cfg.decoder
        e.embed_dim, e.ffn_embed_dim, e.layers, e.attention_heads = 512, 2048, 16, 8
        e.normalize_before, e.relative_positional_embeddings, e.layer_type = True, True, "conformer"
        e.conv_channels = "[64, 64, 128, 128]"
        dc.embed_dim, dc.hidden_size, dc.layers = 512, 512, 2
        cfg.joint_dim = 512
        cfg.max_source_positions, cfg.max_target_positions = 3600, 200
        model = SpeechTransformerTransducerModelBase.build_model(cfg, task).to(dev).eval()
        task.build_frontend(dev)
        lf = LF.LongFormTransducer(task, LF.LongFormPlan.from_seconds(LF.samples_per_frame(task.frontend, model.encoder), 16000,
                                                                      args.window_s, args.overlap_s), args.max_tokens, args.batch_size)
        shim = LF.LongFormTransducerModel(model, lf, search=(args.beam, 1, False, False))
        dec = TransducerFrameBeamDecoder([shim], d, beam_size=args.beam)
        rng = np.random.default_rng(2)

        def run(wave):
            t0 = time.perf_counter()
            E, enc_len = dec.encode({"net_input": shim.net_input(wave)})
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            tokens, lengths, _, _ = dec.search(E, enc_len)
            n_tok = int(lengths[0, 0])  # (synchronises)
            t2 = time.perf_counter()
            return t1 - t0, t2 - t1, E.shape[1], n_tok

        run((rng.standard_normal(int(min(args.pipeline_seconds, 90.0) * 16000)) * 800).astype(np.float32))  # warm-up: allocator, GEMM workspaces
        wave = (rng.standard_normal(int(args.pipeline_seconds * 16000)) * 800).astype(np.float32)
        runs = [run(wave) for _ in range(args.pipeline_calls)]
        enc_s, search_s = [r[0] for r in runs], [r[1] for r in runs]
        total = [a + b for a, b in zip(enc_s, search_s)]
        frames, n_tok = runs[0][2], runs[0][3]
        res.update({"pipeline_seconds": args.pipeline_seconds, "pipeline_windows": lf.plan.num_windows(len(wave)), "pipeline_calls": args.pipeline_calls,
                    "beam": args.beam, "pipeline_frames": frames, "pipeline_tokens": n_tok,
                    "pipeline_s": round(float(np.median(total)), 3), "pipeline_s_min_max": [round(min(total), 3), round(max(total), 3)],
                    "encode_s": round(float(np.median(enc_s)), 3), "encode_s_min_max": [round(min(enc_s), 3), round(max(enc_s), 3)],
                    "search_s": round(float(np.median(search_s)), 3), "search_s_min_max": [round(min(search_s), 3), round(max(search_s), 3)],
                    "search_us_per_frame": round(float(np.median(search_s)) / frames * 1e6, 2),
                    "pipeline_rtf": round(float(np.median(total)) / args.pipeline_seconds, 6),
                    "search_bytes": LF.frame_beam_search_bytes(frames, args.beam, 512), "max_tokens": args.max_tokens, "batch_size": args.batch_size})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
