#!/usr/bin/env python3
"""Resampler in front of the fbank, measured: one batch of the training benchmark's shape (24 utterances, <= 26 000 frames at
16 kHz) held on the device as int16 samples at --rate, `ea_resample_batch_i16` and then `ea_fbank_batch` on its output, beside
`ea_fbank_batch_i16` on a 16 kHz batch of the same durations.  Times are device events around `--reps` launches after a warm-up;
bytes are what the algorithm needs (every int16 sample read once, every fp32 output written once).  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_resample.py ...` for per-kernel times (a run of its own).

    python tools/bench_resample.py --rate 48000 [--reps 50] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from espresso_amd import kernels as K  # noqa: E402
from espresso_amd.data import synthetic  # noqa: E402
from espresso_amd.data.gpu_frontend import GpuFbankFrontend  # noqa: E402
from espresso_amd.data.resample import resample_plan  # noqa: E402


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py needs the GPU")
    dev = torch.device("cuda:0")
    fo = 16000
    batches, n16 = synthetic.make_batches(2000, max_tokens=26000, max_sentences=24, seed=1)
    batch = max(batches, key=lambda b: int(synthetic.num_frames(n16[b]).max()) * len(b))  # the fullest batch
    seconds = n16[batch] / float(fo)
    n_in = [int(round(s * args.rate)) for s in seconds]
    plan = resample_plan(args.rate, fo)
    n_out = [plan.n_out(n) for n in n_in]
    rng = np.random.default_rng(1)

    def batch_i16(lens):
        off = np.zeros(len(lens) + 1, dtype=np.int64)
        off[1:] = np.cumsum(lens)
        wav = torch.from_numpy(rng.integers(-3000, 3000, size=int(off[-1]), dtype=np.int16)).to(dev)
        return wav, torch.from_numpy(off).to(dev)

    wav_in, off_in = batch_i16(n_in)
    wav_16, off_16 = batch_i16(n_out)
    out_off = off_16
    out = torch.empty(sum(n_out), dtype=torch.float32, device=dev)
    taps, first = plan.device(dev)
    fe = GpuFbankFrontend(dev)
    frames = [fe.num_frames(n) for n in n_out]
    B, Tmax = len(batch), max(frames)

    def resample():
        K.resample_batch(wav_in, off_in, out, out_off, B, taps, first, plan.in_unit, max(n_out))

    def fbank(w):
        return lambda: K.fbank_batch(w, out_off, B, fe.tables, None, None, Tmax, want_sum=False)

    t_rs = timed(resample, args.reps)
    t_fb32 = timed(fbank(out), args.reps)
    t_fb16 = timed(fbank(wav_16), args.reps)
    byts = 2 * sum(n_in) + 4 * sum(n_out)
    res = {"rate": args.rate, "utterances": B, "frames_padded": B * Tmax, "audio_s": float(seconds.sum()), "phases": plan.phases,
           "taps": plan.K, "samples_in": sum(n_in), "samples_out": sum(n_out), "resample_s": t_rs, "resample_bytes": byts,
           "resample_GBps": byts / t_rs * 1e-9, "flop": 2 * plan.K * sum(n_out), "fbank_on_resampled_fp32_s": t_fb32,
           "fbank_i16_at_16k_s": t_fb16, "reps": args.reps}
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
