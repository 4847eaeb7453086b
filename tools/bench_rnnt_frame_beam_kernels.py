"""Time of the offline frame-synchronous transducer beam search kernels alone: ea_rnnt_frame_beam_step (T calls) + _finish of
a given build of the library, on seeded logits (B 24, T 200, V 5004, beam 10, K 10; blank mostly ahead), without and with LM
rows.  `--lib PATH` loads that library file directly (only the three entry points are bound), so two builds can be timed on
the same box: run it in a fresh process per build, alternating, three times each, and quote both triples.  One JSON line:
median / min / max microseconds per frame over 7 timed searches after one warm-up (device events around the whole loop), and a
checksum of the results, which must agree between builds."""
import argparse
import ctypes
import json
import os

import torch

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--lib", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "espresso_amd", "csrc", "libespresso_amd.so"))
ap.add_argument("--tag", default="tree")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_rnnt_frame_beam_kernels.py measures on the GPU: no device found")
path, tag = args.lib, args.tag
lib = ctypes.CDLL(path)
c_int, c_long, c_float, vp = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
lib.ea_rnnt_frame_beam_workspace_bytes.restype = c_long
lib.ea_rnnt_frame_beam_workspace_bytes.argtypes = [c_int, c_int, c_int]
lib.ea_rnnt_frame_beam_step.restype = c_int
lib.ea_rnnt_frame_beam_step.argtypes = [vp, c_long, vp, c_long, c_int, vp, vp, vp, vp, vp] + [c_int] * 7 + [c_float, c_float, c_int, vp]
lib.ea_rnnt_frame_beam_finish.restype = c_int
lib.ea_rnnt_frame_beam_finish.argtypes = [vp] + [c_int] * 6 + [vp, vp, vp, vp, vp]
dev = "cuda:0"
B, T, V, beam, K = 24, 200, 5004, 10, 10
g = torch.Generator(device=dev).manual_seed(0)
x = torch.randn(8, B * beam, V, device=dev, generator=g) * 3
x[:, :, 0] += 6.0  # blank mostly ahead, as with a trained model
lm = torch.log_softmax(torch.randn(B * beam, V, device=dev, generator=g), -1)
ws = torch.empty(lib.ea_rnnt_frame_beam_workspace_bytes(B, T, beam), dtype=torch.uint8, device=dev)
in_len = torch.full((B,), T, dtype=torch.int32, device=dev)
par, tok = torch.empty(B * beam, dtype=torch.int32, device=dev), torch.empty(B * beam, dtype=torch.int32, device=dev)
keep = torch.empty(B * beam, dtype=torch.uint8, device=dev)
tokens = torch.empty(B, 3, T, dtype=torch.int32, device=dev)
lengths, scores = torch.empty(B, 3, dtype=torch.int32, device=dev), torch.empty(B, 3, device=dev)
nhyp = torch.empty(B, dtype=torch.int32, device=dev)
st = vp(torch.cuda.current_stream().cuda_stream)
p = lambda t: vp(t.data_ptr())

def search(with_lm):
    for t in range(T):
        rc = lib.ea_rnnt_frame_beam_step(p(x[t % 8]), V, p(lm) if with_lm else None, V, 0, p(in_len), p(ws), p(par), p(tok), p(keep), B, T, V,
                                         beam, K, 0, -1, 1.0, 0.3 if with_lm else 0.0, t, st)
        assert rc == 0, rc
    assert lib.ea_rnnt_frame_beam_finish(p(ws), B, T, beam, 3, 1, 1, p(tokens), p(lengths), p(scores), p(nhyp), st) == 0

out = {"lib": tag}
for with_lm in (False, True):
    search(with_lm)
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        search(with_lm)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / T * 1e3)
    ts.sort()
    out["lm" if with_lm else "no_lm"] = {"us_per_frame_median": round(ts[3], 2), "min": round(ts[0], 2), "max": round(ts[-1], 2)}
out["check"] = [int(lengths[:, 0].sum()), float(scores[:, 0].sum())]
print(json.dumps(out), flush=True)
