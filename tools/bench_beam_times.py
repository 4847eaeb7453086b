"""Time of the kernels of the four token-level beam searches with and without time stamps, for a given build of the library:
the CTC prefix beam search offline (no LM: the whole utterance in one launch; with LM rows: one launch per frame) and streamed
(pieces of 40 frames), and the frame-synchronous transducer beam search offline and streamed (one frame per call), on seeded
inputs (B 24, V 5004, beam 10, K 10; CTC T 400, transducer T 200).  `--times` calls the ea_*_times_* entry points instead of
their twins.  `--lib PATH` loads that library file directly (the prototypes come from include/espresso_amd.h; entry points the
file does not export are skipped), so the build before time stamps can be timed on the same box: run it in a fresh process per
arm (parent, tree, tree --times), alternating, three times each, and quote the triples.  One JSON line: median / min / max
microseconds per frame over 7 timed searches after one warm-up (device events around the whole search), and a checksum of the
results, which must agree between the arms."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from espresso_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--lib", default=_lib.LIB_PATH)
ap.add_argument("--tag", default="tree")
ap.add_argument("--times", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_beam_times.py measures on the GPU: no device found")
lib = ctypes.CDLL(args.lib)
for name, (restype, argtypes) in _lib.parse_header().items():
    fn = getattr(lib, name, None) if ("ctc_prefix_beam" in name or "rnnt_frame_beam" in name) else None
    if fn is not None:
        fn.restype, fn.argtypes = restype, argtypes
dev = "cuda:0"
B, V, beam, K, NB = 24, 5004, 10, 10, 3
N = B * beam
g = torch.Generator(device=dev).manual_seed(0)
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def buf(nbytes):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)


def outputs(T):
    return [torch.empty(B, NB, T, dtype=torch.int32, device=dev), torch.empty(B, NB, dtype=torch.int32, device=dev),
            torch.empty(B, NB, device=dev), torch.empty(B, dtype=torch.int32, device=dev)]


par, tok = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
keep = torch.empty(N, dtype=torch.uint8, device=dev)
lm = torch.log_softmax(torch.randn(N, V, device=dev, generator=g), -1)
slots = torch.arange(B, dtype=torch.int32, device=dev)
TW = (None, None, None, 0, 0)  # no context graph
times = args.times

# ---- CTC
Tc, PIECE = 400, 40
z = torch.randn(B * Tc, V, device=dev, generator=g) * 2.0
peak = torch.where(torch.rand(B * Tc, device=dev, generator=g) < 0.5, torch.zeros(B * Tc, dtype=torch.long, device=dev),
                   torch.randint(1, V, (B * Tc,), device=dev, generator=g))
z[torch.arange(B * Tc, device=dev), peak] += 8.0
xc = torch.log_softmax(z, -1).contiguous()
del z
len_c = torch.full((B,), Tc, dtype=torch.int32, device=dev)
ws_c = buf(lib.ea_ctc_prefix_beam_workspace_bytes(B, Tc, beam))
tws_c = buf(lib.ea_ctc_prefix_beam_times_workspace_bytes(B, Tc, beam)) if times else None
out_c = outputs(Tc)
tout_c = [torch.empty(B, NB, Tc, dtype=torch.int32, device=dev), torch.empty(B, NB, device=dev)]


def ctc_step(lm_rows, t0, t1):
    lmargs = (p(lm_rows), V if lm_rows is not None else 0, p(par) if lm_rows is not None else None, p(tok) if lm_rows is not None else None,
              p(keep) if lm_rows is not None else None)
    tail = (B, Tc, V, beam, K, 0, 0.4 if lm_rows is not None else 0.0, 0.0, t0, t1, st)
    if times:
        rc = lib.ea_ctc_prefix_beam_times_step(p(xc), V, 0, p(len_c), p(ws_c), p(tws_c), *lmargs, None, None, None, 0, 0, *tail)
    else:
        rc = lib.ea_ctc_prefix_beam_step(p(xc), V, 0, p(len_c), p(ws_c), *lmargs, *tail)
    assert rc == 0, rc


def ctc_finish(lm_rows):
    a = (p(lm_rows), V if lm_rows is not None else 0, 0.4 if lm_rows is not None else 0.0, 0.0, 2)
    o = [p(t) for t in out_c]
    if times:
        rc = lib.ea_ctc_prefix_beam_times_finish(p(ws_c), p(tws_c), *a, None, 0, B, Tc, beam, NB, 1, *o, p(tout_c[0]), p(tout_c[1]), st)
    else:
        rc = lib.ea_ctc_prefix_beam_finish(p(ws_c), *a, B, Tc, beam, NB, 1, *o, st)
    assert rc == 0, rc


def ctc_offline():
    ctc_step(None, 0, Tc)
    ctc_finish(None)


def ctc_offline_lm():
    for t in range(Tc):
        ctc_step(lm, t, t + 1)
    ctc_finish(lm)


state_c = buf(B * lib.ea_ctc_prefix_beam_stream_state_bytes(Tc, beam))
tstate_c = buf(B * lib.ea_ctc_prefix_beam_stream_times_state_bytes(Tc, beam)) if times else None
n_new = torch.full((B,), PIECE, dtype=torch.int32, device=dev)
row_off = torch.arange(B, dtype=torch.int32, device=dev) * PIECE
# pieces packed stream by stream: [Tc / PIECE][B][PIECE][V] views of the batch-major rows
xs = xc.view(B, Tc // PIECE, PIECE, V).transpose(0, 1).contiguous()


def ctc_streamed():
    if times:
        assert lib.ea_ctc_prefix_beam_stream_times_reset(p(state_c), p(tstate_c), p(slots), B, B, Tc, beam, st) == 0
    else:
        assert lib.ea_ctc_prefix_beam_stream_reset(p(state_c), p(slots), B, B, Tc, beam, st) == 0
    for k in range(Tc // PIECE):
        head = (p(xs[k]), V, 0, B * PIECE, p(slots), p(n_new), p(row_off), 0, PIECE, B, p(state_c))
        tail = (None, 0, None, None, None, *TW, B, Tc, V, beam, K, 0, 0.0, 0.0, st)
        rc = lib.ea_ctc_prefix_beam_stream_times_step(*head, p(tstate_c), *tail) if times else lib.ea_ctc_prefix_beam_stream_step(*head, *tail)
        assert rc == 0, rc
    o = [p(t) for t in out_c]
    a = (p(slots), B, None, 0, 0.0, 0.0, -1, None, 0, B, Tc, beam, NB, 1, Tc)
    if times:
        rc = lib.ea_ctc_prefix_beam_stream_times_finish(p(state_c), p(tstate_c), *a, *o, p(tout_c[0]), p(tout_c[1]), st)
    else:
        rc = lib.ea_ctc_prefix_beam_stream_finish(p(state_c), *a, *o, st)
    assert rc == 0, rc


# ---- transducer
Tr = 200
xr = torch.randn(8, N, V, device=dev, generator=g) * 3
xr[:, :, 0] += 6.0  # blank mostly ahead, as with a trained model
len_r = torch.full((B,), Tr, dtype=torch.int32, device=dev)
ws_r = buf(lib.ea_rnnt_frame_beam_workspace_bytes(B, Tr, beam))
tws_r = buf(lib.ea_rnnt_frame_beam_times_workspace_bytes(B, Tr, beam)) if times else None
out_r = outputs(Tr)
tout_r = [torch.empty(B, NB, Tr, dtype=torch.int32, device=dev), torch.empty(B, NB, device=dev)]


def rnnt_offline(with_lm=False):
    for t in range(Tr):
        head = (p(xr[t % 8]), V, p(lm) if with_lm else None, V, 0, p(len_r), p(ws_r))
        tail = (B, Tr, V, beam, K, 0, -1, 1.0, 0.3 if with_lm else 0.0, t, st)
        if times:
            rc = lib.ea_rnnt_frame_beam_times_step(*head, p(tws_r), p(par), p(tok), p(keep), *TW, *tail)
        else:
            rc = lib.ea_rnnt_frame_beam_step(*head, p(par), p(tok), p(keep), *tail)
        assert rc == 0, rc
    o = [p(t) for t in out_r]
    if times:
        rc = lib.ea_rnnt_frame_beam_times_finish(p(ws_r), p(tws_r), None, 0, B, Tr, beam, NB, 1, 1, *o, p(tout_r[0]), p(tout_r[1]), st)
    else:
        rc = lib.ea_rnnt_frame_beam_finish(p(ws_r), B, Tr, beam, NB, 1, 1, *o, st)
    assert rc == 0, rc


state_r = buf(B * lib.ea_rnnt_frame_beam_stream_state_bytes(Tr, beam))
tstate_r = buf(B * lib.ea_rnnt_frame_beam_stream_times_state_bytes(Tr, beam)) if times else None
one = torch.ones(B, dtype=torch.int32, device=dev)


def rnnt_streamed():
    if times:
        assert lib.ea_rnnt_frame_beam_stream_times_reset(p(state_r), p(tstate_r), p(slots), B, 0, B, Tr, beam, st) == 0
    else:
        assert lib.ea_rnnt_frame_beam_stream_reset(p(state_r), p(slots), B, B, Tr, beam, st) == 0
    for t in range(Tr):
        head = (p(xr[t % 8]), V, None, V, 0, p(slots), p(one), 0, B, p(state_r))
        tail = (B, Tr, V, beam, K, 0, -1, 1.0, 0.0, st)
        if times:
            rc = lib.ea_rnnt_frame_beam_stream_times_step(*head, p(tstate_r), p(par), p(tok), p(keep), *TW, *tail)
        else:
            rc = lib.ea_rnnt_frame_beam_stream_step(*head, p(par), p(tok), p(keep), *tail)
        assert rc == 0, rc
    o = [p(t) for t in out_r]
    if times:
        rc = lib.ea_rnnt_frame_beam_stream_times_finish(p(state_r), p(tstate_r), p(slots), B, B, Tr, beam, None, 0, NB, 1, 1, Tr, *o,
                                                        p(tout_r[0]), p(tout_r[1]), st)
    else:
        rc = lib.ea_rnnt_frame_beam_stream_finish(p(state_r), p(slots), B, B, Tr, beam, NB, 1, 1, Tr, *o, st)
    assert rc == 0, rc


out = {"lib": args.tag, "times": times}
for name, fn, T, res in (("ctc_offline", ctc_offline, Tc, out_c), ("ctc_offline_lm", ctc_offline_lm, Tc, out_c),
                         ("ctc_streamed", ctc_streamed, Tc, out_c), ("rnnt_offline", rnnt_offline, Tr, out_r),
                         ("rnnt_offline_lm", lambda: rnnt_offline(True), Tr, out_r), ("rnnt_streamed", rnnt_streamed, Tr, out_r)):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / T * 1e3)
    ts.sort()
    out[name] = {"us_per_frame_median": round(ts[3], 2), "min": round(ts[0], 2), "max": round(ts[-1], 2),
                 "check": [int(res[1][:, 0].sum()), round(float(res[2][:, 0].sum()), 3)]}
print(json.dumps(out), flush=True)
