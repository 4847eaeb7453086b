"""Measure the long-form per-token posterior kernel (csrc/prefix_posterior_long.hip) once: its error against float64 at
recording scale and its time per anti-diagonal of tiles.  A tool, not a test: the float64 oracle takes about a minute per input
on the host.

Error (`--T --U --V`, default 24 000 frames, 6 000 tokens, 64 symbols).  A synthetic CTC model that agrees with the transcript:
every token gets one frame of its own at a random even position (so a blank frame lies between neighbours), the logits are
N(0, 1) plus `bonus` on the frame's label (blank elsewhere), log-softmax in float64, stored as fp32.  Two inputs: `peaked` (bonus
8) and `flat` (bonus 2, the mass spread over many alignments, |total| an order of magnitude larger).  The oracle is the recurrence
of include/espresso_amd.h in numpy float64 on the fp32 values; reported are the largest errors of Psi and total, of the tokens'
factors log c_1 .. log c_U (largest, median, 99.9th percentile) and, apart, of the end factor log c_end = total - Psi_U, whose
two terms are not neighbours and share no error, and ulp32(|total|).  `--oracle-dir` keeps the oracle's result between runs (keyed by the input's shape, seed and a
checksum of the matrix).  On the peaked input 2 % of the tokens are then replaced at random and the mean log c of the correct and
of the replaced tokens is reported: what the factors are for.

Time (`--hour`).  The two recordings of DESIGN.md section 8.5: T = 90 000, (a) V = 5 000, U = 12 000 and (b) V = 32, U = 54 000,
log-softmax of 3 N(0, 1), random targets with 5 % adjacent repeats; `kernels.ctc_prefix_posteriors_long`, device events around the
call, median (min - max) of `--calls` calls after one warm-up call, and the same divided by the nI + nJ - 1 anti-diagonals.

Prints one JSON line."""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

BLANK = 0


def synthetic_model(T, U, V, bonus, seed):
    """(x fp32 [T][V] log-probs, y int32 [U]) of the module docstring."""
    rng = np.random.default_rng(seed)
    y = rng.integers(1, V, size=U).astype(np.int32)
    starts = np.sort(rng.choice(T // 2, size=U, replace=False)) * 2
    label = np.full(T, BLANK)
    label[starts] = y
    z = rng.standard_normal((T, V))
    z[np.arange(T), label] += bonus
    z -= z.max(-1, keepdims=True)
    return (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32), y


def oracle(x, y, progress=None):
    """float64 (psi [U], total) of the CTC prefix recurrence on x [T][V] (any float dtype), y [U]."""
    T, U = x.shape[0], len(y)
    S = 2 * U + 1
    lab = np.full(S, BLANK)
    lab[1::2] = y
    allow2 = np.zeros(S, dtype=bool)
    allow2[3::2] = lab[3::2] != lab[1:-2:2]
    a = np.full(S, -np.inf)
    a[0] = x[0, BLANK]
    psi = np.full(U, -np.inf)
    if U:
        a[1] = x[0, lab[1]]
        psi[0] = a[1]
    c1, c2 = np.full(S, -np.inf), np.full(S, -np.inf)
    t_last = time.perf_counter()
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            e = x[t, lab].astype(np.float64)
            c1[1:] = a[:-1]
            c2[2:] = a[:-2]
            c2[~allow2] = -np.inf
            enter = np.logaddexp(c1, c2) + e
            psi = np.logaddexp(psi, enter[1::2])
            a = np.logaddexp(a + e, enter)
            if progress and time.perf_counter() - t_last > 30:
                t_last = time.perf_counter()
                print(f"| oracle {progress}: frame {t} of {T}", file=sys.stderr, flush=True)
        total = np.logaddexp(a[S - 1], a[S - 2] if S > 1 else -np.inf)
    return psi, float(total)


def cached_oracle(x, y, tag, cache_dir):
    key = f"{tag}_{x.shape[0]}_{len(y)}_{x.shape[1]}_{hashlib.sha1(x.tobytes() + y.tobytes()).hexdigest()[:16]}.npz"
    path = os.path.join(cache_dir, key) if cache_dir else None
    if path and os.path.exists(path):
        d = np.load(path)
        return d["psi"], float(d["total"]), 0.0
    t0 = time.perf_counter()
    psi, total = oracle(x, y, progress=tag)
    sec = time.perf_counter() - t0
    if path:
        os.makedirs(cache_dir, exist_ok=True)
        np.savez(path, psi=psi, total=np.float64(total))
    return psi, total, sec


def factors(psi, total):
    chain = np.concatenate([[0.0], psi, [total]])
    with np.errstate(invalid="ignore"):
        d = np.minimum(chain[1:] - chain[:-1], 0.0)
    return np.where(np.isneginf(chain[1:]), -np.inf, d)


def max_err(got, want):
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    m = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), m), "the kernel's -inf / NaN pattern differs from the oracle's"
    return float(np.abs(got[m] - want[m]).max()) if m.any() else 0.0


def timed(K, x, y, V, calls):
    T = x.shape[0]
    tb, ts = K.ctc_viterbi_long_tile()
    diagonals = -(-T // tb) + -(-(2 * y.numel() + 1) // ts) - 1
    ms = []
    for k in range(calls + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        K.ctc_prefix_posteriors_long(x, y, T, V, BLANK)
        b.record()
        torch.cuda.synchronize()
        if k:  # (the first call warms up)
            ms.append(a.elapsed_time(b))
    ms.sort()
    med = ms[len(ms) // 2]
    return {"ms": round(med, 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3), "anti_diagonals": diagonals,
            "us_per_anti_diagonal": round(med * 1000.0 / diagonals, 2), "us_per_frame_of_a_tile": round(med * 1000.0 / diagonals / tb, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=24000)
    ap.add_argument("--U", type=int, default=6000)
    ap.add_argument("--V", type=int, default=64)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--oracle-dir", default=None, help="keep the float64 oracle's results here between runs")
    ap.add_argument("--oracle-only", action="store_true", help="compute (and keep) the oracles on the host, touch no device")
    ap.add_argument("--hour", action="store_true", help="also time the two one-hour recordings of DESIGN.md section 8.5")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    T, U, V = args.T, args.U, args.V
    res = {"T": T, "U": U, "V": V}
    inputs = {tag: synthetic_model(T, U, V, bonus, seed) for tag, bonus, seed in (("peaked", 8.0, 1), ("flat", 2.0, 2))}
    oracles = {tag: cached_oracle(x, y, tag, args.oracle_dir) for tag, (x, y) in inputs.items()}
    if args.oracle_only:
        print(json.dumps({tag: {"total": o[1], "oracle_seconds": round(o[2], 1)} for tag, o in oracles.items()}))
        return
    from espresso_amd import kernels as K

    dev = torch.device("cuda:0")
    for tag, (x, y) in inputs.items():
        psi64, total64, sec = oracles[tag]
        xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        logc, total, psi = (t.cpu().numpy() for t in K.ctc_prefix_posteriors_long(xd, yd, T, V, BLANK, want_psi=True))
        f64 = factors(psi64, total64)
        err = np.abs(logc[:U].astype(np.float64) - f64[:U])
        r = {"total": round(total64, 3), "ulp_total": float(np.spacing(np.float32(abs(total64)))), "oracle_seconds": round(sec, 1),
             "max_err_psi": max_err(psi, psi64), "max_err_total": max_err(total[0], total64),
             "max_err_logc_tokens": max_err(logc[:U], f64[:U]), "median_err_logc_tokens": float(np.median(err)),
             "p999_err_logc_tokens": float(np.quantile(err, 0.999)), "logc_end": round(float(f64[U]), 3),
             "err_logc_end": max_err(logc[U], f64[U]), "mean_logc": float(logc[:U].mean())}
        r.update(timed(K, xd, yd, V, args.calls))
        res[tag] = r
        if tag == "peaked":  # 2 % of the transcript replaced: what the factors say about the replaced tokens
            rng = np.random.default_rng(3)
            bad = rng.random(U) < 0.02
            y2 = y.copy()
            y2[bad] = (y[bad] - 1 + rng.integers(1, V - 1, size=int(bad.sum()))) % (V - 1) + 1  # another id in [1, V)
            assert (y2[bad] != y[bad]).all() and y2.min() >= 1 and y2.max() < V
            lc = K.ctc_prefix_posteriors_long(xd, torch.from_numpy(y2).to(dev), T, V, BLANK)[0].cpu().numpy()[:U]
            res["replaced"] = {"tokens": int(bad.sum()), "mean_logc_correct": float(lc[~bad].mean()),
                               "mean_logc_replaced": float(lc[bad].mean())}
    if args.hour:
        g = torch.Generator(device=dev).manual_seed(0)
        for tag, (v, u) in (("hour_a_V5000_U12000", (5000, 12000)), ("hour_b_V32_U54000", (32, 54000))):
            x = torch.log_softmax(torch.randn(90000, v, generator=g, device=dev) * 3.0, -1)
            y = torch.randint(1, v, (u,), generator=g, device=dev, dtype=torch.int32)
            rep = torch.rand(u, generator=g, device=dev) < 0.05
            rep[0] = False
            idx = torch.arange(u, device=dev)
            y = y[torch.where(rep, idx - 1, idx)].contiguous()  # (a repeat copies its left neighbour's draw)
            from espresso_amd import _lib

            res[tag] = dict(timed(K, x, y, v, args.calls), workspace_bytes=int(_lib.lib().ea_ctc_prefix_long_workspace_bytes(90000, u)))
            del x
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
