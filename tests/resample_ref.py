"""fp64 reference of the polyphase resampler (espresso_amd/data/resample.py, csrc/resample.hip): the definition, restated.

    g = gcd(fi, fo), in_unit = fi / g, phases = fo / g, fc = 0.99 * 0.5 * min(fi, fo), W = 6 / (2 fc)
    phase p, t_out = p / fo:  lo_p = ceil((t_out - W) fi), hi_p = floor((t_out + W) fi),
    weight of input i in [lo_p, hi_p] at t = i / fi - t_out:  h(t) / fi
    h(t) = 0.5 (1 + cos(2 pi fc / 6 t)) sin(2 pi fc t) / (pi t) for |t| < W, h(0) = 2 fc, else 0
    y[j] = sum_k taps[j mod phases][k] x[first[j mod phases] + (j div phases) in_unit + k],  x = 0 outside [0, n)
    n_out = ceil(n fo / fi)

`table64` is that in numpy fp64; `apply64` evaluates y in fp64 on WHATEVER table it is given (the fp32 table of the code under
test, so that the table's rounding is an exact operand and not an error), on absolute indices with bases as the kernel takes
them, and returns per output the value and S_j = sum_k |w_k x_k|, the magnitude the fp32 rounding bound scales with."""
import math

import numpy as np

MUTATIONS = ("first_shifted", "phases_reversed", "right_edge_not_padded")


def geometry(fi, fo):
    g = math.gcd(fi, fo)
    return fi // g, fo // g  # in_unit, phases


def table64(fi, fo):
    """(taps fp64 [phases][K], first int64 [phases], K, in_unit, phases)"""
    in_unit, phases = geometry(fi, fo)
    fc = 0.99 * 0.5 * min(fi, fo)
    W = 6 / (2.0 * fc)
    rows, first = [], []
    for p in range(phases):
        t_out = p / fo
        lo, hi = math.ceil((t_out - W) * fi), math.floor((t_out + W) * fi)
        i = np.arange(lo, hi + 1, dtype=np.float64)
        t = i / fi - t_out
        with np.errstate(invalid="ignore", divide="ignore"):
            h = 0.5 * (1.0 + np.cos(2.0 * np.pi * fc / 6 * t)) * np.sin(2.0 * np.pi * fc * t) / (np.pi * t)
        h[t == 0.0] = 2.0 * fc
        h[np.abs(t) >= W] = 0.0
        rows.append(h / fi)
        first.append(lo)
    K = max(len(r) for r in rows)
    taps = np.zeros((phases, K), dtype=np.float64)
    for p, r in enumerate(rows):
        taps[p, :len(r)] = r
    return taps, np.asarray(first, dtype=np.int64), K, in_unit, phases


def n_out(n, fi, fo):
    return -((-n * fo) // fi)


def apply64(x, taps, first, in_unit, count, in_base=0, out_base=0, mut=None):
    """outputs out_base .. out_base + count of the samples x held from absolute index in_base on.  Returns (y, S), both fp64."""
    x = np.asarray(x, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    first = np.asarray(first, dtype=np.int64)
    phases, K = taps.shape
    j = out_base + np.arange(count, dtype=np.int64)
    p, u = j % phases, j // phases
    if mut == "phases_reversed":
        p = phases - 1 - p
    start = first[p] + u * in_unit + (1 if mut == "first_shifted" else 0)
    idx = start[:, None] + np.arange(K, dtype=np.int64)[None, :] - in_base
    n = len(x)
    ok = (idx >= 0) & (idx < n)
    if mut == "right_edge_not_padded":  # reads past the end repeat the last sample instead of 0
        xk = np.where(idx >= 0, x[np.clip(idx, 0, max(n - 1, 0))] if n else 0.0, 0.0)
    else:
        xk = np.where(ok, x[np.clip(idx, 0, max(n - 1, 0))] if n else 0.0, 0.0)
    prod = taps[p] * xk
    return prod.sum(1), np.abs(prod).sum(1)


def resample64(x, fi, fo, taps32=None):
    """a whole utterance offline; with the fp32 table of the code under test when given, else with the fp64 one"""
    taps, first, K, in_unit, phases = table64(fi, fo)
    if taps32 is not None:
        taps = taps32
    return apply64(x, taps, first, in_unit, n_out(len(x), fi, fo))
