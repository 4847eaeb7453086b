"""TEST INFRASTRUCTURE ONLY — plain references for the front-end kernels of espresso_amd/csrc/fbank.hip.

fbank64       the pipeline of fbank_kernel in float64 on the operands the kernel receives (the fp32 / int16 samples, the fp32 window,
              twiddle-free: an exact 512-point DFT by np.fft in float64, the fp32 mel weights through the mel_start / mel_len /
              mel_woff tables, the fp32 pre-emphasis constant, the fp32 CMVN mean and std), with the per-element hard bound of
              tests/test_frontend_kernels.py's docstring (`tol`) and, for the mutation tests, one deliberate defect (`mut`)
fbank_emul32  the same pipeline in numpy float32 with the kernel's own algorithm (the lane sums and the xor butterfly of wave_sum,
              the radix-2 DIT butterflies in the kernel's stage order on its twiddle table, sqrt then square, a running mel sum),
              vectorised over frames.  Not bit-equal to the kernel (fused multiply-adds): the yardstick of the rms bound
utt_sum64, specaugment64, feature_stats64     the remaining kernels, in float64"""
import math

import numpy as np

E23 = 2.0 ** -23
ETA = 7 * 2.0 ** -24      # Higham's FFT constant: twiddle error 2^-24 + four roundings of a butterfly times sqrt(2), rounded up
NFFT, LOG2N = 512, 9
LOG_FLOOR = float(np.finfo(np.float32).eps)
PREEMPH = float(np.float32(0.97))

MUTATIONS = ("frame_start", "window_index", "preemph_096", "no_replicate_pad", "no_dc_removal", "mel_shift", "mel_weight_dropped",
             "no_log_floor", "cmvn_on_padding", "sample_leak", "magnitude")


def num_frames(n, flen, fshift):
    return 0 if n < flen else 1 + (n - flen) // fshift


def tables_np(tab):
    """the dict of build_tables("cpu", ...) as numpy arrays"""
    return {k: v.detach().cpu().numpy() for k, v in tab.items()}


def dense_bank(tab, nmel):
    """float64 [nmel][256] from the sparse tables (what the kernel's inner loop multiplies with)"""
    W = np.zeros((nmel, NFFT // 2), dtype=np.float64)
    for m in range(nmel):
        s, n, o = int(tab["mel_start"][m]), int(tab["mel_len"][m]), int(tab["mel_woff"][m])
        W[m, s:s + n] = tab["mel_w"][o:o + n].astype(np.float64)
    return W


def _frame_index(off, b, flen, fshift, Tmax):
    n = int(off[b + 1] - off[b])
    nfr = num_frames(n, flen, fshift)
    nf = max(min(nfr, Tmax), 0)
    idx = int(off[b]) + np.arange(flen)[None, :] + fshift * np.arange(nf)[:, None]
    return nfr, nf, idx


def fbank64(wav, off, tab, Tmax, nmel, flen, fshift, mean=None, std=None, preemph=PREEMPH, log_floor=LOG_FLOOR, mut=None, mut_utt=0,
            want_tol=True):
    """-> dict: feat f64 [B][Tmax][nmel] (rows at or beyond an utterance's frame count are 0), nfr int [B] (not clamped to Tmax),
    valid bool [B][Tmax], tol f64 [B][Tmax][nmel] (0 on padding rows).  tab: tables_np(build_tables("cpu", ...))."""
    assert mut is None or mut in MUTATIONS
    wav = np.asarray(wav)
    B = len(off) - 1
    w64 = wav.astype(np.float64)
    win = tab["window"].astype(np.float64)
    W = dense_bank(tab, nmel)
    mlen = tab["mel_len"].astype(np.float64)
    if mut == "mel_shift":
        W = np.concatenate([np.zeros((nmel, 1)), W[:, :-1]], axis=1)
    if mut == "mel_weight_dropped":
        m = nmel // 2
        W[m, int(tab["mel_start"][m]) + int(tab["mel_len"][m]) // 2] = 0.0
    if mut == "window_index":
        win = np.concatenate([win[1:], win[-1:]])
    pre = 0.96 if mut == "preemph_096" else float(preemph)
    feat = np.zeros((B, max(Tmax, 0), nmel))
    tol = np.zeros_like(feat)
    valid = np.zeros((B, max(Tmax, 0)), dtype=bool)
    nfrs = np.zeros(B, dtype=np.int64)
    m64 = None if mean is None else np.asarray(mean, dtype=np.float32).astype(np.float64)
    s64 = None if std is None else np.asarray(std, dtype=np.float32).astype(np.float64)
    for b in range(B):
        nfr, nf, idx = _frame_index(off, b, flen, fshift, Tmax)
        nfrs[b] = nfr
        if mut == "cmvn_on_padding" and m64 is not None:
            feat[b, nf:] = (0.0 - m64) / s64
        if nf == 0:
            continue
        valid[b, :nf] = True
        if mut == "frame_start":
            idx = np.minimum(idx + 1, len(w64) - 1)
        x = w64[idx]
        if mut == "sample_leak" and b == mut_utt:
            x = x.copy()
            x[-1, -1] = w64[int(off[b + 1])]
        d = x if mut == "no_dc_removal" else x - x.mean(axis=1, keepdims=True)
        prev = np.concatenate([d[:, :1], d[:, :-1]], axis=1)
        if mut == "no_replicate_pad":
            prev[:, 0] = 0.0
        pe = d - pre * prev
        y = pe * win
        X = np.fft.fft(np.pad(y, ((0, 0), (0, NFFT - flen))), axis=1)
        aX = np.abs(X[:, :NFFT // 2])
        P = aX if mut == "magnitude" else aX * aX
        e = P @ W.T
        with np.errstate(divide="ignore"):
            ef = e if mut == "no_log_floor" else np.maximum(e, log_floor)
            v = np.log(ef)
        r = v if m64 is None else (v - m64) / s64
        feat[b, :nf] = r
        if not want_tol or mut is not None:
            continue
        # ---- the hard bound (tests/test_frontend_kernels.py, BOUND 1), term by term
        em = 15 * E23 * np.abs(x).mean(axis=1, keepdims=True)                  # the mean: 8 + 6 additions, the division
        dd = em + E23 * np.abs(d)                                              # x - mean
        dprev = np.concatenate([dd[:, :1], dd[:, :-1]], axis=1)
        dpe = dd + pre * dprev + 2 * E23 * (np.abs(d) + pre * np.abs(prev))    # the product with 0.97, the subtraction
        dy = win * dpe + E23 * np.abs(y)                                       # the product with the window
        normX = math.sqrt(NFFT) * np.sqrt((y * y).sum(axis=1, keepdims=True))  # ||X||_2 over the 512 bins (Parseval)
        delta = LOG2N * ETA * normX + dy.sum(axis=1, keepdims=True)            # |dX_q| <= ||dX||_2 (FFT) + ||dy||_1 (its input)
        dP = 2 * aX * delta + delta * delta + 5 * E23 * (aX + delta) ** 2      # re^2, im^2, +, sqrtf, the square
        de = dP @ W.T + (mlen + 1) * E23 * ((P + dP) @ W.T)                    # the running sum of mel_len products
        up = np.log(np.maximum(e + de, log_floor)) - v
        dn = v - np.log(np.maximum(e - de, log_floor))
        tl = np.maximum(up, dn) + 2 * E23 * np.abs(v)                          # logf charged 2 ulp
        tol[b, :nf] = tl if m64 is None else tl / s64 + 2 * E23 * np.abs(r)    # the subtraction and the division of CMVN
    return {"feat": feat, "nfr": nfrs, "valid": valid, "tol": tol}


def _bitrev9():
    return np.array([int(format(i, "09b")[::-1], 2) for i in range(NFFT)])


def fbank_emul32(wav, off, tab, Tmax, nmel, flen, fshift, mean=None, std=None, preemph=PREEMPH, log_floor=LOG_FLOOR):
    """-> f32 [B][Tmax][nmel]: fbank_kernel's algorithm in numpy float32 (every operation rounds once: no fused multiply-add)"""
    f32 = np.float32
    wav = np.asarray(wav)
    B = len(off) - 1
    win, tw = tab["window"].astype(f32), tab["twiddle"].astype(f32).reshape(-1, 2)
    st_, ln_, wo_, mw = tab["mel_start"], tab["mel_len"], tab["mel_woff"], tab["mel_w"].astype(f32)
    rev = _bitrev9()
    lanes = np.arange(64)
    feat = np.zeros((B, max(Tmax, 0), nmel), dtype=f32)
    for b in range(B):
        _, nf, idx = _frame_index(off, b, flen, fshift, Tmax)
        if nf == 0:
            continue
        x = np.zeros((nf, NFFT), dtype=f32)
        x[:, :flen] = wav[idx].astype(f32)
        s = np.zeros((nf, 64), dtype=f32)
        for k in range(8):                      # `sum += x[k]` per lane, then wave_sum's xor butterfly
            s = s + x[:, 64 * k:64 * k + 64]
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        mu = s[:, :1] / f32(flen)
        d = x[:, :flen] - mu
        prev = np.concatenate([d[:, :1], d[:, :-1]], axis=1)
        y = (d - f32(preemph) * prev) * win
        re = np.zeros((nf, NFFT), dtype=f32)
        im = np.zeros((nf, NFFT), dtype=f32)
        re[:, rev[:flen]] = y
        j = np.arange(NFFT // 2)
        for st in range(LOG2N):
            half = 1 << st
            pos = j & (half - 1)
            i0 = ((j >> st) << (st + 1)) + pos
            i1 = i0 + half
            wx, wy = tw[pos << (LOG2N - 1 - st), 0], tw[pos << (LOG2N - 1 - st), 1]
            ar, ai, br, bi = re[:, i0], im[:, i0], re[:, i1], im[:, i1]
            tr = br * wx - bi * wy
            ti = br * wy + bi * wx
            re[:, i0], im[:, i0], re[:, i1], im[:, i1] = ar + tr, ai + ti, ar - tr, ai - ti
        mag = np.sqrt(re[:, :256] * re[:, :256] + im[:, :256] * im[:, :256])
        pw = mag * mag
        e = np.zeros((nf, nmel), dtype=f32)
        for q in range(int(ln_[:nmel].max())):
            live = ln_[:nmel] > q
            col = np.where(live, st_[:nmel] + q, 0)
            wq = np.where(live, mw[np.minimum(wo_[:nmel] + q, len(mw) - 1)], f32(0))
            e = np.where(live[None, :], e + pw[:, col] * wq[None, :], e).astype(f32)
        v = np.log(np.maximum(e, f32(log_floor))).astype(f32)
        if mean is not None:
            v = ((v - np.asarray(mean, dtype=f32)) / np.asarray(std, dtype=f32)).astype(f32)
        feat[b, :nf] = v
    return feat


def utt_sum64(feat):
    """(sum, sum of magnitudes) per utterance of a stored feature tensor [B][Tmax][nmel] (padding rows are zero)"""
    f = np.asarray(feat, dtype=np.float64)
    return f.sum(axis=(1, 2)), np.abs(f).sum(axis=(1, 2))


def specaugment64(feat, lens, utt_sum, fmask, tmask, use_mean, mask_value):
    """specaug_kernel: -> (out f64 [B][Tmax][nmel], masked bool, val f64 [B]).  Masks int [B][n][2] = (start, width) or None; an
    utterance with lens[b] <= 0 is left alone; the value is utt_sum[b] / (lens[b] nmel) with use_mean"""
    out = np.asarray(feat, dtype=np.float64).copy()
    B, Tmax, nmel = out.shape
    masked = np.zeros(out.shape, dtype=bool)
    val = np.zeros(B)
    for b in range(B):
        n = int(lens[b])
        if n <= 0:
            continue
        val[b] = float(utt_sum[b]) / (float(n) * float(nmel)) if use_mean else float(np.float32(mask_value))
        for f0, fw in ([] if fmask is None else np.asarray(fmask)[b]):
            if fw > 0:
                masked[b, :n, f0:f0 + fw] = True
        for t0, tw in ([] if tmask is None else np.asarray(tmask)[b]):
            if tw > 0:
                masked[b, t0:t0 + tw, :] = True
        out[b][masked[b]] = val[b]
    return out, masked, val


def feature_stats64(feat, lens, acc0, calls=1):
    """feature_stats_kernel `calls` times onto acc0 f64 [2 nmel + 1] -> (acc, mag): mag = |acc0| + calls * sum |v| (sum v^2)"""
    f = np.asarray(feat, dtype=np.float64)
    B, Tmax, nmel = f.shape
    acc, mag = np.asarray(acc0, dtype=np.float64).copy(), np.abs(np.asarray(acc0, dtype=np.float64))
    for b in range(B):
        n = max(min(int(lens[b]), Tmax), 0)
        v = f[b, :n]
        acc[:nmel] += calls * v.sum(axis=0)
        acc[nmel:2 * nmel] += calls * (v * v).sum(axis=0)
        acc[2 * nmel] += calls * n
        mag[:nmel] += calls * np.abs(v).sum(axis=0)
        mag[nmel:2 * nmel] += calls * (v * v).sum(axis=0)
    return acc, mag
