"""The front-end kernels (espresso_amd/csrc/fbank.hip: fbank_kernel<float / int16_t>, specaug_kernel, feature_stats_kernel behind
ea_fbank_batch, ea_fbank_batch_i16, ea_specaugment, ea_feature_stats) one launch at a time against the plain fp64 restatement in
tests/frontend_ref.py, through the C ABI with build_tables on the device, every element of every output.

BUFFERS (tests/test_convmodule_kernels.py's Buf).  Every device tensor is a view into a larger allocation: NaN guards around fp32
inputs (the last utterance ends at the guard), guards of an extreme value around integer inputs (-32768 around int16 samples,
INT32_MIN around lengths, mask lists and the mel index tables: a negative length or width is skipped, nothing is dereferenced
through it; -1 around the int64 offsets), a sentinel bit pattern around outputs, checked after the call.  feat starts as NaN (or as
known data for ea_specaugment, which updates it), utt_sum as zeros and acc as known data (both accumulate), out_len as the sentinel.
Neighbouring utterances are drawn 16 times apart in scale.  No element is excluded from any comparison.

BOUND 1 (hard, derived, per element; frontend_ref.fbank64 computes it next to the value).  e = 2^-23 per fp32 rounding (one
rounding is 2^-24 relative: the factor two pays for second-order terms), all magnitudes in fp64 on the kernel's operands:
  mean      15 e mean|x|                        fbank.hip:57-62: 8 running additions, 6 wave steps, the division
  x - mean  dd = that + e |d|                   :66
  pre-emph  dpe = dd_i + 0.97 dd_(i-1) + 2 e (|d_i| + 0.97 |d_(i-1)|)          :78, the product and the subtraction
  window    dy = w_i dpe + e |y_i|              :78 (the fp32 window table is an operand, not charged)
  FFT       delta = log2(512) eta ||X||_2 + ||dy||_1,  eta = 7 * 2^-24        :93-109.  Higham (Accuracy and Stability of Numerical
            Algorithms, 24.1): ||fl(X) - X||_2 <= log2(N) eta ||X||_2 with eta = mu + gamma_4 (sqrt 2 + mu); mu = 2^-24 for a
            correctly rounded twiddle table (asserted below), gamma_4 = 4 * 2^-24 for the four roundings of a butterfly output:
            6.66 * 2^-24, rounded up.  One bin can carry the whole vector's error, and the whole input perturbation.
  power     dP = 2 |X_q| delta + delta^2 + 5 e (|X_q| + delta)^2              :115-116: re^2, im^2, +, sqrtf, the square
  mel       de = sum_q w_q dP_q + (mel_len + 1) e sum_q w_q (P_q + dP_q)      :127, the running sum of mel_len products
  log       max(log(max(e + de, floor)) - v, v - log(max(e - de, floor))) + 2 e |v|      :128.  The first term is de / e to first
            order; it is taken exactly because log is concave (de / e is no bound on the lower side).  The device logf's ulp is not
            documented on this machine: 2 ulp are charged.
  CMVN      tol / std + 2 e |(v - mean) / std|  :129, the subtraction and the division
On flat-spectrum noise this bound is loose (median about 4e-4; the share of elements above 1e-2 is printed per case): it cannot
false-fail, it catches gross faults, and it is the whole statement for the high-dynamic-range utterance.

BOUND 2 (sharp).  Per flat-spectrum case the rms over all valid elements of (kernel - fbank64) must be <= 2 x the rms of
(fbank_emul32 - fbank64) on the same case: the emulation is the kernel's algorithm in numpy float32, the same count of roundings in
other places (no fused multiply-add); the factor 2 covers sampling noise and a 2-ulp logf.  The emulation's rms comes from the
references alone and is printed per case.  The mutation tests must fail THIS bound (or, where the defect touches no valid element
or makes one non-finite, the exact check it violates).

EXACT.  Padding rows (frame >= the utterance's count, < Tmax) are +0 in their bits.  Rows >= Tmax are not stored (the next utterance's
rows and the trailing sentinel are intact) and not summed.  out_len = 1 + (N - frame_len) / frame_shift or 0, NOT clamped to Tmax
(pinned here and in include/espresso_amd.h).  An all-zero and a constant utterance (integer samples: the mean is exact) give
e = 0 in every bin: every element equals the floored log, CMVN applied in fp32 (a subtraction and a division, both correctly
rounded), bit for bit.  The floored log is ONE fp32 value, the device's logf(2^-23): it is read from a launch of the same batch
without CMVN, where every element of both utterances must hold it, and held to the 2 ulp charged to logf above.  (Measured on
gfx950: -15.94238567352295, 0.55 ulp from log(2^-23) = -15.942385152878742 and one ulp from the correctly rounded
-15.942384719848633 that numpy gives: demanding numpy's value fails at every element, so the device's logf is not correctly
rounded here, within its bound.)  ea_fbank_batch_i16 on the same integer samples is bit-identical to ea_fbank_batch.
utt_sum   against the fp64 sum of the kernel's own stored features: (16 ceil(nmel / 64) + 6 + blocks) e sum|v| (:124-137: a lane adds
          ceil(nmel / 64) values per frame, 6 wave steps, a wavefront 4 frames, 4 atomics per block: 4 blocks + ceil(nmel / 64) + 10
          roundings of 2^-24, below this), asserted to stay below one frame's share.
ea_specaugment   unmasked elements, padding rows and a len = 0 utterance bit-unchanged; masked = mask_value exactly, or
          utt_sum[b] / (n nmel) within 3 e with use_mean (:148: two conversions, an exact product, one division).
ea_feature_stats  count exact; sums within (64 + blocks + 1) 2^-52 (|acc0| + sum|v|) (or sum v^2) (:171-179: 64 running fp64 additions,
          one fp64 atomic per block of every call).

FINDING.  fbank_launch returned for Tmax <= 0 before anything wrote out_len, which kernels.fbank_batch allocates uninitialised and
ea_specaugment uses as a loop bound; it is now set to 0 (test_fbank_batch_without_a_single_frame fails on the parent commit).

The first tests need no GPU: fbank64 against oracle/fbank_ref.py, the tables, the mask-range property of draw_masks, eleven
mutations, every case of every GPU test built on the CPU with its preconditions asserted."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from espresso_amd.data.fbank_tables import build_tables
from oracle import fbank_ref
from tests import frontend_ref as FR
from tests.test_convmodule_kernels import _INT, _SENTINEL, DEV, Buf, _check, _gen, _st, _sync, inp, lib, out  # noqa: F401 (lib: the fixture)

gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
E23 = 2.0 ** -23
I32_MIN = -2 ** 31
CONFIGS = [(80, 16000), (40, 16000), (128, 16000), (80, 8000), (23, 8000)]


def _geom(rate):
    return int(rate * 0.025), int(rate * 0.010)


@functools.lru_cache(maxsize=None)
def _tab(nmel, rate):
    return FR.tables_np(build_tables("cpu", nmel, _geom(rate)[0], 512, float(rate)))


def _ptr(b):
    return None if b is None else b.p


class IBuf:
    """an integer device tensor between guards of `guard` (an input) or of the sentinel (an output, which also starts as it)"""

    def __init__(self, data=None, dtype=torch.int32, guard=None, n=None, pad=128):
        self.out = data is None
        n = n if self.out else data.numel()
        fill = (_SENTINEL[F32] if self.out else guard)
        full = torch.full((n + 2 * pad,), fill, dtype=dtype)
        if not self.out:
            full[pad:pad + n] = data.reshape(-1).to(dtype)
        self.full, self.pad, self.n, self.fill = full.to(DEV), pad, n, fill
        self.t = self.full[pad:pad + n]

    @property
    def p(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool((self.full[:self.pad] == self.fill).all()) and bool((self.full[self.pad + self.n:] == self.fill).all())

    def untouched(self):
        return self.out and bool((self.full == self.fill).all())

    def cpu(self):
        return self.t.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(what, got, want):
    bad = _bits(got) != _bits(want)
    if got.shape != want.shape or bool(bad.any()):
        i = tuple(int(k) for k in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ in their bits, first at {i}: got {float(got[i])!r}, want {float(want[i])!r}")


def _outside(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------ the references and the tables (CPU)
def _counts(flen, fshift):
    """0, one short of a frame, one frame, one short of two, two, 17, 33 and 50 frames (the longest last, a ragged tail on two)"""
    return [0, flen - 1, flen, flen + fshift - 1, flen + fshift, flen + 16 * fshift, flen + 32 * fshift + 7, flen + 50 * fshift - 1]


def _noise_batch(seed, flen, fshift, counts=None):
    """integer-valued flat-spectrum noise at int16 scale, utterance b at 25 * 16^(b % 3) with a DC offset of a quarter of it"""
    rng = np.random.default_rng(seed)
    counts = _counts(flen, fshift) if counts is None else counts
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    parts = []
    for b, n in enumerate(counts):
        sc = 25.0 * 16.0 ** (b % 3)
        parts.append(np.clip(np.rint(rng.standard_normal(n) * sc + 0.25 * sc), -32767, 32767))
    return np.concatenate(parts).astype(np.float32), off


def _cmvn(nmel, seed):
    rng = np.random.default_rng(1000 + seed)
    return (rng.standard_normal(nmel) * 2 + 8).astype(np.float32), (rng.random(nmel) + 2.0).astype(np.float32)


def _oracle_fbank_512(wav, nmel, rate):
    """oracle.fbank_ref.fbank's statements with its own povey_window and mel_banks, the FFT padded to 512 points whatever the frame
    length.  fbank_kernel always transforms 512 points; the oracle (as Kaldi) pads a 200-sample frame of 8 kHz audio to 256, so at
    8 kHz the oracle's own entry point computes another quantity (twice as coarse a spectrum).  At 16 kHz the two are the same
    function, which the caller asserts bit for bit."""
    wl, ws = _geom(rate)
    wav = np.asarray(wav, dtype=np.float32)
    if wav.shape[0] < wl:
        return np.zeros((0, nmel), dtype=np.float32)
    m = 1 + (wav.shape[0] - wl) // ws
    frames = wav[np.arange(wl)[None, :] + ws * np.arange(m)[:, None]].astype(np.float32)
    frames = frames - frames.mean(axis=1, keepdims=True, dtype=np.float32)
    prev = np.concatenate([frames[:, :1], frames[:, :-1]], axis=1)
    frames = (frames - np.float32(0.97) * prev) * fbank_ref.povey_window(wl)[None, :]
    spec = np.fft.rfft(np.pad(frames, ((0, 0), (0, 512 - wl))).astype(np.float32), axis=1)
    power = (np.abs(spec).astype(np.float32)) ** np.float32(2.0)
    bank = np.pad(fbank_ref.mel_banks(nmel, 512, float(rate)), ((0, 0), (0, 1)))
    return np.log(np.maximum(power.astype(np.float32) @ bank.T, fbank_ref.EPS)).astype(np.float32)


@pytest.mark.parametrize("nmel,rate", CONFIGS)
def test_reference_matches_the_fp32_oracle(nmel, rate):
    """fbank64 == oracle.fbank_ref.fbank + global_cmvn per utterance (at 8 kHz: the oracle's statements at the kernel's 512 points,
    _oracle_fbank_512).  The oracle is fp32 end to end (measured 4.6e-5 from fp64 on white noise), so the bound is fbank64's own
    derived fp32 bound, which covers any correctly ordered fp32 evaluation of the chain with an FFT of at most log2(512) stages —
    and 1e-3 absolute, check_frontend's figure, as a ceiling on it here"""
    flen, fshift = _geom(rate)
    wav, off = _noise_batch(3, flen, fshift)
    mean, std = _cmvn(nmel, 3)
    for cm in (None, (mean, std)):
        r = FR.fbank64(wav, off, _tab(nmel, rate), 51, nmel, flen, fshift, *(cm or (None, None)))
        assert list(r["nfr"]) == [0, 0, 1, 1, 2, 17, 33, 50]
        for b in range(len(off) - 1):
            o = _oracle_fbank_512(wav[off[b]:off[b + 1]], nmel, rate)
            if rate == 16000:
                assert np.array_equal(o, fbank_ref.fbank(wav[off[b]:off[b + 1]], nmel, float(rate)))
            if cm:
                o = fbank_ref.global_cmvn(o, mean.astype(np.float64), std.astype(np.float64))
            n = int(r["nfr"][b])
            assert o.shape == (n, nmel) and r["valid"][b].sum() == n
            assert np.all(np.abs(o - r["feat"][b, :n]) <= np.minimum(r["tol"][b, :n], 1e-3)), (nmel, rate, b)
            assert np.all(r["feat"][b, n:] == 0) and np.all(r["tol"][b, n:] == 0)
    # SpecAugment and the statistics against the oracle's mask fill and plain numpy
    feat = r["feat"][5:6, :17].astype(np.float32)
    fm, tm = np.array([[[3, 5], [0, 0], [nmel - 4, 4]]]), np.array([[[2, 3], [16, 1]]])
    us, _ = FR.utt_sum64(feat)
    got, masked, val = FR.specaugment64(feat, [17], us, fm, tm, True, 0.0)
    want = fbank_ref.specaugment_apply(feat[0].astype(np.float64), fm[0].tolist(), tm[0].tolist(), None)
    assert np.allclose(got[0], want, rtol=1e-13, atol=0) and masked.sum() == 17 * 9 + 4 * nmel - 4 * 9
    got0, _, _ = FR.specaugment64(feat, [17], us, fm, tm, False, -1.5)
    assert np.array_equal(got0[0], fbank_ref.specaugment_apply(feat[0].astype(np.float64), fm[0].tolist(), tm[0].tolist(), -1.5))
    acc, mag = FR.feature_stats64(feat, [11], np.zeros(2 * nmel + 1), calls=2)
    assert np.allclose(acc[:nmel], 2 * feat[0, :11].astype(np.float64).sum(0)) and acc[2 * nmel] == 22
    assert np.allclose(acc[nmel:2 * nmel], 2 * (feat[0, :11].astype(np.float64) ** 2).sum(0)) and np.all(mag[:nmel] >= np.abs(acc[:nmel]))


@pytest.mark.parametrize("nmel,rate", CONFIGS)
def test_tables(nmel, rate):
    """what fbank_kernel assumes of build_tables: a filter never reaches past bin 255 (above it the LDS row holds FFT output, not
    power); mel_woff is the running sum of mel_len and mel_w the bank's non-zero spans; window and twiddles within 1 fp32 ulp of their
    fp64 formulas; the bank equals the oracle's"""
    flen, _ = _geom(rate)
    t = _tab(nmel, rate)
    st, ln, wo, w = t["mel_start"], t["mel_len"], t["mel_woff"], t["mel_w"]
    assert st.dtype == ln.dtype == wo.dtype == np.int32 and w.dtype == t["window"].dtype == t["twiddle"].dtype == np.float32
    assert len(st) == len(ln) == len(wo) == nmel and np.all(st >= 0) and np.all(ln >= 0) and np.all(st + ln <= 256)
    assert np.array_equal(wo, np.concatenate([[0], np.cumsum(ln)[:-1]])) and len(w) == int(ln.sum())
    bank = fbank_ref.mel_banks(nmel, 512, float(rate))
    assert np.array_equal(FR.dense_bank(t, nmel), bank.astype(np.float64))
    for m in range(nmel):       # (128 bins at 16 kHz: the triangles of bins 3.. are narrower than an FFT bin, some hold none: len 0)
        assert ln[m] == 0 or (w[wo[m]] > 0 and w[wo[m] + ln[m] - 1] > 0), m
    assert int((ln == 0).sum()) <= (4 if nmel == 128 else 0)
    assert t["window"].shape == (flen,) and np.all(t["window"] >= 0) and np.all(t["window"] <= 1)
    k = np.arange(256, dtype=np.float64)
    tw = np.stack([np.cos(2 * np.pi * k / 512), -np.sin(2 * np.pi * k / 512)], axis=1)
    assert t["twiddle"].shape == (256, 2) and np.all(np.abs(t["twiddle"] - tw) <= np.maximum(np.spacing(np.abs(tw).astype(np.float32)), 2.0 ** -60))


@pytest.mark.parametrize("flen", [400, 200])
def test_window_table_within_one_ulp_of_the_fp64_formula(flen):
    """Fails on the parent commit, where build_tables took the window as torch.hann_window(fp32) ** 0.85, all in fp32: there
    0.5 - 0.5 cos(x) cancels towards the frame's ends.  Measured then: flen = 400: 187 of 400 values more than 1 ulp away; i = 1:
    table 2.65134557e-04, fp64 formula 2.65150977e-04, 6.2e-5 relative (564 ulp); at most 12 ulp over samples 50..349.  flen = 200:
    80 of 200; worst at i = 197: 168 ulp.  build_tables now evaluates Kaldi's formula in fp64 and rounds once.  No bound in this
    file rests on this property (the fp32 window table is an operand of every reference here)."""
    t = FR.tables_np(build_tables("cpu", 80, flen, 512, 16000.0))
    i = np.arange(flen, dtype=np.float64)
    win = (0.5 - 0.5 * np.cos(2 * np.pi * i / (flen - 1))) ** 0.85
    err = np.abs(t["window"] - win)
    ulp = np.spacing(win.astype(np.float32)).astype(np.float64)
    worst = int(np.argmax(err / np.maximum(ulp, 1e-300)))
    print(f"window flen={flen}: worst at i={worst}: table {t['window'][worst]!r}, fp64 {win[worst]!r}, {err[worst] / ulp[worst]:.1f} ulp")
    assert np.all(err <= ulp), f"{int((err > ulp).sum())} of {flen} window values are more than 1 ulp from the fp64 formula"


def test_drawn_masks_lie_inside_the_utterance():
    """specaug_kernel clips nothing: every mask AdaptiveSpecAugmentTransform.draw_masks returns must lie in [0, n) x [0, nmel)"""
    from espresso_amd.data.feature_transforms import AdaptiveSpecAugmentTransform as SA

    configs = [({"freq_mask_N": 2, "freq_mask_F": 27, "time_mask_pm": 0.04, "time_mask_ps": 0.04}, 80),
               ({"freq_mask_N": 2, "freq_mask_F": 27, "time_mask_N": 2, "time_mask_T": 40, "time_mask_p": 1.0}, 80),
               ({"freq_mask_N": 3, "freq_mask_F": 40, "time_mask_N": 10, "time_mask_T": 100, "time_mask_p": 0.2}, 40),
               ({"freq_mask_N": 1, "freq_mask_F": 23, "time_mask_pm": 1.0, "time_mask_ps": 1.0}, 23)]
    state = np.random.get_state()
    drawn = 0
    try:
        for cfg, nmel in configs:
            sa = SA.from_config_dict(cfg)
            for n in [1, 2, 3, 4, 5, 7, 25, 26, 49, 50, 51, 100, 333, 1000, 3000]:
                for seed in range(8):
                    np.random.seed(1000 * n + seed)
                    fm, tm = sa.draw_masks(n, nmel)
                    assert len(tm) <= sa.max_time_masks() and len(fm) <= sa.freq_mask_n
                    for f0, f in fm:
                        assert 0 <= f and 0 <= f0 and f0 + f <= nmel, (cfg, n, seed, f0, f)
                    for t0, t in tm:
                        assert 0 <= t and 0 <= t0 and t0 + t <= n, (cfg, n, seed, t0, t)
                    drawn += len(fm) + len(tm)
            assert sa.draw_masks(0, nmel) == ([], [])
    finally:
        np.random.set_state(state)
    assert drawn > 2000


# ------------------------------------------------------------------ ea_fbank_batch: cases
class Fb:
    """one ea_fbank_batch launch (and its int16 twin).  tmax: "max", or a number; kind: "noise" (bound 2 applies) or "signals" (an
    all-zero, a constant and a high-dynamic-range utterance among noise)"""

    def __init__(self, nmel, rate, cmvn, usum, olen, tmax="max", kind="noise"):
        self.__dict__.update(nmel=nmel, rate=rate, cmvn=cmvn, usum=usum, olen=olen, tmax=tmax, kind=kind)

    def __repr__(self):
        return "Fb(" + ", ".join(f"{k}={v!r}" for k, v in self.__dict__.items()) + ")"


FB_CASES = [Fb(80, 16000, True, True, True), Fb(80, 16000, False, False, False, 17), Fb(40, 16000, True, False, True, 16),
            Fb(128, 16000, False, True, False, 49), Fb(80, 8000, True, True, True), Fb(80, 8000, False, False, True, 17),
            Fb(128, 16000, True, True, True, 16), Fb(40, 16000, False, True, False, 49),
            Fb(80, 16000, True, True, True, "max", "signals"), Fb(80, 8000, False, True, True, 17, "signals")]


def _signals_batch(seed, flen, fshift):
    """noise, zeros (3 frames), noise, a constant (17 frames), noise, a loud tone over weak noise (20 frames), noise (33 frames)"""
    rng = np.random.default_rng(seed)
    counts = [flen + fshift, flen + 2 * fshift, flen, flen + 16 * fshift + 5, flen + 3 * fshift, flen + 19 * fshift, flen + 32 * fshift + 7]
    wav, off = _noise_batch(seed, flen, fshift, counts)
    wav[off[1]:off[2]] = 0.0
    wav[off[3]:off[4]] = 1000.0
    n = counts[5]
    wav[off[5]:off[6]] = np.rint(20000.0 * np.sin(2 * np.pi * 0.0937 * np.arange(n)) + 2.0 * rng.standard_normal(n))
    return wav, off, {"zero": 1, "const": 3, "hdr": 5}


@functools.lru_cache(maxsize=None)
def _fb_plan_cached(key):
    return _fb_build(*key)


def _fb_plan(c):
    return _fb_plan_cached((c.nmel, c.rate, c.cmvn, c.tmax, c.kind))


def _fb_build(nmel, rate, cmvn, tmax, kind):
    """the case's data, both references and the bounds; shared by the GPU test, its CPU twin and the mutation tests, never changed"""
    P = types.SimpleNamespace()
    P.flen, P.fshift = _geom(rate)
    seed = nmel + rate // 1000
    if kind == "noise":
        P.wav, P.off = _noise_batch(seed, P.flen, P.fshift)
        P.special = {}
    else:
        P.wav, P.off, P.special = _signals_batch(seed, P.flen, P.fshift)
    assert np.array_equal(P.wav, np.rint(P.wav)) and np.abs(P.wav).max() <= 32767      # the int16 twin takes the same samples
    P.B = len(P.off) - 1
    P.tab = _tab(nmel, rate)
    P.mean, P.std = _cmvn(nmel, seed) if cmvn else (None, None)
    full = [FR.num_frames(int(P.off[b + 1] - P.off[b]), P.flen, P.fshift) for b in range(P.B)]
    P.Tmax = max(full) if tmax == "max" else tmax
    assert 0 < P.Tmax <= max(full) and (tmax == "max" or P.Tmax < max(full))
    P.ref = FR.fbank64(P.wav, P.off, P.tab, P.Tmax, nmel, P.flen, P.fshift, P.mean, P.std)
    assert list(P.ref["nfr"]) == full
    P.valid = torch.from_numpy(P.ref["valid"])
    P.feat, P.tol = torch.from_numpy(P.ref["feat"]), torch.from_numpy(P.ref["tol"])
    assert bool((P.tol[P.valid] > 0).all()) and bool((P.tol[~P.valid] == 0).all()) and bool(torch.isfinite(P.tol).all())
    P.emul = torch.from_numpy(FR.fbank_emul32(P.wav, P.off, P.tab, P.Tmax, nmel, P.flen, P.fshift, P.mean, P.std))
    P.noise_rows = P.valid.clone()
    for b in P.special.values():
        P.noise_rows[b] = False
    P.rms_emul = _rms(P.emul, P.feat, P.noise_rows)
    big = float((P.tol[P.noise_rows] > 1e-2).double().mean())
    print(f"fbank nmel={nmel} rate={rate} cmvn={cmvn} Tmax={P.Tmax} {kind}: emulation rms {P.rms_emul:.3e}, hard bound median "
          f"{float(P.tol[P.noise_rows].median()):.2e}, share above 1e-2 {big:.4f}")
    # preconditions: the emulation obeys the hard bound; its rms is fp32's (a few 1e-5 before CMVN's division), far below the 1e-3
    # of check_frontend; the exact utterances are exact in the reference itself
    assert bool(((P.emul.double() - P.feat).abs() <= P.tol).all())
    assert 1e-7 < P.rms_emul < 5e-5
    P.floor_row = _floor_row(P, nmel, np.log(np.float32(FR.LOG_FLOOR)))
    for k in ("zero", "const"):
        if k in P.special:
            b = P.special[k]
            rows = P.feat[b][P.valid[b]]
            f64 = np.full(nmel, np.log(FR.LOG_FLOOR)) if P.mean is None else (np.log(FR.LOG_FLOOR) - P.mean.astype(np.float64)) / P.std.astype(np.float64)
            assert len(rows) >= 1 and bool((rows == torch.from_numpy(f64)).all())      # e = 0 in every bin of every frame
    return P


def _rms(a, ref, rows):
    d = (a.double() - ref)[rows]
    return float(torch.sqrt((d * d).mean()))


def _floor_row(P, nmel, floor_log):
    """fp32 [nmel]: the floored log (one fp32 value) through CMVN in fp32 — a subtraction and a division, each correctly rounded"""
    row = np.full(nmel, floor_log, dtype=np.float32)
    return torch.from_numpy(row if P.mean is None else ((row - P.mean) / P.std).astype(np.float32))


def _fb_compare(what, c, P, feat, olen=None, usum=None, floor_log=None):
    """every assertion on one launch's outputs (CPU tensors); the mutation tests call it with a mutated reference in place of feat.
    floor_log: the device's own logf(floor) (run_fbank reads it from a launch without CMVN and holds it to 2 ulp); None: numpy's"""
    nmel = c.nmel
    _check(what + " feat", feat, P.feat, P.tol)
    pad = ~P.valid
    assert bool((_bits(feat)[pad] == 0).all()), f"{what}: a padding row is not +0"
    row = P.floor_row if floor_log is None else _floor_row(P, nmel, floor_log)
    for k in ("zero", "const"):
        if k in P.special:
            b = P.special[k]
            _same_bits(f"{what} the {k} utterance", feat[b][P.valid[b]], row.expand(int(P.valid[b].sum()), nmel))
    if P.rms_emul is not None and bool(P.noise_rows.any()):
        rms = _rms(feat, P.feat, P.noise_rows)
        print(f"{what}: rms {rms:.3e} against fp64, the fp32 emulation's {P.rms_emul:.3e}, ratio {rms / P.rms_emul:.3f}")
        assert rms <= 2 * P.rms_emul, f"{what}: rms {rms:.3e} is {rms / P.rms_emul:.2f} x the fp32 emulation's {P.rms_emul:.3e}"
    if olen is not None:
        assert olen.tolist() == list(P.ref["nfr"]), (what, olen.tolist())    # the full count, not clamped to Tmax
    if usum is not None:
        s, mag = FR.utt_sum64(feat.numpy())
        blocks = -(-P.Tmax // 16)
        tol = (16 * -(-nmel // 64) + 6 + blocks) * E23 * mag
        rows = np.maximum(P.ref["valid"].sum(1), 1)
        assert np.all(tol <= mag / rows), f"{what}: the bound of utt_sum no longer sees one frame"
        _check(what + " utt_sum", usum, torch.from_numpy(s), torch.from_numpy(tol))


def _tables_on_device(c):
    T = build_tables(DEV, c.nmel, _geom(c.rate)[0], 512, float(c.rate))
    f = {k: inp(T[k].cpu()) for k in ("window", "twiddle", "mel_w")}
    i = {k: IBuf(T[k].cpu(), guard=I32_MIN) for k in ("mel_start", "mel_len", "mel_woff")}
    return f, i


def _fb_call(lib, c, P, i16, tabs=None, B=None, Tmax=None, nmel=None, flen=None):
    f, i = tabs or _tables_on_device(c)
    wav = torch.from_numpy(P.wav)
    bw = IBuf(wav, torch.int16, guard=-32768) if i16 else inp(wav)
    bo = IBuf(torch.from_numpy(P.off), torch.int64, guard=-1)
    bm, bs = (inp(torch.from_numpy(P.mean)), inp(torch.from_numpy(P.std))) if c.cmvn else (None, None)
    feat = out((P.B, P.Tmax, c.nmel), F32)
    usum = out((P.B,), F32, torch.zeros(P.B)) if c.usum else None
    olen = IBuf(n=P.B) if c.olen else None
    fn = lib.ea_fbank_batch_i16 if i16 else lib.ea_fbank_batch
    rc = fn(bw.p, bo.p, P.B if B is None else B, f["window"].p, f["twiddle"].p, i["mel_start"].p, i["mel_len"].p, i["mel_woff"].p, f["mel_w"].p,
            _ptr(bm), _ptr(bs), feat.p, _ptr(usum), _ptr(olen), P.Tmax if Tmax is None else Tmax, c.nmel if nmel is None else nmel,
            P.flen if flen is None else flen, P.fshift, FR.PREEMPH, FR.LOG_FLOOR, _st())
    _sync()
    for b in (feat, usum, olen):
        assert b is None or b.intact(), (c, "stored outside the tensor")
    return rc, feat, usum, olen


def run_fbank(lib, c):
    P = _fb_plan(c)
    if lib is None:
        return P
    tabs = _tables_on_device(c)
    rc, feat, usum, olen = _fb_call(lib, c, P, False, tabs)
    assert rc == 0, (c, rc)
    tag = repr(c)
    floor_log = _device_floor_log(lib, c, P, tabs) if P.special else None
    _fb_compare(tag, c, P, feat.cpu(), olen and olen.cpu(), usum and usum.cpu(), floor_log)
    rc, feat2, usum2, olen2 = _fb_call(lib, c, P, True, tabs)
    assert rc == 0, (c, rc)
    _same_bits(tag + " int16 against fp32 samples", feat2.cpu(), feat.cpu())
    _fb_compare(tag + " int16", c, P, feat2.cpu(), olen2 and olen2.cpu(), usum2 and usum2.cpu(), floor_log)
    return P


def _device_floor_log(lib, c, P, tabs):
    """the one fp32 value the device's logf gives for the floor, read from the all-zero utterance of the same batch without CMVN:
    every element of the all-zero and the constant utterance holds it, and it is within the 2 ulp charged to logf of log(floor)"""
    plain = Fb(c.nmel, c.rate, False, False, False, c.tmax, c.kind)
    Q = types.SimpleNamespace(**{**P.__dict__, "mean": None, "std": None})
    rc, feat, _, _ = _fb_call(lib, plain, Q, False, tabs)
    assert rc == 0
    feat = feat.cpu()
    v = feat[P.special["zero"], 0, 0].clone()
    want = np.log(FR.LOG_FLOOR)
    print(f"device logf(floor) = {float(v)!r}, numpy float32 {float(np.log(np.float32(FR.LOG_FLOOR)))!r}, fp64 {want!r}")
    assert abs(float(v) - want) <= 2 * 2.0 ** -20, float(v)        # ulp(15.94) = 2^-20
    for k in ("zero", "const"):
        rows = feat[P.special[k]][P.valid[P.special[k]]]
        _same_bits(f"{c} without CMVN: the {k} utterance", rows, v.expand_as(rows))
    return float(v)


def _rounded(P, feat=None):
    """a correct fp32 output: the fp64 reference rounded once; the all-zero and the constant utterance as the exact fp32 chain"""
    good = (P.feat if feat is None else feat).float()
    for k in ("zero", "const"):
        if k in P.special:
            b = P.special[k]
            good[b][P.valid[b]] = P.floor_row
    return good


def test_fbank_cases_on_the_cpu():
    """every case's data, references and preconditions; a correct output (fp64 rounded to fp32) and the emulation pass every check"""
    for c in FB_CASES:
        P = run_fbank(None, c)
        good = _rounded(P)
        us =torch.from_numpy(FR.utt_sum64(good.numpy())[0]).float()
        _fb_compare("correct " + repr(c), c, P, good, torch.tensor(list(P.ref["nfr"]), dtype=torch.int32), us)
    cut = [c for c in FB_CASES if c.tmax != "max"]
    assert {c.tmax for c in cut} == {16, 17, 49} and all(max(_fb_plan(c).ref["nfr"]) > c.tmax for c in cut)


# frame_start ... : which utterance a mutation that names one works on (sample_leak: utterance 6's last frame reads the first sample
# of utterance 7, which is 16 times louder)
@pytest.mark.parametrize("mut", FR.MUTATIONS)
def test_fbank_mutations_fall_outside_the_bounds(mut):
    """a correct output with one defect is rejected by _fb_compare — by bound 2 wherever the defect moves a valid element to a finite
    value (asserted separately), by the exact padding check for cmvn_on_padding, as non-finite for no_log_floor"""
    c = FB_CASES[0] if mut != "no_log_floor" else FB_CASES[8]
    P = _fb_plan(c)
    bad64 = torch.from_numpy(FR.fbank64(P.wav, P.off, P.tab, P.Tmax, c.nmel, P.flen, P.fshift, P.mean, P.std, mut=mut, mut_utt=6)["feat"])
    bad = _rounded(P, bad64) if mut != "no_log_floor" else bad64.float()
    if mut == "no_replicate_pad":
        # NOT observable, at any precision: the povey window is exactly 0 at sample 0, the only sample whose pre-emphasis reads the pad
        assert float(P.tab["window"][0]) == 0.0 and float((bad64 - P.feat).abs().max()) < 1e-12
        return
    assert _outside(lambda: _fb_compare(mut, c, P, bad)), mut
    if mut == "cmvn_on_padding":
        assert bool((bad[~P.valid] != 0).any()) and bool((bad[P.valid] == P.feat.float()[P.valid]).all())
    elif mut == "no_log_floor":
        assert bool(torch.isinf(bad[P.special["zero"]][P.valid[P.special["zero"]]]).all())
    else:
        rms = _rms(bad, P.feat, P.noise_rows)
        print(f"{mut}: rms {rms:.3e}, {rms / P.rms_emul:.1f} x the emulation's")
        assert rms > 2 * P.rms_emul, (mut, rms, P.rms_emul)


# ------------------------------------------------------------------ ea_fbank_batch: GPU
@gpu
@pytest.mark.parametrize("c", FB_CASES, ids=repr)
def test_fbank_batch(lib, c):
    """fbank_kernel<float> and <int16_t>: 80 / 40 / 128 bins (one and two trips of the mel loop, a ragged second one), 16 kHz and
    8 kHz (frame_len 400 and 200), Tmax = the batch maximum (50: a ragged fourth block), 16, 17 and 49, each optional pointer given
    and NULL"""
    run_fbank(lib, c)


@gpu
def test_fbank_batch_refuses_and_leaves_outputs_alone(lib):
    """frame_len = 513 and nmel = 129 return -2, B <= 0 returns 0: feat, utt_sum and out_len are untouched"""
    c = FB_CASES[0]
    P = _fb_plan(c)
    for i16 in (False, True):
        for kw, want in (({"flen": 513}, -2), ({"nmel": 129}, -2), ({"B": 0}, 0), ({"B": -3}, 0)):
            rc, feat, usum, olen = _fb_call(lib, c, P, i16, **kw)
            assert rc == want, (kw, rc)
            assert feat.untouched() and olen.untouched() and usum.intact() and bool((usum.cpu() == 0).all()), kw


@gpu
def test_fbank_batch_without_a_single_frame(lib):
    """every utterance shorter than one frame: Tmax = 0.  kernels.fbank_batch must return defined lengths (0) and an empty feature
    tensor; through the C ABI feat and utt_sum are untouched and out_len is 0.  (The parent commit returned before writing out_len.)"""
    from espresso_amd import kernels as K

    c = FB_CASES[0]
    flen, fshift = _geom(c.rate)
    wav, off = _noise_batch(1, flen, fshift, [0, flen - 1, 17, flen - 1])
    T = build_tables(DEV, c.nmel, flen, 512, float(c.rate))
    for w in (torch.from_numpy(wav), torch.from_numpy(wav).to(torch.int16)):
        feat, out_len, utt_sum = K.fbank_batch(w.to(DEV), torch.from_numpy(off).to(DEV), 4, T, None, None, 0, nmel=c.nmel)
        _sync()
        assert feat.shape == (4, 0, c.nmel) and feat.numel() == 0
        assert out_len.cpu().tolist() == [0, 0, 0, 0] and utt_sum.cpu().tolist() == [0.0] * 4
    P = types.SimpleNamespace(wav=wav, off=off, B=4, Tmax=1, mean=None, std=None, flen=flen, fshift=fshift)
    for tm in (0, -1):
        rc, feat, usum, olen = _fb_call(lib, Fb(80, 16000, False, True, True), P, False, Tmax=tm)
        assert rc == 0 and feat.untouched() and bool((usum.cpu() == 0).all())
        assert olen.cpu().tolist() == [0, 0, 0, 0]
    rc, feat, usum, olen = _fb_call(lib, Fb(80, 16000, False, True, False), P, True, Tmax=0)    # out_len == NULL
    assert rc == 0 and feat.untouched()


# ------------------------------------------------------------------ ea_specaugment
class Sa:
    def __init__(self, B, nmel, use_mean, nf=True, nt=True):
        self.__dict__.update(B=B, nmel=nmel, use_mean=use_mean, nf=nf, nt=nt)

    def __repr__(self):
        return "Sa(" + ", ".join(f"{k}={v!r}" for k, v in self.__dict__.items()) + ")"


SA_CASES = [Sa(5, 80, True), Sa(5, 40, False), Sa(1, 80, False), Sa(1, 40, True), Sa(5, 80, True, nf=False), Sa(5, 40, False, nt=False),
            Sa(5, 80, False, nf=False, nt=False)]
SA_TMAX = 41


def _sa_plan(c):
    """lengths 37, 0, 41 (= Tmax), 1, 12; utterance 0: n fw = 37 * 7 = 259 elements (no multiple of 256), a width-0 entry between
    real ones, overlapping frequency masks, one ending at nmel; a time mask ending at n, two overlapping, a width-0 one"""
    P = types.SimpleNamespace()
    g = _gen(c.B * 100 + c.nmel)
    nmel = c.nmel
    P.lens = [37, 0, 41, 1, 12][:c.B]
    feat = torch.randn(c.B, SA_TMAX, nmel, generator=g) * 3 + 1
    for b, n in enumerate(P.lens):
        feat[b, n:] = 0.0
    P.feat = feat
    fm = [[(5, 7), (0, 0), (9, 11), (nmel - 6, 6)], [(1, 2), (3, 4), (0, 0), (0, 0)], [(0, nmel), (0, 0), (0, 0), (0, 0)],
          [(0, 0), (nmel - 1, 1), (0, 0), (0, 1)], [(0, 0), (0, 0), (0, 0), (0, 0)]][:c.B]
    tm = [[(30, 7), (0, 0), (3, 5), (6, 4)], [(0, 1), (0, 0), (0, 0), (0, 0)], [(40, 1), (0, 3), (0, 0), (0, 0)],
          [(0, 1), (0, 0), (0, 0), (0, 0)], [(0, 0), (5, 0), (11, 1), (0, 0)]][:c.B]
    P.fm = np.array(fm, dtype=np.int32) if c.nf else None
    P.tm = np.array(tm, dtype=np.int32) if c.nt else None
    for b, n in enumerate(P.lens):      # the kernel's preconditions (utterance 1 has len 0: its entries are never read as masks)
        if n == 0:
            continue
        assert n <= SA_TMAX
        assert P.fm is None or all(0 <= f0 and 0 <= w and f0 + w <= nmel for f0, w in P.fm[b])
        assert P.tm is None or all(0 <= t0 and 0 <= w and t0 + w <= n for t0, w in P.tm[b])
    assert 37 * 7 % 256 != 0
    P.usum = torch.from_numpy(FR.utt_sum64(feat.numpy())[0]).float()
    P.mask_value = -2.5
    P.ref, P.masked, P.val = FR.specaugment64(feat.numpy(), P.lens, P.usum.numpy(), P.fm, P.tm, c.use_mean, P.mask_value)
    P.masked = torch.from_numpy(P.masked)
    if c.nf or c.nt:
        assert bool(P.masked[0].any()) and not bool(P.masked[0].all())
    assert not bool(P.masked[:, :, :][torch.tensor([[t >= n for t in range(SA_TMAX)] for n in P.lens])].any())   # no padding row masked
    return P


def _sa_compare(what, c, P, got):
    keep = ~P.masked
    assert bool((_bits(got)[keep] == _bits(P.feat)[keep]).all()), f"{what}: an element outside every mask changed"
    ref = torch.from_numpy(P.ref)
    tol = (3 * E23 * ref.abs() if c.use_mean else torch.zeros_like(ref)) * P.masked
    _check(what, got, ref, tol)


def test_specaugment_cases_on_the_cpu():
    for c in SA_CASES:
        P = _sa_plan(c)
        good = torch.from_numpy(P.ref).float()
        _sa_compare("correct", c, P, good)
        if c.nf or c.nt:
            bad = good.clone()
            bad[0, 36, 5 if c.nf else 0] = P.feat[0, 36, 5 if c.nf else 0]      # the last row of a mask left out
            assert _outside(lambda: _sa_compare("a masked element missed", c, P, bad))
            bad = good.clone()
            bad[0, 37, 5] = good[0, 36, 5] + 1.0                                 # one row too many: a padding row written
            assert _outside(lambda: _sa_compare("a padding row written", c, P, bad))


@gpu
@pytest.mark.parametrize("c", SA_CASES, ids=repr)
def test_specaugment(lib, c):
    P = _sa_plan(c)
    feat = out((c.B, SA_TMAX, c.nmel), F32, P.feat)
    lens = IBuf(torch.tensor(P.lens), guard=I32_MIN)
    us = inp(P.usum) if c.use_mean else None
    fm = IBuf(torch.from_numpy(P.fm), guard=I32_MIN) if c.nf else None
    tm = IBuf(torch.from_numpy(P.tm), guard=I32_MIN) if c.nt else None
    rc = lib.ea_specaugment(feat.p, lens.p, _ptr(us), _ptr(fm), _ptr(tm), 4 if c.nf else 0, 4 if c.nt else 0, c.B, SA_TMAX, c.nmel,
                            int(c.use_mean), P.mask_value, _st())
    _sync()
    assert rc == 0 and feat.intact(), (c, rc)
    _sa_compare(repr(c), c, P, feat.cpu())
    assert lib.ea_specaugment(feat.p, lens.p, _ptr(us), _ptr(fm), _ptr(tm), 4 if c.nf else 0, 4 if c.nt else 0, 0, SA_TMAX, c.nmel,
                              int(c.use_mean), 77.0, _st()) == 0    # B = 0: nothing
    _sync()
    _sa_compare(repr(c) + " after B = 0", c, P, feat.cpu())


# ------------------------------------------------------------------ ea_feature_stats
FS_TMAX = [1, 64, 65, 130]
FS_NMEL = [23, 80, 128]


def _fs_plan(Tmax, nmel, nan_tail):
    P = types.SimpleNamespace()
    g = _gen(Tmax * 1000 + nmel)
    P.lens = [0, 1, Tmax, Tmax + 5, Tmax // 2 + 1]
    B = len(P.lens)
    col = 16.0 ** ((torch.arange(nmel) % 3) - 1).float()
    P.feat = (torch.randn(B, Tmax, nmel, generator=g) * 2 + 1) * col * (4.0 ** torch.arange(B).float()).view(B, 1, 1)
    P.clean = P.feat.clone()
    for b, n in enumerate(P.lens):
        P.feat[b, n:] = float("nan") if nan_tail else 0.0
        P.clean[b, n:] = 0.0
    P.acc0 = torch.randn(2 * nmel + 1, generator=g, dtype=F64) * 10
    P.acc0[nmel:2 * nmel].abs_()
    P.acc0[2 * nmel] = 12345.0
    acc, mag = FR.feature_stats64(P.clean.numpy(), P.lens, P.acc0.numpy(), calls=2)
    P.acc, P.mag = torch.from_numpy(acc), torch.from_numpy(mag)
    blocks = 2 * B * -(-Tmax // 64)
    P.tol = (64 + blocks + 1) * 2.0 ** -52 * P.mag
    P.tol[2 * nmel] = 0.0
    frames = sum(min(n, Tmax) for n in P.lens)
    assert float(P.acc[2 * nmel]) == 12345.0 + 2 * frames
    assert bool((P.tol[:2 * nmel] < P.mag[:2 * nmel] / (2 * frames) * 2.0 ** -20).all())     # far below one frame's share
    return P


def test_feature_stats_cases_on_the_cpu():
    for Tmax in FS_TMAX:
        for nmel in FS_NMEL:
            P = _fs_plan(Tmax, nmel, False)
            _check("correct", P.acc, P.acc, P.tol)
            short, _ = FR.feature_stats64(P.clean.numpy(), [0, 1, Tmax - 1, Tmax + 5, Tmax // 2 + 1], P.acc0.numpy(), calls=2)
            if Tmax > 1:
                assert _outside(lambda: _check("the last frame dropped", torch.from_numpy(short), P.acc, P.tol))


@gpu
@pytest.mark.parametrize("nmel", FS_NMEL)
@pytest.mark.parametrize("Tmax", FS_TMAX)
def test_feature_stats(lib, Tmax, nmel):
    """feature_stats_kernel: one frame, one whole block of 64, one frame into the second, a ragged third; 23, 80 and 128 of the 128
    threads live; lengths 0, 1, Tmax, Tmax + 5 (clamped); two calls onto a pre-filled acc; with NaN beyond each length once"""
    for nan_tail in ((False, True) if Tmax == 65 else (False,)):
        P = _fs_plan(Tmax, nmel, nan_tail)
        feat, lens, acc = inp(P.feat), IBuf(torch.tensor(P.lens), guard=I32_MIN), out((2 * nmel + 1,), F64, P.acc0)
        for _ in range(2):
            assert lib.ea_feature_stats(feat.p, lens.p, acc.p, len(P.lens), Tmax, nmel, _st()) == 0
        _sync()
        assert acc.intact()
        _check(f"feature_stats Tmax={Tmax} nmel={nmel} nan_tail={nan_tail}", acc.cpu(), P.acc, P.tol)


@gpu
def test_feature_stats_refuses_129_bins(lib):
    feat, lens, acc = inp(torch.zeros(1, 2, 129)), IBuf(torch.tensor([2]), guard=I32_MIN), out((259,), F64)
    assert lib.ea_feature_stats(feat.p, lens.p, acc.p, 1, 2, 129, _st()) == -2
    assert lib.ea_feature_stats(feat.p, lens.p, acc.p, 0, 2, 128, _st()) == 0
    assert lib.ea_feature_stats(feat.p, lens.p, acc.p, 1, 0, 128, _st()) == 0
    _sync()
    assert acc.untouched()
