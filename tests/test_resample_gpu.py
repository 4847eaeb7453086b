"""resample_kernel (csrc/resample.hip) one launch at a time against the fp64 restatement of tests/resample_ref.py, and
StreamResampler on the device against the offline launch.  The cases, their preconditions, the bound and the three defects that
fall outside it are built and checked on the CPU in tests/test_resample.py.

Buffers as in tests/test_frontend_kernels.py: inputs lie between NaN (fp32) or -32768 (int16, a value no case holds) guards,
outputs start as NaN between sentinel guards, no element is excluded from a comparison.

Paths of the kernel and the case that takes each: the input span staged in LDS with the table beside it (48000, 44100, 11025 ->
16000: 1, 160 and 640 phases; 8000 -> 16000; 16000 -> 8000), the table read from global memory (16001 -> 16000: 16 000 rows),
the span too long to stage (256000 -> 16000: 16 inputs per output) and a `first` table that is not the definition's (scattered
starts: the staged span does not apply and every read is bounds-checked in global memory)."""
import numpy as np
import pytest
import torch

from espresso_amd.data import resample as RS
from tests import resample_ref as RR
from tests.test_convmodule_kernels import DEV, _check, _st, _sync, inp, lib, out  # noqa: F401 (lib: the fixture)
from tests.test_frontend_kernels import IBuf, _ptr, _same_bits
from tests.test_resample import GPU_PAIRS, PAIRS, TILE, case, impulse_expected

gpu = pytest.mark.gpu
F32 = torch.float32


def _launch(lib, plan, wav, in_off, out_off, i16=False, in_base=None, out_base=None, B=None, max_out=None, K=None, phases=None,
            in_unit=None, taps=None, first=None):
    """one launch through the C ABI; returns (rc, the output buffer)"""
    wav = torch.as_tensor(wav)
    bw = IBuf(wav, torch.int16, guard=-32768) if i16 else inp(wav.to(F32))
    bi = IBuf(torch.as_tensor(in_off), torch.int64, guard=-1)
    bo = IBuf(torch.as_tensor(out_off), torch.int64, guard=-1)
    bib = None if in_base is None else IBuf(torch.as_tensor(in_base), torch.int64, guard=-1)
    bob = None if out_base is None else IBuf(torch.as_tensor(out_base), torch.int64, guard=-1)
    bt = inp(torch.from_numpy(plan.taps if taps is None else taps))
    bf = IBuf(torch.from_numpy(plan.first if first is None else first), guard=-2 ** 31)
    y = out((int(out_off[-1]),), F32)
    n = len(in_off) - 1
    counts = np.diff(np.asarray(out_off))
    fn = lib.ea_resample_batch_i16 if i16 else lib.ea_resample_batch
    rc = fn(bw.p, bi.p, _ptr(bib), y.p, bo.p, _ptr(bob), n if B is None else B, bt.p, bf.p, plan.phases if phases is None else phases,
            plan.K if K is None else K, plan.in_unit if in_unit is None else in_unit,
            int(counts.max()) if max_out is None else max_out, _st())
    _sync()
    assert y.intact(), "stored outside the output"
    return rc, y


def _run_case(lib, c):
    tag = f"{c.fi} -> {c.fo}"
    rc, y = _launch(lib, c.plan, c.wav, c.in_off, c.out_off)
    assert rc == 0, (tag, rc)
    _check(tag, y.cpu(), torch.from_numpy(c.y64), torch.from_numpy(c.tol))
    rc, y16 = _launch(lib, c.plan, c.wav, c.in_off, c.out_off, i16=True)
    assert rc == 0, (tag, rc)
    _same_bits(tag + " int16 against fp32 samples", y16.cpu(), y.cpu())


@gpu
@pytest.mark.parametrize("fi,fo", GPU_PAIRS)
def test_resample_batch(lib, fi, fo):
    """every output of a ragged batch with an empty utterance within (K + 2) 2^-24 S_j of fp64; int16 samples give the same bits"""
    _run_case(lib, case(fi, fo))


@gpu
def test_scattered_first_table_takes_the_checked_path(lib):
    """a table whose starts are not the definition's (phase p reads from first[p] + 3000 (p % 7)): the same sum, per element,
    through bounds-checked global reads -- no read or store leaves the buffers whatever the table says"""
    c = case(44100, 16000)
    first = (c.plan.first.astype(np.int64) + 3000 * (np.arange(c.plan.phases) % 7) - 9000).astype(np.int32)
    ys, Ss = [], []
    for b in range(len(c.lens)):
        y, S = RR.apply64(c.wav[c.in_off[b]:c.in_off[b + 1]], c.plan.taps, first, c.plan.in_unit, c.nout[b])
        ys.append(y)
        Ss.append(S)
    y64, S = np.concatenate(ys), np.concatenate(Ss)
    assert np.count_nonzero(S) > 100
    rc, y = _launch(lib, c.plan, c.wav, c.in_off, c.out_off, first=first)
    assert rc == 0
    _check("scattered first", y.cpu(), torch.from_numpy(y64), torch.from_numpy((c.K + 2) * 2.0 ** -24 * S))


@gpu
@pytest.mark.parametrize("fi,fo", PAIRS)
def test_unit_impulse_reads_one_tap_per_output(lib, fi, fo):
    """x = 1 at sample i0 and 0 elsewhere: y[j] is taps[p][i0 - first[p] - u in_unit] bit for bit (or +0): phase, unit and first
    index of every output, in both sample formats"""
    plan = RS.resample_plan(fi, fo)
    n = TILE * fi // fo + 2 * plan.in_unit + 7
    for i0 in (plan.in_unit + 3, n - 1, 0):
        x = np.zeros(n, dtype=np.float32)
        x[i0] = 1.0
        want = torch.from_numpy(impulse_expected(plan, n, i0))
        for i16 in (False, True):
            rc, y = _launch(lib, plan, x, [0, n], [0, plan.n_out(n)], i16=i16)
            assert rc == 0
            _same_bits(f"{fi} -> {fo} impulse at {i0}", y.cpu(), want)


@gpu
def test_identity_plan_returns_the_input_bits(lib):
    plan = RS.resample_plan(16000, 16000)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2500, generator=g) * 1000
    x[7] = -0.0
    off = [0, 1200, 1200, 2500]
    rc, y = _launch(lib, plan, x, off, off)
    assert rc == 0
    got, want = y.cpu(), x + 0.0  # (acc starts at +0: a -0 sample comes out as +0, every other value as itself)
    _same_bits("identity", got, want)


@gpu
def test_return_codes_and_nothing_written(lib):
    c = case(48000, 16000)
    for i16 in (False, True):
        for kw, want in (({"B": 0}, 0), ({"B": -2}, 0), ({"max_out": 0}, 0), ({"max_out": -5}, 0), ({"K": 4097}, -2),
                         ({"phases": 0}, -2), ({"phases": -1}, -2), ({"in_unit": 0}, -2), ({"in_unit": -3}, -2)):
            rc, y = _launch(lib, c.plan, c.wav, c.in_off, c.out_off, i16=i16, **kw)
            assert rc == want, (kw, rc)
            assert y.untouched(), kw


@gpu
def test_bases_past_2_to_the_32(lib):
    """a stream that has run for days: 1500 held samples whose first has absolute index U in_unit, outputs from U phases on, U =
    2^33 -- the bits of the same samples at base 0 (whole units shift nothing but the indices), for fp32 and int16 samples"""
    c = case(44100, 16000)
    plan, U = c.plan, 2 ** 33
    x = c.wav[c.in_off[4]:c.in_off[4] + 1500]
    cnt = plan.n_out(1500)
    assert U * plan.phases > 2 ** 32 and U * plan.in_unit > 2 ** 32
    for i16 in (False, True):
        rc, y0 = _launch(lib, plan, x, [0, 1500], [0, cnt], i16=i16)
        rc2, y1 = _launch(lib, plan, x, [0, 1500], [0, cnt], i16=i16, in_base=[U * plan.in_unit], out_base=[U * plan.phases])
        assert rc == 0 and rc2 == 0
        _same_bits("bases past 2^32", y1.cpu(), y0.cpu())
        # and a window of outputs in the middle, from held samples that start later: what a running stream asks for
        j0, j1 = 400, 520
        a = max(0, plan.start(j0))
        rc3, y2 = _launch(lib, plan, x[a:], [0, 1500 - a], [0, j1 - j0], i16=i16, in_base=[U * plan.in_unit + a],
                          out_base=[U * plan.phases + j0])
        assert rc3 == 0
        _same_bits("a running stream's piece", y2.cpu(), y0.cpu()[j0:j1])


# ------------------------------------------------------------------ Resampler and StreamResampler on the device
def _offline(x, fi, fo=16000, dtype=F32):
    r = RS.Resampler(DEV, fo)
    w = torch.from_numpy(x).to(dtype).to(DEV)
    y, off, n = r(w, torch.tensor([0, len(x)], dtype=torch.int64).to(DEV), [len(x)], [fi])
    return y


def _noise(n, seed):
    return np.rint(np.random.default_rng(seed).standard_normal(n) * 2000).astype(np.float32)


@gpu
def test_resampler_mixed_batch(lib):
    """rates 48000, 16000, 16000, 44100, 48000 in one batch: every slot holds the bits of that utterance resampled alone, the
    16 kHz ones their input bits; lengths and offsets are the plan's; int16 samples give the same"""
    rates = [48000, 16000, 16000, 44100, 48000]
    xs = [_noise(n, 10 + k) for k, n in enumerate((3001, 700, 5, 4410, 0))]
    off = np.zeros(6, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in xs])
    r = RS.Resampler(DEV, 16000)
    for dtype in (F32, torch.int16):
        wav = torch.from_numpy(np.concatenate(xs)).to(dtype).to(DEV)
        y, yoff, n_out = r(wav, torch.from_numpy(off).to(DEV), [len(x) for x in xs], rates)
        _sync()
        assert n_out == [RR.n_out(len(x), fi, 16000) for x, fi in zip(xs, rates)] == [1001, 700, 5, 1600, 0]
        assert yoff.cpu().tolist() == [0] + np.cumsum(n_out).tolist() and y.dtype == F32 and y.numel() == sum(n_out)
        yo = yoff.cpu().tolist()
        for b, (x, fi) in enumerate(zip(xs, rates)):
            want = torch.from_numpy(x) if fi == 16000 else _offline(x, fi).cpu()
            _same_bits(f"utterance {b} at {fi}", y[yo[b]:yo[b + 1]].cpu(), want)
    y48 = _offline(xs[0], 48000).cpu().double()
    ref, S = RR.apply64(xs[0], RS.resample_plan(48000, 16000).taps, RS.resample_plan(48000, 16000).first, 3, 1001)
    _check("Resampler 48000 -> 16000", y48, torch.from_numpy(ref), torch.from_numpy(39 * 2.0 ** -24 * S))


@gpu
@pytest.mark.parametrize("piece", [1, 7, "in_unit", 1000])
def test_stream_equals_offline_bit_for_bit(lib, piece):
    """two streams of different rates fed together in pieces of `piece` samples each, the shorter one finishing early (and a
    third at the front-end's rate, which passes through): the concatenated pieces are the offline launch's bits"""
    n = {1: (700, 300), 7: (3000, 1000)}.get(piece, (9000, 2500))
    rates = (44100, 8000, 16000)
    xs = [_noise(n[0], 1), _noise(n[1], 2), _noise(n[1], 3)]
    want = [_offline(x, fi).cpu() if fi != 16000 else torch.from_numpy(x) for x, fi in zip(xs, rates)]
    sr = RS.StreamResampler(DEV, 16000)
    ids = ["a", "b", "c"]
    sr.open(ids, rates)
    step = [RS.resample_plan(fi, 16000).in_unit if piece == "in_unit" else piece for fi in rates]
    pos, got, live = [0, 0, 0], [[], [], []], [0, 1, 2]
    held = 0
    while live:
        pieces, final = [], []
        for k in live:
            a, b = pos[k], min(len(xs[k]), pos[k] + step[k])
            pieces.append(torch.from_numpy(xs[k][a:b]))
            final.append(b >= len(xs[k]))
            pos[k] = b
        outs = sr.accept([ids[k] for k in live], pieces, final)
        for k, o, f in zip(list(live), outs, final):
            got[k].append(o.cpu())
            if f:
                sr.close([ids[k]])
                live.remove(k)
            else:
                held = max(held, sr.held(ids[k]))
    _sync()
    assert held <= 34 + 3  # K + ceil(fi / fo) of the 44.1 kHz stream, the larger of the two
    for k in range(3):
        _same_bits(f"stream {ids[k]} at {rates[k]} in pieces of {step[k]}", torch.cat(got[k]), want[k])
