"""The polyphase resampler on the CPU: the plan against the fp64 definition (tests/resample_ref.py), the quality of the filter, the
host bookkeeping of StreamResampler with the reference as its kernel, and every case of tests/test_resample_gpu.py with its
preconditions: a correct output (fp64 rounded once) passes the GPU cases' bound, three defects each fall outside it.

THE BOUND of the GPU cases, per element:  |y - y64| <= (K + 2) 2^-24 S_j,  S_j = sum_k |w_k x_k|.
y64 is the fp64 sum of the products of the fp32 table and the samples (both exact operands: integers below 2^15 and the table as
the kernel reads it, so neither is charged).  The kernel's K fused multiply-adds each round once, by at most 2^-24 of a partial
sum that S_j bounds (in magnitude; the relative bound 2^-24 is half an ulp); the + 2 pays for the second-order terms
((1 + 2^-24)^K - 1 - K 2^-24 < 2 * 2^-24 up to K = 4096)."""
import functools
import types

import numpy as np
import pytest
import torch

from espresso_amd.data import resample as RS
from tests import resample_ref as RR

E24 = 2.0 ** -24
TILE = 1024  # outputs per workgroup of resample_kernel
# fi -> fo: (phases, K) of the issue's table
TABLE = {(48000, 16000): (1, 37), (96000, 16000): (1, 73), (32000, 16000): (1, 25), (44100, 16000): (160, 34),
         (22050, 16000): (320, 17), (11025, 16000): (640, 13), (8000, 16000): (2, 13), (16000, 8000): (1, 25)}
# the GPU cases: one phase; 160 phases; 640 phases (the largest table kept in LDS); up-sampling; to 8 kHz; 16 000 phases (the table
# stays in global memory)
PAIRS = [(48000, 16000), (44100, 16000), (11025, 16000), (8000, 16000), (16000, 8000), (16001, 16000)]
# and one whose input span per tile (16 inputs per output) is too long to stage in LDS: the kernel's bounds-checked global path
UNSTAGED = (256000, 16000)
GPU_PAIRS = PAIRS + [UNSTAGED]


# ------------------------------------------------------------------ the cases (shared with the GPU tests)
@functools.lru_cache(maxsize=None)
def table(fi, fo):
    return RR.table64(fi, fo)


def crossing_length(fi, fo):
    """the shortest utterance with more outputs than a tile: one more (up-sampling, an input brings ceil(fo / fi): that many)"""
    n = TILE * fi // fo + 1
    assert RR.n_out(n - 1, fi, fo) <= TILE < RR.n_out(n, fi, fo) <= TILE + -(-fo // fi)
    return n


@functools.lru_cache(maxsize=None)
def case(fi, fo):
    """four utterances 16 times apart in scale -- 5 samples (shorter than half the filter), 2 in_unit, 2 in_unit + 7, and one whose
    last output is the first of a second tile -- and an empty one between them; integer samples, so that the int16 kernel reads
    the same numbers"""
    plan = RS.resample_plan(fi, fo)
    in_unit, phases = RR.geometry(fi, fo)
    lens = [5, 2 * in_unit, 0, 2 * in_unit + 7, crossing_length(fi, fo)]
    rng = np.random.default_rng(fi + fo)
    parts, k = [], 0
    for n in lens:
        sc = 2.0 * 16.0 ** k
        x = np.clip(np.rint(rng.standard_normal(n) * sc), -32767, 32767)
        if n:
            x[-1] = sc  # (the right edge is visible: see the mutation right_edge_not_padded)
            k += 1
        parts.append(x)
    in_off = np.zeros(len(lens) + 1, dtype=np.int64)
    in_off[1:] = np.cumsum(lens)
    nout = [plan.n_out(n) for n in lens]
    out_off = np.zeros(len(lens) + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(nout)
    c = types.SimpleNamespace(fi=fi, fo=fo, plan=plan, lens=lens, wav=np.concatenate(parts).astype(np.float32), in_off=in_off,
                              nout=nout, out_off=out_off, K=plan.K)
    c.y64, c.S = reference(c)
    c.tol = (plan.K + 2) * E24 * c.S
    # preconditions
    assert lens[0] < plan.K / 2 or fo > fi  # (up-sampling by 2: 13 taps reach 6 inputs each way)
    assert nout[2] == 0 and TILE < nout[4] <= TILE + -(-fo // fi) and (nout[4] == TILE + 1 or fo == 2 * fi)  # (16001 -> 16000: 2 in_unit alone are 32 tiles)
    assert np.all(c.wav == np.rint(c.wav)) and np.abs(c.wav).max() <= 32767
    assert [RR.n_out(n, fi, fo) for n in lens] == nout
    return c


def reference(c, mut=None, taps=None):
    ys, Ss = [], []
    for b, n in enumerate(c.lens):
        y, S = RR.apply64(c.wav[c.in_off[b]:c.in_off[b + 1]], c.plan.taps if taps is None else taps, c.plan.first, c.plan.in_unit,
                          c.nout[b], mut=mut)
        ys.append(y)
        Ss.append(S)
    return np.concatenate(ys), np.concatenate(Ss)


def within_bound(c, y):
    y = np.asarray(y, dtype=np.float64)
    return y.shape == c.y64.shape and bool(np.all(np.isfinite(y))) and bool(np.all(np.abs(y - c.y64) <= c.tol))


def impulse_expected(plan, n, i0):
    """the exact output of a unit impulse at sample i0 of an utterance of n samples: one tap per output, or +0"""
    j = np.arange(plan.n_out(n), dtype=np.int64)
    p, u = j % plan.phases, j // plan.phases
    k = i0 - plan.first[p].astype(np.int64) - u * plan.in_unit
    ok = (k >= 0) & (k < plan.K)
    return np.where(ok, plan.taps[p, np.clip(k, 0, plan.K - 1)], np.float32(0.0)).astype(np.float32) + np.float32(0.0)


# ------------------------------------------------------------------ the plan
@pytest.mark.parametrize("fi,fo", sorted(set(TABLE) | set(PAIRS)))
def test_plan_is_the_definition(fi, fo):
    taps, first, K, in_unit, phases = table(fi, fo)
    plan = RS.resample_plan(fi, fo)
    assert (plan.K, plan.in_unit, plan.phases) == (K, in_unit, phases)
    if (fi, fo) in TABLE:
        assert (phases, K) == TABLE[(fi, fo)]
    assert plan.taps.dtype == np.float32 and plan.taps.shape == (phases, K)
    assert np.array_equal(plan.taps, taps.astype(np.float32))
    assert plan.first.dtype == np.int32 and np.array_equal(plan.first, first)
    sums = taps.sum(1)
    assert 1.0 <= sums.min() and sums.max() <= 1.0009, (sums.min(), sums.max())
    # start(j) never decreases (what the staged span of a tile and StreamResampler's trimming rely on)
    assert np.all(np.diff(first) >= 0) and first[0] + in_unit >= first[-1]
    assert RS.resample_plan(fi, fo) is plan  # cached


def test_table_sizes_of_the_largest_cases():
    assert RS.resample_plan(11025, 16000).taps.size == 8320
    assert RS.resample_plan(16001, 16000).taps.size == 16000 * 13  # 832 KB: more than a workgroup's LDS


@pytest.mark.parametrize("fi,fo", PAIRS + [(96000, 16000)])
def test_n_out(fi, fo):
    plan = RS.resample_plan(fi, fo)
    assert plan.n_out(0) == 0 and plan.n_out(1) == -(-fo // fi)  # one input sample lasts 1 / fi: ceil(fo / fi) outputs
    u = plan.in_unit
    for m in (1, 3):
        assert plan.n_out(m * u) == m * plan.phases
        assert plan.n_out(m * u + 1) == m * plan.phases + -(-plan.phases // u)  # ceil(m phases + phases / u)
        assert plan.n_out(m * u - 1) == m * plan.phases - plan.phases // u  # ceil(m phases - phases / u)
    for n in (5, 999, 16000, 44100, 123457):
        assert plan.n_out(n) == -(-n * fo // fi) == RS.resampled_length(n, fi, fo) == RR.n_out(n, fi, fo)
        assert (plan.n_out(n) - 1) * fi < n * fo <= plan.n_out(n) * fi  # the outputs with time < n / fi, all of them


def test_n_out_pinned():
    p = RS.resample_plan(48000, 16000)  # in_unit 3
    assert [p.n_out(n) for n in (0, 1, 2, 3, 4, 5, 6, 7)] == [0, 1, 1, 1, 2, 2, 2, 3]
    p = RS.resample_plan(44100, 16000)  # 441 in, 160 out
    assert [p.n_out(n) for n in (0, 1, 440, 441, 442, 3000)] == [0, 1, 160, 160, 161, 1089]
    p = RS.resample_plan(8000, 16000)
    assert [p.n_out(n) for n in (0, 1, 2, 3)] == [0, 2, 4, 6]


def test_identity_plan():
    p = RS.resample_plan(16000, 16000)
    assert (p.phases, p.K, p.in_unit) == (1, 1, 1) and p.taps.tolist() == [[1.0]] and p.first.tolist() == [0] and p.n_out(77) == 77


def test_refusals():
    with pytest.raises(NotImplementedError, match="96001.*16000"):
        RS.ResamplePlan(96001, 16000)  # 16 000 phases x 73 taps > 2^20
    for fi, fo in ((0, 16000), (16000, 0), (-8000, 16000)):
        with pytest.raises(NotImplementedError, match=str(fi)):
            RS.ResamplePlan(fi, fo)
        with pytest.raises(NotImplementedError):
            RS.resampled_length(10, fi, fo)


# ------------------------------------------------------------------ quality (the reference alone)
def _tones(fs, n, freqs):
    t = np.arange(n) / fs
    return sum(a * np.sin(2 * np.pi * f * t) for f, a in freqs)


@pytest.mark.parametrize("fi", [48000, 44100])
def test_quality(fi):
    fo, n = 16000, 3000
    pair = ((1000.0, 1000.0), (3000.0, 500.0))
    y, _ = RR.resample64(_tones(fi, n, pair), fi, fo)
    ideal = _tones(fo, len(y), pair)
    err = np.abs(y - ideal)[100:-100].max()
    print(f"{fi} -> {fo}: 1 kHz + 3 kHz pair within {err:.3f} of the ideal signal")
    assert err <= 1.0
    y12, _ = RR.resample64(_tones(fi, n, ((12000.0, 1000.0),)), fi, fo)
    leak = np.abs(y12)[100:-100].max()
    print(f"{fi} -> {fo}: a 12 kHz tone of amplitude 1000 comes out at {leak:.3f}")
    assert leak < 3.0
    signal = pytest.importorskip("scipy.signal")
    g = np.gcd(fi, fo)
    z = signal.resample_poly(_tones(fi, n, pair), fo // g, fi // g)
    m = min(len(z), len(y))
    d = np.abs(z[:m] - y[:m])[100:-100].max()
    print(f"{fi} -> {fo}: within {d:.3f} of scipy.signal.resample_poly")
    assert d <= 5.0


# ------------------------------------------------------------------ StreamResampler's bookkeeping, the reference as its kernel
def _ref_launch(plan, wav, in_off, in_base, out, out_off, out_base, B, max_out):
    io_, oo = in_off.tolist(), out_off.tolist()
    for b in range(B):
        cnt = oo[b + 1] - oo[b]
        assert 0 <= cnt <= max_out
        y, _ = RR.apply64(wav[io_[b]:io_[b + 1]].numpy(), plan.taps, plan.first, plan.in_unit, cnt,
                          in_base=int(in_base[b]), out_base=int(out_base[b]))
        out[oo[b]:oo[b + 1]] = torch.from_numpy(y.astype(np.float32))


@pytest.mark.parametrize("piece", [1, 7, 441, 1000, 5000])
def test_stream_bookkeeping_equals_offline(piece, monkeypatch):
    fi, fo, n = 44100, 16000, 5000
    plan = RS.resample_plan(fi, fo)
    x = np.rint(np.random.default_rng(5).standard_normal(n) * 1000).astype(np.float32)
    want = RR.apply64(x, plan.taps, plan.first, plan.in_unit, plan.n_out(n))[0].astype(np.float32)
    sr = RS.StreamResampler("cpu", fo)
    monkeypatch.setattr(sr, "_launch", _ref_launch)
    sr.open(["a"], [fi])
    got, worst = [], 0
    for a in range(0, n, piece):
        b = min(n, a + piece)
        (y,) = sr.accept(["a"], [torch.from_numpy(x[a:b])], b >= n)
        got.append(y.numpy())
        if b < n:
            worst = max(worst, sr.held("a"))
    got = np.concatenate(got)
    print(f"pieces of {piece}: held at most {worst} samples (K = {plan.K})")
    assert worst <= plan.K + -(-fi // fo)
    assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))
    sr.close(["a"])
    assert not sr.streams


def test_stream_passes_the_frontend_rate_through(monkeypatch):
    sr = RS.StreamResampler("cpu", 16000)
    monkeypatch.setattr(sr, "_launch", lambda *a: pytest.fail("a launch for audio at the front-end's rate"))
    sr.open([0], [16000])
    x = torch.arange(10, dtype=torch.float32)
    (y,) = sr.accept([0], [x], True)
    assert y is x


# ------------------------------------------------------------------ the GPU cases: data, preconditions, mutations
@pytest.mark.parametrize("fi,fo", GPU_PAIRS)
def test_gpu_cases_on_the_cpu(fi, fo):
    """a correct output (the fp64 value rounded once to fp32) is inside the bound; so is an fp32 emulation of the kernel's loop"""
    c = case(fi, fo)
    assert within_bound(c, c.y64.astype(np.float32))
    # the bound is no looser than a few ulp of the output where nothing cancels, and never 0 where the output is not
    assert np.all(c.tol[c.S > 0] > 0) and np.all((c.y64 == 0) | (c.S > 0))
    b = 3  # an fp32 chain in the kernel's order for one utterance: inside the bound
    x = c.wav[c.in_off[b]:c.in_off[b + 1]]
    j = np.arange(c.nout[b])
    p, u = j % c.plan.phases, j // c.plan.phases
    acc = np.zeros(len(j), dtype=np.float32)
    for k in range(c.K):
        i = c.plan.first[p].astype(np.int64) + u * c.plan.in_unit + k
        xv = np.where((i >= 0) & (i < len(x)), x[np.clip(i, 0, len(x) - 1)], 0).astype(np.float64)
        acc = (c.plan.taps[p, k].astype(np.float64) * xv + acc.astype(np.float64)).astype(np.float32)  # one rounding: an fma
    sl = slice(int(c.out_off[b]), int(c.out_off[b + 1]))
    assert np.all(np.abs(acc - c.y64[sl]) <= c.tol[sl])
    # the impulse case pins one tap per output
    n, i0 = c.lens[3], c.plan.in_unit + 3
    e = impulse_expected(c.plan, n, i0)
    imp = np.zeros(n)
    imp[i0] = 1.0
    y, _ = RR.apply64(imp, c.plan.taps, c.plan.first, c.plan.in_unit, c.plan.n_out(n))
    assert np.array_equal(y.astype(np.float32), e) and np.count_nonzero(e) >= min(c.K, 3)


@pytest.mark.parametrize("mut", RR.MUTATIONS)
@pytest.mark.parametrize("fi,fo", GPU_PAIRS)
def test_mutations_fall_outside_the_bound(fi, fo, mut):
    c = case(fi, fo)
    bad, _ = reference(c, mut=mut)
    if mut == "phases_reversed" and c.plan.phases == 1:
        assert np.array_equal(bad, c.y64)  # one phase: nothing to reverse
        return
    assert not within_bound(c, bad.astype(np.float32)), (fi, fo, mut)
    n_bad = int((np.abs(bad - c.y64) > c.tol).sum())
    print(f"{fi} -> {fo} {mut}: {n_bad} of {len(bad)} outputs outside the bound")


# ------------------------------------------------------------------ host behaviour
def test_resampler_returns_its_arguments_at_the_frontend_rate():
    r = RS.Resampler("cpu", 16000)
    wav, off, n = torch.zeros(30), torch.tensor([0, 10, 30]), [10, 20]
    out = r(wav, off, n, [16000, 16000])
    assert out[0] is wav and out[1] is off and out[2] is n


def _samples(sources, rate=16000):
    return [{"id": i, "utt_id": f"u{i}", "source": s, "target": None, "text": None} for i, s in enumerate(sources)]


def test_training_collate_keeps_todays_batch_at_the_frontend_rate():
    from espresso_amd.data import asr_dataset as AD

    rng = np.random.default_rng(0)
    src = [rng.standard_normal(n).astype(np.float32) for n in (4000, 9000, 6100)]
    b = AD.collate(_samples(src), pad_idx=1, eos_idx=2)
    assert sorted(b) == sorted(["id", "utt_id", "nsentences", "ntokens", "net_input", "target", "text", "wav", "wav_offsets",
                                "num_samples", "id_list", "audio_seconds"])
    assert b["utt_id"] == ["u1", "u2", "u0"] and b["num_samples"] == [9000, 6100, 4000]
    assert b["net_input"]["src_lengths"].tolist() == [AD.samples_to_frames(n) for n in (9000, 6100, 4000)]
    assert torch.equal(b["wav"], torch.from_numpy(np.concatenate([src[1], src[2], src[0]])))
    assert b["audio_seconds"] == 19100 / 16000.0


def test_training_collate_sorts_by_resampled_frames_and_carries_rates():
    from espresso_amd.data import asr_dataset as AD
    from espresso_amd.data.audio_utils import RatedWave

    rng = np.random.default_rng(1)
    # 20 000 samples at 48 kHz are 6 667 at 16 kHz: the longest array is the shortest utterance
    src = [RatedWave(rng.standard_normal(20000), 48000), rng.standard_normal(9000).astype(np.float32),
           RatedWave(rng.standard_normal(5000), 8000)]
    b = AD.collate(_samples(src), pad_idx=1, eos_idx=2)
    assert b["utt_id"] == ["u2", "u1", "u0"]
    assert b["wav_rates"] == [8000, 16000, 48000] and b["num_samples"] == [5000, 9000, 20000]
    assert b["net_input"]["src_lengths"].tolist() == [AD.samples_to_frames(n) for n in (10000, 9000, 6667)]
    assert abs(b["audio_seconds"] - (5000 / 8000 + 9000 / 16000 + 20000 / 48000)) < 1e-12
    assert b["wav"].dtype == torch.float32 and b["wav"].numel() == 34000


def test_recognizer_collate_and_budget():
    from espresso_amd import speech_recognize as SR

    waves = [np.zeros(4800, np.float32), np.zeros(1600, np.float32)]
    s = SR.collate([0, 1], ["a", "b"], waves, "cpu", [16000, 16000], 16000)
    assert sorted(s) == ["net_input", "num_samples", "utt_ids", "wav", "wav_offsets"]
    assert sorted(SR.collate([0, 1], ["a", "b"], waves, "cpu")) == sorted(s)
    m = SR.collate([0, 1], ["a", "b"], waves, "cpu", [48000, 16000], 16000)
    assert m["wav_rates"] == [48000, 16000] and m["num_samples"] == [4800, 1600]
    assert SR.lengths_at(waves, [48000, 16000], 16000) == [1600, 1600]
    assert SR.audio_seconds(m) == 0.2 and SR.audio_seconds(s) == 0.4


def test_dataset_sizes_and_wav2num_frames_from_a_48k_header(tmp_path):
    from espresso_amd.data import asr_dataset as AD
    from espresso_amd.data.audio_utils import LazyWave, RatedWave, write_wav
    from espresso_amd.tools import wav2num_frames as W

    p48, p16 = str(tmp_path / "a48.wav"), str(tmp_path / "a16.wav")
    write_wav(p48, np.zeros(48000), 48000)
    write_wav(p16, np.zeros(16000), 16000)
    want = AD.samples_to_frames(16000)
    assert want == 98
    assert W.process(f"u1 {p48}\n") == f"u1 {want}" and W.process(f"u2 {p16}\n") == f"u2 {want}"
    ds = AD.AudioWaveDataset(["u1", "u2"], [p48, p16])
    assert ds.sizes.tolist() == [want, want]
    a, b = ds[0], ds[1]
    assert isinstance(a, RatedWave) and a.sample_rate == 48000 and len(a) == 48000
    assert type(b) is np.ndarray and len(b) == 16000
    ds.lazy = True
    a, b = ds[0], ds[1]
    assert isinstance(a, LazyWave) and (a.sample_rate, len(a)) == (48000, 48000) and (b.sample_rate, len(b)) == (16000, 16000)
    batch = AD.collate(_samples([a, b]), pad_idx=1, eos_idx=2)
    assert batch["wav"].dtype == torch.int16 and batch["wav_rates"] == [48000, 16000] and batch["audio_seconds"] == 2.0
    plain = AD.collate(_samples([b]), pad_idx=1, eos_idx=2)
    assert "wav_rates" not in plain and plain["audio_seconds"] == 1.0
