"""Long-form forced alignment on the host (tools/forced_aligner.py `cut_segments`, speech_align --long-form's parser and
refusals, the C ABI of csrc/align_long.hip as far as it runs without a GPU) and the float64 reference of tests/long_align_ref.py
against brute-force enumeration.  The kernels are tested in tests/test_long_align_gpu.py."""
import ctypes

import numpy as np
import pytest

from tests import long_align_ref as ref
from tests.test_forced_align import _ctc_brute


# ------------------------------------------------------------------------------------------------ cut_segments
def _words(rng, n, max_len=6, max_gap=9):
    """n words [(text, start, end)] with random lengths and gaps (a gap may be 0), and the recording's frame count."""
    t = int(rng.integers(0, 5))
    out = []
    for k in range(n):
        ln = int(rng.integers(1, max_len + 1))
        out.append((f"w{k}", t, t + ln))
        t += ln + int(rng.integers(0, max_gap + 1))
    return out, t + int(rng.integers(0, 4))


@pytest.mark.parametrize("seed", range(8))
def test_cut_segments_partition_the_words_and_cut_only_in_silence(seed):
    from espresso_amd.tools.forced_aligner import cut_segments

    rng = np.random.default_rng(seed)
    for n in (1, 2, 5, 40):
        for max_frames, min_gap in ((12, 3), (30, 1), (30, 6), (1000, 2), (5, 50)):
            words, n_frames = _words(rng, n)
            segs = cut_segments(words, n_frames, max_frames, min_gap)
            # every word in exactly one segment, in order
            assert [a for a, _, _, _, _ in segs] == [0] + [b for _, b, _, _, _ in segs[:-1]] and segs[-1][1] == n
            assert all(a < b for a, b, _, _, _ in segs)
            pad = min_gap // 2
            assert segs[0][2] == max(0, words[0][1] - pad) and segs[-1][3] == min(n_frames, words[-1][2] + pad)
            for k, (a, b, s, e, overlong) in enumerate(segs):
                assert 0 <= s <= words[a][1] and words[b - 1][2] <= e <= n_frames  # no word is cut
                assert overlong == (e - s > max_frames)
                gaps = [words[i + 1][1] - words[i][2] for i in range(a, b - 1)]
                if overlong:
                    assert all(g < min_gap for g in gaps)  # nothing left to cut at
                if k + 1 < len(segs):  # the cut: inside a gap of at least min_gap, at prev.end + gap // 2
                    gap = words[b][1] - words[b - 1][2]
                    assert gap >= min_gap and e == segs[k + 1][2] == words[b - 1][2] + gap // 2
            if max_frames == 1000:
                assert len(segs) == 1 and not segs[0][4]


def test_cut_segments_longest_gap_then_middle_then_earlier():
    from espresso_amd.tools.forced_aligner import cut_segments

    # gaps 4, 6, 4: the longest
    words = [("a", 0, 10), ("b", 14, 24), ("c", 30, 40), ("d", 44, 54)]
    assert cut_segments(words, 54, 30, 2) == [(0, 2, 0, 27, False), (2, 4, 27, 54, False)]
    # gaps 6, 2, 6 at 10..16 and 38..44 of a segment [0, 50]: the first is 12 from the middle, the second 16
    words = [("a", 0, 10), ("b", 16, 26), ("c", 28, 38), ("d", 44, 50)]
    assert cut_segments(words, 50, 40, 0)[0] == (0, 1, 0, 13, False)
    # the mirror image: the later gap is nearer the middle
    words = [("a", 0, 6), ("b", 12, 22), ("c", 24, 34), ("d", 40, 50)]
    assert cut_segments(words, 50, 40, 0)[-1] == (3, 4, 37, 50, False)
    # gaps 6 and 6 at 10..16 and 34..40 of [0, 50]: equally far from the middle, the earlier one
    words = [("a", 0, 10), ("b", 16, 34), ("c", 40, 50)]
    assert cut_segments(words, 50, 45, 0) == [(0, 1, 0, 13, False), (1, 3, 13, 50, False)]
    # a long word between short gaps: no gap of 5 frames, the segment stays and is flagged
    words = [("a", 0, 30), ("b", 32, 60)]
    assert cut_segments(words, 64, 20, 5) == [(0, 2, 0, 62, True)]
    # padding by min_gap // 2, clamped to the recording
    assert cut_segments([("a", 1, 5)], 6, 20, 6) == [(0, 1, 0, 6, False)]
    assert cut_segments([("a", 10, 15)], 40, 20, 6) == [(0, 1, 7, 18, False)]


def test_cut_segments_empty():
    from espresso_amd.tools.forced_aligner import cut_segments

    assert cut_segments([], 100, 20, 3) == []


# ------------------------------------------------------------------------------------------------ parser and refusals
BASE = ["--path", "none.pt", "--dict", "none.txt", "--wav-scp", "none.scp", "--text", "none"]


@pytest.mark.parametrize("name,what", [("speech_transformer_transducer_base", "transducer"), ("speech_transformer_base", "attention")])
def test_long_form_refuses_models_without_ctc_logits_before_loading(name, what):
    from espresso_amd import speech_align

    with pytest.raises(NotImplementedError, match=f"encoder-only CTC models, not for the {what} model"):
        speech_align.main(BASE + ["--long-form", "--model", name])


def test_long_form_option_refusals():
    from espresso_amd import speech_align

    with pytest.raises(NotImplementedError, match="--confidence: the posterior kernel holds at most 1023 tokens"):
        speech_align.main(BASE + ["--long-form", "--confidence"])
    with pytest.raises(ValueError, match="--segments-dir .* give --long-form too"):
        speech_align.main(BASE + ["--segments-dir", "out"])
    with pytest.raises(ValueError, match="--segment-max-s .* give --long-form too"):
        speech_align.main(BASE + ["--segment-max-s", "10"])
    with pytest.raises(ValueError, match="--segment-min-silence-s .* give --long-form too"):
        speech_align.main(BASE + ["--segment-min-silence-s", "0.2"])
    with pytest.raises(ValueError, match="--long-form-window-s configures --long-form"):
        speech_align.main(BASE + ["--long-form-window-s", "20"])
    with pytest.raises(ValueError, match="give --segments-dir too"):
        speech_align.main(BASE + ["--long-form", "--segment-max-s", "10"])


def test_parser_has_the_long_form_and_segment_options():
    from espresso_amd import speech_align

    a = speech_align.get_parser().parse_args(BASE)
    assert (a.long_form, a.long_form_window_s, a.segments_dir, a.segment_max_s, a.segment_min_silence_s) == (False, None, None, None, None)
    assert (speech_align.DEFAULT_SEGMENT_MAX_S, speech_align.DEFAULT_SEGMENT_MIN_SILENCE_S) == (20.0, 0.3)
    p = speech_align.get_parser()
    text = p.format_help()
    assert "--long-form-guard-frames" in text and "--segment-min-silence-s" in text and "--segments-dir" in text
    helps = {o: a.help for a in p._actions for o in a.option_strings}
    for opt in ("--segment-max-s", "--segment-min-silence-s"):  # both defaults say that they are uncalibrated
        assert "uncalibrated" in helps[opt], opt


def test_check_long_form_args_tolerates_a_parser_without_streaming():
    from espresso_amd import speech_kws, speech_recognize
    from espresso_amd.tools import long_form as LF

    a = speech_recognize.get_parser().parse_args(BASE[:6] + ["--search", "ctc", "--long-form", "--streaming"])
    with pytest.raises(NotImplementedError, match="no --streaming"):
        LF.check_long_form_args(a)
    delattr(a, "streaming")
    LF.check_long_form_args(a)
    a = speech_kws.get_parser().parse_args(BASE[:6] + ["--keywords", "k", "--long-form", "--streaming"])
    with pytest.raises(NotImplementedError, match="no --streaming"):
        LF.check_long_form_args(a, tool="speech_kws")


# ------------------------------------------------------------------------------------------------ ABI (no GPU needed)
def _tile(lib):
    tb, ts = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.ea_ctc_viterbi_long_tile(ctypes.byref(tb), ctypes.byref(ts)) == 0
    return tb.value, ts.value


def test_abi_tile_and_workspace():
    from espresso_amd import _lib

    lib = _lib.lib()  # loads without a GPU and exports every symbol of the header
    for name in ("ea_ctc_viterbi_long_tile", "ea_ctc_viterbi_long_workspace_bytes", "ea_ctc_viterbi_long_align"):
        assert name in _lib.parse_header()
    tb, ts = _tile(lib)
    assert tb >= 1 and ts >= 16 and ts % 2 == 0
    ws = lib.ea_ctc_viterbi_long_workspace_bytes
    Ts = [0, 1, tb - 1, tb, tb + 1, 5 * tb + 3, 90000, 10 ** 6]
    Us = [0, 1, 7, ts // 2 - 1, ts // 2, ts // 2 + 1, 1023, 12000, 54000, 10 ** 5]
    for T in Ts:
        for U in Us:
            assert ws(T, U) >= 4 * T * -(-(2 * U + 1) // 16), (T, U)
    for U in Us:
        assert [ws(T, U) for T in Ts] == sorted(ws(T, U) for T in Ts)  # monotone in T
    for T in Ts:
        assert [ws(T, U) for U in Us] == sorted(ws(T, U) for U in Us)  # and in U
    big = ws(10 ** 6, 10 ** 5)
    assert big > 2 ** 31 and big > 0 and isinstance(big, int)  # a long, not a wrapped int
    assert ws(-1, 5) == 0 and ws(5, -1) == 0


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("seed", range(4))
def test_reference_vs_brute_force_with_frame_lp(seed):
    rng = np.random.default_rng(40 + seed)
    blank, n = 0, 0
    for V in (2, 3, 4):
        for T in range(1, 8):
            for U in range(0, 4):
                for trial in range(2):
                    y = list(rng.integers(1, V, size=U))
                    x = ref.quantised_lprobs(rng, T, V) if trial == 0 else np.log(rng.dirichlet(np.ones(V), size=T))
                    if trial == 0:
                        x = np.round(x / 4)  # few distinct values: ties on most frames
                    st, sc = _ctc_brute(x, T, y, blank)
                    fl, ts, te, flp, osc, _ = ref.align(x, y, blank)
                    assert flp.shape == (T,) and fl.shape == (T,) and ts.shape == te.shape == (U,)
                    if st is None:
                        assert osc == -np.inf and (fl == -2).all() and (ts == -1).all() and (te == -1).all() and (flp == 0).all()
                        continue
                    n += 1
                    lab = [blank if s % 2 == 0 else y[s // 2] for s in st]
                    assert osc == sc and list(fl) == [s // 2 if s % 2 else -1 for s in st]
                    assert list(flp) == [x[t, k] for t, k in enumerate(lab)]
                    assert osc == pytest.approx(flp.sum(), abs=1e-9)
    assert n > 100


def test_reference_fills_and_empty_cases():
    x = ref.quantised_lprobs(np.random.default_rng(0), 5, 4)
    fl, ts, te, flp, sc, _ = ref.align(x, [], 0)
    assert (fl == -1).all() and sc == x[:, 0].sum() and list(flp) == list(x[:, 0])
    fl, ts, te, flp, sc, _ = ref.align(x[:0], [], 0)
    assert sc == 0.0 and fl.shape == flp.shape == (0,)
    fl, ts, te, flp, sc, _ = ref.align(x[:0], [1], 0)
    assert sc == -np.inf and list(ts) == [-1]
    fl, ts, te, flp, sc, _ = ref.align(x[:2], [1, 1], 0)  # a repeat needs the blank between
    assert sc == -np.inf and (fl == -2).all() and (flp == 0).all()
    y = ref.targets_with_repeats(np.random.default_rng(1), 400, 37, 0)
    assert 0 not in y and 30 < int((y[1:] == y[:-1]).sum()) < 100
