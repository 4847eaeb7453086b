"""Long-form per-token posteriors on the host: the `--long-form-posteriors` option of speech_recognize and speech_align (parser,
help, refusals), the C ABI of csrc/prefix_posterior_long.hip as far as it runs without a GPU, and the `confidence` file of
speech_align --segments-dir on hand-made spans and posteriors.  The kernels are tested in tests/test_long_posteriors_gpu.py."""
import ctypes
import math

import numpy as np
import pytest

BASE = ["--path", "none.pt", "--dict", "none.txt", "--wav-scp", "none.scp", "--text", "none"]
FAMILY = "--long-form-posteriors configures --long-form: give --long-form too"


# ------------------------------------------------------------------------------------------------ parser and refusals
def test_option_without_long_form_is_refused_in_both_tools():
    from espresso_amd import speech_align, speech_recognize

    with pytest.raises(ValueError, match=FAMILY):
        speech_align.main(BASE + ["--long-form-posteriors"])
    for search in ("ctc", "ctc_beam"):
        with pytest.raises(ValueError, match=FAMILY):
            speech_recognize.main(BASE[:6] + ["--search", search, "--long-form-posteriors"])


def test_option_is_refused_with_the_lexicon_search():
    from espresso_amd import speech_recognize

    with pytest.raises(NotImplementedError, match="--long-form-posteriors scores the model's sub-word tokens: no --ngram-lm"):
        speech_recognize.main(BASE[:6] + ["--search", "ctc_beam", "--long-form", "--long-form-posteriors", "--ngram-lm", "none.arpa"])


def test_confidence_stays_refused_with_long_form_and_says_so_as_before():
    """--confidence keeps its cap: the new option is the uncapped path, the old refusals and their messages do not change."""
    from espresso_amd import speech_align, speech_recognize

    with pytest.raises(NotImplementedError, match="--confidence: the posterior kernel holds at most 1023 tokens per transcript"):
        speech_align.main(BASE + ["--long-form", "--long-form-posteriors", "--confidence"])
    with pytest.raises(NotImplementedError, match="--confidence: the posterior kernel holds at most 1023 tokens per hypothesis"):
        speech_recognize.main(BASE[:6] + ["--search", "ctc", "--long-form", "--long-form-posteriors", "--confidence"])


def test_option_is_in_the_help_of_both_tools_and_not_of_speech_kws():
    from espresso_amd import speech_align, speech_kws, speech_recognize

    for tool in (speech_align, speech_recognize):
        p = tool.get_parser()
        helps = {o: a.help for a in p._actions for o in a.option_strings}
        assert "--long-form-posteriors" in p.format_help()
        assert "not been measured" in helps["--long-form-posteriors"], tool.__name__  # the calibration is unmeasured, and says so
    assert speech_align.get_parser().parse_args(BASE).long_form_posteriors is False
    assert speech_recognize.get_parser().parse_args(BASE[:6] + ["--long-form", "--long-form-posteriors"]).long_form_posteriors is True
    assert "--long-form-posteriors" not in speech_kws.get_parser().format_help()
    assert "--long-form-window-s" in speech_kws.get_parser().format_help()  # (the shared family is still there)


# ------------------------------------------------------------------------------------------------ ABI (no GPU needed)
def test_header_declares_the_entry_points_and_the_workspace_follows_the_aligners_tile():
    from espresso_amd import _lib

    decl = _lib.parse_header()
    assert decl["ea_ctc_prefix_long_workspace_bytes"] == (ctypes.c_long, [ctypes.c_long, ctypes.c_long])
    assert len(decl["ea_ctc_prefix_long_posteriors"][1]) == 13 and decl["ea_ctc_prefix_long_posteriors"][0] is ctypes.c_int
    lib = _lib.lib()
    tb, ts = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.ea_ctc_viterbi_long_tile(ctypes.byref(tb), ctypes.byref(ts)) == 0
    tb, ts = tb.value, ts.value
    ws = lib.ea_ctc_prefix_long_workspace_bytes
    # the workspace steps exactly where the aligner's tile says a frame block or a state tile is added: the two files agree
    for U in (0, 5, ts):
        assert ws(1, U) == ws(tb, U) < ws(tb + 1, U) == ws(2 * tb, U) < ws(2 * tb + 1, U)
    for T in (1, 3 * tb):
        assert ws(T, 0) == ws(T, ts // 2 - 1) < ws(T, ts // 2) == ws(T, ts - 1) < ws(T, ts)
    assert ws(0, 0) > 0 and ws(0, 10 ** 5) > 4 * (2 * 10 ** 5 + 1)  # T = 0: alpha, psi and the flags
    # alpha [S] + edge [tiles][T][2] + psi [U] fp32, padded to whole tiles: an hour against 54 000 tokens is about 77 MB
    T, U = 90000, 54000
    nI, nJ = -(-T // tb), -(-(2 * U + 1) // ts)
    assert 0 <= ws(T, U) - (4 * nJ * ts + 8 * nJ * nI * tb + 2 * nJ * ts) <= 1 << 16
    assert 70e6 < ws(T, U) < 80e6 and ws(T, U) * 20 < lib.ea_ctc_viterbi_long_workspace_bytes(T, U)
    big = ws(10 ** 7, 10 ** 5)
    assert big > 2 ** 31 and isinstance(big, int)  # a long, not a wrapped int
    assert ws(-1, 5) == 0 and ws(5, -1) == 0 and ws(2 ** 30 + 1, 5) == 0 and ws(5, 2 ** 28 + 1) == 0
    assert ws(2 ** 30, 5) > 0 and ws(5, 2 ** 28) > 0
    for T, V, U in ((-1, 8, 2), (20, 8, -1), (20, 0, 2), (2 ** 30 + 1, 8, 2), (20, 8, 2 ** 28 + 1)):  # refused before any launch
        assert lib.ea_ctc_prefix_long_posteriors(None, 8, 0, None, None, None, None, None, T, V, U, 0, None) == -2
    assert lib.ea_ctc_prefix_long_posteriors(None, 7, 0, None, None, None, None, None, 20, 8, 2, 0, None) == -2  # ld < V
    for blank in (-1, 8):
        assert lib.ea_ctc_prefix_long_posteriors(None, 8, 0, None, None, None, None, None, 20, 8, 2, blank, None) == -2


# ------------------------------------------------------------------------------------------------ word factors and the confidence file
SYMS = ["<space>", "a", "b", "c", "▁de", "f", "▁g"]


class _Dict:
    space_word = "<space>"

    def __getitem__(self, i):
        return SYMS[i]


def test_word_log_factors_group_as_unit_confidences():
    from espresso_amd.tools.token_posteriors import segment_confidence, unit_confidences, word_log_factors

    rng = np.random.default_rng(0)
    for ids in ([1, 2, 0, 3, 0, 0, 1], [0, 1, 0], [4, 5, 6, 5, 4], [1, 4, 5, 0, 6], [], [0, 0]):
        syms = [SYMS[i] for i in ids]
        f = (-rng.random(len(ids)) * 3).tolist()
        rows = word_log_factors(syms, f)
        want = unit_confidences(syms, f, "word")
        assert len(rows) == len(want) and all(math.exp(sum(r)) == pytest.approx(w, rel=1e-12) for r, w in zip(rows, want))
        assert sum(len(r) for r in rows) == sum(s != "<space>" for s in syms)  # every token of a word once, no <space>
    # word product, mean over the words' tokens, min over the words; the empty segment
    rows = [[math.log(0.5), math.log(0.5)], [math.log(0.9)], [math.log(0.1), 0.0, 0.0]]
    mean, low, n = segment_confidence(rows)
    assert n == 3 and low == pytest.approx(0.1) and mean == pytest.approx((2 * math.log(0.5) + math.log(0.9) + math.log(0.1)) / 6)
    assert segment_confidence(rows[:2]) == (pytest.approx((2 * math.log(0.5) + math.log(0.9)) / 3), pytest.approx(0.25), 2)
    assert segment_confidence([]) == (0.0, 1.0, 0)
    mean, low, n = segment_confidence([[-math.inf, -1.0]])  # a token the model gives no mass: probability 0, not NaN
    assert mean == -math.inf and low == 0.0 and n == 1


def test_confidence_file_on_hand_made_spans(tmp_path):
    from espresso_amd import speech_align
    from espresso_amd.tools.forced_aligner import cut_segments, utterance_units

    # words ab | c | (a long silence) | b | ac: tokens a b <space> c <space> b <space> a c
    tokens = [1, 2, 0, 3, 0, 2, 0, 1, 3]
    start = [2, 4, 6, 8, 10, 40, 43, 45, 47]
    end = [4, 6, 7, 10, 11, 43, 44, 47, 50]
    post = np.log(np.array([0.9, 0.5, 0.99, 0.2, 0.98, 0.8, 0.97, 0.5, 0.5], dtype=np.float32))
    r = {"tokens": np.array(tokens), "start": np.array(start), "end": np.array(end), "frames": 60, "token_posteriors": post,
         "frame_lp": np.full(60, -0.5, dtype=np.float32)}
    d = _Dict()
    words = utterance_units(r, d, "word")
    assert [w for w, _, _ in words] == ["ab", "c", "b", "ac"]
    segs = cut_segments(words, 60, 30, 5)
    assert [(a, b) for a, b, _, _, _ in segs] == [(0, 2), (2, 4)]
    speech_align.write_segments(str(tmp_path), [("rec", r)], d, 0.04, 30, 5)
    before = {n: (tmp_path / n).read_bytes() for n in ("segments", "text", "scores")}
    speech_align.write_confidence(str(tmp_path), [("rec", r)], d, 30, 5)
    assert {n: (tmp_path / n).read_bytes() for n in before} == before  # the three files of write_segments are not touched
    lines = [l.split() for l in (tmp_path / "confidence").read_text().splitlines()]
    assert [l[0] for l in lines] == [l.split()[0] for l in before["segments"].decode().splitlines()] == ["rec_0000", "rec_0001"]
    p = np.exp(post.astype(np.float64))
    want = [((post[0] + post[1] + post[3]) / 3, min(p[0] * p[1], p[3]), 2), ((post[5] + post[7] + post[8]) / 3, min(p[5], p[7] * p[8]), 2)]
    for l, (mean, low, n) in zip(lines, want):
        assert len(l) == 4 and int(l[3]) == n
        assert float(l[1]) == pytest.approx(float(mean), abs=5e-5) and float(l[2]) == pytest.approx(float(low), abs=5e-5)
    assert float(lines[0][2]) == pytest.approx(0.2, abs=5e-5) and float(lines[1][2]) == pytest.approx(0.25, abs=5e-5)
