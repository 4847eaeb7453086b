"""Long-form recognition for transducer models on the host: the fp64 restatement of the feature rule
(tests/long_form_features_ref.py) checks itself, every case of the GPU test has a margin above the fp32 error bound, and the
command line refuses what --long-form-transducer does not do on argument parsing alone.  The kernels are tested in
tests/test_long_form_transducer_gpu.py."""
import math

import numpy as np
import pytest

from tests import long_form_features_ref as fref


def _two_windows(rng, Tw, Of, D):
    """Two windows with identical overlap rows."""
    Hf = Tw - Of
    x = rng.standard_normal((2, Tw, D))
    x[1, :Of] = x[0, Hf:]
    return x, [Tw, Tw], Hf


def test_identical_overlap_rows_give_zero_and_the_middle_cut():
    rng = np.random.default_rng(0)
    for Tw, Of in ((16, 5), (16, 4), (8, 1), (24, 8)):
        x, counts, Hf = _two_windows(rng, Tw, Of, 12)
        lo, hi = Hf, Tw
        for j in range(lo, hi):
            assert fref.distance(x[0, j], x[1, j - lo], 12) == 0.0
        for guard in (0, 2):
            for edge in (0, 1):
                cs, ss, margin = fref.cuts(x, counts, Hf, 12, edge, guard)
                cands = list(range(lo + edge, hi - edge + 1))
                want = min(cands, key=lambda c: (abs(2 * c - (lo + hi)), c)) if cands else (lo + hi) // 2
                assert cs == [want] and ss == [0.0] and margin == math.inf
    # lo + hi odd: two cuts are equally near the middle, the smaller one wins
    x, counts, Hf = _two_windows(rng, 16, 5, 12)
    assert fref.cuts(x, counts, Hf, 12, 0, 0)[0] == [Hf + 2]


def test_distance_lies_in_0_2_and_columns_past_D_are_not_read():
    rng = np.random.default_rng(1)
    a = rng.standard_normal(9)
    assert fref.distance(a, -a, 9) == pytest.approx(2.0)
    assert fref.distance(a, np.zeros(9), 9) == pytest.approx(1.0)
    assert fref.distance(np.zeros(9), np.zeros(9), 9) == 0.0  # den == 0
    b = a.copy()
    b[6:] = 1e9
    assert fref.distance(a, b, 6) == 0.0


def test_a_planted_stretch_of_agreement_is_found():
    rng = np.random.default_rng(2)
    Tw, Of, D = 40, 12, 16
    Hf = Tw - Of
    for plant in (2, 6, 9):
        x, counts = fref.windows_with_planted_agreement(rng, 3, Tw, Hf, D, D, Tw, [plant, plant])
        for guard in (1, 2):
            cs, ss, margin = fref.cuts(x, counts, Hf, D, 2, guard)
            for n, c in enumerate(cs):
                lo = (n + 1) * Hf
                # the guard range [c - guard, c + guard) holds the planted frame, and the least disagreement around it
                assert c - guard <= lo + plant < c + guard, (plant, guard, cs)
                assert -0.1 < ss[n] < 0.0
            assert margin > 0
        own = fref.owners(counts, cs, Hf)
        rows = fref.stitch_rows(x, counts, cs, Hf, D)
        assert rows.shape == (2 * Hf + Tw, D)
        for t, (n, j) in enumerate(own):
            assert np.array_equal(rows[t], x[n, j, :D])


def test_guard_zero_and_no_candidates_take_the_fallbacks():
    rng = np.random.default_rng(3)
    Tw, Of, D = 24, 8, 8
    Hf = Tw - Of
    x, counts = fref.windows_with_planted_agreement(rng, 2, Tw, Hf, D, D, Tw, [3])
    lo, hi = Hf, Tw
    s = [-fref.distance(x[0, j], x[1, j - lo], D) for j in range(lo, hi)]
    # guard 0: the range [c, c) is empty, score(c) = s at the overlap frame nearest c (hi - 1 for c == hi)
    c, sc, ranked = fref.junction(x, counts, 0, Hf, D, 0, 0)
    by_c = dict((cc, v) for v, cc in ranked)
    assert [by_c[cc] for cc in range(lo, hi + 1)] == s + [s[-1]]
    assert sc == max(s) and c == lo + int(np.argmax(s)) == lo + 3
    # first > last: the middle, scored as any cut is
    c, sc, ranked = fref.junction(x, counts, 0, Hf, D, 5, 2)
    assert ranked == [] and c == (lo + hi) // 2 and sc == min(s[c - 2 - lo: c + 2 - lo])
    # no overlap at all
    assert fref.junction(x, [Hf, Tw], 0, Hf, D, 0, 2) == (lo, 0.0, [])


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_every_gpu_case_has_a_margin_above_the_fp32_bound(dtype):
    """The GPU test compares a cut with the fp64 cut where the fp64 lead of the best score over the next lower one exceeds the
    fp32 error bound of both (2 x bound(D)): here every case is shown to have such a lead, so none is left uncompared."""
    uncompared = 0
    for case in fref.GPU_CASES:
        name, Nw, Tw, Of, D, ld, last, offset, edge, guard = case
        x, counts, Hf, plant = fref.gpu_case(case, dtype)
        cs, ss, margin = fref.cuts(x, counts, Hf, D, edge, guard)
        assert all(-2.0 <= s <= 0.0 for s in ss)
        if not margin > 2 * fref.bound(D):
            uncompared += 1
    assert uncompared == 0
    assert fref.bound(512) == pytest.approx(4 * 516 / 2 ** 24) and fref.bound(512) < 1.3e-4


# ------------------------------------------------------------------------------------------------ the command line
BASE = ["--path", "none.pt", "--dict", "none.txt", "--wav-scp", "none.scp"]
LFT = ["--long-form-transducer"]


@pytest.mark.parametrize("extra,exc,match", [
    (["--search", "transducer_frame_beam", "--long-form"], NotImplementedError, "--long-form-transducer and --long-form"),
    (["--search", "transducer_greedy", "--streaming"], NotImplementedError, "--long-form-transducer .* no --streaming"),
    (["--search", "ctc"], NotImplementedError, "--long-form-transducer .* not --search ctc .*--long-form"),
    (["--search", "ctc_beam"], NotImplementedError, "--long-form-transducer .* not --search ctc_beam"),
    (["--search", "beam"], NotImplementedError, "--long-form-transducer .* not --search beam"),
    (["--search", "transducer_beam"], NotImplementedError, "--long-form-transducer .* --search transducer_beam: the Adaptive Expansion Search"),
    (["--search", "transducer_frame_beam", "--confidence"], NotImplementedError, "--long-form-transducer .* --confidence"),
    (["--search", "transducer_greedy", "--print-alignment", "--results-path", "x"], NotImplementedError, "--long-form-transducer .* --print-alignment"),
    (["--search", "transducer_frame_beam", "--path", "a.pt:b.pt"], NotImplementedError, "--long-form-transducer takes one model"),
    (["--search", "transducer_frame_beam", "--long-form-window-s", "0"], ValueError, "--long-form-window-s must be positive"),
])
def test_refusals_fire_on_argument_parsing_alone(extra, exc, match):
    from espresso_amd import speech_recognize

    with pytest.raises(exc, match=match):
        speech_recognize.main(BASE + LFT + extra)


def test_model_kind_refusals_name_the_flag():
    from espresso_amd.tools import long_form as LF

    with pytest.raises(NotImplementedError, match="--long-form-transducer is implemented for transducer models, not for the ctc model .*--long-form"):
        LF.require_transducer_model("speech_transformer_encoder_model")
    with pytest.raises(NotImplementedError, match="--long-form-transducer is implemented for transducer models, not for the attention model"):
        LF.require_transducer_model("speech_transformer_base")
    LF.require_transducer_model("speech_transformer_transducer_base")


def test_long_form_itself_keeps_refusing_transducers_and_names_the_new_flag():
    from espresso_amd import speech_recognize
    from espresso_amd.tools import long_form as LF

    with pytest.raises(NotImplementedError, match="--search ctc and --search ctc_beam, not --search transducer_greedy .*--long-form-transducer"):
        speech_recognize.main(BASE + ["--search", "transducer_greedy", "--long-form"])
    with pytest.raises(NotImplementedError, match="encoder-only CTC models, not for the transducer model .*--long-form-transducer"):
        LF.require_ctc_model("speech_transformer_transducer_base")
    with pytest.raises(ValueError, match="give --long-form too"):
        speech_recognize.main(BASE + ["--search", "transducer_greedy", "--long-form-guard-frames", "3"])


def test_the_flag_is_in_the_help_and_says_uncalibrated():
    from espresso_amd import speech_recognize

    text = " ".join(speech_recognize.get_parser().format_help().split())
    assert "--long-form-transducer" in text
    at = text.index("--long-form-transducer transducer_greedy / transducer_frame_beam")
    assert "uncalibrated" in text[at: at + 1200]


def test_the_options_of_long_form_configure_the_transducer_plan():
    from espresso_amd import speech_recognize

    args = speech_recognize.get_parser().parse_args(BASE + LFT + ["--search", "transducer_greedy", "--long-form-window-s", "20",
                                                                   "--long-form-overlap-s", "4", "--long-form-edge-frames", "3",
                                                                   "--long-form-guard-frames", "1"])
    from espresso_amd.tools import long_form as LF

    LF.check_long_form_transducer_args(args)
    LF.check_long_form_args(args)  # (no "give --long-form too")
    plan = LF.LongFormPlan.from_seconds(640, 16000, args.long_form_window_s, args.long_form_overlap_s, args.long_form_edge_frames,
                                        args.long_form_guard_frames)
    assert (plan.Tw, plan.Of, plan.Hf, plan.edge, plan.guard) == (500, 100, 400, 3, 1)
