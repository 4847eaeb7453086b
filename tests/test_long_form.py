"""Long-form recognition on the host (espresso_amd/tools/long_form.py against tests/long_form_ref.py): the window plan and its
frame grid against `frontend.num_frames` and `output_lengths` as they stand, the refusals, and the reference's own stitched
decode of planted spike trains.  The kernels are tested in tests/test_long_form_gpu.py."""
import math
import types

import numpy as np
import pytest

from espresso_amd.tools import long_form as LF
from tests import long_form_ref as ref

G = 640  # the recipes' samples per encoder frame: frame shift 160 x stride 4


class _Frontend:
    """The frame arithmetic of GpuFbankFrontend without its device tables."""
    frame_len, frame_shift, sample_rate, specaug, device = 400, 160, 16000, None, "cpu"

    def num_frames(self, n):
        from espresso_amd.data.gpu_frontend import GpuFbankFrontend

        return GpuFbankFrontend.num_frames(self, n)


def _model():
    """`output_lengths` of the recipes' sub-sampler (four 3x3 convolutions, time strides 1, 2, 1, 2)."""
    from espresso_amd.modules.speech_convolutions import ConvBNReLU

    pre = ConvBNReLU([4, 4, 4, 4], [(3, 3)] * 4, [(1, 1), (2, 2), (1, 1), (2, 2)])
    return types.SimpleNamespace(output_lengths=pre.output_lengths, pre_encoder=pre, training=False)


PLANS = [(40 * G, 8 * G), (50 * G, 2 * G), (9 * G, 4 * G), (30 * 16000 // G * G, 6 * 16000 // G * G)]


@pytest.mark.parametrize("W,O", PLANS)
def test_window_plan_covers_and_sits_on_the_frame_grid(W, O):
    fe, model = _Frontend(), _model()
    plan = LF.LongFormPlan(G, W, O)
    assert LF.samples_per_frame(fe, model) == G and LF.time_stride(model) == 4
    LF.check_grid(fe, model, plan)
    H = W - O
    assert (plan.Tw, plan.Of, plan.Hf) == (W // G, O // G, H // G)
    sizes = [400, 401, G, O, O + 1, W - 1, W, W + 1, W + H - 1, W + H, W + H + 1, H + O, H + O + 1, 2 * H + O + 1, 3 * H + O, 3 * H + O + 1,
             5 * H + O + 777, 7 * W + 12345]
    for N in sizes:
        wins = plan.windows(N)
        assert wins == ref.plan(N, W, O), N
        Nw = len(wins)
        assert Nw == max(1, math.ceil((N - O) / H)) == plan.num_windows(N)
        # cover: consecutive windows start a hop apart, overlap by O, and the last one ends with the recording
        assert wins[0][0] == 0 and wins[-1][0] + wins[-1][1] == N
        for n, (a, ln) in enumerate(wins):
            assert a == n * H and (ln == W if n < Nw - 1 else 0 < ln <= W)
        if Nw > 1:
            assert O < wins[-1][1] <= W  # no window lies wholly inside its predecessor
        # the frame grid: a full window has W / g frames, and the windows' frames add up to the recording's
        counts = LF.window_frames(fe, model, plan, N)
        assert all(c == plan.Tw for c in counts[:-1])
        offline = -(-fe.num_frames(N) // 4)
        assert int(model.output_lengths(fe.num_frames(N))) == offline
        assert (Nw - 1) * plan.Hf + counts[-1] == offline, N
        # front-end frame f of window n is the recording's frame n * H / 160 + f: same first sample
        for n, (a, ln) in enumerate(wins):
            assert a % fe.frame_shift == 0 and (n * H // fe.frame_shift) * fe.frame_shift == a
            if Nw > 1:
                assert a // fe.frame_shift + fe.num_frames(ln) <= fe.num_frames(N)


def test_plan_refusals():
    with pytest.raises(ValueError, match="half the window"):
        LF.LongFormPlan(G, 10 * G, 5 * G)
    with pytest.raises(ValueError, match="half the window"):
        LF.LongFormPlan(G, 10 * G, 7 * G)
    with pytest.raises(ValueError, match="two encoder frames"):
        LF.LongFormPlan(G, 10 * G, 1 * G)
    with pytest.raises(ValueError, match="multiples"):
        LF.LongFormPlan(G, 10 * G + 1, 2 * G)
    with pytest.raises(ValueError, match="edge frames"):
        LF.LongFormPlan(G, 40 * G, 8 * G, edge_frames=5)
    LF.LongFormPlan(G, 40 * G, 8 * G, edge_frames=4, guard_frames=0)
    p = LF.LongFormPlan.from_seconds(G, 16000)
    assert (p.W, p.O, p.edge, p.guard) == (480000, 96000, 37, 2)  # 30 s, 6 s, a quarter of 150 frames, 2


def test_grid_refusals_name_what_breaks():
    fe, model = _Frontend(), _model()
    plan = LF.LongFormPlan(G, 40 * G, 8 * G)
    odd = _Frontend()
    odd.dither = 1.0
    with pytest.raises(NotImplementedError, match="dither"):
        LF.check_grid(odd, model, plan)
    norm = _Frontend()
    norm.utterance_cmvn = True
    with pytest.raises(NotImplementedError, match="utterance_cmvn"):
        LF.check_grid(norm, model, plan)
    with pytest.raises(NotImplementedError, match="samples per encoder frame"):
        LF.check_grid(fe, model, LF.LongFormPlan(320, 40 * 320, 8 * 320))
    k5 = _model()
    k5.pre_encoder = types.SimpleNamespace(kernel_sizes=[(5, 5)])
    with pytest.raises(NotImplementedError, match="kernel size"):
        LF.check_grid(fe, k5, plan)
    wide = _Frontend()
    wide.frame_len = 1200  # a window then has fewer frames than W / g
    with pytest.raises(NotImplementedError, match="encoder frames, not"):
        LF.check_grid(wide, model, plan)


def test_command_line_refusals():
    from espresso_amd import speech_kws, speech_recognize

    base = ["--path", "none.pt", "--dict", "none.txt", "--wav-scp", "none.scp"]
    with pytest.raises(NotImplementedError, match="no --streaming"):
        speech_recognize.main(base + ["--search", "ctc", "--long-form", "--streaming"])
    with pytest.raises(NotImplementedError, match="--search ctc and --search ctc_beam"):
        speech_recognize.main(base + ["--search", "transducer_greedy", "--long-form"])
    with pytest.raises(NotImplementedError, match="--confidence"):
        speech_recognize.main(base + ["--search", "ctc", "--long-form", "--confidence"])
    with pytest.raises(ValueError, match="give --long-form too"):
        speech_recognize.main(base + ["--search", "ctc", "--long-form-window-s", "20"])
    with pytest.raises(NotImplementedError, match="no --streaming"):
        speech_kws.main(base + ["--keywords", "none.txt", "--long-form", "--streaming"])
    for tool in (speech_recognize, speech_kws):
        text = tool.get_parser().format_help()
        assert "--long-form-guard-frames" in text and "uncalibrated" in text


# ------------------------------------------------------------------------------------------------ the reference's own decode
BLANK = 0


def _spike_train(T, V, spikes, rng):
    """Log-probs [T][V]: blank everywhere but at the (frame, token) spikes, with a little noise in the other columns."""
    p = rng.uniform(0.001, 0.004, size=(T, V))
    p[:, BLANK] = 1.0
    for t, k in spikes:
        p[t, BLANK] = 0.01
        p[t, k] = 1.0
    return np.log(p / p.sum(axis=1, keepdims=True))


def _windows_of(lp, Tw, Hf, Nw):
    """The recording's rows sliced into windows [Nw][Tw][V] (+ counts); rows past a short last window are NaN."""
    T, V = lp.shape
    out = np.full((Nw, Tw, V), np.nan)
    counts = []
    for n in range(Nw):
        c = min(Tw, T - n * Hf)
        out[n, :c] = lp[n * Hf: n * Hf + c]
        counts.append(c)
    return out, counts


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("guard", [0, 2])
def test_reference_stitch_decodes_a_spike_train_with_noisy_window_edges(seed, guard):
    rng = np.random.default_rng(seed)
    V, Tw, Of, E = 12, 40, 12, 3
    Hf = Tw - Of
    Nw = 4
    T = (Nw - 1) * Hf + int(rng.integers(Of + 1, Tw + 1))
    frames = sorted(rng.choice(np.arange(1, T - 1), size=T // 4, replace=False).tolist())
    lp = _spike_train(T, V, [(t, int(rng.integers(1, V))) for t in frames], rng)
    wins, counts = _windows_of(lp, Tw, Hf, Nw)
    # what a window computes near its own ends is not to be trusted: noise in the first E frames of every window but the first
    # and the last E of every window but the last (the recording's own ends lie in one window only)
    for n in range(Nw):
        if n > 0:
            wins[n, :E] = ref.log_softmax64(rng.normal(size=(E, V)) * 4)
        if n < Nw - 1:
            wins[n, Tw - E:] = ref.log_softmax64(rng.normal(size=(E, V)) * 4)
    cut_list, scores, _ = ref.cuts(wins, counts, Hf, V, BLANK, E, guard)
    for n, c in enumerate(cut_list):
        assert (n + 1) * Hf + E <= c <= n * Hf + Tw - E
    got = ref.stitch(wins, counts, cut_list, Hf, V)
    assert got.shape == lp.shape and not np.isnan(got).any()
    assert ref.greedy(got, BLANK) == ref.greedy(lp, BLANK)


def test_guard_keeps_a_token_that_a_bare_mid_cut_drops():
    """Two windows put the same token's spike on different sides of the overlap's middle: window n one frame late, window n + 1
    one frame early.  A cut fixed at the middle, without the rule (guard 0, no scoring), takes neither -- the token is dropped.
    The rule (guard 2) scores every cut within two frames of either spike by the spike's low blank log-prob and moves away, so
    the token comes whole from one window."""
    rng = np.random.default_rng(0)
    V, Tw, Of = 8, 24, 8
    Hf = Tw - Of
    T = Hf + Tw
    lo, hi = Hf, Tw
    mid = (lo + hi) // 2
    spikes = [(3, 2), (9, 5), (T - 4, 3)]
    tok = 6
    truth = _spike_train(T, V, spikes + [(mid, tok)], rng)
    seen_a = _spike_train(T, V, spikes + [(mid, tok)], rng)      # window n: at the middle frame, which a mid-cut gives away
    seen_b = _spike_train(T, V, spikes + [(mid - 1, tok)], rng)  # window n + 1: one frame earlier, which a mid-cut gives away too
    wins = np.full((2, Tw, V), np.nan)
    wins[0] = seen_a[:Tw]
    wins[1] = seen_b[Hf:]
    counts = [Tw, Tw]
    want = ref.greedy(truth, BLANK)
    assert tok in want
    bare = ref.stitch(wins, counts, [mid], Hf, V)
    assert ref.greedy(bare, BLANK) == [k for k in want if k != tok]  # dropped
    cut_list, scores, _ = ref.cuts(wins, counts, Hf, V, BLANK, 1, 2)
    assert abs(cut_list[0] - mid) >= 2 and scores[0] > math.log(0.9)
    assert ref.greedy(ref.stitch(wins, counts, cut_list, Hf, V), BLANK) == want
