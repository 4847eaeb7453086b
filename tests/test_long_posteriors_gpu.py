"""Long-form per-token posteriors on the device (csrc/prefix_posterior_long.hip, kernels.ctc_prefix_posteriors_long,
`LongFormCTCAligner(token_posteriors=True)`, `--long-form-posteriors` of speech_align and speech_recognize): the tiled kernel
against the float64 oracle of tests/prefix_posterior_ref.py, bit for bit against the one-workgroup kernel
`kernels.ctc_prefix_posteriors` wherever that one takes the problem, the conventions of the header, and the whole path on the tiny
CTC fixture model and the two command lines.  Every shape is built from `ea_ctc_viterbi_long_tile`.

The bound against float64.  For every case and each of Psi, total and the finite factors log c, `e32` is the largest error that
a plain numpy float32 restatement of the recurrence (`_restate_fp32`: the oracle's statements on float32 arrays, numpy's
correctly rounded exp / log) shows for that quantity against the float64 oracle on the same inputs; the kernel's error in it
must stay within 8 * max(e32, ulp32(scale)) (the margin of DESIGN.md section 3.6 for the 1-ulp hardware exp / log) and within that
section's derived worst case 3 * (T + U + 2) * ulp32(scale).  (One e32 per quantity asks more than one e32 for all three: the
factors' own e32 is far below Psi's, whose neighbours' errors cancel in a factor.)  `scale` is |total|, and where total is -inf (the transcript does not fit the frames, which is so for every T up to
2 TB + 1 against 3 1/2 state tiles) the largest finite |Psi_i|, which is what |total| is the largest of when it is finite.  -inf
must sit exactly where the oracle has it."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import prefix_posterior_ref as pref
from tests.long_align_ref import targets_with_repeats

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
BLANK = 0
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib
    from espresso_amd import kernels as K

    _lib.lib()
    return K


def _peaked_lprobs(rng, T, V, sharp=3.0):
    z = rng.standard_normal((T, V)) * sharp
    z -= z.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def _on_device(x, dtype, ld=None):
    """x float64 [T][V] -> (the device matrix [T][V] in dtype, a view of a [T][ld] buffer whose pad columns hold NaN when ld is
    given; the same values as float64 on the host)."""
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV)
    if ld is not None:
        buf = torch.full((x.shape[0], ld), float("nan"), dtype=dtype, device=DEV)
        buf[:, : x.shape[1]] = xd
        xd = buf[:, : x.shape[1]]
    return xd, xd.double().cpu().numpy().reshape(x.shape)


def _run(K, xd, y, V, blank=BLANK, ld=None):
    """The kernel on a device matrix and host ids: (logc float32 [U + 1], total float32 scalar, psi float32 [U]) as numpy."""
    yd = torch.from_numpy(np.asarray(y, dtype=np.int32)).to(DEV)
    T = xd.shape[0]
    logc, total, psi = K.ctc_prefix_posteriors_long(xd, yd, T, V, blank, ld=ld, want_psi=True)
    assert logc.shape == (len(y) + 1,) and total.shape == (1,) and psi.shape == (len(y),)
    assert logc.dtype == total.dtype == psi.dtype == torch.float32
    return logc.cpu().numpy(), total.cpu().numpy()[0], psi.cpu().numpy()


def _restate_fp32(x, y, blank):
    """`ctc_prefix_oracle`'s recurrence, every value and every operation in numpy float32.  Returns (psi [U], total)."""
    x = np.asarray(x, dtype=np.float32)
    T, U = x.shape[0], len(y)
    S = 2 * U + 1
    ninf = np.float32(-np.inf)
    lab = np.array([blank if s % 2 == 0 else y[s // 2] for s in range(S)])
    allow2 = np.zeros(S, dtype=bool)
    allow2[3::2] = lab[3::2] != lab[1:-2:2]
    a = np.full(S, ninf, dtype=np.float32)
    psi = np.full(U, ninf, dtype=np.float32)
    a[0] = x[0, blank]
    if S > 1:
        a[1] = x[0, lab[1]]
        psi[0] = a[1]
    for t in range(1, T):
        c1 = np.concatenate([[ninf], a[:-1]]).astype(np.float32)
        c2 = np.concatenate([[ninf, ninf], a[:-2]]).astype(np.float32) if S > 1 else np.full(S, ninf, dtype=np.float32)
        c2[~allow2] = ninf
        e = x[t, lab]
        with np.errstate(invalid="ignore"):
            enter = np.logaddexp(c1, c2) + e
            psi = np.logaddexp(psi, enter[1::2])
            a = np.logaddexp(a + e, enter)
        assert enter.dtype == psi.dtype == a.dtype == np.float32
    with np.errstate(invalid="ignore"):
        total = np.logaddexp(a[S - 1], a[S - 2] if S > 1 else ninf)
    return psi, np.float32(total)


def _finite_err(got, want):
    """Largest |got - want| over the entries where `want` is finite (0 when there is none)."""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    m = np.isfinite(want)
    return float(np.abs(got[m] - want[m]).max()) if m.any() else 0.0


def _reference(x64, y, blank=BLANK):
    """The float64 oracle, the float32 restatement's error against it, and the two bounds of the module docstring."""
    T, U = x64.shape[0], len(y)
    psi, total = pref.ctc_prefix_oracle(x64, T, [int(k) for k in y], blank)
    logc, _ = pref.factors(psi, total)
    psi32, total32 = _restate_fp32(x64, y, blank)
    logc32, _ = pref.factors(psi32.astype(np.float64), float(total32))
    assert np.array_equal(np.isneginf(psi32), np.isneginf(psi)) and np.isneginf(total32) == np.isneginf(total)
    e32 = {"psi": _finite_err(psi32, psi), "total": _finite_err(total32, total), "logc": _finite_err(logc32, logc)}
    finite = [abs(total)] if np.isfinite(total) else []
    finite += list(np.abs(psi[np.isfinite(psi)]))
    ulp = float(np.spacing(np.float32(max(finite)))) if finite else 0.0
    return {"psi": psi, "total": total, "logc": logc, "e32": e32, "ulp": ulp, "bound": {k: 8 * max(e, ulp) for k, e in e32.items()},
            "worst": 3 * (T + U + 2) * ulp}


def _assert_within(got, want, bound, what):
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert not np.isnan(got).any(), what
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), (what, np.nonzero(np.isneginf(got) != np.isneginf(want))[0][:10])
    err = _finite_err(got, want)
    assert err <= bound, (what, err, bound)
    return err


# ------------------------------------------------------------------------------------------------ against the float64 oracle
V_ORACLE, LD_ORACLE = 20, 24
ORACLE_FRAMES = ("TB-1", "TB", "TB+1", "2TB+1", "17TB+1")  # the last one holds the transcript: total is finite there


def _oracle_frames(TB):
    return dict(zip(ORACLE_FRAMES, (TB - 1, TB, TB + 1, 2 * TB + 1, 17 * TB + 1)))


@functools.lru_cache(maxsize=None)
def _oracle_case(TB, TS, frames, dtype_name):
    """Inputs and reference of one case, computed once: (device matrix, y, T, reference)."""
    U = 7 * TS // 4  # S = 2U + 1 spans 3 1/2 state tiles
    T =_oracle_frames(TB)[frames]
    rng = np.random.default_rng([21, T])
    y = targets_with_repeats(rng, U, V_ORACLE, BLANK)
    assert int((y[1:] == y[:-1]).sum()) > U // 10
    # logits of unit variance: many alignments of comparable mass, so the log-add-exps matter (at 3 N(0, 1) one path dominates,
    # most of them return their larger argument and the kernel's errors are the restatement's own to four digits)
    xd, x64 = _on_device(_peaked_lprobs(rng, T, V_ORACLE, sharp=1.0), DTYPES[dtype_name], ld=LD_ORACLE)
    return xd, y, T, _reference(x64, y)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("frames", ORACLE_FRAMES)
def test_against_the_float64_oracle(frames, dtype_name):
    """S = 2U + 1 over 3 1/2 state tiles (U = 7 TS / 4 = 1792 tokens with repeats), T around one and two frame blocks and,
    beyond the issue's list, T = 17 TB + 1, which holds the transcript, so that a finite total, the sum rule and the CTC loss
    are checked on the tiled shape too.  V = 20 from a matrix of row pitch 24 whose pad columns hold NaN.
    MI355X, one run (largest error of Psi / total / log c against its bound 8 * max(e32, ulp)): see DESIGN.md section 3.10."""
    K = _need_gpu()
    TB, TS = K.ctc_viterbi_long_tile()
    xd, y, T, ref = _oracle_case(TB, TS, frames, dtype_name)
    U = len(y)
    assert (2 * U + 1) > 3 * TS and (2 * U + 1) % TS not in (0, 1)
    logc, total, psi = _run(K, xd, y, V_ORACLE, ld=LD_ORACLE)
    errs = [_finite_err(psi, ref["psi"]), _finite_err(total, ref["total"]), _finite_err(logc, ref["logc"])]
    e32, bound = ref["e32"], ref["bound"]
    print(f"T {T} U {U} {dtype_name}: total {ref['total']:.3f}, ulp {ref['ulp']:.3e}, worst case {ref['worst']:.3e}; Psi / total / log c: "
          f"e32 {e32['psi']:.3e} {e32['total']:.3e} {e32['logc']:.3e}, bound {bound['psi']:.3e} {bound['total']:.3e} {bound['logc']:.3e}, "
          f"kernel {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e}")
    assert max(bound.values()) <= ref["worst"]
    for got, key in ((psi, "psi"), (total, "total"), (logc, "logc")):
        _assert_within(got, ref[key], bound[key], key)
    assert (logc[np.isfinite(logc)] <= 0).all()
    n_reach = int(np.isfinite(ref["psi"]).sum())
    if T <= 2 * TB + 1:  # too few frames: at most T tokens can have started, total and the rest are -inf (exactly, checked above)
        assert 0 < n_reach <= T < U and np.isneginf(ref["total"]) and np.isneginf(psi[T:]).all() and np.isneginf(logc[T:]).all()
        return
    assert n_reach == U and np.isfinite(ref["total"])
    # the sum rule: the factors add up to total, up to what the clamp at 0 took away
    chain = np.concatenate([[0.0], psi.astype(np.float64), [float(total)]])
    clamped = float(np.maximum(np.diff(chain), 0).sum())
    assert abs(float(logc.astype(np.float64).sum()) - ref["total"]) <= bound["total"] + clamped, (logc.astype(np.float64).sum(), ref["total"], clamped)
    lp = torch.from_numpy(xd.double().cpu().numpy()).unsqueeze(1)  # [T][1][V] float64 on the host
    loss = torch.nn.functional.ctc_loss(lp, torch.from_numpy(y.astype(np.int64)).unsqueeze(0), torch.tensor([T]), torch.tensor([U]),
                                        blank=BLANK, reduction="sum")
    assert abs(float(total) + float(loss)) <= bound["total"], (float(total), float(loss))


# ------------------------------------------------------------------------------------------------ against the one-workgroup kernel
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("frames", ["TB-1", "3TB+5", "10TB+3"])
@pytest.mark.parametrize("U", [0, 1, 7, 511, 512, 1023])
def test_bit_identical_to_the_one_workgroup_kernel(U, frames, dtype_name):
    """Both kernels call prefix_frame of csrc/ctc_lattice.h and so do the same fp32 operations in the same order: logc, total and psi are
    `torch.equal` to ea_ctc_prefix_posteriors' at one hypothesis.  U = 512 and 1023 put the +1 / +2 moves and the hand-over of
    the accumulators across the first state-tile border, T = 3 TB + 5 the scores and accumulators across three frame blocks;
    up to T = 3 TB + 5 the frames do not hold 511 tokens and more (early factors finite, the rest -inf in both) and no alignment
    reaches state TS, so T = 10 TB + 3, beyond the issue's list, is there for the second state tile to be computed and every
    total to be finite.  U = 0: the new kernel alone, against the sum of the blank column."""
    K = _need_gpu()
    TB, TS = K.ctc_viterbi_long_tile()
    assert 2 * 511 + 1 < TS < 2 * 512 + 1
    T = {"TB-1": TB - 1, "3TB+5": 3 * TB + 5, "10TB+3": 10 * TB + 3}[frames]
    V = 50
    rng = np.random.default_rng([13, U, T])
    y = targets_with_repeats(rng, U, V, BLANK)
    xd, x64 = _on_device(_peaked_lprobs(rng, T, V), DTYPES[dtype_name])
    yd = torch.from_numpy(y).to(DEV)
    logc, total, psi = K.ctc_prefix_posteriors_long(xd, yd, T, V, BLANK, want_psi=True)
    assert not bool(torch.isnan(logc).any() | torch.isnan(total).any() | torch.isnan(psi).any())
    if U == 0:
        want = np.float32(0)
        for t in range(T):  # (the kernel's order: frame by frame in fp32)
            want = np.float32(want + np.float32(x64[t, BLANK]))
        assert logc.shape == (1,) and psi.shape == (0,) and float(total[0]) == float(logc[0])
        assert abs(float(total[0]) - x64[:, BLANK].sum()) <= 8 * float(np.spacing(np.float32(abs(x64[:, BLANK].sum()))))
        assert float(total[0]) == float(want)
        return
    one = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)  # noqa: E731
    ologc, ototal, opsi = K.ctc_prefix_posteriors(xd, yd.view(1, U).contiguous(), one(0), one(T), one(U), 1, T, V, BLANK, want_psi=True)
    assert torch.equal(total.view(torch.int32), ototal.view(torch.int32)), (float(total[0]), float(ototal[0]))
    assert torch.equal(psi.view(torch.int32), opsi[0].view(torch.int32)), int((psi != opsi[0]).sum())
    assert torch.equal(logc.view(torch.int32), ologc[0].view(torch.int32)), int((logc != ologc[0]).sum())
    if T >= U + int((y[1:] == y[:-1]).sum()):
        assert bool(torch.isfinite(total).all()) and bool(torch.isfinite(logc).all())
    else:
        assert float(total[0]) == -np.inf and bool(torch.isfinite(logc[:8]).all()) and float(logc[-1]) == -np.inf


# ------------------------------------------------------------------------------------------------ conventions
def test_no_frames():
    K = _need_gpu()
    V = 6
    none = torch.zeros(0, V, dtype=torch.float32, device=DEV)
    logc, total, psi = _run(K, none, [], V)  # T = 0, U = 0: the empty sequence, probability 1
    assert total == 0.0 and list(logc) == [0.0] and psi.size == 0
    logc, total, psi = _run(K, none, [2, 3], V)  # T = 0, U = 2
    assert total == -np.inf and (logc == -np.inf).all() and logc.shape == (3,) and (psi == -np.inf).all()


def test_infeasible_transcripts_give_minus_infinity_never_nan():
    K = _need_gpu()
    TB, TS = K.ctc_viterbi_long_tile()
    rng = np.random.default_rng(3)
    V = 9
    for U in (5, TS // 2 + 3):
        y = (np.arange(U) % (V - 1) + 1).astype(np.int32)  # no equal neighbours
        for T, yy in ((U - 1, y), (U, np.concatenate([y[:2], y[1:U - 1]]).astype(np.int32))):  # too few frames; a repeat in U frames
            xd, x64 = _on_device(_peaked_lprobs(rng, T, V), torch.float32)
            ref = _reference(x64, yy)
            logc, total, psi = _run(K, xd, yy, V)
            assert total == -np.inf and logc[-1] == -np.inf and not np.isnan(logc).any() and not np.isnan(psi).any()
            assert np.isfinite(logc[:2]).all() and np.isfinite(psi[:2]).all()  # the early factors are finite
            first = int(np.nonzero(np.isneginf(logc))[0][0])
            assert np.isneginf(logc[first:]).all() and np.isfinite(logc[:first]).all()  # -inf from the first Psi = -inf on
            for got, key in ((psi, "psi"), (total, "total"), (logc, "logc")):
                _assert_within(got, ref[key], ref["bound"][key], key)
        xd, x64 = _on_device(_peaked_lprobs(rng, U, V), torch.float32)  # U tokens in exactly U frames: the one path
        logc, total, psi = _run(K, xd, y, V)
        want = sum(x64[t, y[t]] for t in range(U))
        assert np.isfinite(total) and abs(total - want) <= U * float(np.spacing(np.float32(abs(want))))  # (U adds, 1/2 ulp each)


def test_bad_targets_give_nan_everywhere():
    K = _need_gpu()
    TB, TS = K.ctc_viterbi_long_tile()
    rng = np.random.default_rng(5)
    V = 7
    U = TS // 2 + 40  # the bad id sits in the first or in the second state tile
    T = 2 * U
    xd, _ = _on_device(_peaked_lprobs(rng, T, V), torch.float32)
    good = (np.arange(U) % (V - 1) + 1).astype(np.int32)
    for bad_id in (V, -1, 10 ** 6, BLANK):
        for pos in (0, U - 1):
            y = good.copy()
            y[pos] = bad_id
            logc, total, psi = _run(K, xd, y, V)
            assert np.isnan(total) and np.isnan(logc).all() and np.isnan(psi).all(), (bad_id, pos)
    logc, total, psi = _run(K, xd, good, V)
    assert np.isfinite(total) and np.isfinite(logc).all() and np.isfinite(psi).all()
    logc, total, psi = _run(K, xd[:, : V - 1].contiguous(), np.minimum(good, V - 3), V - 1, blank=V - 2)  # another blank column
    assert np.isfinite(total) and np.isfinite(logc).all()
    logc, total, psi = _run(K, xd[:, : V - 1].contiguous(), np.minimum(good, V - 2), V - 1, blank=V - 2)  # ... which some targets name
    assert np.isnan(total) and np.isnan(logc).all()


def test_argument_refusals(monkeypatch):
    K = _need_gpu()
    from espresso_amd import _lib

    x = torch.zeros(20, 8, dtype=torch.float32, device=DEV)
    y = torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="ea_ctc_prefix_long_posteriors"):
        K.ctc_prefix_posteriors_long(x, y, 20, 8, 8)  # blank outside the vocabulary
    with pytest.raises(RuntimeError, match="ea_ctc_prefix_long_posteriors"):
        K.ctc_prefix_posteriors_long(x, y, 20, 8, -1)
    with pytest.raises(RuntimeError, match="ea_ctc_prefix_long_posteriors"):
        K.ctc_prefix_posteriors_long(x, y, 20, 8, 0, ld=7)  # ld < V
    lib = _lib.lib()
    for T, V, U in ((-1, 8, 2), (20, 8, -1), (20, 0, 2)):
        assert lib.ea_ctc_prefix_long_posteriors(None, 8, 0, None, None, None, None, None, T, V, U, 0, None) != 0
    # more workspace than the device has free: refused with the figures, nothing allocated
    need = int(lib.ea_ctc_prefix_long_workspace_bytes(20, 2))
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (need - 1, 1 << 40))
    with pytest.raises(ValueError) as e:
        K.ctc_prefix_posteriors_long(x, y, 20, 8, 0)
    msg = str(e.value)
    assert str(need) in msg and str(need - 1) in msg and "T = 20" in msg and "U = 2" in msg
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (need, 1 << 40))
    logc, total = K.ctc_prefix_posteriors_long(x, y, 20, 8, 0)
    assert logc.shape == (3,) and bool(torch.isfinite(total).all())


# ------------------------------------------------------------------------------------------------ the tiny model
WINDOW_S, OVERLAP_S = 1.6, 0.32  # 40 and 8 encoder frames of 40 ms
G = 640
POST_KEYS = {"token_posteriors", "end_posterior", "posterior_score"}


def _tiny(tmp_path):
    """(task with its front-end, model, checkpoint options of the command line) for the tiny CTC fixture model."""
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from tests.gpu_checks import build_tiny_model, load_fixture, load_ref_state

    _, sd, _, _ = load_fixture("ref_conformer_ctc_tiny")
    (tmp_path / "dict.txt").write_text("".join(f"t{i} 1\n" for i in range(35)) + "<space> 1\n")  # (the fixture's V = 40)
    block = {"_name": "speech_transformer_encoder_model", "dropout": 0.0, "layernorm_embedding": True,
             "encoder": {"embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4, "normalize_before": True,
                         "relative_positional_embeddings": True, "layer_type": "conformer", "conv_channels": "[64, 64, 16, 16]"}}
    (tmp_path / "cfg.json").write_text(json.dumps(block))
    torch.save({"model": {"encoder." + k: v for k, v in sd.items()}}, str(tmp_path / "m.pt"))
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(
        dict=str(tmp_path / "dict.txt"), autoregressive=False, criterion_name="ctc_loss"))
    task.build_frontend(torch.device(DEV))
    model = build_tiny_model("conformer").to(DEV).eval()
    load_ref_state(model, sd)
    base = ["--path", str(tmp_path / "m.pt"), "--model-config", str(tmp_path / "cfg.json"), "--dict", str(tmp_path / "dict.txt")]
    return task, model, base


def _wave(seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(16000 * seconds)
    env = 0.2 + np.abs(np.sin(np.arange(n) / 2100.0))  # louder and quieter stretches
    return np.round(rng.standard_normal(n) * 800 * env).astype(np.float32)


def _long_form(task, model):
    from espresso_amd.tools import long_form as LF

    plan = LF.LongFormPlan.from_seconds(LF.samples_per_frame(task.frontend, model), 16000, WINDOW_S, OVERLAP_S)
    assert (plan.g, plan.Tw, plan.Of, plan.Hf) == (G, 40, 8, 32)
    return LF, plan


def _bits(v):
    return np.asarray(v, dtype=np.float32).view(np.int32)


def test_three_windows_through_the_model(tmp_path):
    K = _need_gpu()
    from espresso_amd.tools.forced_aligner import LongFormCTCAligner

    task, model, _ = _tiny(tmp_path)
    LF, plan = _long_form(task, model)
    d = task.target_dictionary
    wave = _wave((2 * plan.H + 15000) / 16000.0, 6)
    assert len(plan.windows(len(wave))) == 3
    tokens = np.random.default_rng(8).integers(5, 40, size=40).tolist()
    aligner = LongFormCTCAligner(task, model, plan, d, token_posteriors=True)
    encode, seen = aligner.long_form.encode, []
    aligner.long_form.encode = lambda m, w: seen.append(encode(m, w)) or seen[-1]  # (the matrix the aligner itself saw)
    r = aligner.align(wave, tokens)
    (lprobs, in_len, cuts, scores), = seen
    T, V = lprobs.shape[1], lprobs.shape[2]
    tg = torch.tensor(tokens, dtype=torch.int32, device=DEV)
    logc, total = K.ctc_prefix_posteriors_long(lprobs[0], tg, T, V, d.bos())
    assert r["token_posteriors"].dtype == np.float32 and r["token_posteriors"].shape == (40,)
    assert np.array_equal(_bits(r["token_posteriors"]), _bits(logc[:40].cpu().numpy()))
    assert _bits(r["end_posterior"]) == _bits(logc[40].item()) and _bits(r["posterior_score"]) == _bits(total[0].item())
    assert np.isfinite(r["posterior_score"]) and np.isfinite(r["token_posteriors"]).all() and (r["token_posteriors"] <= 0).all()
    assert r["posterior_score"] >= r["score"]  # all alignments against the best one
    # the one-workgroup kernel takes 40 tokens too: the same bits on the same matrix
    one = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)  # noqa: E731
    ologc, ototal = K.ctc_prefix_posteriors(lprobs[0], tg.view(1, 40), one(0), one(T), one(40), 1, T, V, d.bos())
    assert torch.equal(logc.view(torch.int32), ologc[0].view(torch.int32)) and torch.equal(total.view(torch.int32), ototal.view(torch.int32))
    # every other key is what the aligner gives without the flag
    plain = LongFormCTCAligner(task, model, plan, d).align(wave, tokens)
    assert set(r) == set(plain) | POST_KEYS and not (set(plain) & POST_KEYS)
    for key, v in plain.items():
        got = r[key]
        if isinstance(v, np.ndarray):
            assert got.dtype == v.dtype and np.array_equal(got, v) and (v.dtype != np.float32 or np.array_equal(_bits(got), _bits(v))), key
        else:
            assert type(got) is type(v) and got == v, key


def test_one_window_through_the_model_equals_the_utterance_aligner(tmp_path):
    _need_gpu()
    from espresso_amd.speech_recognize import collate
    from espresso_amd.tools.forced_aligner import CTCForcedAligner, LongFormCTCAligner

    task, model, _ = _tiny(tmp_path)
    _, plan = _long_form(task, model)
    d = task.target_dictionary
    wave = _wave(1.1, 5)
    tokens = np.random.default_rng(9).integers(5, 40, size=9).tolist()
    r = LongFormCTCAligner(task, model, plan, d, token_posteriors=True).align(wave, tokens)
    s = task.prepare_sample(collate([0], ["0"], [wave], torch.device(DEV)), train=False)
    want = CTCForcedAligner([model], d, token_posteriors=True).align(s, [tokens])[0]
    assert r["feasible"] and want["feasible"] and np.isfinite(want["posterior_score"])
    assert np.array_equal(_bits(r["token_posteriors"]), _bits(want["token_posteriors"]))
    assert _bits(r["end_posterior"]) == _bits(want["end_posterior"]) and _bits(r["posterior_score"]) == _bits(want["posterior_score"])
    assert set(want) <= set(r)


# ------------------------------------------------------------------------------------------------ the command lines
LF_OPTS = ["--long-form", "--long-form-window-s", str(WINDOW_S), "--long-form-overlap-s", str(OVERLAP_S)]


def _write_scp(tmp_path, waves):
    from espresso_amd.data import audio_utils

    scp = []
    for u, w in waves.items():
        audio_utils.write_wav(str(tmp_path / f"{u}.wav"), w)
        scp.append(f"{u} {tmp_path / (u + '.wav')}\n")
    (tmp_path / "wav.scp").write_text("".join(scp))
    return ["--wav-scp", str(tmp_path / "wav.scp")]


def test_cli_align_writes_probabilities_and_the_confidence_file(tmp_path, capsys):
    _need_gpu()
    from espresso_amd import speech_align

    task, model, base = _tiny(tmp_path)
    _, plan = _long_form(task, model)
    rng = np.random.default_rng(10)
    waves = {"long": _wave((2 * plan.H + 15000) / 16000.0, 6), "short": _wave(1.2, 7)}
    texts = {}
    for u, n_words in (("long", 16), ("short", 3)):
        words = [" ".join(f"t{k}" for k in rng.integers(1, 35, size=int(rng.integers(2, 4)))) for _ in range(n_words)]
        texts[u] = " <space> ".join(words)
    (tmp_path / "text").write_text("".join(f"{u} {t}\n" for u, t in texts.items()))
    common = base + _write_scp(tmp_path, waves) + ["--text", str(tmp_path / "text"), "--unit", "word"] + LF_OPTS + \
        ["--segment-max-s", "0.8", "--segment-min-silence-s", "0.04"]
    res = {}
    for tag, extra in (("plain", []), ("post", ["--long-form-posteriors"])):
        res[tag] = speech_align.main(common + ["--output", str(tmp_path / f"{tag}.ctm"), "--scores", str(tmp_path / f"{tag}.scores"),
                                               "--segments-dir", str(tmp_path / tag)] + extra)
    capsys.readouterr()
    for name in ("segments", "text", "scores"):  # byte for byte what the run without the option writes
        assert (tmp_path / "post" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
    assert (tmp_path / "post.scores").read_bytes() == (tmp_path / "plain.scores").read_bytes()
    assert not (tmp_path / "plain" / "confidence").exists()
    plain = [l.split() for l in (tmp_path / "plain.ctm").read_text().splitlines()]
    post = [l.split() for l in (tmp_path / "post.ctm").read_text().splitlines()]
    assert [l[:5] for l in post] == [l[:5] for l in plain] and all(l[5] == "1.00" for l in plain)
    assert all(0.0 <= float(l[5]) <= 1.0 for l in post) and any(l[5] != "1.00" for l in post)
    seg = [l.split() for l in (tmp_path / "post" / "segments").read_text().splitlines()]
    conf = [l.split() for l in (tmp_path / "post" / "confidence").read_text().splitlines()]
    txt = [l.split() for l in (tmp_path / "post" / "text").read_text().splitlines()]
    assert [l[0] for l in conf] == [l[0] for l in seg] and len(seg) >= 3
    for c, t in zip(conf, txt):
        assert len(c) == 4 and int(c[3]) == len(t) - 1 >= 1 and float(c[1]) <= 0.0 and 0.0 <= float(c[2]) <= 1.0
    for u in waves:  # one factor per token of the transcript, <space> included
        r = res["post"][u]
        assert POST_KEYS <= set(r) and not (POST_KEYS & set(res["plain"][u]))
        assert len(r["token_posteriors"]) == len(texts[u].split())


def test_cli_recognize_prints_a_confidence_line_per_hypothesis(tmp_path, capsys):
    _need_gpu()
    from espresso_amd import speech_recognize

    task, model, base = _tiny(tmp_path)
    _, plan = _long_form(task, model)
    waves = {"rec": _wave((2 * plan.H + 15000) / 16000.0, 6), "short": _wave(1.2, 7)}
    common = base + _write_scp(tmp_path, waves)
    base = common + ["--search", "ctc_beam", "--beam", "4", "--nbest", "2"] + LF_OPTS
    capsys.readouterr()
    speech_recognize.main(base)
    plain = capsys.readouterr().out.splitlines()
    speech_recognize.main(base + ["--long-form-posteriors"])
    post = capsys.readouterr().out.splitlines()
    hyp = [l for l in plain if l.startswith("H-")]
    assert len(hyp) >= 3 and not any(l.startswith("C-") for l in plain)
    assert [l for l in post if l.startswith("H-")] == hyp  # tokens, scores and order are the search's
    assert [l for l in post if not l.startswith("C-") and not l.startswith("Recognized")] == \
        [l for l in plain if not l.startswith("Recognized")]
    for k, line in enumerate(post):
        if line.startswith("H-"):  # its C- line follows: one probability per token of the text, then that of ending there
            utt, text = line[2:].split("\t")[:2]
            nxt = post[k + 1]
            assert nxt.startswith(f"C-{utt}\t"), (line, nxt)
            probs = [float(v) for v in nxt.split("\t")[1].split()]
            assert len(probs) == len(text.split()) + 1 and all(0.0 <= p <= 1.0 for p in probs)
    assert sum(l.startswith("C-") for l in post) == len(hyp)
    # the greedy search takes the option too
    speech_recognize.main(common + ["--search", "ctc"] + LF_OPTS + ["--long-form-posteriors"])
    out = capsys.readouterr().out.splitlines()
    assert sum(l.startswith("H-") for l in out) == sum(l.startswith("C-") for l in out) == 2
