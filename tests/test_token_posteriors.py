"""Per-token posteriors of CTC and transducer hypotheses (csrc/prefix_posterior.hip, tools/token_posteriors.py, --confidence).

CPU: the float64 oracles (tests/prefix_posterior_ref.py) against brute-force enumeration, the identities (factors <= 0, they add
up to log P(y | x) = -ctc_loss), the edge cases, and the host logic (argument checks, CTM confidences, the C- line).
GPU (-m gpu): both kernels against the oracles reading the same inputs, one mid-size case each with a measured bound, every
offline decoder with token_posteriors=True on the fixture models, and the two command-line tools.

Mid-size cases (T = 200, U = 60), largest |kernel - float64 oracle| on a Psi or the total, measured on the MI355X: CTC 2.185e-4
(total -598.1, ulp 6.1e-5), transducer 1.451e-5 (total -80.6, ulp 7.6e-6); MID_CTC_MEASURED / MID_RNNT_MEASURED hold them rounded
up, the tests assert 8x."""
import itertools
import os

import numpy as np
import pytest
import torch

from tests.prefix_posterior_ref import (ctc_brute_sequences, ctc_prefix_oracle, factors, prefix_mass, rnnt_brute_sequence,
                                        rnnt_lattice_of, rnnt_prefix_oracle)

DEV = "cuda:0"
SCORE_TOL = 1e-4  # tests/test_ctc_prefix_beam.py: the project's fp32-vs-float64 bound at these sizes
# largest |kernel - float64 oracle| over every Psi and total of the mid-size cases, measured on the MI355X; the tests assert 8x
# (the headroom of the project's measured bounds, LM_TOL) and that 8x stays below 3 * (T + U + 2) * ulp(|total|)
MID_CTC_MEASURED = 2.2e-4
MID_RNNT_MEASURED = 1.5e-5


def _lse(z, axis=-1):
    return np.logaddexp.reduce(z, axis=axis, keepdims=True)


def _peaked(rng, T, V, sharp=4.0, scale=1.0):
    """Log-softmax rows with one clearly preferred token per frame (blank half of the time), like a trained CTC model."""
    z = scale * rng.standard_normal((T, V))
    z[np.arange(T), np.where(rng.random(T) < 0.5, 0, rng.integers(1, V, T))] += sharp
    return z - _lse(z)


# ------------------------------------------------------------------------------------------------ oracles vs brute force
@pytest.mark.parametrize("T", [1, 2, 4, 5])
def test_ctc_oracle_vs_brute_force(T):
    rng = np.random.default_rng(T)
    V, blank = 3, 0
    for trial in range(3):
        x = np.log(rng.dirichlet(np.ones(V), size=T))
        probs = ctc_brute_sequences(x, T, blank)
        assert abs(sum(probs.values()) - 1.0) < 1e-12
        assert len(probs) > 1 and () in probs
        for y, p in probs.items():  # every reachable label sequence, every one of its prefixes
            psi, total = ctc_prefix_oracle(x, T, list(y), blank)
            assert abs(np.exp(total) - p) < 1e-12, (y, total, p)
            for i in range(len(y)):
                assert abs(np.exp(psi[i]) - prefix_mass(probs, y[: i + 1])) < 1e-12, (y, i)
                assert abs(psi[i] - np.log(prefix_mass(probs, y[: i + 1]))) < 1e-12, (y, i)
        # an unreachable sequence (a repeat needs a blank between: 2T - 1 > T frames for T >= 2)
        if T >= 2:
            y = [1] * T
            assert y and tuple(y) not in probs
            psi, total = ctc_prefix_oracle(x, T, y, blank)
            assert total == -np.inf and psi[-1] == -np.inf and psi[0] > -np.inf


def test_rnnt_oracle_vs_brute_force():
    from tests.transducer_frame_beam_ref import TableModel

    T, V, blank, max_len = 3, 3, 0, 9
    table = TableModel(V, seed=3, blank=blank, sharp=3.0, scale=1.0)

    def logp(t, prefix):  # (blank raised: the mass of long label sequences, the enumeration's tail, must be small)
        z = table.row(0, t, prefix).astype(np.float64)
        z[blank] += 4.5
        return z - _lse(z)[0]

    seqs = {}
    for n in range(max_len + 1):
        for y in itertools.product((1, 2), repeat=n):
            seqs[y] = rnnt_brute_sequence(logp, T, y, blank)
    tail = 1.0 - sum(seqs.values())  # the mass of the label sequences longer than the enumeration
    assert 0.0 <= tail < 2e-3, tail
    checked = 0
    for y in itertools.chain.from_iterable(itertools.product((1, 2), repeat=n) for n in range(5)):
        lpb, lpy = rnnt_lattice_of(logp, T, y, blank)
        psi, total = rnnt_prefix_oracle(lpb, lpy, T, len(y))
        assert abs(np.exp(total) - seqs[y]) < 1e-12
        for i in range(len(y)):
            enum = prefix_mass(seqs, y[: i + 1])
            got = float(np.exp(psi[i]))
            assert enum - 1e-12 <= got <= enum + tail + 1e-12, (y, i, got, enum, tail)
            checked += 1
    assert checked > 50


# ------------------------------------------------------------------------------------------------ identities, edge cases
def test_ctc_identities_on_random_inputs():
    rng = np.random.default_rng(0)
    for T, U, V in [(12, 3, 6), (30, 8, 9), (9, 0, 4), (1, 1, 5), (40, 13, 20)]:
        x = np.log(rng.dirichlet(np.ones(V), size=T))
        y = list(rng.integers(1, V, size=U))
        if U >= 3:
            y[2] = y[1]  # a repeat
        psi, total = ctc_prefix_oracle(x, T, y, 0)
        logc, score = factors(psi, total)
        assert (logc <= 0).all() and logc.shape == (U + 1,)
        assert logc.sum() == pytest.approx(score, abs=1e-10)
        assert (np.diff(np.concatenate([[0.0], psi, [total]])) <= 1e-12).all()  # a longer prefix is never more likely
        ref = -torch.nn.functional.ctc_loss(torch.from_numpy(x).unsqueeze(1), torch.tensor([y], dtype=torch.long).reshape(1, U),
                                            torch.tensor([T]), torch.tensor([U]), blank=0, reduction="none")
        assert score == pytest.approx(float(ref[0]), abs=1e-9)


def test_rnnt_identities_on_random_inputs():
    rng = np.random.default_rng(1)
    for T, U in [(1, 0), (1, 2), (7, 3), (13, 5)]:
        p = rng.uniform(0.05, 0.95, size=(T, U + 1))
        lpb, lpy = np.log(p), np.log1p(-p) + np.log(rng.uniform(0.1, 1.0, size=(T, U + 1)))
        psi, total = rnnt_prefix_oracle(lpb, lpy, T, U)
        logc, score = factors(psi, total)
        assert (logc <= 0).all() and logc.sum() == pytest.approx(score, abs=1e-10)
        beta = np.full((T + 1, U + 2), -np.inf)  # the backward sweep: an independent value of log P(y | x)
        for t in range(T - 1, -1, -1):
            for u in range(U, -1, -1):
                blk = lpb[t, u] if (t == T - 1 and u == U) else lpb[t, u] + beta[t + 1, u]
                beta[t, u] = np.logaddexp(blk, lpy[t, u] + beta[t, u + 1] if u < U else -np.inf)
        assert score == pytest.approx(beta[0, 0], abs=1e-10)
    assert rnnt_prefix_oracle(lpb, lpy, 0, 2)[1] == -np.inf


def test_ctc_edge_cases():
    x = np.log(np.full((3, 4), 0.25))
    psi, total = ctc_prefix_oracle(x, 3, [1, 1], 0)  # "a a": 1 blank 1 is the only alignment
    assert total == pytest.approx(3 * np.log(0.25)) and psi[1] == pytest.approx(3 * np.log(0.25))
    assert psi[0] == pytest.approx(np.log(0.25 + 0.25 ** 2 + 0.25 ** 3))  # token 1 starts at frame 0, 1 or 2, after blanks
    psi, total = ctc_prefix_oracle(x, 2, [1, 1], 0)  # infeasible: -inf without NaN, from the first impossible prefix on
    logc, score = factors(psi, total)
    assert score == -np.inf and logc[0] > -np.inf and logc[1] == -np.inf and logc[2] == -np.inf and not np.isnan(logc).any()
    psi, total = ctc_prefix_oracle(x, 3, [], 0)  # U = 0: one factor, the all-blank path
    logc, score = factors(psi, total)
    assert psi.shape == (0,) and logc.shape == (1,) and logc[0] == pytest.approx(3 * np.log(0.25)) == score
    psi, total = ctc_prefix_oracle(x, 1, [2], 0)  # T = 1
    assert psi[0] == pytest.approx(np.log(0.25)) and total == pytest.approx(np.log(0.25))
    assert ctc_prefix_oracle(x, 0, [], 0)[1] == 0.0 and ctc_prefix_oracle(x, 0, [1], 0)[1] == -np.inf
    z = x.copy()
    z[:, 2] = -np.inf  # zero probability
    logc, score = factors(*ctc_prefix_oracle(z, 3, [1, 2], 0))
    assert score == -np.inf and logc[0] > -np.inf and logc[1] == -np.inf and not np.isnan(logc).any()


# ------------------------------------------------------------------------------------------------ GPU: the kernels
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


def _check_rows(logc, total, psi, refs, tol, what):
    """Kernel rows (numpy) against [(psi, total)] float64 references: Psi and total within tol, factors within 2 tol, -inf exactly,
    positions past U zero.  Returns the largest finite error on a Psi or total."""
    worst = 0.0
    for n, (rpsi, rtot) in enumerate(refs):
        U = len(rpsi)
        rc, _ = factors(rpsi, rtot)
        for got, ref, t in [(psi[n, :U], rpsi, tol), (total[n: n + 1], np.array([rtot]), tol), (logc[n, : U + 1], rc, 2 * tol)]:
            assert not np.isnan(got).any(), (what, n)
            inf = ref == -np.inf
            assert (got[inf] == -np.inf).all() and np.isfinite(got[~inf]).all(), (what, n, got, ref)
            if (~inf).any():
                err = float(np.abs(got[~inf] - ref[~inf]).max())
                assert err <= t, (what, n, err, t)
                if t == tol:
                    worst = max(worst, err)
        assert (logc[n, : U + 1] <= 0).all() and (logc[n, U + 1:] == 0).all() and (psi[n, U:] == 0).all(), (what, n)
    return worst


CTC_US = (0, 1, 8, 9, 16, 17)  # a thread owns 8 tokens (16 states): either side of the first two ownership boundaries


def _ctc_hyps(rng, V, in_len):
    """Hypotheses for a batch: every U of CTC_US for every utterance, with repeated adjacent labels; many are infeasible."""
    Lmax = max(CTC_US)
    tg, tl, utt = [], [], []
    for b in range(len(in_len)):
        for U in CTC_US:
            y = rng.integers(1, V, size=U)
            for u in range(1, U):
                if rng.random() < 0.25:
                    y[u] = y[u - 1]
            tg.append(np.concatenate([y, np.zeros(Lmax - U, dtype=np.int64)]))
            tl.append(U)
            utt.append(b)
    return np.array(tg, dtype=np.int32), np.array(tl, dtype=np.int32), np.array(utt, dtype=np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,ld", [(20, 20), (20, 32), (5004, 5056)])
def test_ctc_kernel_vs_oracle(V, ld, dtype):
    _need_gpu()
    from espresso_amd import kernels as K

    rng = np.random.default_rng(V + ld)
    for T in (1, 3, 4, 5, 14):  # either side of the 4-frame prefetch
        in_len = np.array(sorted({0, 1, max(T - 2, 1), T}), dtype=np.int32)
        B = len(in_len)
        x = _peaked(rng, B * T, V, sharp=4.0, scale=2.0).astype(np.float32)
        wide = torch.full((B * T, ld), float("nan"))
        wide[:, :V] = torch.from_numpy(x)
        xd = wide.to(DEV, dtype)[:, :V]
        x_seen = xd.float().cpu().numpy().astype(np.float64).reshape(B, T, V)  # what the kernel reads (bf16-rounded for bf16)
        tg, tl, utt = _ctc_hyps(rng, V, in_len)
        logc, total, psi = K.ctc_prefix_posteriors(xd, torch.from_numpy(tg).to(DEV), torch.from_numpy(utt).to(DEV),
                                                   torch.from_numpy(in_len).to(DEV), torch.from_numpy(tl).to(DEV), B, T, V, 0,
                                                   ld=ld, want_psi=True)
        refs = [ctc_prefix_oracle(x_seen[utt[n]], int(in_len[utt[n]]), list(tg[n, : tl[n]]), 0) for n in range(len(tl))]
        feasible = sum(r[1] > -np.inf for r in refs)
        assert (feasible >= 3 or T == 1) and feasible < len(refs)
        worst = _check_rows(logc.cpu().numpy(), total.cpu().numpy(), psi.cpu().numpy(), refs, SCORE_TOL, (T, V, ld))
        print(f"ctc V {V} ld {ld} T {T} {dtype}: {feasible}/{len(refs)} feasible, max |Psi - oracle| {worst:.2e}")


@pytest.mark.gpu
def test_ctc_kernel_shared_utterance_bad_ids_and_refusals():
    _need_gpu()
    from espresso_amd import kernels as K

    rng = np.random.default_rng(5)
    B, T, V = 2, 12, 7
    x = _peaked(rng, B * T, V).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    in_len = torch.tensor([12, 9], dtype=torch.int32, device=DEV)
    #           three hypotheses of utterance 1 (an n-best list), one of utterance 0, then: id 9 >= V, blank as a target, bad row
    tg = torch.tensor([[1, 2, 3], [1, 2, 0], [4, 4, 5], [1, 2, 3], [1, 9, 3], [0, 0, 0], [1, 2, 3]], dtype=torch.int32, device=DEV)
    tl = torch.tensor([3, 2, 3, 3, 3, 1, 3], dtype=torch.int32, device=DEV)
    utt = torch.tensor([1, 1, 1, 0, 0, 1, 2], dtype=torch.int32, device=DEV)
    logc, total, psi = (t.cpu().numpy() for t in K.ctc_prefix_posteriors(xd, tg, utt, in_len, tl, B, T, V, 0, want_psi=True))
    x64 = x.astype(np.float64).reshape(B, T, V)
    lens = [12, 9]
    refs = [ctc_prefix_oracle(x64[int(utt[n])], lens[int(utt[n])], tg[n, : int(tl[n])].tolist(), 0) for n in range(4)]
    _check_rows(logc[:4], total[:4], psi[:4], refs, SCORE_TOL, "shared")
    assert psi[0, 1] == psi[1, 1] and psi[0, 0] == psi[1, 0]  # a shared prefix has one Psi
    assert total[0] != total[3]  # the same tokens under another utterance's log-probs
    for n in (4, 5, 6):
        assert np.isnan(total[n]) and np.isnan(logc[n]).all() and np.isnan(psi[n]).all()
    assert abs(logc[0].sum() - total[0]) < 4 * SCORE_TOL
    with pytest.raises(RuntimeError):
        K.ctc_prefix_posteriors(xd, torch.zeros(1, 1024, dtype=torch.int32, device=DEV), utt[:1], in_len, tl[:1], B, T, V, 0)
    with pytest.raises(RuntimeError):
        K.ctc_prefix_posteriors(xd, tg, utt, in_len, tl, B, T, V, V)  # blank outside [0, V)
    K.ctc_prefix_posteriors(xd, torch.zeros(1, 1023, dtype=torch.int32, device=DEV), utt[:1], in_len, tl[:1] * 0, B, T, V, 0)


RNNT_US = (0, 1, 5, 63, 64, 65)  # one lane per u: either side of the wave boundary


def _rnnt_lattice(rng, B, T, U1):
    p = rng.uniform(0.05, 0.95, size=(B, T, U1))
    lpb = np.log(p).astype(np.float32)
    lpy = (np.log1p(-p) + np.log(rng.uniform(0.2, 1.0, size=(B, T, U1)))).astype(np.float32)
    return lpb, lpy


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2, 7, 13])
def test_rnnt_kernel_vs_oracle(T):
    _need_gpu()
    from espresso_amd import _lib
    from espresso_amd import kernels as K
    from espresso_amd.kernels import _p, _stream

    rng = np.random.default_rng(T)
    for Umax in RNNT_US:
        U1 = Umax + 1
        # rows: the full lattice, T_b < T, U_b < U1 - 1, T_b = 0
        Tl = np.array([T, max(T - 1, 1), T, 0], dtype=np.int32)
        Ul = np.array([Umax, Umax, Umax // 2, Umax], dtype=np.int32)
        B = len(Tl)
        lpb, lpy = _rnnt_lattice(rng, B, T, U1)
        dl = [torch.from_numpy(a).to(DEV) for a in (lpb, lpy, Tl, Ul)]
        logc, total, psi = (t.cpu().numpy() for t in K.rnnt_prefix_posteriors(*dl, want_psi=True))
        refs = [rnnt_prefix_oracle(lpb[b].astype(np.float64), lpy[b].astype(np.float64), int(Tl[b]), int(Ul[b])) for b in range(B)]
        worst = _check_rows(logc, total, psi, refs, SCORE_TOL, (T, Umax))
        assert total[3] == -np.inf and (logc[3, : Umax + 1] == -np.inf).all()
        alpha, beta = torch.empty_like(dl[0]), torch.empty_like(dl[0])
        loss = torch.empty(B, dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib().ea_rnnt_scan(_p(dl[0]), _p(dl[1]), _p(dl[2]), _p(dl[3]), _p(alpha), _p(beta), _p(loss), B, T, U1,
                                           _stream()), "ea_rnnt_scan")
        assert np.abs(total[:3] + loss.cpu().numpy()[:3]).max() <= SCORE_TOL  # total = -loss of the same lattice
        print(f"rnnt T {T} U {Umax}: max |Psi - oracle| {worst:.2e}")
    with pytest.raises(RuntimeError):
        z = torch.zeros(1, 1, 1025, device=DEV)
        K.rnnt_prefix_posteriors(z, z, dl[2][:1], dl[3][:1])


def _mid_bound(measured, T, U, total):
    bound = 8 * measured
    derived = 3 * (T + U + 2) * float(np.spacing(np.float32(abs(total))))
    assert bound < derived, (bound, derived)
    return bound


@pytest.mark.gpu
def test_ctc_kernel_mid_size():
    """T = 200, U = 60: 1e-4 is not derivable here (fp32 log-domain sums lose about one ulp of |alpha| per step).  The bound is
    8x the error measured on the MI355X (MID_CTC_MEASURED), and must itself stay below the derived worst case."""
    _need_gpu()
    from espresso_amd import kernels as K

    rng = np.random.default_rng(200)
    T, U, V = 200, 60, 50
    x = _peaked(rng, T, V, sharp=4.0, scale=2.0).astype(np.float32)
    y = rng.integers(1, V, size=U)
    y[10] = y[9]
    tg = torch.from_numpy(y.astype(np.int32)).reshape(1, U).to(DEV)
    one = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)  # noqa: E731
    logc, total, psi = (t.cpu().numpy() for t in K.ctc_prefix_posteriors(torch.from_numpy(x).to(DEV), tg, one(0), one(T), one(U), 1,
                                                                         T, V, 0, want_psi=True))
    rpsi, rtot = ctc_prefix_oracle(x.astype(np.float64), T, list(y), 0)
    err = max(float(np.abs(psi[0] - rpsi).max()), abs(float(total[0]) - rtot))
    print(f"ctc mid-size: total {rtot:.3f}, max |Psi - oracle| {err:.3e}, ulp {np.spacing(np.float32(abs(rtot))):.3e}")
    bound = _mid_bound(MID_CTC_MEASURED, T, U, rtot)
    assert np.isfinite(rtot) and err <= bound, (err, bound)
    assert np.abs(logc[0] - factors(rpsi, rtot)[0]).max() <= 2 * bound


@pytest.mark.gpu
def test_rnnt_kernel_mid_size():
    """As test_ctc_kernel_mid_size for the transducer kernel (MID_RNNT_MEASURED)."""
    _need_gpu()
    from espresso_amd import kernels as K

    rng = np.random.default_rng(201)
    T, U = 200, 60
    lpb, lpy = _rnnt_lattice(rng, 1, T, U + 1)
    one = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)  # noqa: E731
    logc, total, psi = (t.cpu().numpy() for t in K.rnnt_prefix_posteriors(torch.from_numpy(lpb).to(DEV), torch.from_numpy(lpy).to(DEV),
                                                                          one(T), one(U), want_psi=True))
    rpsi, rtot = rnnt_prefix_oracle(lpb[0].astype(np.float64), lpy[0].astype(np.float64), T, U)
    err = max(float(np.abs(psi[0] - rpsi).max()), abs(float(total[0]) - rtot))
    print(f"rnnt mid-size: total {rtot:.3f}, max |Psi - oracle| {err:.3e}, ulp {np.spacing(np.float32(abs(rtot))):.3e}")
    bound = _mid_bound(MID_RNNT_MEASURED, T, U, rtot)
    assert np.isfinite(rtot) and err <= bound, (err, bound)
    assert np.abs(logc[0] - factors(rpsi, rtot)[0]).max() <= 2 * bound


# ------------------------------------------------------------------------------------------------ host logic
def _args(extra):
    from espresso_amd import speech_recognize as sr

    return sr.get_parser().parse_args(["--path", "m.pt", "--dict", "d.txt", "--wav-scp", "w.scp"] + extra)


@pytest.mark.parametrize("extra", [["--search", "ctc"], ["--search", "ctc_beam"], ["--search", "ctc_beam", "--lm-path", "lm.pt"],
                                   ["--search", "ctc_beam", "--token-ngram-lm", "a.arpa"], ["--search", "ctc_beam", "--hotwords", "h.txt"],
                                   ["--search", "transducer_greedy"], ["--search", "transducer_beam"],
                                   ["--search", "transducer_frame_beam"]])
def test_check_confidence_args_accepts(extra):
    from espresso_amd import speech_recognize as sr

    sr.check_confidence_args(_args(extra + ["--confidence"]))
    sr.check_confidence_args(_args(extra))


@pytest.mark.parametrize("extra,word", [(["--search", "beam"], "--search beam"), ([], "--search beam"),
                                        (["--search", "ctc_beam", "--ngram-lm", "a.arpa"], "--ngram-lm"),
                                        (["--search", "ctc", "--streaming"], "streamed"),
                                        (["--search", "transducer_greedy", "--streaming"], "streamed"),
                                        (["--search", "ctc_beam", "--ngram-lm", "a.arpa", "--streaming"], "streamed"),
                                        (["--search", "ctc_stream_beam", "--streaming"], "streamed"),
                                        (["--search", "transducer_stream_beam", "--streaming"], "streamed"),
                                        (["--search", "ctc", "--path", os.pathsep.join(["a.pt", "b.pt"])], "ensembles")])
def test_check_confidence_args_refuses_by_name_before_loading(extra, word, tmp_path):
    from espresso_amd import speech_recognize as sr

    with pytest.raises(NotImplementedError, match=word):
        sr.check_confidence_args(_args(extra + ["--confidence"]))
    if "--streaming" not in extra and "--ngram-lm" not in extra:  # main refuses before it opens the (missing) checkpoint
        with pytest.raises(NotImplementedError, match=word):
            sr.main(["--path", str(tmp_path / "missing.pt"), "--dict", "d.txt", "--wav-scp", "w.scp", "--confidence"] + extra)
    args = _args(["--search", "transducer_beam", "--confidence"])
    args.model_predicts_eos = True
    with pytest.raises(NotImplementedError, match="eos"):
        sr.check_confidence_args(args)


def test_transducer_decoders_refuse_posteriors_with_model_predicts_eos():
    from espresso_amd.data.asr_dictionary import AsrDictionary
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder

    d = AsrDictionary.from_symbols([f"t{i}" for i in range(8)], enable_bos=True)
    with pytest.raises(NotImplementedError, match="model_predicts_eos"):
        TransducerFrameBeamDecoder([None], d, token_posteriors=True, model_predicts_eos=True)
    assert TransducerFrameBeamDecoder([None], d).posteriors is None


def _dict(tmp_path, symbols):
    from espresso_amd.data.asr_dictionary import AsrDictionary

    p = tmp_path / "dict.txt"
    p.write_text("".join(f"{s} 1\n" for s in symbols))
    return AsrDictionary.load(str(p), enable_bos=True)


def test_ctm_confidences_character_dictionary(tmp_path):
    from espresso_amd import speech_recognize as sr

    d = _dict(tmp_path, list("abc") + ["<space>"])
    a, b, c, sp = (d.index(s) for s in ("a", "b", "c", "<space>"))
    p = [0.9, 0.5, 0.25, 0.8, 0.123]
    hypo = {"tokens": torch.tensor([a, b, sp, d.eos(), c]), "times": torch.tensor([2, 4, 6, 7, 9]),
            "token_posteriors": torch.tensor(np.log(p), dtype=torch.float32)}
    strip = {d.eos(), d.pad()}
    assert sr.hypothesis_ctm_lines("u1", hypo, d, strip, "token", 0.04) == [
        "u1 1 0.080 0.040 a 0.90", "u1 1 0.160 0.040 b 0.50", "u1 1 0.240 0.040 <space> 0.25", "u1 1 0.360 0.040 c 0.12"]
    # a word: the product over its own tokens; <space> and the stripped symbol contribute to no word
    assert sr.hypothesis_ctm_lines("u1", hypo, d, strip, "word", 0.04) == ["u1 1 0.080 0.120 ab 0.45", "u1 1 0.360 0.040 c 0.12"]
    del hypo["token_posteriors"]  # without --confidence: the column stays 1.00
    assert sr.hypothesis_ctm_lines("u1", hypo, d, strip, "word", 0.04) == ["u1 1 0.080 0.120 ab 1.00", "u1 1 0.360 0.040 c 1.00"]


def test_ctm_confidences_sentencepiece_dictionary(tmp_path):
    from espresso_amd.tools.forced_aligner import ctm_lines, utterance_units
    from espresso_amd.tools.token_posteriors import unit_confidences

    syms = ["▁he", "llo", "▁wor", "ld", "▁", "x"]
    d = _dict(tmp_path, syms)
    p = [0.5, 0.5, 0.9, 0.8, 0.5, 0.4]
    r = {"tokens": np.array([d.index(s) for s in syms]), "start": np.array([1, 3, 6, 8, 11, 12]), "end": np.array([2, 4, 7, 10, 12, 13])}
    conf = unit_confidences(syms, np.log(p), "word")
    assert conf == pytest.approx([0.25, 0.72, 0.2])  # the mark belongs to its piece
    assert ctm_lines("u", utterance_units(r, d, "word"), 0.04, confidences=conf) == [
        "u 1 0.040 0.120 hello 0.25", "u 1 0.240 0.160 world 0.72", "u 1 0.440 0.080 x 0.20"]
    assert unit_confidences(syms, np.log(p), "token") == pytest.approx(p)
    with pytest.raises(AssertionError):
        ctm_lines("u", utterance_units(r, d, "word"), 0.04, confidences=conf[:2])


def test_confidence_line_format():
    from espresso_amd.tools.token_posteriors import confidence_line

    assert confidence_line("utt-1", np.log([0.5, 0.98765, 1.0]), float(np.log(0.25))) == "C-utt-1\t0.5000 0.9877 1.0000 0.2500"
    assert confidence_line("u", [], 0.0) == "C-u\t1.0000"
    assert confidence_line("u", [-np.inf], -np.inf) == "C-u\t0.0000 0.0000"


def test_compact_and_spread_rows_on_the_host():
    from espresso_amd.tools.token_posteriors import MAX_LABELS, compact_labels, nbest_rows, spread_factors

    tokens = torch.tensor([[0, 5, 0, 6, 7, 1], [4, 4, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]])
    labels, n, pos = compact_labels(tokens, torch.tensor([6, 2, 6]), (0, 1))
    assert labels.tolist() == [[5, 6, 7, 0, 0, 0], [4, 4, 0, 0, 0, 0], [0] * 6] and n.tolist() == [3, 2, 0]
    logc = torch.tensor([[-1.0, -2.0, -3.0, -4.0, 0, 0, 0], [-0.5, -0.25, -0.125, 0, 0, 0, 0], [-7.0, 0, 0, 0, 0, 0, 0]])
    tok, end, total = spread_factors(logc, torch.tensor([-10.0, -0.875, -7.0]), n, pos, 6)
    assert tok.tolist() == [[0, -1.0, 0, -2.0, -3.0, 0], [-0.5, -0.25, 0, 0, 0, 0], [0] * 6]
    assert end.tolist() == [-4.0, -0.125, -7.0] and total.tolist() == [-10.0, -0.875, -7.0]
    ln, utt = nbest_rows(torch.tensor([[3, 9], [2, 2]], dtype=torch.int32), torch.tensor([1, 2], dtype=torch.int32))
    assert ln.tolist() == [3, 0, 2, 2] and utt.tolist() == [0, 0, 1, 1]
    assert MAX_LABELS == 1023


# ------------------------------------------------------------------------------------------------ GPU: through the models
def _hyp_key(h):
    return (h["tokens"].tolist(), float(h["score"]), None if "times" not in h else h["times"].tolist(),
            None if "viterbi_score" not in h else float(h["viterbi_score"]))


def _same_search(on, off):
    """Tokens, scores (and times) of the hypotheses with posteriors are those of the search without, bit for bit."""
    assert len(on) == len(off)
    for a, b in zip(on, off):
        assert len(a) == len(b) and len(a) >= 1
        for x, y in zip(a, b):
            assert torch.equal(x["tokens"].cpu(), y["tokens"].cpu()) and torch.equal(x["score"].cpu(), y["score"].cpu())
            assert _hyp_key(x) == _hyp_key(y)
            assert "token_posteriors" not in y and x["token_posteriors"].shape == x["tokens"].shape


def _check_hyp(h, rpsi, rtot, labels_at, what):
    """One hypothesis' keys against the float64 (psi, total) of its label sequence; labels_at: their positions in tokens."""
    rc, _ = factors(rpsi, rtot)
    tok = h["token_posteriors"].cpu().numpy().astype(np.float64)
    assert np.isfinite(rtot), what
    assert np.abs(tok[labels_at] - rc[:-1]).max(initial=0.0) <= 2 * SCORE_TOL, (what, tok, rc)
    rest = np.ones(len(tok), dtype=bool)
    rest[labels_at] = False
    assert (tok[rest] == 0).all() and (tok <= 0).all()
    assert abs(float(h["end_posterior"]) - rc[-1]) <= 2 * SCORE_TOL and abs(float(h["posterior_score"]) - rtot) <= SCORE_TOL, what
    ulp = float(np.spacing(np.float32(abs(rtot) + 1.0)))
    assert abs(tok.sum() + float(h["end_posterior"]) - float(h["posterior_score"])) <= (len(tok) + 2) * ulp, what


@pytest.mark.gpu
def test_ctc_decoders_with_token_posteriors():
    _need_gpu()
    from espresso_amd.tools.ctc_decoder import CTCDecoder
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder
    from tests.gpu_checks import _Task, build_tiny_model, load_fixture, load_ref_state

    g, sd, _, _ = load_fixture("ref_conformer_ctc_tiny")
    model = build_tiny_model("conformer").to(DEV).eval()
    load_ref_state(model, sd)
    d = _Task(40).target_dictionary
    sample = {"net_input": {"src_tokens": torch.from_numpy(g["feats"]).to(DEV), "src_lengths": torch.from_numpy(g["lengths"]).to(DEV)}}
    with torch.no_grad():
        net_out = model(**sample["net_input"])
        lp = model.get_normalized_probs(net_out, log_probs=True).transpose(0, 1).float().cpu().numpy().astype(np.float64)
    enc = net_out["src_lengths"][0].cpu().numpy()
    makers = {"greedy": lambda **kw: CTCDecoder([model], d, **kw),
              "beam": lambda **kw: CTCPrefixBeamSearchDecoder([model], d, beam_size=4, nbest=3, **kw),
              "beam_times_bonus": lambda **kw: CTCPrefixBeamSearchDecoder([model], d, beam_size=4, nbest=2, insertion_bonus=0.3,
                                                                          token_times=True, **kw)}
    seen = 0
    for name, make in makers.items():
        on, off = make(token_posteriors=True).generate([model], sample), make().generate([model], sample)
        _same_search(on, off)
        for b, utt in enumerate(on):
            for h in utt:
                y = h["tokens"].tolist()
                rpsi, rtot = ctc_prefix_oracle(lp[b], int(enc[b]), y, d.bos())
                _check_hyp(h, rpsi, rtot, np.arange(len(y)), (name, b, y))
                seen += len(y)
        if "times" in name:
            assert all("times" in h for u in on for h in u)
        if name == "greedy":  # the forced aligner on the same tokens: the same kernel on the same log-probs
            from espresso_amd.tools.forced_aligner import CTCForcedAligner

            res = CTCForcedAligner([model], d, token_posteriors=True).align(sample, [u[0]["tokens"].tolist() for u in on])
            plain = CTCForcedAligner([model], d).align(sample, [u[0]["tokens"].tolist() for u in on])
            for r, q, u in zip(res, plain, on):
                assert "token_posteriors" not in q and r["score"] == q["score"] and list(r["start"]) == list(q["start"])
                assert np.abs(r["token_posteriors"] - u[0]["token_posteriors"].numpy()).max(initial=0.0) <= 2 * SCORE_TOL
                assert abs(r["end_posterior"] - float(u[0]["end_posterior"])) <= 2 * SCORE_TOL
                assert abs(r["posterior_score"] - float(u[0]["posterior_score"])) <= SCORE_TOL and r["score"] <= r["posterior_score"] + SCORE_TOL
    assert seen > 20


@pytest.mark.gpu
def test_ctc_scorer_does_not_synchronise():
    _need_gpu()
    from espresso_amd.data.asr_dictionary import AsrDictionary
    from espresso_amd.tools.token_posteriors import CTCTokenPosteriors, score_rows

    d = AsrDictionary.from_symbols([f"t{i}" for i in range(16)], enable_bos=True)
    V = len(d)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(_peaked(rng, 2 * 9, V).astype(np.float32)).to(DEV).view(2, 9, V)
    tokens = torch.tensor([[5, d.bos(), 6, d.pad()], [7, 7, d.pad(), d.pad()], [d.pad()] * 4], dtype=torch.int32, device=DEV)
    lengths = torch.tensor([3, 2, 0], dtype=torch.int32, device=DEV)
    utt = torch.tensor([0, 1, 1], dtype=torch.int32, device=DEV)
    enc_len = torch.tensor([9, 7], device=DEV)
    scorer = CTCTokenPosteriors(d)
    ref = [t.clone() for t in score_rows(scorer, x, enc_len, tokens, lengths, utt, (d.bos(), d.pad()))]  # warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = score_rows(scorer, x, enc_len, tokens, lengths, utt, (d.bos(), d.pad()))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(out, ref):
        assert torch.equal(a, b)
    tok, end, total = (t.cpu().numpy() for t in out)
    x64 = x.cpu().numpy().astype(np.float64)
    for n, (b, L, y) in enumerate([(0, 9, [5, 6]), (1, 7, [7, 7]), (1, 7, [])]):
        rpsi, rtot = ctc_prefix_oracle(x64[b], L, y, d.bos())
        rc, _ = factors(rpsi, rtot)
        assert abs(total[n] - rtot) <= SCORE_TOL and abs(end[n] - rc[-1]) <= 2 * SCORE_TOL
    assert tok[0, 1] == 0 and tok[0, 3] == 0 and tok[0, 0] < 0 and tok[0, 2] < 0  # the blank inside the row gets no factor


def _transducer_fixture():
    from tests.test_forced_align import _transducer_fixture as fixture

    return fixture()


def _check_transducer_hyps(aligner, sample, hyps, blank, what):
    """Every hypothesis against the oracle on the lattice the device builds for its labels (rank by rank: one lattice per
    utterance), and its posterior_score against -loss of that lattice."""
    from espresso_amd.tools.forced_aligner import _pad_targets

    seen = 0
    for rank in range(max(len(u) for u in hyps)):
        rows = [u[rank] if rank < len(u) else None for u in hyps]
        labels = [[t for t in (h["tokens"].tolist() if h is not None else []) if t != blank] for h in rows]
        tg, tl = _pad_targets(labels, None, 0, DEV)
        lpb, lpy, enc_len, loss = aligner.lattice(sample, tg, tl)
        lpb, lpy, enc_len, loss = lpb.double().cpu().numpy(), lpy.double().cpu().numpy(), enc_len.cpu().numpy(), loss.cpu().numpy()
        for b, h in enumerate(rows):
            if h is None:
                continue
            at = np.array([k for k, t in enumerate(h["tokens"].tolist()) if t != blank], dtype=np.int64)
            rpsi, rtot = rnnt_prefix_oracle(lpb[b], lpy[b], int(enc_len[b]), len(labels[b]))
            _check_hyp(h, rpsi, rtot, at, (what, rank, b, labels[b]))
            assert abs(float(h["posterior_score"]) + float(loss[b])) <= SCORE_TOL, (what, rank, b)
            seen += len(labels[b])
    return seen


@pytest.mark.gpu
def test_transducer_decoders_with_token_posteriors(monkeypatch):
    _need_gpu()
    from espresso_amd.tools import token_posteriors as TP
    from espresso_amd.tools.forced_aligner import TransducerForcedAligner
    from espresso_amd.tools.transducer_beam_search_decoder import TransducerBeamSearchDecoder
    from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder
    from espresso_amd.tools.transducer_greedy_decoder import TransducerGreedyDecoder

    model, d, sample, _ = _transducer_fixture()
    aligner = TransducerForcedAligner([model], d)
    makers = {"greedy": lambda **kw: TransducerGreedyDecoder([model], d, **kw),
              "beam": lambda **kw: TransducerBeamSearchDecoder([model], d, beam_size=3, **kw),
              "frame_beam": lambda **kw: TransducerFrameBeamDecoder([model], d, beam_size=4, nbest=2, token_times=True, **kw)}
    seen = 0
    for name, make in makers.items():
        on, off = make(token_posteriors=True).generate([model], sample), make().generate([model], sample)
        _same_search(on, off)
        seen += _check_transducer_hyps(aligner, sample, on, d.bos(), name)
        if name == "greedy":  # the forced aligner on the labels the search emitted: the same lattice, the same kernel
            labels = [[t for t in u[0]["tokens"].tolist() if t != d.bos()] for u in on]
            res = TransducerForcedAligner([model], d, token_posteriors=True).align(sample, labels)
            for r, y, u in zip(res, labels, on):
                got = u[0]["token_posteriors"].cpu().numpy()[[k for k, t in enumerate(u[0]["tokens"].tolist()) if t != d.bos()]]
                assert list(r["tokens"]) == y and np.abs(r["token_posteriors"] - got).max(initial=0.0) <= 2 * SCORE_TOL
                assert abs(r["posterior_score"] - float(u[0]["posterior_score"])) <= SCORE_TOL
                assert r["score"] <= r["posterior_score"] + SCORE_TOL  # the best path is one of the paths
        if name == "frame_beam":  # groups of one hypothesis (a budget below one lattice) give the same rows
            monkeypatch.setattr(TP, "JOINT_GROUP_BYTES", 1)
            again = make(token_posteriors=True).generate([model], sample)
            monkeypatch.undo()
            for u, v in zip(on, again):
                for x, y in zip(u, v):
                    assert torch.equal(x["token_posteriors"], y["token_posteriors"]) and torch.equal(x["posterior_score"], y["posterior_score"])
    assert seen > 5


@pytest.mark.gpu
def test_transducer_fused_and_materialised_posteriors_agree():
    """The bound of test_forced_align.test_transducer_fused_and_materialised_lattices_align_alike (0.05: the fused lattice
    skips the bf16 rounding of the logits)."""
    _need_gpu()
    from espresso_amd.tools.token_posteriors import TransducerTokenPosteriors

    model, d, sample, targets = _transducer_fixture()
    ni = sample["net_input"]
    with torch.no_grad():
        enc = model.encoder(ni["src_tokens"], ni["src_lengths"])
        enc_len = enc["src_lengths"][0]
        B = enc_len.numel()
        E = model.joint_encoder_branch(enc["_x_bt"][0])
        E = E.view(B, E.shape[0] // B, E.shape[1])
    L = max(len(t) for t in targets)
    tokens = torch.tensor([t + [0] * (L - len(t)) for t in targets], dtype=torch.int32, device=DEV)
    lengths = torch.tensor([len(t) for t in targets], dtype=torch.int32, device=DEV)
    utt = torch.arange(B, dtype=torch.int32, device=DEV)
    cf, tf = TransducerTokenPosteriors(model, d).score(E, enc_len, tokens, lengths, utt)
    cp, tp = TransducerTokenPosteriors(model, d, fused=False).score(E, enc_len, tokens, lengths, utt)
    assert torch.isfinite(tf).all() and (tf - tp).abs().max() < 0.05 and (cf - cp).abs().max() < 0.05
    ulp = float(np.spacing(np.float32(float(tf.abs().max()) + 1.0)))  # each factor is one rounded difference of two Psi
    assert (cf <= 0).all() and (cf.double().sum(1) - tf.double()).abs().max() <= (L + 2) * ulp


# ------------------------------------------------------------------------------------------------ GPU: the command line
def _cli(capsys, main, argv):
    capsys.readouterr()
    main(argv)
    return capsys.readouterr().out.splitlines()


@pytest.mark.gpu
def test_cli_confidence_recognize_and_align(tmp_path, capsys, monkeypatch):
    """speech_recognize --confidence --ctm on the CTC checkpoint of the streamed decoder's CLI test: the H- lines and, but for its
    last column, the CTM are those of the run without the flag (whose column stays 1.00); the C- lines and the column carry the
    decoder's numbers.  speech_align --confidence on the recognised texts: the same column for a given transcript."""
    _need_gpu()
    from espresso_amd import speech_align
    from espresso_amd import speech_recognize as sr
    from espresso_amd.tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder
    from espresso_amd.tools.token_posteriors import confidence_line
    from tests.test_streaming_ctc_prefix_beam import _cli_fixture

    d, utts, base = _cli_fixture(tmp_path)
    args = base + ["--search", "ctc_beam", "--beam", "5", "--nbest", "2", "--ctc-beam-size-token", "4", "--batch-size", "2"]
    plain = _cli(capsys, sr.main, args + ["--ctm", str(tmp_path / "plain.ctm")])
    seen = []
    generate = CTCPrefixBeamSearchDecoder.generate

    def recording(self, models, sample, **kw):
        hyps = generate(self, models, sample, **kw)
        seen.extend(zip(sample["utt_ids"], hyps))
        return hyps

    monkeypatch.setattr(CTCPrefixBeamSearchDecoder, "generate", recording)
    conf = _cli(capsys, sr.main, args + ["--ctm", str(tmp_path / "conf.ctm"), "--confidence"])
    monkeypatch.undo()
    timing = lambda l: l.startswith("Recognized ")  # noqa: E731  (the one line that differs from run to run)
    assert [l for l in conf if not l.startswith("C-") and not timing(l)] == [l for l in plain if not timing(l)]
    assert not any(l.startswith("C-") for l in plain)
    hyps = dict(seen)
    assert sorted(hyps) == sorted(utts)
    strip = {d.eos(), d.pad()}  # what `recognize` strips from a CTC hypothesis' text: such a token has no C- entry and no CTM line

    def kept(h):
        return [f for t, f in zip(h["tokens"].tolist(), h["token_posteriors"].tolist()) if t not in strip]

    # every H- line is followed by the C- line of its hypothesis, with the decoder's numbers
    k = 0
    for i, line in enumerate(conf):
        if line.startswith("H-"):
            utt = line.split("\t")[0][2:]
            rank = sum(1 for l in conf[:i] if l.startswith("H-" + utt + "\t"))
            h = hyps[utt][rank]
            assert conf[i + 1] == confidence_line(utt, kept(h), float(h["end_posterior"])), (utt, rank)
            vals = [float(v) for v in conf[i + 1].split("\t")[1].split(" ")]
            assert len(vals) == len(line.split("\t")[1].split()) + 1 and all(0.0 <= v <= 1.0 for v in vals)
            k += 1
    assert k == 2 * len(utts)
    plain_ctm = (tmp_path / "plain.ctm").read_text().splitlines()
    conf_ctm = (tmp_path / "conf.ctm").read_text().splitlines()
    assert plain_ctm and all(l.endswith(" 1.00") for l in plain_ctm)
    assert [l.rsplit(" ", 1)[0] for l in conf_ctm] == [l.rsplit(" ", 1)[0] for l in plain_ctm]
    want = [f"{np.exp(f):.2f}" for u in utts for f in kept(hyps[u][0])]
    assert [l.rsplit(" ", 1)[1] for l in conf_ctm] == want and len(set(want)) > 1

    # the recognised texts as given transcripts
    best = {}
    for line in plain:
        if line.startswith("H-"):
            best.setdefault(line.split("\t")[0][2:], line.split("\t")[1])
    (tmp_path / "text").write_text("".join(f"{u} {best[u]}\n" for u in utts))
    a_args = base + ["--text", str(tmp_path / "text"), "--batch-size", "2"]
    speech_align.main(a_args + ["--output", str(tmp_path / "a_plain.ctm")])
    res = speech_align.main(a_args + ["--output", str(tmp_path / "a_conf.ctm"), "--confidence"])
    a_plain = (tmp_path / "a_plain.ctm").read_text().splitlines()
    a_conf = (tmp_path / "a_conf.ctm").read_text().splitlines()
    assert a_plain and all(l.endswith(" 1.00") for l in a_plain)
    assert [l.rsplit(" ", 1)[0] for l in a_conf] == [l.rsplit(" ", 1)[0] for l in a_plain]
    want = [f"{np.exp(f):.2f}" for u in utts for f in res[u]["token_posteriors"]]
    assert [l.rsplit(" ", 1)[1] for l in a_conf] == want
    for u in utts:  # (the aligners' numbers are held to the decoders' and the oracle in test_*_decoders_with_token_posteriors)
        r = res[u]
        assert r["feasible"] and len(r["token_posteriors"]) == len(r["tokens"]) and (r["token_posteriors"] <= 0).all()
        ulp = float(np.spacing(np.float32(abs(r["posterior_score"]) + 1.0)))
        assert abs(float(r["token_posteriors"].astype(np.float64).sum()) + r["end_posterior"] - r["posterior_score"]) <= (len(r["tokens"]) + 2) * ulp
    words = speech_align.main(a_args + ["--output", str(tmp_path / "a_word.ctm"), "--confidence", "--unit", "word"])
    assert words.keys() == res.keys() and len((tmp_path / "a_word.ctm").read_text().splitlines()) == len(utts)  # no <space>: one word each
