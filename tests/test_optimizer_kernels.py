"""The optimizer kernels (espresso_amd/csrc/optim.hip: sumsq_kernel, clip_coef_kernel, adam_kernel behind ea_grad_sumsq, ea_clip_coef,
ea_adam_step) one launch at a time against the plain fp64 restatement in tests/optim_ref.py, through the C ABI, every element of
every output.

BUFFERS (tests/test_convmodule_kernels.py's Buf).  Every device tensor is a view into a larger allocation: NaN guards around
read-only inputs, a sentinel bit pattern around everything a call writes (p, g, m, v, p_bf16, the sum, the two coefficients),
checked after the call.  p, g, m, v and the sum start as known data (the calls update them in place), p_bf16 starts as NaN.  No
element is excluded from any comparison.

BOUNDS.  Derived from the arithmetic, none measured.  e = 2^-23 per fp32 rounding (one rounding is 2^-24 relative, the factor two
pays for the second-order terms).  Division and sqrtf are taken as correctly rounded: csrc/Makefile compiles with -O3 and no
fast-math / -ffast-math / approximate-division flag, which is hipcc's default of IEEE division and square root on the device.
  ea_grad_sumsq   (4 iterations + 12 + blocks) e (|pre-fill| + sum g^2)
                  optim.hip:18-27: a thread adds four squares per trip (`iterations` trips of the grid-stride loop, 4 roundings
                  each counting the products), 6 wave steps, 4 block partials (the + 12 with the squares' own roundings), one
                  atomic per block onto `out`.  Asserted to stay below the square of the smallest planted heavy element.
  ea_clip_coef    coef[1]: 3 e |norm| (pre_scale / denom, sqrtf, the product);  coef[0]: 7 e |coef[0]| (the same three, `+ 1e-6`,
                  the division, fminf exact, the product with the scale);  optim.hip:33-41
  ea_adam_step    optim.hip:71-76, gs = coef[0] (1 without coef), all against fp64 on the same fp32 operands:
                  m   3 e (|m beta1| + |(1 - beta1) g gs|)       g gs, the two products, the addition (1 - beta: exact for beta >= 1/2)
                  v   6 e (v beta2 + (1 - beta2) (g gs)^2)       gg enters twice (2), two products, v beta2, the addition
                  den = sqrt(v) + eps: tv / (2 sqrt(v)) + e sqrt(v) + e den       q = m / den: tm / den + |m| tden / den^2 + e |q|
                  upd = -step_size q: step_size tq + 2 e |upd|   (step_size is computed in double and rounded to fp32 once: one e)
                  p   [2 e |p wd lr| + e |p1|, p1 = p + p (-wd lr): the scalar product, the product, the addition] + tupd + e |p'|
                  p_bf16 == the round-to-nearest-even bf16 of the kernel's own stored p, bit for bit; g all +0, or bit-unchanged
                  with zero_grad = 0.
  skip path       coef[0] NaN / +inf / -inf (optim.hip:46): p, m, v keep their bits, p_bf16 = bf16(p), g is zeroed when zero_grad
                  is set and kept otherwise (include/espresso_amd.h).  FlatAdam.clip_and_step (espresso_amd/optim/adam.py:36)
                  counts such a step: step_count, and with it the bias correction, advances.

FINDING.  clip_coef_kernel turned a non-finite norm into a FINITE coef[0] whenever it clipped: max_norm / (inf + 1e-6) = 0 and
fminf(1, NaN) = 1, so the skip path of adam_kernel could not be reached from an overflowed gradient and the step was applied
(moments decayed on a zero gradient, or NaN written into single parameters).  test_clip_coef's inf / NaN cases fail on the parent.

The first tests need no GPU: the reference against torch.optim.AdamW in float64; six mutations of a correct step and one of the sum
that must fall outside these bounds; every case of every GPU test built on the CPU with its preconditions asserted."""
import math
import zlib

import pytest
import torch

from tests import optim_ref as O
from tests.test_convmodule_kernels import Buf, _check, _gen, _st, _sync, inp, lib, out  # noqa: F401 (lib: the fixture)

gpu = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
E23 = 2.0 ** -23
LR, B1, B2, EPS = 1e-2, 0.9, 0.98, 1e-8
SUMSQ_GRID, ADAM_GRID = 2048 * 1024, 4096 * 1024


def _ptr(b):
    return None if b is None else b.p


def _same_bits(what, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    w = {F32: torch.int32, BF: torch.int16}[got.dtype]
    bad = got.view(w) != want.view(w)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ in their bits, first at {int(bad.nonzero()[0])}"


def _outside(fn):
    """True if the comparison `fn` rejects (the mutation tests)"""
    try:
        fn()
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------ the reference against torch (CPU)
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_reference_matches_torch_adamw_in_float64(wd):
    """optim_ref.adam_step == torch.optim.AdamW in float64 over six steps, within 1e-11 of scale: AdamW divides by
    sqrt(v) / sqrt(1 - beta2^t) + eps', which is fairseq's sqrt(v) + eps with eps' = eps / sqrt(1 - beta2^t)"""
    g = _gen(5)
    lr, b1, b2, eps, wdf = O.f32(LR), O.f32(B1), O.f32(B2), O.f32(EPS), O.f32(wd)
    p = torch.randn(64, generator=g, dtype=F64)
    tp = p.clone().requires_grad_()
    opt = torch.optim.AdamW([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wdf)
    m, v = torch.zeros(64, dtype=F64), torch.zeros(64, dtype=F64)
    for t in range(1, 7):
        grad = torch.randn(64, generator=g, dtype=F64) * 10.0 ** (t - 3)
        gs = 0.37 if t % 2 else 1.0
        r = O.adam_step(p, grad, m, v, gs, lr, b1, b2, eps, wdf, t)
        tp.grad = grad * gs
        opt.param_groups[0]["eps"] = eps / math.sqrt(1.0 - b2 ** t)
        opt.step()
        p, m, v = r["p"], r["m"], r["v"]
        st = opt.state[tp]
        for name, a, b in (("p", p, tp.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
            assert float((a - b).abs().max()) <= 1e-11 * float(b.abs().max()), (t, name)
    assert abs(O.sumsq(torch.tensor([3.0, 4.0]), 1.0) - 26.0) < 1e-12
    c0, c1 = O.clip_coef(25.0, 1.0, 4.0, 1.0)
    assert abs(c1 - 1.25) < 1e-12 and abs(c0 - 0.25 / (1.25 + O.f32(1e-6))) < 1e-12
    assert O.clip_coef(25.0, 2.0, None, 0.0) == (2.0, 10.0) and O.clip_coef(0.0, 0.5, None, 3.0) == (0.5, 0.0)
    for bad in (math.inf, math.nan):
        c0, c1 = O.clip_coef(bad, 1.0, 4.0, 2.0)
        assert not math.isfinite(c0) and not math.isfinite(c1)


# ------------------------------------------------------------------ ea_grad_sumsq
SUMSQ_N = [1, 3, 4, 5, 1023, 1024, 1025, 4099, SUMSQ_GRID + 1027]
HEAVY_SHARE = 0.05


def _sumsq_blocks(n):
    return min((n + 1023) // 1024, 2048)


def _sumsq_chain(n):
    blocks = _sumsq_blocks(n)
    return 4 * -(-n // (blocks * 1024)) + 12 + blocks


def _sumsq_plan(n, prefill):
    """g with the scales 16^(i / 4 % 3 - 1) and heavy elements of HEAVY_SHARE of the light total each at index 0, n - 1, the first
    element of the last partial float4 and the first element of the second grid-stride trip -> (g, heavy indices, pre-fill, ref, tol)"""
    gen = _gen(7 * n + 1)
    i = torch.arange(n)
    g = (torch.randn(n, generator=gen).double() * 16.0 ** ((i // 4) % 3 - 1).double())
    heavy = sorted({0, n - 1} | ({(n // 4) * 4} if n % 4 else set()) | ({SUMSQ_GRID} if n > SUMSQ_GRID else set()))
    g[heavy] = 0.0
    light = float((g.float().double() ** 2).sum())
    g[heavy] = math.sqrt(HEAVY_SHARE * light) if light > 0 else 3.0
    g = g.float()
    pre = O.f32(0.37 * (light + 1.0)) if prefill else 0.0
    ref = O.sumsq(g, pre)
    tol = _sumsq_chain(n) * E23 * ref
    assert tol < float(g[heavy].double().min()) ** 2, (n, "the bound no longer sees one heavy element")
    if n > SUMSQ_GRID:
        assert _sumsq_blocks(n) == 2048 and _sumsq_chain(n) == 8 + 12 + 2048
    return g, heavy, pre, ref, tol


def _sumsq_compare(what, got, ref, tol):
    _check(what, got.reshape(1), torch.tensor([ref], dtype=F64), torch.tensor([tol], dtype=F64))


def run_sumsq(lib, n, prefill):
    g, heavy, pre, ref, tol = _sumsq_plan(n, prefill)
    if lib is None:
        return g, heavy, pre, ref, tol
    bg, bo = inp(g), out((1,), F32, torch.tensor([pre]))
    rc = lib.ea_grad_sumsq(bg.p, n, bo.p, _st())
    _sync()
    assert rc == 0 and bo.intact(), (n, rc)
    _sumsq_compare(f"sumsq n={n} prefill={prefill}", bo.cpu(), ref, tol)


def test_sumsq_cases_on_the_cpu_and_a_dropped_heavy_element():
    """every case's preconditions; the sum without any one of its heavy elements, rounded to fp32, is outside the bound"""
    for n in SUMSQ_N:
        for prefill in (False, True):
            g, heavy, pre, ref, tol = run_sumsq(None, n, prefill)
            _sumsq_compare("correct", torch.tensor(ref).float(), ref, tol)
            for h in heavy:
                mutated = torch.tensor(ref - float(g[h].double()) ** 2).float()
                assert _outside(lambda: _sumsq_compare("heavy element omitted", mutated, ref, tol)), (n, h)


@gpu
@pytest.mark.parametrize("n", SUMSQ_N)
def test_grad_sumsq(lib, n):
    """sumsq_kernel: one thread, a lone tail, one float4, a float4 and a tail, a block minus one, one block, one more, four blocks
    and a tail, and 2048 * 1024 + 1027 — the only size at which the grid-stride loop takes a second trip; onto 0 and onto a pre-fill"""
    run_sumsq(lib, n, False)
    run_sumsq(lib, n, True)


@gpu
def test_grad_sumsq_of_nothing(lib):
    bo = out((1,), F32)
    assert lib.ea_grad_sumsq(None, 0, bo.p, _st()) == 0
    _sync()
    assert bo.untouched()


# ------------------------------------------------------------------ ea_clip_coef
# (sumsq, pre_scale, denom or None, max_norm)
CLIP = [(25.0, 1.0, None, 0.0), (25.0, 0.5, 4.0, 0.0),          # max_norm = 0: no clipping
        (25.0, 1.0, None, 7.5), (25.0, 1.0, 4.0, 2.0),          # norm below max_norm
        (25.0, 1.0, None, 2.0), (1.0e12, 3.0, 4.0, 2.0), (3.7e-9, 1.0, 128.0, 1e-6),   # above
        (25.0, 1.0, None, 5.0), (4.0, 1.0, 2.0, 1.0),           # equal: the 1e-6 makes the coefficient just below 1
        (0.0, 0.75, None, 2.0), (0.0, 1.0, 4.0, 0.0)]           # sumsq = 0: the coefficient is the scale
CLIP_BAD = [(math.inf, 1.0, None, 2.0), (math.nan, 1.0, None, 2.0), (math.inf, 1.0, 4.0, 0.0), (math.nan, 0.5, 4.0, 0.0),
            (math.inf, 1.0, 4.0, 1e30), (25.0, 1.0, 0.0, 2.0)]  # (the last: a zero denominator, a non-finite scale)


def _call_clip(lib, ss, pre_scale, denom, max_norm):
    bs, bc = inp(torch.tensor([ss], dtype=F32)), out((2,), F32)
    bd = None if denom is None else inp(torch.tensor([denom], dtype=F32))
    rc = lib.ea_clip_coef(bs.p, pre_scale, _ptr(bd), max_norm, bc.p, _st())
    _sync()
    assert rc == 0 and bc.intact(), (ss, pre_scale, denom, max_norm, rc)
    return bc


def _clip_compare(what, got, case):
    ss, pre_scale, denom, max_norm = case
    c0, c1 = O.clip_coef(O.f32(ss), pre_scale, None if denom is None else O.f32(denom), max_norm)
    ref = torch.tensor([c0, c1], dtype=F64)
    _check(what, got, ref, torch.tensor([7 * E23, 3 * E23], dtype=F64) * ref.abs())
    if ss == 0.0:
        assert float(got[1]) == 0.0


def test_clip_cases_on_the_cpu():
    for case in CLIP:
        c0, c1 = O.clip_coef(O.f32(case[0]), case[1], case[2], case[3])
        assert math.isfinite(c0) and math.isfinite(c1) and c0 > 0
        _clip_compare(f"clip {case}", torch.tensor([c0, c1]).float(), case)
        assert _outside(lambda: _clip_compare("norm reported unscaled", torch.tensor([c0, c1 * 1.00001]).float(), case)) or c1 == 0
    for case in CLIP_BAD:
        c0, c1 = O.clip_coef(case[0], case[1], case[2], case[3])
        assert not math.isfinite(c0) and not math.isfinite(c1), case


@gpu
def test_clip_coef(lib):
    """clip_coef_kernel: both floats between sentinels, every branch; a non-finite norm must give a non-finite coefficient (the
    parent commit gave 0 for inf and the plain scale for NaN wherever max_norm > 0)"""
    for case in CLIP:
        _clip_compare(f"clip {case}", _call_clip(lib, *case).cpu(), case)
    for case in CLIP_BAD:
        got = _call_clip(lib, *case).cpu()
        assert not math.isfinite(float(got[0])), (case, "coef[0] is finite: ea_adam_step would apply the step", float(got[0]))
        assert not math.isfinite(float(got[1])), (case, float(got[1]))


# ------------------------------------------------------------------ ea_adam_step
class Adam:
    """one ea_adam_step launch.  coef: None (NULL), "clip" (read back from ea_clip_coef's own output) or a float placed in coef[0]"""

    def __init__(self, n, t, wd=0.0, coef=None, bf=True, zg=1):
        self.__dict__.update(n=n, t=t, wd=wd, coef=coef, bf=bf, zg=zg)

    def __repr__(self):
        return "Adam(" + ", ".join(f"{k}={v!r}" for k, v in self.__dict__.items()) + ")"


def _adam_operands(c):
    """p ~ N(0, 1); |g| = 2^k (1 + u), k uniform in [-20, 20]; m and v at g's magnitude and non-zero; elements with g = 0, with
    m = v = 0, with both; at t = 1 every third element has m = v = 0 and g != 0 (the first step's state)"""
    n = c.n
    gen = _gen(zlib.crc32(repr(c).encode()))
    mag = torch.exp2(torch.randint(-20, 21, (n,), generator=gen).double()) * (1 + torch.rand(n, generator=gen).double())
    sign = lambda: 1 - 2 * torch.randint(0, 2, (n,), generator=gen).double()
    p = torch.randn(n, generator=gen)
    g = (mag * sign()).float()
    m = (0.3 * mag * (0.25 + torch.rand(n, generator=gen).double()) * sign()).float()
    v = (mag * mag * (0.2 + torch.rand(n, generator=gen).double())).float()
    i = torch.arange(n)
    g[i % 7 == 3] = 0.0
    zero_state = (i % 11 == 5) | (i % 77 == 3)          # the second set has g = 0 as well
    if c.t == 1:
        zero_state |= i % 3 == 1
    m[zero_state] = 0.0
    v[zero_state] = 0.0
    if n >= 80:
        assert bool(((g == 0) & (v == 0)).any()) and bool(((g != 0) & (v == 0)).any()) and bool(((g == 0) & (v != 0)).any())
    assert bool((((g.double() * 2.0 ** -24) ** 2 * 0.001) >= 2.0 ** -126)[g != 0].all())   # the squares stay normal
    return p, g, m, v


def _clip_inputs(g):
    """the call that produces coef for the "clip" cases: the gradient's own fp64 sum of squares, scale 1 / 4, max_norm at half the
    scaled norm (it clips: coef[0] is about 1 / 8)"""
    ss = O.f32(O.sumsq(g))
    return (ss, 1.0, 4.0, O.f32(math.sqrt(ss) / 8) if ss > 0 else 2.0)


def _adam_compare(what, c, ops, gs, got_p, got_m, got_v, mut=None):
    ref = O.adam_step(*ops, gs, LR, B1, B2, EPS, c.wd, c.t)
    _check(what + " exp_avg", got_m, ref["m"], ref["tm"])
    _check(what + " exp_avg_sq", got_v, ref["v"], ref["tv"])
    _check(what + " p", got_p, ref["p"], ref["tp"])
    return ref


def run_adam(lib, c):
    p, g, m, v = ops = _adam_operands(c)
    n = c.n
    if c.coef == "clip":
        gs = O.f32(O.clip_coef(*_clip_inputs(g))[0])
        assert 0 < gs <= 0.25 and (gs < 0.13 or not bool(g.any()))      # it clips
    else:
        gs = 1.0 if c.coef is None else c.coef
    ref = O.adam_step(*ops, gs, LR, B1, B2, EPS, c.wd, c.t)
    # precondition: the bound of p stays a few roundings of p and of the largest possible step (|m / denom| <= 1 / (1 - beta1))
    assert bool((ref["tp"] < 2.0 ** -18 * (ref["p"].abs() + O.step_size(LR, B1, B2, c.t) / (1 - B1))).all())
    if lib is None:
        return ref
    bp, bg, bm, bv = out((n,), F32, p), out((n,), F32, g), out((n,), F32, m), out((n,), F32, v)
    b16 = out((n,), BF) if c.bf else None
    bc = None
    if c.coef == "clip":
        bc = _call_clip(lib, *_clip_inputs(g))
        gs = float(bc.cpu()[0])
        assert 0 < gs <= 0.25
    elif c.coef is not None:
        bc = out((2,), F32, torch.tensor([c.coef, 0.0]))
    rc = lib.ea_adam_step(bp.p, bg.p, bm.p, bv.p, _ptr(b16), n, _ptr(bc), LR, B1, B2, EPS, c.wd, c.t, c.zg, _st())
    _sync()
    assert rc == 0, (c, rc)
    for b in (bp, bg, bm, bv, b16, bc):
        assert b is None or b.intact(), (c, "stored outside the tensor")
    tag = repr(c)
    _adam_compare(tag, c, ops, gs, bp.cpu(), bm.cpu(), bv.cpu())
    if b16 is not None:
        _same_bits(tag + " p_bf16 against the stored p", b16.cpu(), O.bf16_rne(bp.cpu()))
    _same_bits(tag + " g", bg.cpu(), torch.zeros(n) if c.zg else g)
    return ref


ADAM_SMALL = [Adam(n, t, wd, coef, bf, zg)
              for k, n in enumerate([1, 3, 4, 5, 1027])
              for j, (t, wd, coef, bf, zg) in enumerate([(1, 0.0, None, True, 1), (2, 0.01, "clip", True, 1), (1000, 0.01, None, False, 0),
                                                         (100000, 0.0, "clip", True, 0), (1, 0.01, "clip", False, 1), (2, 0.0, None, True, 0)])]
ADAM_LARGE = [Adam(ADAM_GRID + 1027, 2, 0.01, "clip", True, 1), Adam(ADAM_GRID + 1027, 1000, 0.0, None, False, 0)]


def test_adam_cases_on_the_cpu():
    for c in ADAM_SMALL + [Adam(80, 1, 0.01, "clip"), Adam(4099, 100000)]:
        run_adam(None, c)
    for c in ADAM_LARGE:
        blocks = min((c.n + 1023) // 1024, 4096)
        assert blocks == 4096 and c.n > blocks * 1024      # the grid-stride loop takes a second trip, with a tail of three


@pytest.mark.parametrize("mut", O.MUTATIONS)
def test_adam_mutations_fall_outside_the_bounds(mut):
    """a correct step (the fp64 reference rounded to fp32) passes; with one defect it does not"""
    c = Adam(1027, 2, 0.01, "clip")
    ops = _adam_operands(c)
    gs = O.f32(O.clip_coef(*_clip_inputs(ops[1]))[0])
    good = O.adam_step(*ops, gs, LR, B1, B2, EPS, c.wd, c.t)
    _adam_compare("correct", c, ops, gs, good["p"].float(), good["m"].float(), good["v"].float())
    bad = O.adam_step(*ops, gs, LR, B1, B2, EPS, c.wd, c.t, mut=mut)
    assert _outside(lambda: _adam_compare(mut, c, ops, gs, bad["p"].float(), bad["m"].float(), bad["v"].float())), mut
    # ... and p alone is enough for every defect that reaches it
    if mut != "tail_element_skipped":
        assert _outside(lambda: _check(mut + " p", bad["p"].float(), good["p"], good["tp"])), mut


@gpu
@pytest.mark.parametrize("c", ADAM_SMALL, ids=repr)
def test_adam_step(lib, c):
    """adam_kernel: one thread with a tail of 1 and 3, one float4, a float4 and a tail, a block and a tail; steps 1, 2, 1000, 100000;
    with and without weight decay, coef, p_bf16, zero_grad"""
    run_adam(lib, c)


@gpu
@pytest.mark.parametrize("c", ADAM_LARGE, ids=repr)
def test_adam_step_grid_stride_second_trip(lib, c):
    """n = 4096 * 1024 + 1027: the only path that runs at the model's 80 M parameters"""
    run_adam(lib, c)


@gpu
@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf], ids=["nan", "inf", "-inf"])
def test_adam_step_skips_on_a_non_finite_coefficient(lib, bad):
    """p, m, v keep their bits; p_bf16 = bf16(p); g is zeroed with zero_grad and kept without (include/espresso_amd.h)"""
    for n, zg, bf in ((5, 1, True), (1027, 0, True), (1027, 1, False)):
        c = Adam(n, 2, 0.01, None, bf, zg)
        p, g, m, v = _adam_operands(c)
        bp, bg, bm, bv = out((n,), F32, p), out((n,), F32, g), out((n,), F32, m), out((n,), F32, v)
        b16 = out((n,), BF) if bf else None
        bc = out((2,), F32, torch.tensor([bad, 1.0]))
        rc = lib.ea_adam_step(bp.p, bg.p, bm.p, bv.p, _ptr(b16), n, bc.p, LR, B1, B2, EPS, c.wd, c.t, zg, _st())
        _sync()
        assert rc == 0
        for b in (bp, bg, bm, bv, b16, bc):
            assert b is None or b.intact()
        for name, b, want in (("p", bp, p), ("exp_avg", bm, m), ("exp_avg_sq", bv, v), ("g", bg, torch.zeros(n) if zg else g)):
            _same_bits(f"skip {bad} {name}", b.cpu(), want)
        if bf:
            _same_bits(f"skip {bad} p_bf16", b16.cpu(), O.bf16_rne(p))


@gpu
def test_adam_step_of_nothing(lib):
    bp = out((4,), F32)
    assert lib.ea_adam_step(bp.p, bp.p, bp.p, bp.p, None, 0, None, LR, B1, B2, EPS, 0.0, 1, 1, _st()) == 0
    _sync()
    assert bp.untouched()


@gpu
def test_three_step_trajectory_every_stage(lib):
    """tests/gpu_checks.py:check_adam's run (n = 100003, three steps, scale 1 / 4, max_norm 2, moments from zero, one carried state),
    every stage against fp64 on the kernel's own carried p, m, v, its own sum and its own coefficient"""
    n = 100003
    gen = _gen(0)
    p = torch.randn(n, generator=gen)
    bp, bm, bv = out((n,), F32, p), out((n,), F32, torch.zeros(n)), out((n,), F32, torch.zeros(n))
    b16, bd = out((n,), BF), inp(torch.tensor([4.0]))
    c = Adam(n, 0)
    for t in (1, 2, 3):
        c.t = t
        grad = torch.randn(n, generator=gen) * 3
        bg, bs, bc = out((n,), F32, grad), out((1,), F32, torch.zeros(1)), out((2,), F32)
        before = (bp.cpu().clone(), grad, bm.cpu().clone(), bv.cpu().clone())
        assert lib.ea_grad_sumsq(bg.p, n, bs.p, _st()) == 0
        assert lib.ea_clip_coef(bs.p, 1.0, bd.p, 2.0, bc.p, _st()) == 0
        assert lib.ea_adam_step(bp.p, bg.p, bm.p, bv.p, b16.p, n, bc.p, LR, B1, B2, EPS, 0.0, t, 1, _st()) == 0
        _sync()
        for b in (bp, bg, bm, bv, b16, bs, bc):
            assert b.intact(), t
        ss = O.sumsq(grad)
        _sumsq_compare(f"step {t} sumsq", bs.cpu(), ss, _sumsq_chain(n) * E23 * ss)
        _clip_compare(f"step {t} coef", bc.cpu(), (float(bs.cpu()[0]), 1.0, 4.0, 2.0))
        assert float(bc.cpu()[0]) < 0.25
        _adam_compare(f"step {t}", c, before, float(bc.cpu()[0]), bp.cpu(), bm.cpu(), bv.cpu())
        _same_bits(f"step {t} p_bf16", b16.cpu(), O.bf16_rne(bp.cpu()))
        _same_bits(f"step {t} g", bg.cpu(), torch.zeros(n))
