"""ea_adam_step_capped (espresso_amd/csrc/optim.hip: adam_kernel from a persistent grid of at most `max_blocks` workgroups, the launch
that runs the deferred part of the optimizer pass on the side stream) against ea_adam_step on the same inputs: p, g, m, v and the
bf16 shadow must agree BIT FOR BIT.  Both entry points launch ONE kernel: a first version with a second kernel around a shared
`__device__` body (several float4 groups in flight per thread) differed in single bits of m, v and p at every size, because the
compiler contracts `a * b + c` into an fma or not per lane position and per kernel (in adam_kernel itself lanes 0-1 of a float4 get
a packed fma for exp_avg, lanes 2-3 a multiply and an add).  One case also goes against the fp64 restatement tests/optim_ref.py at
that file's own bounds.

Sizes.  A workgroup takes 1024 elements per trip, so one sweep of the grid is max_blocks * 1024 elements:
  1, 3, 4, 5, 1023, 1024, 1025           the tail path (element loop), one workgroup and one more, one trip
  sweep + 515, 2 * sweep + 515           two and three trips, the last one partial with a tail of three elements
for max_blocks = 1 (sweep 1024; there 1025 already takes two trips) and the shipped cap (espresso_amd.optim.adam.SIDE_MAX_BLOCKS).

Options, crossed in full at the small sizes and covered value by value at the large ones: zero_grad on / off, p_bf16 NULL / given,
weight_decay 0 / 0.01, coef NULL / finite (read back from ea_clip_coef) / +inf / NaN.  On a non-finite coefficient the capped launch
must do what include/espresso_amd.h says of ea_adam_step: p, m, v keep their bits, g is zeroed only with zero_grad, p_bf16 = bf16(p)."""
import math

import pytest
import torch

from espresso_amd.optim.adam import SIDE_MAX_BLOCKS
from tests import optim_ref as O
from tests.test_convmodule_kernels import _st, _sync, lib, out  # noqa: F401 (lib: the fixture)
from tests.test_optimizer_kernels import (B1, B2, BF, EPS, F32, LR, Adam, _adam_compare, _adam_operands, _call_clip, _clip_inputs,
                                          _ptr, _same_bits)

gpu = pytest.mark.gpu
PER_BLOCK = 1024  # elements one workgroup takes per trip (256 threads, one float4 each)
SMALL = [1, 3, 4, 5, 1023, 1024, 1025]
COEFS = [None, "clip", math.inf, math.nan]
FULL = [(zg, bf, wd, coef) for zg in (1, 0) for bf in (True, False) for wd in (0.0, 0.01) for coef in COEFS]
# every value of every option, and each non-finite coefficient with and without zero_grad
FEW = [(1, True, 0.01, "clip"), (0, False, 0.0, None), (1, False, 0.0, math.inf), (0, True, 0.01, math.nan), (1, True, 0.0, math.nan),
       (0, True, 0.01, math.inf)]


def _sizes(max_blocks):
    sweep = max_blocks * PER_BLOCK
    return SMALL + [sweep + 515, 2 * sweep + 515]


CASES = [(mb, n) for mb in (1, SIDE_MAX_BLOCKS) for n in _sizes(mb)]


def test_cases_on_the_cpu():
    """the sizes take the trips the docstring says; the option lists cover every value"""
    trips = lambda n, mb: -(-n // (min(mb, -(-n // PER_BLOCK)) * PER_BLOCK))
    for mb in (1, SIDE_MAX_BLOCKS):
        assert [trips(n, mb) for n in _sizes(mb)] == [1] * (len(SMALL) - 1) + [2 if mb == 1 else 1, 2, 3]
        assert all(n % 4 == 3 and n % PER_BLOCK != 0 for n in _sizes(mb)[-2:])
    for opts in (FULL, FEW):
        assert {o[0] for o in opts} == {0, 1} and {o[1] for o in opts} == {True, False} and {o[2] for o in opts} == {0.0, 0.01}
        assert {repr(o[3]) for o in opts} == {repr(c) for c in COEFS}
        assert {(o[0], repr(o[3])) for o in opts} >= {(z, repr(c)) for z in (0, 1) for c in (math.inf, math.nan)}
    assert SIDE_MAX_BLOCKS >= 1


def _launch(lib, capped, ops, c, coef_buf, max_blocks):
    p, g, m, v = ops
    n = c.n
    bufs = [out((n,), F32, p), out((n,), F32, g), out((n,), F32, m), out((n,), F32, v), out((n,), BF) if c.bf else None]
    args = [b.p if b is not None else None for b in bufs] + [n, _ptr(coef_buf), LR, B1, B2, EPS, c.wd, c.t, c.zg]
    rc = lib.ea_adam_step_capped(*args, max_blocks, _st()) if capped else lib.ea_adam_step(*args, _st())
    assert rc == 0, (c, capped, rc)
    return bufs


def _run(lib, n, max_blocks, opts, t=2):
    ops = _adam_operands(Adam(n, t))
    clip = None
    for zg, bf, wd, coef in opts:
        c = Adam(n, t, wd, coef, bf, zg)
        if coef == "clip":
            clip = clip or _call_clip(lib, *_clip_inputs(ops[1]))
            bc = clip
        else:
            bc = None if coef is None else out((2,), F32, torch.tensor([coef, 0.0]))
        whole = _launch(lib, False, ops, c, bc, max_blocks)
        capped = _launch(lib, True, ops, c, bc, max_blocks)
        _sync()
        tag = f"max_blocks={max_blocks} {c!r}"
        for name, a, b in zip(("p", "g", "m", "v", "p_bf16"), whole, capped):
            if a is None:
                continue
            assert b.intact(), (tag, name, "stored outside the tensor")
            w = torch.int32 if a.dtype == F32 else torch.int16
            if not torch.equal(a.t.view(w), b.t.view(w)):
                _same_bits(f"{tag} {name}", b.cpu(), a.cpu())  # (names the first element)
        assert bc is None or bc.intact()
        if isinstance(coef, float) and not math.isfinite(coef):
            for name, b, want in (("p", capped[0], ops[0]), ("m", capped[2], ops[2]), ("v", capped[3], ops[3]),
                                  ("g", capped[1], torch.zeros(n) if zg else ops[1])):
                _same_bits(f"{tag} skip: {name}", b.cpu(), want)
            if bf:
                _same_bits(f"{tag} skip: p_bf16", capped[4].cpu(), O.bf16_rne(ops[0]))


@gpu
@pytest.mark.parametrize("max_blocks,n", CASES)
def test_capped_launch_equals_the_whole_launch_bit_for_bit(lib, max_blocks, n):
    _run(lib, n, max_blocks, FULL if n <= 1025 else FEW)


@gpu
def test_first_step_state(lib):
    """t = 1 (every third element starts with m = v = 0) and a late step, two trips of the shipped grid"""
    for t in (1, 100000):
        _run(lib, SIDE_MAX_BLOCKS * PER_BLOCK + 515, SIDE_MAX_BLOCKS, FEW[:2], t=t)


@gpu
def test_capped_launch_against_the_fp64_reference(lib):
    """tests/optim_ref.py's bounds (the ones tests/test_optimizer_kernels.py holds ea_adam_step to), three trips of the shipped grid"""
    c = Adam(2 * SIDE_MAX_BLOCKS * PER_BLOCK + 515, 2, 0.01, "clip", True, 1)
    ops = _adam_operands(c)
    bc = _call_clip(lib, *_clip_inputs(ops[1]))
    gs = float(bc.cpu()[0])
    assert 0 < gs <= 0.25
    bp, bg, bm, bv, b16 = _launch(lib, True, ops, c, bc, SIDE_MAX_BLOCKS)
    _sync()
    for b in (bp, bg, bm, bv, b16):
        assert b.intact()
    _adam_compare(repr(c), c, ops, gs, bp.cpu(), bm.cpu(), bv.cpu())
    _same_bits("p_bf16 against the stored p", b16.cpu(), O.bf16_rne(bp.cpu()))
    _same_bits("g", bg.cpu(), torch.zeros(c.n))


@gpu
def test_capped_launch_of_nothing_and_bad_grid(lib):
    bp = out((4,), F32)
    assert lib.ea_adam_step_capped(bp.p, bp.p, bp.p, bp.p, None, 0, None, LR, B1, B2, EPS, 0.0, 1, 1, 8, _st()) == 0
    assert lib.ea_adam_step_capped(bp.p, bp.p, bp.p, bp.p, None, 4, None, LR, B1, B2, EPS, 0.0, 1, 1, 0, _st()) != 0
    _sync()
    assert bp.untouched()


@gpu
def test_clip_coef_clear(lib):
    """ea_clip_coef_clear: ea_clip_coef's two floats, bit for bit, and the accumulator zero afterwards; ea_clip_coef leaves it"""
    for ss, pre, denom, mx in ((25.0, 1.0, 4.0, 2.0), (25.0, 0.5, None, 0.0), (math.inf, 1.0, 4.0, 2.0), (math.nan, 1.0, None, 2.0)):
        bd = None if denom is None else out((1,), F32, torch.tensor([denom]))
        got = []
        for clear in (False, True):
            bs, bc = out((1,), F32, torch.tensor([ss])), out((2,), F32)
            fn = lib.ea_clip_coef_clear if clear else lib.ea_clip_coef
            assert fn(bs.p, pre, _ptr(bd), mx, bc.p, _st()) == 0
            _sync()
            assert bs.intact() and bc.intact()
            got.append(bc.cpu())
            left = float(bs.cpu()[0])
            assert (left == 0.0) if clear else (left == ss or (math.isnan(ss) and math.isnan(left))), (ss, clear, left)
        _same_bits(f"coef {ss}", got[1], got[0])
