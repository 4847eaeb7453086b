"""The LayerNorm kernels (espresso_amd/csrc/layernorm.hip: 7 kernels behind 11 entry points) one launch at a time against the plain
fp64 restatement in tests/rowwise_ref.py, through the C ABI, every element of every output.

BUFFERS (tests/test_convmodule_kernels.py's Buf).  Every device tensor is a view into a larger allocation with guards on both sides:
NaN around inputs, a sentinel bit pattern around outputs (checked after the call).  An output starts as NaN (a missed store is a
failure), or as known data where the call accumulates (dgamma, dbeta); the split workspaces start as NaN.  row_zero sits between
guards of 0xff: a flag read outside [0, M) zeroes a row.  No element is excluded from any comparison.

SCALES.  gamma[c] and beta[c] carry the per-chunk scale 16^((c / 8) % 3 - 1); row m is drawn with spread 16^(m % 3 - 1) around the
offset (1 + m % 4) spread: mean[m] and rstd[m] of a neighbouring row, or a chunk one row or eight columns off, cannot pass.  With
M >= 5, row 1 is constant (variance 0: y = beta within the bound), row 2 has an offset 2^6 times its spread, row 3 has a single
non-zero element.

BOUNDS.  Derived from the arithmetic, none measured.  e = 2^-23 is charged for every fp32 rounding (one rounding is 2^-24
relative: the factor two pays for the second-order terms) and for v_rcp_f32 / v_rsq_f32 (1 ulp, as for common.h:128-132);
ulp(x) = the bf16 step at |x|; k8 = 16-byte chunks per lane (1: C <= 512, 2: C <= 1024, 4); all references are fp64 on the same
bf16 / fp32 operands.
  mean     em = (4 k8 + 7) e mean_c|x| + 2 e |mean|
           ln_fwd_kernel, layernorm.hip:116-129 (`s += v0 + v1`: one pair addition, 4 k8 running additions, the 6 steps of wave_sum;
           `/ (float)C`), ln_fwd_rows_kernel :195-206 (the same with k8 = 1, wave_sum_dpp's 6 additions; `* inv_c`: v_rcp_f32 and a
           multiplication, the 2 e)
  rstd     rel_r rstd,  rel_r = ((8 k8 + 12) / 2 + 1) e + em^2 / (var + eps)
           :130-142, :207-221: x - mean_f = (x - mean) + D with one D for the row, |D| <= em, and sum_c (x - mean) = 0, so the
           variance moves by D^2 exactly (the em^2 term) and by its roundings: the subtraction (twice in the square), the square, 8 k8
           running additions, 6 wave steps, `/ C` (2), `+ eps` — (8 k8 + 12) e of var + eps, halved by the square root; rsqrtf 1 ulp
  y        keep ((rel_r + 5 e) |x - mean| rstd |gamma| + em rstd |gamma| + 2 e |beta|)   [+ ulp(ref) for a bf16 output]
           :156-158, :233-235: the subtraction, two multiplications, the addition of beta, the keep-scale.  em rstd |gamma| holds the
           term |mean| 2^-23 rstd |gamma|: the error of x - mean where the offset dominates the spread (rows 1 and 2)
  y2 of ea_layernorm_fwd2: the same, the reference evaluated on the kernel's own stored y1 (ln_fwd2_rows_kernel :299-333)
  dx       (8 k8 + 18) e dx_mag,  dx_mag = rstd (|g| + mean_c|g| + |xhat| mean_c|g xhat|) + |dx_add|   [+ ulp(ref)]
           ln_bwd_accum8 :61-77, ln_bwd_finish8 :79-90, ln_bwd_kernel :398-431, ln_bwd2_kernel :536-557: dv = dy keep and g = dv gamma
           round once each, xhat twice; s1 and s2 are sums of 8 k8 running additions and 6 wave steps times inv_c (2): (8 k8 + 10) e
           and (8 k8 + 12) e of their magnitudes; g - s1, the fma and the product with rstd round once each (3 e of the whole), the
           addition of dx_add once: every term is covered by (8 k8 + 18) e of its magnitude
  out2     from bf16(dx): a2 dr keep2 rounds twice in fp32.  The kernel's fp32 dx may sit on the other side of a bf16 rounding tie than
           the fp64 dx, so the reference is taken at bf16(dx - t) and bf16(dx + t), t = dx's fp32 bound: tolerance = half their distance
           + ulp + 2 e.  The CPU test asserts that the two ends differ on at most 2 % of a case's elements.  (out2 is also compared
           with the kernel's own stored dx, where no window is needed.)
  dgamma, dbeta      chain e mag,  mag = |pre-fill| + sum_m |dv xhat| (or |dv|),
           chain = rows a wavefront adds + 4 (the fold over the block's wavefronts, :479-485) + the depth of what follows + 4 (dv, xhat
           twice, the product).  Workspace path: 8 rows per block, 2 per wavefront; ln_param_reduce_kernel :606-623 adds ceil(per / 4)
           partial rows per thread, 3 in the block, and `rs` atomics land on the pre-fill in any order.  Atomic path: one atomic per
           block.  This is at most (rows + partial rows + a small constant) 2^-23 mag, and unlike that it stays below one row's
           share at M = 4100.
  workspace column sums after _bwd_dx / _bwd2_dx: (2 + 4 + 4) e mag; ea_layernorm_param_reduce from given partial rows:
           (ceil(per / 4) + 3 + rs) e mag
Every sum's bound is asserted to stay below one average row's share (_sees_one_row), and the fp32 part of y's bound below 1/64 of the
chunk's scale (a neighbouring chunk is 16 times larger or smaller).  Bit-identity statements (the pair against the single kernels,
outputs a call must not touch) take no tolerance.

ea_layernorm_bwd2_dx never stores the gradient d between its two norms; it is compared bit for bit with ea_layernorm_bwd_dx followed
by ea_layernorm_bwd_dx2 at EVERY shape, and those two are compared with the reference stage by stage (the second on the stored d),
which is the pair's restatement with the kernel's own rounding of d.

The first tests need no GPU: the reference against F.layer_norm and autograd in float64; seven mutations of a correct output that
must fall outside these bounds; every case of every GPU test built on the CPU with the bounds' preconditions asserted."""
import ctypes
import types
import zlib

import pytest
import torch
import torch.nn.functional as TF

from tests import rowwise_ref as R
from tests.test_convmodule_kernels import _INT, _SENTINEL, DEV, Buf, _check, _check_bf16, _gen, _sees_one_row, _st, _sync, _ulp, inp, lib, out  # noqa: F401 (lib: the fixture)
from tests.test_subsample_kernels import _same_values

gpu = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
E23 = 2.0 ** -23
TIE_CAP = 0.02


def _k8(C):
    return 1 if C <= 512 else (2 if C <= 1024 else 4)


def _close(a, b):
    return a.shape == b.shape and float((a - b).abs().max()) <= 1e-11 * max(float(b.abs().max()), 1e-300)


# ------------------------------------------------------------------ data
def _chunk_scale(C):
    return 16.0 ** ((torch.arange(C) // 8) % 3 - 1).double()


def _affine(g, C):
    sc = _chunk_scale(C)
    return (sc * (1.0 + 0.25 * torch.randn(C, generator=g).double())).float(), (sc * torch.randn(C, generator=g).double()).float()


def _row_scale(M, shift=0):
    return 16.0 ** ((torch.arange(M) + shift) % 3 - 1).double()


def _rows(g, M, C, single=True):
    """bf16 [M][C]: row m around (1 + m % 4) spread with spread 16^(m % 3 - 1), sign alternating; the three statistics rows.
    single = False (the backward cases): without the row of a single non-zero element — its xhat takes two values only, so the two
    projections of the backward force dx = 0 at that element exactly, and the fp32 dx is rounding noise of either sign"""
    sp = _row_scale(M).view(M, 1)
    off = sp * (1 + torch.arange(M) % 4).view(M, 1) * (1 - 2 * (torch.arange(M) % 2)).view(M, 1)
    x = off + sp * torch.randn(M, C, generator=g).double()
    if M >= 5:
        x[1] = 2.5
        x[2] = 4.0 + torch.randn(C, generator=g).double() / 16
        if single:
            x[3] = 0.0
            x[3, (3 * C) // 5] = 3.0
    return x.to(BF)


def _flags(M, tail):
    """row_zero: the first row, the last row, one in the middle; `tail`: also M - 3 (inside the clamped tail of the rows kernel)"""
    z = torch.zeros(M, dtype=torch.uint8)
    z[0] = z[M - 1] = z[M // 2] = 1
    if tail and M >= 4:
        z[M - 3] = 1
    return z


def _dev_flags(z):
    """uint8 [M] on the device between two guards of 0xff -> (holder, pointer)"""
    full = torch.full((z.numel() + 256,), 255, dtype=torch.uint8)
    full[128:128 + z.numel()] = z
    full = full.to(DEV)
    return full, ctypes.c_void_p(full.data_ptr() + 128)


def _ptr(b):
    return None if b is None else b.p


# ------------------------------------------------------------------ bounds
def _fwd_tols(ref, gamma, beta, C):
    """(bound of mean [M], of rstd [M], the fp32 part of y's bound [M][C]) — module docstring"""
    k8 = _k8(C)
    em = (4 * k8 + 7) * E23 * ref["a1"] + 2 * E23 * ref["absmean"]
    rel_r = ((8 * k8 + 12) / 2 + 1) * E23 + em * em / ref["w"]
    r = ref["rstd"].view(-1, 1)
    ga, be = R.f64(gamma).abs(), R.f64(beta).abs()
    ty = ref["keep"] * ((rel_r.view(-1, 1) + 5 * E23) * ref["absd"] * r * ga + em.view(-1, 1) * r * ga + 2 * E23 * be)
    return em, rel_r * ref["rstd"], ty


def _fwd_preconditions(what, ref, gamma, beta, C):
    """the fp32 part of y's bound stays below 1/64 of the chunk's scale (times the element's |xhat| where that is above 1)"""
    _, _, ty = _fwd_tols(ref, gamma, beta, C)
    xhat = (ref["absd"] * ref["rstd"].view(-1, 1)).clamp_min(1.0)
    lim = ref["keep"] * _chunk_scale(C) * xhat / 64
    live = ref["keep"] > 0
    assert bool((ty[live] < lim[live]).all()), f"{what}: the bound of y has grown past 1/64 of a chunk's scale"


def _fwd_compare(what, ref, gamma, beta, C, y, mean, rstd):
    """y (bf16 or fp32), mean, rstd (or None) against a reference dict of R.ln_fwd"""
    tm, tr, ty = _fwd_tols(ref, gamma, beta, C)
    if mean is not None:
        _check(what + " mean", mean, ref["mean"], tm)
    if rstd is not None:
        _check(what + " rstd", rstd, ref["rstd"], tr)
    if y.dtype == BF:
        _check_bf16(what + " y", y, ref["y"], ty)
    else:
        _check(what + " y", y, ref["y"], ty)


def _dx_tol(ref, C):
    return (8 * _k8(C) + 18) * E23 * ref["dx_mag"]


def _out2_window(ref, C, a2):
    """(middle, half-width + roundings) of out2 over the fp32 window of dx, and the share of elements whose two ends differ"""
    t = _dx_tol(ref, C)
    lo, hi = R.second_output(ref["dx"] - t, a2, ref["keep2"]), R.second_output(ref["dx"] + t, a2, ref["keep2"])
    big = torch.maximum(lo.abs(), hi.abs())
    share = float((lo != hi).double().mean())
    return (lo + hi) / 2, (hi - lo).abs() / 2 + _ulp(big) + 2 * E23 * big, share


def _reduce_depth(nblk, largest=None):
    """ea_layernorm_param_reduce's split (layernorm.hip:766-776; the group's comes from its largest item) -> additions a value passes
    through: ceil(per / 4) in a thread, 3 in the block, one atomic per row split"""
    rs = min(max((largest or nblk) // 32, 1), 32)
    per = -(-nblk // rs)
    return -(-per // 4) + 3 + rs


def _rows_per_block(M, ws):
    if ws:
        return 8
    return max(4, -(-(-(-M // 512)) // 4) * 4)


def _param_chain(M, ws):
    rpb = _rows_per_block(M, ws)
    nblk = -(-M // rpb)
    chain = rpb // 4 + 4 + (_reduce_depth(nblk) if ws else nblk) + 4
    assert chain <= M + nblk + 16   # never wider than rows + partial rows + a small constant
    return chain


def _param_compare(what, ref, M, ws, dgamma, dbeta):
    chain = _param_chain(M, ws)
    for k, got in (("dgamma", dgamma), ("dbeta", dbeta)):
        tol = chain * E23 * ref[k + "_mag"]
        _sees_one_row(f"{what} {k}", tol, ref[k + "_mag"], M)
        _check(f"{what} {k}", got, ref[k], tol)


# ------------------------------------------------------------------ the reference against torch (CPU, no GPU needed)
def test_reference_matches_torch_in_float64():
    """tests/rowwise_ref.py == F.layer_norm and autograd in float64, within 1e-11 of every tensor's scale: row_zero, dropout, dx_add,
    pre-filled dgamma / dbeta, the second output, the pair; every `mag` equals the expression over absolute values"""
    g = _gen(11)
    M, C, eps = 7, 24, 1e-3
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x, gamma, beta, dy, add = rnd(M, C) + 3 * rnd(M, 1), rnd(C), rnd(C), rnd(M, C), rnd(M, C)
    rz = torch.tensor([1, 0, 0, 1, 0, 0, 1], dtype=torch.uint8)
    live = (1.0 - rz.double()).view(M, 1)
    for drop in (None, (77, 0.3)):
        kp = torch.ones(M, C, dtype=F64) if drop is None else R.keep(*drop, M, C)
        if drop is not None:
            flat = torch.from_numpy(R.dropout_ref.keep_mask(drop[0], M * C, drop[1])).view(M, C)
            assert torch.equal(kp != 0, flat) and 0 < int(flat.sum()) < M * C
            assert torch.equal(kp[kp != 0], torch.full_like(kp[kp != 0], R.drop_params(drop[1])[1]))
        for flags in (None, rz):
            lv = torch.ones(M, 1, dtype=F64) if flags is None else live
            xg, gg, bg = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
            y = TF.layer_norm(xg, (C,), gg, bg, R.f32_eps(eps)) * kp * lv
            f = R.ln_fwd(x, gamma, beta, eps, flags, drop)
            assert _close(f["y"], y.detach()) and _close(f["mean"], x.mean(1)) and _close(f["rstd"], 1 / torch.sqrt(x.var(1, unbiased=False) + R.f32_eps(eps)))
            assert _close(f["y_mag"], ((x - x.mean(1, keepdim=True)).abs() * f["rstd"].view(M, 1) * gamma.abs() + beta.abs()) * kp * lv)
            assert _close(f["absd"], (x - x.mean(1, keepdim=True)).abs()) and _close(f["a1"], x.abs().mean(1)) and _close(f["absmean"], x.mean(1).abs())
            (y * dy).sum().backward()
            dg0, db0 = rnd(C), rnd(C)
            b = R.ln_bwd(x, dy, gamma, f["mean"], f["rstd"], flags, drop, add, dg0, db0, out2=(0.5, (5, 0.5)))
            assert _close(b["dx"], xg.grad + add) and _close(b["dgamma"], dg0 + gg.grad) and _close(b["dbeta"], db0 + bg.grad)
            assert _close(b["dgamma_mag"], dg0.abs() + b["term_g"].abs().sum(0)) and _close(b["dbeta_mag"], db0.abs() + (dy * kp * lv).abs().sum(0))
            assert torch.equal(b["out2"], 0.5 * R.keep(5, 0.5, M, C) * b["dx"].float().to(BF).double())
            assert bool((b["dx_mag"] >= b["dx"].abs() * (1 - 1e-12)).all())
            part = R.ln_bwd(x, dy, gamma, f["mean"], f["rstd"], flags, drop, rows=[0, 2, 3, 4, 5, 6])
            assert _close(part["dgamma"] + b["term_g"][1], b["dgamma"] - dg0)
    assert torch.equal(R.keep(9, 0.4, M, C, shift=8).reshape(-1)[:-8], R.keep(9, 0.4, M, C).reshape(-1)[8:])
    # the pair: y1 = LN(x), y2 = LN(y1); the gradient arriving at y1 is dy1 through the next norm plus dx_add on the residual path
    g2, b2 = rnd(C), rnd(C)
    xg = x.clone().requires_grad_()
    y1 = TF.layer_norm(xg, (C,), gamma, beta, R.f32_eps(eps))
    y2 = TF.layer_norm(y1, (C,), g2, b2, R.f32_eps(eps))
    (y2 * dy).sum().backward(retain_graph=True)
    gx_through = xg.grad.clone()
    (gy1,) = torch.autograd.grad((y1 * add).sum(), xg)
    f1 = R.ln_fwd(x, gamma, beta, eps)
    f2 = R.ln_fwd(f1["y"], g2, b2, eps)
    p1, p2 = R.ln_bwd_pair(f1["y"], dy, g2, f2["mean"], f2["rstd"], add, x, gamma, f1["mean"], f1["rstd"], out2=(2.0, None), rnd=lambda t: t)
    assert _close(p2["dx"], gx_through + gy1) and torch.equal(p1["d"], p1["dx"]) and torch.equal(p2["out2"], 2.0 * R.bf16_rne(p2["dx"]))
    p1r, _ = R.ln_bwd_pair(f1["y"], dy, g2, f2["mean"], f2["rstd"], add, x, gamma, f1["mean"], f1["rstd"])
    assert torch.equal(p1r["d"], p1["dx"].float().to(BF).double())


# ------------------------------------------------------------------ cases
class Fwd:
    """one ea_layernorm_fwd / _fwd_f32out launch"""

    def __init__(self, M, C, f32=False, eps=1e-5, rz=False, p=0.0, no_mean=False, no_rstd=False):
        self.__dict__.update(M=M, C=C, f32=f32, eps=eps, rz=rz, p=p, no_mean=no_mean, no_rstd=no_rstd)

    def __repr__(self):
        return "Fwd(" + ", ".join(f"{k}={v!r}" for k, v in self.__dict__.items()) + ")"


def _seed_of(c):
    return 0x9E3779B97F4A7C15 ^ zlib.crc32(repr(c).encode())


def _fwd_plan(c):
    P = types.SimpleNamespace()
    g = _gen(zlib.crc32(repr(c).encode()))
    P.x = _rows(g, c.M, c.C)
    P.gamma, P.beta = _affine(g, c.C)
    P.rz = _flags(c.M, tail=True) if c.rz else None
    P.seed = _seed_of(c)
    P.drop = (P.seed, c.p) if c.p else None
    P.ref = R.ln_fwd(P.x, P.gamma, P.beta, c.eps, P.rz, P.drop)
    _fwd_preconditions(repr(c), P.ref, P.gamma, P.beta, c.C)
    return P


def run_fwd(lib, c):
    """lib = None: the CPU part alone"""
    P = _fwd_plan(c)
    if lib is None:
        return P
    M, C = c.M, c.C
    bx, bg, bb = inp(P.x), inp(P.gamma), inp(P.beta)
    by = out((M, C), F32 if c.f32 else BF)
    bm, br = (None if c.no_mean else out((M,), F32)), (None if c.no_rstd else out((M,), F32))
    hold, rzp = _dev_flags(P.rz) if c.rz else (None, None)
    thr, scale = R.drop_params(c.p) if c.p else (0, 1.0)
    fn = lib.ea_layernorm_fwd_f32out if c.f32 else lib.ea_layernorm_fwd
    rc = fn(bx.p, bg.p, bb.p, by.p, _ptr(bm), _ptr(br), M, C, c.eps, rzp, P.seed, thr, scale, _st())
    _sync()
    assert rc == 0, (c, rc)
    for b in (by, bm, br):
        assert b is None or b.intact(), (c, "stored outside the tensor")
    _fwd_compare(repr(c), P.ref, P.gamma, P.beta, C, by.cpu(), bm and bm.cpu(), br and br.cpu())
    return P


def _fwd_options(M, C, f32=False):
    return [Fwd(M, C, f32, rz=True), Fwd(M, C, f32, p=0.5), Fwd(M, C, f32, p=0.1), Fwd(M, C, f32, rz=True, p=0.1), Fwd(M, C, f32, no_mean=True),
            Fwd(M, C, f32, no_rstd=True), Fwd(M, C, f32, eps=1e-3), Fwd(M, C, f32, eps=1e-3, rz=True, p=0.5, no_mean=True, no_rstd=True)]


FWD_C = [8, 40, 504, 512, 520, 1024, 1032, 1536, 2048]
FWD_M = [1, 3, 4, 5, 37]
ROWS_C = [8, 504, 512]
ROWS_M = [2048, 2049, 2063]


def _takes_rows_kernel(M, C):
    """ea_layernorm_fwd's dispatch (layernorm.hip:656)"""
    return C <= 512 and M >= 2048


@gpu
@pytest.mark.parametrize("C", FWD_C)
def test_forward_single_row_kernel(lib, C):
    """ln_fwd_kernel<1, 2, 4>: one live lane, a ragged row, 63 lanes, full; lane 0 alone in the second chunk (520); an idle fourth
    chunk (1536); M = 1, 3, 4, 5, 37: less than a block, a whole block, one row into the second, ten blocks"""
    for M in FWD_M:
        assert not _takes_rows_kernel(M, C)
        run_fwd(lib, Fwd(M, C))
    for c in _fwd_options(37, C):
        run_fwd(lib, c)


@gpu
def test_forward_grid_stride_second_trip(lib):
    """M = 4101: 1026 blocks of four rows are clamped to 1024 (layernorm.hip:661-662), the first wavefronts walk a second row"""
    M = 4101
    assert (M + 3) // 4 > 1024 and ((M + 3) // 4 + 1) // 2 <= 1024
    run_fwd(lib, Fwd(M, 520))
    run_fwd(lib, Fwd(M, 520, rz=True, p=0.1))


@gpu
@pytest.mark.parametrize("C", ROWS_C)
def test_forward_rows_kernel(lib, C):
    """ln_fwd_rows_kernel<4> (C <= 512 and M >= 2048): M % 16 = 0, 1, 15 — the last wavefront's rows are clamped to M - 1, the flags
    with them (row M - 3 and row M - 1 flagged, M - 2 not)"""
    for M in ROWS_M:
        assert _takes_rows_kernel(M, C) and not _takes_rows_kernel(2047, C) and not _takes_rows_kernel(M, 520)
        run_fwd(lib, Fwd(M, C))
    for c in _fwd_options(2063, C):
        run_fwd(lib, c)
    run_fwd(lib, Fwd(2049, C, rz=True, p=0.5))


@gpu
@pytest.mark.parametrize("C", FWD_C)
def test_forward_fp32_output(lib, C):
    """ea_layernorm_fwd_f32out: the fp32 y against the fp32 bound alone, no bf16 step"""
    run_fwd(lib, Fwd(5, C, f32=True))
    run_fwd(lib, Fwd(5, C, f32=True, rz=True, p=0.1, eps=1e-3))


@gpu
def test_forward_fp32_output_grid_stride(lib):
    run_fwd(lib, Fwd(4101, 8, f32=True))
    run_fwd(lib, Fwd(4101, 8, f32=True, rz=True, p=0.5, no_rstd=True))


# ------------------------------------------------------------------ the forward pair
def _fwd2_plan(M, C):
    P = types.SimpleNamespace()
    g = _gen(1000 * M + C)
    P.x = _rows(g, M, C)
    P.g1, P.b1 = _affine(g, C)
    P.g2, P.b2 = _affine(g, C)
    P.g2, P.b2 = P.g2.flip(0).contiguous(), P.b2.flip(0).contiguous()   # (the second norm's chunk scales are not the first's)
    P.ref1 = R.ln_fwd(P.x, P.g1, P.b1, 1e-5)
    _fwd_preconditions(f"fwd2 {M} {C}", P.ref1, P.g1, P.b1, C)
    return P


def _call_fwd(lib, x, gamma, beta, M, C):
    by, bm, br = out((M, C), BF), out((M,), F32), out((M,), F32)
    bx, bg, bb = inp(x), inp(gamma), inp(beta)
    rc = lib.ea_layernorm_fwd(bx.p, bg.p, bb.p, by.p, bm.p, br.p, M, C, 1e-5, None, 0, 0, 1.0, _st())
    _sync()
    assert rc == 0 and by.intact() and bm.intact() and br.intact()
    return by.cpu(), bm.cpu(), br.cpu()


def run_fwd2(lib, M, C, singles=False):
    P = _fwd2_plan(M, C)
    if lib is None:
        return
    bx, b = inp(P.x), [inp(t) for t in (P.g1, P.b1, P.g2, P.b2)]
    y1, y2 = out((M, C), BF), out((M, C), BF)
    st = [out((M,), F32) for _ in range(4)]
    rc = lib.ea_layernorm_fwd2(bx.p, b[0].p, b[1].p, y1.p, st[0].p, st[1].p, b[2].p, b[3].p, y2.p, st[2].p, st[3].p, M, C, 1e-5, _st())
    _sync()
    assert rc == 0, (M, C, rc)
    for o in [y1, y2] + st:
        assert o.intact(), (M, C, "stored outside the tensor")
    tag = f"fwd2 {M} {C}"
    _fwd_compare(tag + " first", P.ref1, P.g1, P.b1, C, y1.cpu(), st[0].cpu(), st[1].cpu())
    ref2 = R.ln_fwd(y1.cpu(), P.g2, P.b2, 1e-5)   # the second norm starts from the rounded value the kernel stored
    _fwd_compare(tag + " second", ref2, P.g2, P.b2, C, y2.cpu(), st[2].cpu(), st[3].cpu())
    if singles:  # the header's promise: the same results as two ea_layernorm_fwd calls (the rows kernel: M >= 2048)
        assert _takes_rows_kernel(M, C)
        a = _call_fwd(lib, P.x, P.g1, P.b1, M, C)
        bb = _call_fwd(lib, a[0], P.g2, P.b2, M, C)
        for name, got, want in (("y1", y1, a[0]), ("mean1", st[0], a[1]), ("rstd1", st[1], a[2]), ("y2", y2, bb[0]), ("mean2", st[2], bb[1]), ("rstd2", st[3], bb[2])):
            _same_values(f"{tag} {name} against two launches", got.cpu(), want)


@gpu
@pytest.mark.parametrize("C", ROWS_C)
def test_forward_pair(lib, C):
    """ln_fwd2_rows_kernel<4>: M = 1, 15, 16, 17, 37 around the 16 rows of a block; the idle lanes of a narrow row are clamped"""
    for M in (1, 15, 16, 17, 37):
        run_fwd2(lib, M, C)


@gpu
@pytest.mark.parametrize("C", ROWS_C)
def test_forward_pair_equals_two_launches(lib, C):
    run_fwd2(lib, 2063, C, singles=True)


# ------------------------------------------------------------------ the backward
class Bwd:
    """one launch of ea_layernorm_bwd (api "bwd"), _bwd_f32dy ("f32dy"), _bwd_dx ("dx") or _bwd_dx2 ("dx2").  ws: with a workspace;
    opts: pre-filled dgamma / dbeta, dx_add, row_zero + dropout (the forward's mask); mask2: out2 with its own mask (dx2)"""

    def __init__(self, M, C, api="bwd", ws=True, opts=False, mask2=False):
        self.__dict__.update(M=M, C=C, api=api, ws=ws, opts=opts, mask2=mask2)

    def __repr__(self):
        return "Bwd(" + ", ".join(f"{k}={v!r}" for k, v in self.__dict__.items()) + ")"


def _away_from_zero(g, M, C):
    """+-[0.75, 1.25): a gradient whose elements are all of one magnitude, so that dx is not a difference of much larger terms"""
    return (0.75 + 0.5 * torch.rand(M, C, generator=g).double()) * (1 - 2 * torch.randint(0, 2, (M, C), generator=g).double())


def _bwd_plan(c):
    """the case's data and reference.  Cases with a second output are redrawn (salt 0, 1, ...) until the tie window of out2 touches at
    most 2 % of their elements — a property of the fp64 reference and the derived bound alone; a case of 40 elements allows none"""
    for salt in range(16):
        P = _bwd_draw(c, salt)
        if c.api != "dx2" or P.share <= TIE_CAP:
            break
    if c.api == "dx2":
        print(f"{c}: tie-window share {P.share:.5f} (salt {salt})")
        assert P.share <= TIE_CAP, (c, P.share)
    return P


def _bwd_draw(c, salt):
    M, C = c.M, c.C
    P = types.SimpleNamespace()
    g = _gen(zlib.crc32(repr(c).encode()) + salt)
    P.x = _rows(g, M, C, single=False)
    P.gamma, _ = _affine(g, C)
    dy = _row_scale(M, 1).view(M, 1) * _away_from_zero(g, M, C) / _chunk_scale(C)   # (g = dy gamma: one scale per row)
    P.dy = dy.float() if c.api == "f32dy" else dy.to(BF)
    f = R.ln_fwd(P.x, P.gamma, torch.zeros(C), 1e-5)
    P.mean, P.rstd = f["mean"].float(), f["rstd"].float()    # the kernel's inputs: the reference uses the same fp32 values
    P.seed = _seed_of(c)
    with_rz = c.opts and c.api != "dx2"   # (ea_layernorm_bwd_dx2 takes no row_zero / dropout)
    P.rz = _flags(M, tail=False) if with_rz else None
    P.drop = (P.seed, 0.1) if with_rz else None
    P.add = (_row_scale(M, 2).view(M, 1) * torch.randn(M, C, generator=g).double()).to(BF) if c.opts else None
    sc = _chunk_scale(C)
    P.dg0 = (sc * torch.randn(C, generator=g).double()).float() if c.opts else torch.zeros(C)
    P.db0 = (sc * torch.randn(C, generator=g).double()).float() if c.opts else torch.zeros(C)
    P.a2, P.drop2 = 0.5, ((P.seed ^ 0xABCDEF, 0.1) if c.mask2 else None)
    reduced = c.api in ("bwd", "f32dy")
    P.ref = R.ln_bwd(P.x, P.dy, P.gamma, P.mean, P.rstd, P.rz, P.drop, P.add, P.dg0 if reduced else None, P.db0 if reduced else None,
                     out2=(P.a2, P.drop2) if c.api == "dx2" else None)
    # preconditions: the parameter sums see one row; the fp32 window of dx is below 1/8 of a bf16 step of its magnitude
    chain = _param_chain(M, c.ws) if reduced else 10
    for k in ("dgamma", "dbeta"):
        _sees_one_row(f"{c} {k}", chain * E23 * P.ref[k + "_mag"], P.ref[k + "_mag"], M)
    assert bool((_dx_tol(P.ref, C) <= 2.0 ** -10 * P.ref["dx_mag"]).all())
    if c.api == "dx2":
        P.share = _out2_window(P.ref, C, P.a2)[2]
    return P


def _ws_elems(lib, M, C):
    n = lib.ea_layernorm_bwd_workspace_bytes(M, C)
    assert n == -(-M // 8) * 2 * C * 4
    return n // 4


def _check_workspace(what, ws, ref, M, C):
    """after _bwd_dx / _bwd_dx2 / _bwd2_dx: exactly ceil(M / 8) partial rows whose column sums are the reference's; the rest of the
    slab still holds the sentinel"""
    assert ws.intact(), (what, "stored outside the ceil(M / 8) partial rows")
    part = ws.cpu().double().view(-(-M // 8), 2, C)
    assert bool(torch.isfinite(part).all()), (what, "a partial row was not written")
    for i, k in enumerate(("dgamma", "dbeta")):
        _check(f"{what} workspace {k}", part[:, i].sum(0), ref[k], 10 * E23 * ref[k + "_mag"])


def run_bwd(lib, c):
    P = _bwd_plan(c)
    if lib is None:
        return P
    M, C = c.M, c.C
    bx, bdy, bg, bm, br = inp(P.x), inp(P.dy), inp(P.gamma), inp(P.mean), inp(P.rstd)
    badd = inp(P.add) if P.add is not None else None
    dx, dg, db = out((M, C), BF), out((C,), F32, P.dg0), out((C,), F32, P.db0)
    ws = out((_ws_elems(lib, M, C),), F32) if c.ws else None
    hold, rzp = _dev_flags(P.rz) if P.rz is not None else (None, None)
    thr, scale = R.drop_params(P.drop[1]) if P.drop else (0, 1.0)
    o2 = None
    if c.api == "dx2":
        o2 = out((M, C), BF)
        thr2, scale2 = R.drop_params(P.drop2[1]) if P.drop2 else (0, 1.0)
        rc = lib.ea_layernorm_bwd_dx2(bx.p, bdy.p, bg.p, bm.p, br.p, dx.p, dg.p, db.p, M, C, _ptr(badd), ws.p, o2.p, P.a2,
                                      P.drop2[0] if P.drop2 else 0, thr2, scale2, _st())
    else:
        fn = {"bwd": lib.ea_layernorm_bwd, "f32dy": lib.ea_layernorm_bwd_f32dy, "dx": lib.ea_layernorm_bwd_dx}[c.api]
        rc = fn(bx.p, bdy.p, bg.p, bm.p, br.p, dx.p, dg.p, db.p, M, C, rzp, P.seed, thr, scale, _ptr(badd), _ptr(ws), _st())
    _sync()
    assert rc == 0, (c, rc)
    for b in (dx, dg, db, o2):
        assert b is None or b.intact(), (c, "stored outside the tensor")
    tag = repr(c)
    _check_bf16(tag + " dx", dx.cpu(), P.ref["dx"], _dx_tol(P.ref, C))
    if c.api in ("bwd", "f32dy"):
        _param_compare(tag, P.ref, M, c.ws, dg.cpu(), db.cpu())
        if ws is not None:
            assert ws.intact()
    else:   # dx only: the parameter gradients are not this call's to write
        _same_values(tag + " dgamma untouched", dg.cpu(), P.dg0)
        _same_values(tag + " dbeta untouched", db.cpu(), P.db0)
        _check_workspace(tag, ws, P.ref, M, C)
    if o2 is not None:
        mid, tol, _ = _out2_window(P.ref, C, P.a2)
        _check(tag + " out2", o2.cpu(), mid, tol)
        own = P.a2 * P.ref["keep2"] * R.f64(dx.cpu())   # ... and from the dx the kernel stored: two fp32 roundings, one bf16
        _check_bf16(tag + " out2 from the stored dx", o2.cpu(), own, 2 * E23 * own.abs())
    return P


BWD_M = [1, 4, 5, 8, 9, 12, 13, 19]
BWD_C = [8, 40, 512, 520, 1032]
BWD_API = ["bwd", "f32dy", "dx", "dx2"]


@gpu
@pytest.mark.parametrize("C", BWD_C)
@pytest.mark.parametrize("api", BWD_API)
def test_backward_with_workspace(lib, api, C):
    """8 rows per block, two per wavefront (C <= 512: in flight together while `row + 4 < r1`): M = 1, 4, 5 (the second row of
    wavefront 0 alone), 8, 9, 12, 13, 19; plain, and with every option the entry point has"""
    for M in BWD_M:
        run_bwd(lib, Bwd(M, C, api))
        run_bwd(lib, Bwd(M, C, api, opts=True, mask2=True))
    if api == "dx2":
        run_bwd(lib, Bwd(19, C, api, opts=True, mask2=False))


ATOMIC = [(5, 8), (2049, 8), (4100, 8), (5, 1032)]


@gpu
@pytest.mark.parametrize("M,C", ATOMIC)
def test_backward_atomic_path(lib, M, C):
    """workspace == NULL: 4, 8 and 12 rows per block (ln_bwd_rows_per_block, layernorm.hip:692-698), one atomic per block and column"""
    assert _rows_per_block(M, False) == {5: 4, 2049: 8, 4100: 12}[M]
    run_bwd(lib, Bwd(M, C, "bwd", ws=False))
    run_bwd(lib, Bwd(M, C, "bwd", ws=False, opts=True))
    run_bwd(lib, Bwd(M, C, "f32dy", ws=False, opts=True))


# ------------------------------------------------------------------ the backward pair
def _pair_plan(M, C, mask2):
    """as _bwd_plan: redrawn until the tie window of out2 touches at most 2 % of the elements"""
    for salt in range(16):
        P = _pair_draw(M, C, mask2, salt)
        if P.share <= TIE_CAP:
            break
    print(f"pair M={M} C={C} mask2={mask2}: tie-window share {P.share:.5f} (salt {salt})")
    assert P.share <= TIE_CAP
    return P


def _pair_draw(M, C, mask2, salt):
    P = types.SimpleNamespace()
    g = _gen(77 * M + C + int(mask2) + 100003 * salt)
    P.x2 = _rows(g, M, C, single=False)         # the earlier norm's input
    P.g2, b2 = _affine(g, C)
    f2 = R.ln_fwd(P.x2, P.g2, b2, 1e-5)
    P.x1 = R.bf16_rne(f2["y"]).to(BF)           # the later norm's input: the earlier one's output
    P.g1, _ = _affine(g, C)
    P.g1 = P.g1.flip(0).contiguous()
    f1 = R.ln_fwd(P.x1, P.g1, torch.zeros(C), 1e-5)
    P.m1, P.s1, P.m2, P.s2 = f1["mean"].float(), f1["rstd"].float(), f2["mean"].float(), f2["rstd"].float()
    P.dy1 = (_row_scale(M, 1).view(M, 1) * _away_from_zero(g, M, C) / _chunk_scale(C).flip(0)).to(BF)
    # the residual-path gradient dominates d (the first stage's part is about 0.1 of the row's scale) and carries the inverse of the
    # second norm's chunk scale: g = d gamma2 is of one scale per row
    P.add = (32 * _row_scale(M, 1).view(M, 1) * _away_from_zero(g, M, C) / _chunk_scale(C)).to(BF)
    P.a2, P.drop2 = 0.5, ((0x1234567 + M * C, 0.1) if mask2 else None)
    P.ref1 = R.ln_bwd(P.x1, P.dy1, P.g1, P.m1, P.s1, dx_add=P.add)
    for k in ("dgamma", "dbeta"):
        _sees_one_row(f"pair {M} {C} {k}", 10 * E23 * P.ref1[k + "_mag"], P.ref1[k + "_mag"], M)
    # the CPU picture of the second stage (on the reference's own rounding of d): the tie-window share of out2
    _, p2 = R.ln_bwd_pair(P.x1, P.dy1, P.g1, P.m1, P.s1, P.add, P.x2, P.g2, P.m2, P.s2, out2=(P.a2, P.drop2))
    P.share = _out2_window(p2, C, P.a2)[2]
    return P


def run_pair(lib, M, C, mask2):
    P = _pair_plan(M, C, mask2)
    if lib is None:
        return
    n = _ws_elems(lib, M, C)
    ins = {k: inp(getattr(P, k)) for k in ("x1", "dy1", "g1", "m1", "s1", "add", "x2", "g2", "m2", "s2")}
    thr2, scale2 = R.drop_params(P.drop2[1]) if P.drop2 else (0, 1.0)
    seed2 = P.drop2[0] if P.drop2 else 0
    dummy = out((C,), F32, torch.zeros(C))
    tag = f"pair {M} {C} {mask2}"
    # the two launches
    d, wa1 = out((M, C), BF), out((n,), F32)
    rc = lib.ea_layernorm_bwd_dx(ins["x1"].p, ins["dy1"].p, ins["g1"].p, ins["m1"].p, ins["s1"].p, d.p, dummy.p, dummy.p, M, C, None, 0, 0, 1.0,
                                 ins["add"].p, wa1.p, _st())
    _sync()
    assert rc == 0 and d.intact()
    bd = inp(d.cpu())
    dxa, o2a, wa2 = out((M, C), BF), out((M, C), BF), out((n,), F32)
    rc = lib.ea_layernorm_bwd_dx2(ins["x2"].p, bd.p, ins["g2"].p, ins["m2"].p, ins["s2"].p, dxa.p, dummy.p, dummy.p, M, C, None, wa2.p, o2a.p,
                                  P.a2, seed2, thr2, scale2, _st())
    _sync()
    assert rc == 0 and dxa.intact() and o2a.intact()
    # stage by stage against fp64
    _check_bf16(tag + " d", d.cpu(), P.ref1["dx"], _dx_tol(P.ref1, C))
    _check_workspace(tag + " first norm", wa1, P.ref1, M, C)
    ref2 = R.ln_bwd(P.x2, d.cpu(), P.g2, P.m2, P.s2, out2=(P.a2, P.drop2))   # on the d the kernel stored
    _check_bf16(tag + " dx", dxa.cpu(), ref2["dx"], _dx_tol(ref2, C))
    _check_workspace(tag + " second norm", wa2, ref2, M, C)
    mid, tol, _ = _out2_window(ref2, C, P.a2)
    _check(tag + " out2", o2a.cpu(), mid, tol)
    # the one launch: bit for bit the same
    dxb, o2b, wb1, wb2 = out((M, C), BF), out((M, C), BF), out((n,), F32), out((n,), F32)
    rc = lib.ea_layernorm_bwd2_dx(ins["x1"].p, ins["dy1"].p, ins["g1"].p, ins["m1"].p, ins["s1"].p, ins["add"].p, wb1.p, ins["x2"].p, ins["g2"].p,
                                  ins["m2"].p, ins["s2"].p, wb2.p, dxb.p, M, C, o2b.p, P.a2, seed2, thr2, scale2, _st())
    _sync()
    assert rc == 0, (tag, rc)
    for b in (dxb, o2b, wb1, wb2):
        assert b.intact(), (tag, "stored outside the tensor")
    _same_values(tag + " dx against two launches", dxb.cpu(), dxa.cpu())
    _same_values(tag + " out2 against two launches", o2b.cpu(), o2a.cpu())
    _same_values(tag + " first workspace against two launches", wb1.cpu(), wa1.cpu())
    _same_values(tag + " second workspace against two launches", wb2.cpu(), wa2.cpu())
    _same_values(tag + " dgamma / dbeta untouched", dummy.cpu(), torch.zeros(C))
    # without the second output
    dxc, wc1, wc2 = out((M, C), BF), out((n,), F32), out((n,), F32)
    rc = lib.ea_layernorm_bwd2_dx(ins["x1"].p, ins["dy1"].p, ins["g1"].p, ins["m1"].p, ins["s1"].p, ins["add"].p, wc1.p, ins["x2"].p, ins["g2"].p,
                                  ins["m2"].p, ins["s2"].p, wc2.p, dxc.p, M, C, None, P.a2, seed2, thr2, scale2, _st())
    _sync()
    assert rc == 0 and dxc.intact()
    _same_values(tag + " dx without out2", dxc.cpu(), dxa.cpu())


PAIR_C = [8, 40, 504, 512]


@gpu
@pytest.mark.parametrize("C", PAIR_C)
def test_backward_pair(lib, C):
    """ln_bwd2_kernel: ea_layernorm_bwd2_dx == ea_layernorm_bwd_dx then ea_layernorm_bwd_dx2 bit for bit (dx, out2, both workspaces)
    at every M, and those two against fp64 stage by stage; out2 with and without its own mask"""
    for i, M in enumerate(BWD_M + [37]):
        run_pair(lib, M, C, mask2=bool(i % 2))


# ------------------------------------------------------------------ the parameter reduce
RED_C = [8, 40, 64, 512]
RED_M = [8, 504, 512, 520, 8192]   # 1, 63, 64, 65, 1024 partial rows


def _partials(g, nblk, C):
    """fp32 [nblk][2C]: row b at 16^(b % 3 - 1), the columns at their chunk's scale"""
    sc = torch.cat([_chunk_scale(C), _chunk_scale(C).flip(0)])
    return (_row_scale(nblk).view(nblk, 1) * sc * torch.randn(nblk, 2 * C, generator=g).double()).float()


def _reduce_ref(P, C):
    w = P.ws.double()
    P.dg, P.dg_mag = P.dg0.double() + w[:, :C].sum(0), P.dg0.double().abs() + w[:, :C].abs().sum(0)
    P.db, P.db_mag = P.db0.double() + w[:, C:].sum(0), P.db0.double().abs() + w[:, C:].abs().sum(0)


def _reduce_plan(M, C, seed=0):
    P = types.SimpleNamespace()
    g = _gen(31 * M + C + seed)
    P.nblk = -(-M // 8)
    P.ws = _partials(g, P.nblk, C)
    P.dg0, P.db0 = (_chunk_scale(C) * torch.randn(C, generator=g).double()).float(), torch.randn(C, generator=g)
    _reduce_ref(P, C)
    P.depth = _reduce_depth(P.nblk)
    for mag in (P.dg_mag, P.db_mag):
        _sees_one_row(f"reduce {M} {C}", P.depth * E23 * mag, mag, P.nblk + 1)
    return P


def _reduce_compare(tag, P, dg, db):
    _check(tag + " dgamma", dg, P.dg, P.depth * E23 * P.dg_mag)
    _check(tag + " dbeta", db, P.db, P.depth * E23 * P.db_mag)


@gpu
@pytest.mark.parametrize("C", RED_C)
def test_param_reduce(lib, C):
    """ea_layernorm_param_reduce: 2C = 16 and 80 columns are no whole 64-column block; 1, 63, 64 (rs = 2), 65 (per = 33) and 1024
    (rs at its cap of 32) partial rows; onto pre-filled gradients"""
    assert [_reduce_depth(n) for n in (1, 63, 64, 65, 1024)] == [5, 20, 13, 14, 43]
    for M in RED_M:
        P = _reduce_plan(M, C)
        if lib is None:
            continue
        ws, dg, db = inp(P.ws), out((C,), F32, P.dg0), out((C,), F32, P.db0)
        rc = lib.ea_layernorm_param_reduce(ws.p, dg.p, db.p, M, C, _st())
        _sync()
        assert rc == 0, (M, C, rc)
        assert dg.intact() and db.intact()
        _reduce_compare(f"reduce {M} {C}", P, dg.cpu(), db.cpu())


GROUP = [(8, 8), (520, 512), (37, 40), (0, 64), (8192, 8), (13, 512), (504, 64), (65, 40)]


def _group_struct():
    class Item(ctypes.Structure):
        _fields_ = [("workspace", ctypes.c_void_p), ("dgamma", ctypes.c_void_p), ("dbeta", ctypes.c_void_p), ("M", ctypes.c_int), ("C", ctypes.c_int)]

    class Group(ctypes.Structure):
        _fields_ = [("count", ctypes.c_int), ("item", Item * 8)]

    return Group


@gpu
def test_param_reduce_group(lib):
    """ea_layernorm_param_reduce_group: 8 items of mixed (M, C) in one grid sized by the largest (C = 8 next to C = 512, C = 40), an
    item with M = 0 that must be skipped; count = 0 and count = 9"""
    plans = [(_reduce_plan(M, C, seed=i) if M else None) for i, (M, C) in enumerate(GROUP)]
    if lib is None:
        return
    G = _group_struct()()
    G.count = len(GROUP)
    bufs = []
    for i, ((M, C), P) in enumerate(zip(GROUP, plans)):
        if P is None:
            ws, dg, db = None, out((C,), F32), out((C,), F32)
        else:
            ws, dg, db = inp(P.ws), out((C,), F32, P.dg0), out((C,), F32, P.db0)
        bufs.append((ws, dg, db))
        G.item[i].workspace, G.item[i].dgamma, G.item[i].dbeta = (ws.p.value if ws else None), dg.p.value, db.p.value
        G.item[i].M, G.item[i].C = M, C
    rc = lib.ea_layernorm_param_reduce_group(ctypes.byref(G), _st())
    _sync()
    assert rc == 0
    for (M, C), P, (ws, dg, db) in zip(GROUP, plans, bufs):
        if P is None:
            assert dg.untouched() and db.untouched(), "the item with M = 0 was written"
            continue
        assert dg.intact() and db.intact()
        P.depth = _reduce_depth(P.nblk, largest=max(-(-m // 8) for m, _ in GROUP))
        _reduce_compare(f"group item {M} {C}", P, dg.cpu(), db.cpu())
    G.count = 0
    assert lib.ea_layernorm_param_reduce_group(ctypes.byref(G), _st()) == 0
    G.count = 9
    assert lib.ea_layernorm_param_reduce_group(ctypes.byref(G), _st()) == -2
    _sync()
    for (M, C), P, (ws, dg, db) in zip(GROUP, plans, bufs):
        if P is not None:
            _reduce_compare(f"group item {M} {C} after the refused calls", P, dg.cpu(), db.cpu())


# ------------------------------------------------------------------ return codes
@gpu
def test_return_codes(lib):
    """arguments the library rejects before any launch: C % 8 != 0, C = 2056, the pairs with C = 520 or a NULL output / workspace /
    dx_add, _bwd_dx / _bwd_dx2 without a workspace; M = 0 returns 0; every output still holds NaN between intact guards"""
    M = 5
    Cs = 2056
    x, gam, st = inp(torch.zeros(M, Cs, dtype=BF)), inp(torch.ones(Cs)), inp(torch.ones(M))
    y, y2, yf = out((M, Cs), BF), out((M, Cs), BF), out((M, Cs), F32)
    o = [out((M,), F32) for _ in range(4)]
    dg, db, ws, ws2 = out((Cs,), F32), out((Cs,), F32), out((2 * Cs,), F32), out((2 * Cs,), F32)
    s = _st()
    L = lib
    fwd = lambda fn, yy, m, c: fn(x.p, gam.p, gam.p, yy.p, o[0].p, o[1].p, m, c, 1e-5, None, 0, 0, 1.0, s)
    bwd = lambda fn, m, c, w: fn(x.p, x.p, gam.p, st.p, st.p, y.p, dg.p, db.p, m, c, None, 0, 0, 1.0, None, w, s)
    bwd32 = lambda m, c, w: L.ea_layernorm_bwd_f32dy(x.p, yf.p, gam.p, st.p, st.p, y.p, dg.p, db.p, m, c, None, 0, 0, 1.0, None, w, s)
    dx2 = lambda m, c, w: L.ea_layernorm_bwd_dx2(x.p, x.p, gam.p, st.p, st.p, y.p, dg.p, db.p, m, c, None, w, y2.p, 1.0, 0, 0, 1.0, s)
    fwd2 = lambda m, c, a=y.p, b=y2.p, m1=o[0].p, r1=o[1].p, m2=o[2].p, r2=o[3].p: L.ea_layernorm_fwd2(x.p, gam.p, gam.p, a, m1, r1, gam.p, gam.p, b, m2, r2, m, c, 1e-5, s)
    bwd2 = lambda m, c, add=x.p, w1=ws.p, w2=ws2.p: L.ea_layernorm_bwd2_dx(x.p, x.p, gam.p, st.p, st.p, add, w1, x.p, gam.p, st.p, st.p, w2, y.p, m, c, y2.p, 1.0, 0, 0, 1.0, s)
    for C in (12, 2056):
        assert fwd(L.ea_layernorm_fwd, y, M, C) == -2 and fwd(L.ea_layernorm_fwd_f32out, yf, M, C) == -2
        for w in (ws.p, None):
            assert bwd(L.ea_layernorm_bwd, M, C, w) == -2 and bwd32(M, C, w) == -2
        assert bwd(L.ea_layernorm_bwd_dx, M, C, ws.p) == -2 and dx2(M, C, ws.p) == -2
    for C in (12, 520):
        assert fwd2(M, C) == -2 and bwd2(M, C) == -2
    assert fwd2(M, 512, a=None) == -2 and fwd2(M, 512, b=None) == -2
    for k in ("m1", "r1", "m2", "r2"):
        assert fwd2(M, 512, **{k: None}) == -2
    assert bwd2(M, 512, add=None) == -2 and bwd2(M, 512, w1=None) == -2 and bwd2(M, 512, w2=None) == -2
    assert bwd(L.ea_layernorm_bwd_dx, M, 512, None) == -2 and dx2(M, 512, None) == -2
    for m in (0, -3):
        assert fwd(L.ea_layernorm_fwd, y, m, 512) == 0 and fwd(L.ea_layernorm_fwd_f32out, yf, m, 512) == 0 and fwd2(m, 512) == 0
        assert bwd(L.ea_layernorm_bwd, m, 512, ws.p) == 0 and bwd(L.ea_layernorm_bwd, m, 512, None) == 0 and bwd32(m, 512, ws.p) == 0
        assert bwd(L.ea_layernorm_bwd_dx, m, 512, ws.p) == 0 and dx2(m, 512, ws.p) == 0 and bwd2(m, 512) == 0
        assert L.ea_layernorm_param_reduce(ws.p, dg.p, db.p, m, 512, s) == 0
    _sync()
    for b in [y, y2, yf, dg, db, ws, ws2] + o:
        assert b.untouched(), "a refused call wrote to an output"


# ------------------------------------------------------------------ mutations of the reference (CPU, no GPU needed)
def _fails(fn):
    with pytest.raises(AssertionError):
        fn()


def _as_stored(ref, dtype=BF):
    return R.bf16_rne(ref).to(BF) if dtype == BF else ref.float()


@pytest.mark.parametrize("case", [Fwd(37, 520), Fwd(37, 40, rz=True, p=0.1), Fwd(2063, 504, p=0.5), Fwd(5, 1536, f32=True), Fwd(2049, 8, rz=True)], ids=repr)
def test_forward_bounds_see_the_faults_they_are_for(case):
    """A correct output must fall outside the bound of a reference in which one 8-column chunk comes from the neighbouring row, one
    chunk's gamma is shifted by 8 columns, row M - 2 is computed from row M - 1's data (the clamped tail of the rows kernel) or the
    mask is drawn at the index m C + c + 8"""
    c = case
    P = _fwd_plan(c)
    M, C = c.M, c.C
    dt = F32 if c.f32 else BF
    y, mean, rstd = _as_stored(P.ref["y"], dt), P.ref["mean"].float(), P.ref["rstd"].float()
    cmp = lambda ref, ga=P.gamma: _fwd_compare(repr(c), ref, ga, P.beta, C, y, mean, rstd)
    cmp(P.ref)   # the check passes what is right
    # one chunk from the neighbouring row (the same columns: the neighbour's data and statistics, this row's flag and mask)
    r, c0 = M // 2 + 1, (C // 8 // 2) * 8
    xs = P.x.clone()
    xs[r] = P.x[r - 1]
    shifted = R.ln_fwd(xs, P.gamma, P.beta, c.eps, P.rz, P.drop)
    ref = {k: v.clone() for k, v in P.ref.items()}
    for k in ("y", "y_mag", "absd"):
        ref[k][r, c0:c0 + 8] = shifted[k][r, c0:c0 + 8]
    _fails(lambda: _fwd_compare(repr(c), ref, P.gamma, P.beta, C, y, None, None))
    if C >= 24:
        g2 = P.gamma.clone()
        g2[8:16] = P.gamma[16:24]
        _fails(lambda: _fwd_compare(repr(c), R.ln_fwd(P.x, g2, P.beta, c.eps, P.rz, P.drop), g2, P.beta, C, y, None, None))
    xs = P.x.clone()
    xs[M - 2] = P.x[M - 1]   # (row M - 2 is never flagged)
    tail = R.ln_fwd(xs, P.gamma, P.beta, c.eps, P.rz, P.drop)
    _fails(lambda: _fwd_compare(repr(c), tail, P.gamma, P.beta, C, y, None, None))
    _fails(lambda: _fwd_compare(repr(c), tail, P.gamma, P.beta, C, _as_stored(tail["y"], dt), mean, None))
    _fails(lambda: _fwd_compare(repr(c), tail, P.gamma, P.beta, C, _as_stored(tail["y"], dt), None, rstd))
    if c.p:
        _fails(lambda: cmp(R.ln_fwd(P.x, P.gamma, P.beta, c.eps, P.rz, P.drop, drop_shift=8)))


@pytest.mark.parametrize("case", [Bwd(19, 40, "bwd", opts=True), Bwd(13, 520, "f32dy"), Bwd(4100, 8, "bwd", ws=False), Bwd(9, 512, "dx2", opts=True, mask2=True)], ids=repr)
def test_backward_bounds_see_the_faults_they_are_for(case):
    """... one row left out of dgamma / dbeta, one chunk of dx from the neighbouring row, out2's mask drawn 8 elements off"""
    c = case
    P = _bwd_plan(c)
    M, C = c.M, c.C
    dx, dg, db = _as_stored(P.ref["dx"]), P.ref["dgamma"].float(), P.ref["dbeta"].float()
    _check_bf16("dx", dx, P.ref["dx"], _dx_tol(P.ref, C))
    _param_compare("unperturbed", P.ref, M, c.ws, dg, db)
    reduced = c.api in ("bwd", "f32dy")
    live = [m for m in range(M) if P.rz is None or not int(P.rz[m])]
    left_out = live[len(live) // 2]
    part = R.ln_bwd(P.x, P.dy, P.gamma, P.mean, P.rstd, P.rz, P.drop, P.add, P.dg0 if reduced else None, P.db0 if reduced else None,
                    rows=[m for m in range(M) if m != left_out])
    _fails(lambda: _param_compare("one row left out", part, M, c.ws, dg, part["dbeta"].float()))
    _fails(lambda: _param_compare("one row left out", part, M, c.ws, part["dgamma"].float(), db))
    if M >= 9:
        r, c0 = M // 2, (C // 8 // 2) * 8
        ref = {k: P.ref[k].clone() for k in ("dx", "dx_mag")}
        for k in ref:
            ref[k][r, c0:c0 + 8] = P.ref[k][r + 1, c0:c0 + 8]
        _fails(lambda: _check_bf16("dx", dx, ref["dx"], _dx_tol(ref, C)))
    if c.api == "dx2":
        o2 = _as_stored(P.ref["out2"])
        mid, tol, _ = _out2_window(P.ref, C, P.a2)
        _check("out2", o2, mid, tol)
        ref = dict(P.ref, keep2=R.keep(P.drop2[0], P.drop2[1], M, C, shift=8))
        mid, tol, _ = _out2_window(ref, C, P.a2)
        _fails(lambda: _check("out2", o2, mid, tol))


@pytest.mark.parametrize("M,C", [(8, 40), (520, 40), (8, 8), (8192, 512), (504, 64)])
def test_reduce_bounds_see_the_faults_they_are_for(M, C):
    """... the last column block left out of the reduce (what a grid of `2 * C / 64` column blocks did at C = 40: dbeta[24:] kept its
    pre-fill; at C = 8 nothing was added at all), one workspace row left out"""
    P = _reduce_plan(M, C)
    dg, db = P.dg.float(), P.db.float()
    _reduce_compare("unperturbed", P, dg, db)
    if (2 * C) % 64:
        done = 2 * C // 64 * 64
        stale = torch.cat([torch.cat([dg, db])[:done], torch.cat([P.dg0, P.db0])[done:]])
        _fails(lambda: _reduce_compare("last column block left out", P, stale[:C], stale[C:]))
    Q = _reduce_plan(M, C)
    Q.ws[Q.nblk // 2] = 0
    _reduce_ref(Q, C)
    _fails(lambda: _reduce_compare("one workspace row left out", Q, dg, Q.db.float()))
    _fails(lambda: _reduce_compare("one workspace row left out", Q, Q.dg.float(), db))


# ------------------------------------------------------------------ every GPU case on the CPU first
_GPU_TESTS = {
    "test_forward_single_row_kernel": [(C,) for C in FWD_C],
    "test_forward_grid_stride_second_trip": [()],
    "test_forward_rows_kernel": [(C,) for C in ROWS_C],
    "test_forward_fp32_output": [(C,) for C in FWD_C],
    "test_forward_fp32_output_grid_stride": [()],
    "test_forward_pair": [(C,) for C in ROWS_C],
    "test_forward_pair_equals_two_launches": [(C,) for C in ROWS_C],
    "test_backward_with_workspace": [(a, C) for a in BWD_API for C in BWD_C],
    "test_backward_atomic_path": ATOMIC,
    "test_backward_pair": [(C,) for C in PAIR_C],
    "test_param_reduce": [(C,) for C in RED_C],
    "test_param_reduce_group": [()],
}


@pytest.mark.parametrize("name,args", [(n, a) for n in sorted(_GPU_TESTS) for a in _GPU_TESTS[n]], ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_every_case_on_the_cpu_first(name, args):
    """Every case of every GPU test, built without a GPU (lib = None: data, memory images, the fp64 reference, no launch): every sum's
    bound below one row's share, the fp32 part of y's bound below 1/64 of a chunk's scale, dx's below 1/8 of a bf16 step of its
    magnitude, at most 2 % of a case's out2 elements loosened by the tie window"""
    globals()[name](None, *args)


def test_the_cpu_table_lists_every_gpu_test():
    mine = {k for k, f in globals().items() if k.startswith("test_") and callable(f) and any(m.name == "gpu" for m in getattr(f, "pytestmark", []))}
    assert mine - set(_GPU_TESTS) == {"test_return_codes"} and set(_GPU_TESTS) <= mine
