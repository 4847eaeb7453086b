"""The Conformer conv-module kernels (espresso_amd/csrc/convmodule.hip: GLU + depthwise conv, BatchNorm + activation, their
backward passes and the depthwise weight gradient) one kernel at a time against the plain fp64 restatement in
tests/convmodule_ref.py, through the C ABI.

Every device tensor a kernel sees is a view into a larger allocation with 2*TTILE guard rows on both sides: NaN around inputs (a
row consumed outside [0, B*T) poisons the output), a sentinel bit pattern around outputs (checked afterwards), NaN inside outputs
(a missed store is a failure, not a stale match).  Utterances are drawn at different scales, so a halo that reaches into the
neighbouring utterance moves the result by far more than any bound here.

The bounds are derived from the arithmetic, none is measured (ulp(x) = the bf16 step at |x|, tests.gpu_checks._bf_ulp_ok's):
  U          vs fp64 on Y                        ulp(ref)                                    one bf16 store
  Z          vs fp64 on the kernel's U           ulp(ref) + KW 2^-23 sum_k |w u|             fp32 sum of KW products
  stats      vs fp64 on the kernel's Z           2^-18 sum |z|, 2^-18 sum z^2                <= 20 fp32 additions, then fp64 atomics
  mean, rstd, running stats vs fp64 on stats     8 * 2^-23 relative                          a handful of fp32 roundings, rsqrtf
  H          vs fp64 on Z, the kernel's mean/rstd  ulp(ref) + 2^-20 (|z sc| + |sh|)          v_exp / v_rcp: 2^-20 on their term
  red, dgamma, dbeta                             (M 2^-24 + 2^-20) sum |term|                fp32 sum of M terms
  dZ         (with the kernel's own red)         ulp(ref) + 2^-20 rstd |gamma| (|dy| + |r0| + |xhat r1|)
  dY         vs fp64 on dZ, Y                    ulp(ref) + KW 2^-23 sum_k |w dz| * (GLU factor)
  dw         vs fp64 on dZ, the kernel's U       B T 2^-24 sum |dz u|                        fp32 sum of B*T products
Every sum's bound is also asserted to be below what one dropped or duplicated row would contribute (sum |term| / M).  No element
is excluded from any comparison.

In dZ's bound, |dy| is |dH| times the magnitude sum of the derivative's own terms: the sigmoid enters SiLU's derivative
sg + y sg (1 - sg) in two terms, which cancel around y = -1.28 where the derivative crosses zero, and 2^-20 on the terms the
transcendental enters is 2^-20 (sg + |y sg (1 - sg)|) there, not 2^-20 of their difference.  (Identity, ReLU and SiLU at y >= 0:
the same as |dy|.)  With 2^-20 |dy| read as the rounded derivative itself, eval-mode SiLU misses at the one or two elements per
case that sit on the zero crossing — (45, 520): got -8.754e-08, fp64 -9.516e-08, bound 4.7e-10; (2051, 256): got -1.7695e-07,
fp64 -1.7566e-07, bound 9.3e-10 — which is fp32's own rounding of 1 + y (1 - sg), a sum of terms near 1 whose result is near 0.

The first test needs no GPU: it proves the reference itself against torch's own operators in float64."""
import ctypes
import hashlib
import math

import pytest
import torch
import torch.nn.functional as F

from tests import convmodule_ref as R
from tests import gpu_checks as G

gpu = pytest.mark.gpu
DEV = "cuda:0"
TTILE = 64
GUARD = 2 * TTILE
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
_INT = {BF: torch.int16, F32: torch.int32, F64: torch.int64}
_SENTINEL = {BF: 0x5AA5, F32: 0x5AA55AA5, F64: 0x5AA55AA55AA55AA5}
EPS, MOM = 1e-5, 0.1
KWS = [3, 7, 15, 31]


# ------------------------------------------------------------------ the reference against torch's operators (CPU, no GPU needed)
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("T", [1, 5, 65])
@pytest.mark.parametrize("KW", KWS)
def test_reference_matches_torch_operators_in_float64(KW, T, training):
    """tests/convmodule_ref.py == F.glu -> F.conv1d(groups=C, padding=PAD) -> F.batch_norm -> identity / relu / silu in float64,
    forward values, running statistics and every autograd gradient, within 1e-11 of each tensor's scale"""
    B, C = 2, 6
    M, PAD = B * T, R.pad_of(KW)
    g = torch.Generator().manual_seed(100 * KW + T)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-11 * float(b.abs().max())
    for act in (0, 1, 2):
        Y = rnd(B, T, 2 * C).requires_grad_()
        w, gamma, beta = rnd(C, KW).requires_grad_(), (1 + 0.3 * rnd(C)).requires_grad_(), rnd(C).requires_grad_()
        rm, rv, dH = rnd(C), 0.5 + torch.rand(C, generator=g, dtype=F64), rnd(M, C)
        U = F.glu(Y, -1)
        Z = F.conv1d(U.transpose(1, 2), w[:, None, :], groups=C, padding=PAD).transpose(1, 2)
        U.retain_grad(), Z.retain_grad()
        rm_t, rv_t = rm.clone(), rv.clone()
        Hn = F.batch_norm(Z.reshape(M, C), rm_t, rv_t, gamma, beta, training, MOM, EPS)
        H = F.silu(Hn) if act == 2 else (F.relu(Hn) if act == 1 else Hn)
        (H * dH).sum().backward()

        Y2 = Y.detach().reshape(M, 2 * C)
        Ur = R.glu(Y2)
        Zr, _ = R.dwconv(Ur, w, B, T, KW)
        s, q, _ = R.bn_stats(Zr)
        if training:
            mean, rstd, rmn, rvn = R.bn_finalize(s, q, M, EPS, MOM, rm, rv)
            assert close(rmn, rm_t) and close(rvn, rv_t), (act, "running statistics")
        else:
            mean, rstd = rm, 1.0 / torch.sqrt(rv + EPS)
        Hr, _ = R.bn_act(Zr, mean, rstd, gamma, beta, act)
        bw = R.bn_act_bwd(Zr, dH, mean, rstd, gamma, beta, act, training)
        dYr, _ = R.glu_dwconv_bwd(bw["dZ"], Y2, w, B, T, KW)
        dwr, _ = R.dwconv_wgrad(bw["dZ"], Ur, B, T, KW)
        for name, got, want in (("U", Ur, U.detach().reshape(M, C)), ("Z", Zr, Z.detach().reshape(M, C)), ("H", Hr, H.detach()),
                                ("dZ", bw["dZ"], Z.grad.reshape(M, C)), ("dY", dYr, Y.grad.reshape(M, 2 * C)), ("dw", dwr, w.grad),
                                ("dgamma", bw["sum_dy_xhat"], gamma.grad), ("dbeta", bw["sum_dy"], beta.grad)):
            assert close(got, want), (act, name, float((got - want).abs().max()), float(want.abs().max()))


# ------------------------------------------------------------------ buffers and comparisons
@pytest.fixture
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from espresso_amd import _lib

    return _lib.lib()  # the HIP library is the thing under test: a missing one is an error, not a skip


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """A device tensor as a view into a larger allocation: GUARD rows before and after it.  Inputs: NaN guards.  Outputs: guards
    hold a sentinel bit pattern (`intact()`), the tensor itself starts as NaN unless `data` says what it accumulates onto."""

    def __init__(self, shape, dtype, data=None, out=False):
        shape = tuple(shape)
        width = math.prod(shape[1:])
        self.n, self.g, self.dtype, self.out = shape[0] * width, GUARD * width, dtype, out
        self.full = torch.empty(self.n + 2 * self.g, dtype=dtype, device=DEV)
        if out:
            self.full.view(_INT[dtype]).fill_(_SENTINEL[dtype])
        else:
            self.full.fill_(float("nan"))
        inner = self.full[self.g:self.g + self.n]
        if data is None:
            inner.fill_(float("nan"))
        else:
            inner.copy_(data.reshape(-1).to(dtype))
        self.t = inner.view(shape)

    @property
    def p(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def intact(self):
        v = self.full.view(_INT[self.dtype])
        s = _SENTINEL[self.dtype]
        return self.out and bool((v[:self.g] == s).all()) and bool((v[self.g + self.n:] == s).all())

    def untouched(self):  # an output nobody wrote: still all NaN, guards intact
        return self.intact() and bool(torch.isnan(self.t).all())

    def cpu(self):
        return self.t.detach().cpu()

    def bits(self):
        return self.t.view(_INT[self.dtype]).cpu()


def inp(data):
    return Buf(data.shape, data.dtype, data)


def out(shape, dtype, data=None):
    return Buf(shape, dtype, data, out=True)


def _ulp(ref):
    """the bf16 step at |ref| (the definition in tests.gpu_checks._bf_ulp_ok)"""
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -60))) - 7)


def _check(what, got, ref, tol):
    """|got - ref| <= tol for EVERY element (NaN / inf in `got` fail); prints the worst ratio, names the worst element"""
    got = R.f64(got).to(ref.device)
    tol = tol.to(ref.device).expand_as(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.numel() == 0:
        return
    finite = torch.isfinite(got)
    assert bool(finite.all()), f"{what}: {int((~finite).sum())} non-finite elements, first at {tuple(int(i) for i in (~finite).nonzero()[0])}"
    diff = (got - ref).abs()
    i = int((diff - tol).argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
    g_, r_, t_ = float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(tol.reshape(-1)[i])
    print(f"{what}: worst element {idx}: got {g_!r} ref {r_!r} |diff| {abs(g_ - r_):.3e} tol {t_:.3e}")
    assert bool((diff <= tol).all()), f"{what}: {int((diff > tol).sum())} elements outside the bound, worst at {idx}: got {g_!r}, ref {r_!r}, tol {t_:.3e}"


def _check_bf16(what, got, ref, extra=None):
    """a bf16 output against the fp64 value it should be the rounding of: ulp(ref) + extra"""
    extra = torch.zeros_like(ref) if extra is None else extra
    _check(what, got, ref, _ulp(ref) + extra)
    assert G._bf_ulp_ok(got, ref, ulps=1.0, atol=extra.cpu()), what


def _check_rel(what, got, ref, rel):
    _check(what, got, ref, rel * ref.abs())


def _sees_one_row(what, tol, mag, M):
    """the bound of a sum over M rows must stay below one average row's contribution: a dropped or duplicated row shows"""
    tol, mag = tol.expand_as(mag), mag
    nz = mag > 0
    assert bool((tol[nz] < mag[nz] / M).all()), f"{what}: the bound has grown too loose to see one missing row of {M}"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _utts(g, B, T, W):
    """[B*T][W] bf16, utterance b drawn at its own scale in [0.5, 2)"""
    scale = torch.tensor([0.5 * 4.0 ** ((0.618 * b) % 1.0) for b in range(B)]).view(B, 1, 1)
    return (torch.randn(B, T, W, generator=g) * scale).to(BF).reshape(B * T, W)


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------ GLU + depthwise conv: forward, data gradient, weight gradient
def _nslab(B, T):
    nt = (T + TTILE - 1) // TTILE
    return B * ((nt + 1) // 2)


def _conv_case(lib, B, T, C, KW, seed=0, dw_prefill=False):
    M = B * T
    g = _gen(seed + 1000 * KW + T)
    Y, w = _utts(g, B, T, 2 * C), (torch.randn(C, KW, generator=g) / math.sqrt(KW)).float()
    bY, bw = inp(Y), inp(w)
    # ---- forward, with statistics
    bU, bZ, bst = out((M, C), BF), out((M, C), BF), out((2 * C,), F64, torch.zeros(2 * C, dtype=F64))
    assert lib.ea_glu_dwconv_fwd(bY.p, bw.p, bU.p, bZ.p, bst.p, B, T, C, KW, _st()) == 0
    _sync()
    assert bU.intact() and bZ.intact() and bst.intact()
    U, Z, stats = bU.cpu(), bZ.cpu(), bst.cpu()
    _check_bf16("U", U, R.glu(Y))
    Zr, zmag = R.dwconv(U, w, B, T, KW)
    _check_bf16("Z", Z, Zr, KW * 2.0 ** -23 * zmag)
    s, q, sabs = R.bn_stats(Z)
    _check("stats.sum", stats[:C], s, 2.0 ** -18 * sabs)
    _check("stats.sumsq", stats[C:], q, 2.0 ** -18 * q)
    _sees_one_row("stats.sum", 2.0 ** -18 * sabs, sabs, M)
    _sees_one_row("stats.sumsq", 2.0 ** -18 * q, q, M)
    # ---- forward without statistics (eval): same U and Z, bit for bit
    bU2, bZ2 = out((M, C), BF), out((M, C), BF)
    assert lib.ea_glu_dwconv_fwd(bY.p, bw.p, bU2.p, bZ2.p, None, B, T, C, KW, _st()) == 0
    _sync()
    assert bU2.intact() and bZ2.intact()
    assert torch.equal(bU2.bits(), bU.bits()) and torch.equal(bZ2.bits(), bZ.bits()), "stats = NULL changed U or Z"
    # ---- backward: data gradient and weight gradient in one call
    dZ = _utts(g, B, T, C)
    dw0 = torch.randn(C, KW, generator=g).float() if dw_prefill else torch.zeros(C, KW)
    nws = lib.ea_dwconv_wgrad_workspace_bytes(B, T, C, KW) // 4
    assert nws == _nslab(B, T) * C * KW
    bdZ, bUi = inp(dZ), inp(U)
    bdY, bdw, bws = out((M, 2 * C), BF), out((C, KW), F32, dw0), out((nws,), F32)
    assert lib.ea_glu_dwconv_bwd(bdZ.p, bY.p, bUi.p, bw.p, bdY.p, bdw.p, bws.p, B, T, C, KW, _st()) == 0
    _sync()
    assert bdY.intact() and bdw.intact() and bws.intact()
    dYr, dymag = R.glu_dwconv_bwd(dZ, Y, w, B, T, KW)
    _check_bf16("dY", bdY.cpu(), dYr, KW * 2.0 ** -23 * dymag)
    dwr, dwmag = R.dwconv_wgrad(dZ, U, B, T, KW)
    tol = M * 2.0 ** -24 * dwmag
    _check("dw", bdw.cpu(), dw0.double() + dwr, tol)
    _sees_one_row("dw", tol, dwmag, M)
    # ---- the engine's call pattern: data gradient alone (dw = NULL), weight gradient on its own
    bdY2, bdw2, bws2 = out((M, 2 * C), BF), out((C, KW), F32, dw0), out((nws,), F32)
    assert lib.ea_glu_dwconv_bwd(bdZ.p, bY.p, None, bw.p, bdY2.p, None, None, B, T, C, KW, _st()) == 0
    assert lib.ea_dwconv_bwd_weight(bdZ.p, bUi.p, bdw2.p, bws2.p, B, T, C, KW, _st()) == 0
    _sync()
    assert bdY2.intact() and bdw2.intact() and bws2.intact()
    assert torch.equal(bdY2.bits(), bdY.bits()), "dY differs between the combined and the data-only call"
    if _nslab(B, T) < 16:  # (from 16 slabs on, eight slab groups meet in fp32 atomics: the order of the additions is free)
        assert torch.equal(bdw2.bits(), bdw.bits()), "dw differs between the combined call and ea_dwconv_bwd_weight"
    else:
        _check("dw (separate call)", bdw2.cpu(), dw0.double() + dwr, tol)
    return bdw


@gpu
@pytest.mark.parametrize("C", [64, 128, 72, 66])  # one full tile, two, full + ragged 16-byte chunk, C % 8 != 0 (scalar loads everywhere)
@pytest.mark.parametrize("KW", KWS)
def test_glu_dwconv_every_filter_width_and_channel_tile(lib, KW, C):
    _conv_case(lib, 3, 129, C, KW)  # three time tiles: the last weight-gradient block holds one; 6 slabs: the `+=` reduce


@gpu
@pytest.mark.parametrize("C,KW", [(64, 31), (72, 31), (66, 7)])
@pytest.mark.parametrize("T", [1, 5, 14, 15, 16, 63, 64, 65, 128])  # below the halo, around it, TTILE -1 / +0 / +1, two full tiles
def test_glu_dwconv_time_tile_edges(lib, T, C, KW):
    _conv_case(lib, 2, T, C, KW, seed=7)


@gpu
def test_dwconv_weight_gradient_accumulates_onto_dw(lib):
    """dw pre-filled with random values: the gradient is added (B = 3, T = 129: one slab group, the `+=` branch of the reduce)"""
    _conv_case(lib, 3, 129, 72, 15, seed=3, dw_prefill=True)


@gpu
def test_dwconv_weight_gradient_sixteen_slabs_atomic_reduce(lib):
    """B = 8, T = 129: 16 slabs, so eight slab groups add atomically — onto a pre-filled dw as well"""
    assert _nslab(8, 129) == 16
    _conv_case(lib, 8, 129, 72, 7, seed=4)
    _conv_case(lib, 8, 129, 64, 31, seed=5, dw_prefill=True)


def _bits_input(n, seed):
    """n bf16 values +-k * 2^(e - 9) with odd k in [129, 255] (all eight significand bits in use) and e in 0..4 (five binades), from
    integer arithmetic alone (no random generator whose stream could change).  A product of two of them needs 16 bits and the
    products sit in nine binades, so fp32 partial sums of a few hundred of them round: their bits depend on the order of addition."""
    i = torch.arange(n, dtype=torch.int64)
    h = (i * (1103515245 + 81006 * seed) + seed * 12345 + (i >> 7) * 2654435761) >> 8
    k = 129 + 2 * (h % 64)
    sign = 1 - 2 * ((h >> 7) % 2)
    e = (h >> 11) % 5
    return (sign * k).double().mul(torch.exp2((e - 9).double())).to(BF)


# sha256 of dw (fp32 [72][31], onto zeros) for the case below, recorded from the kernel as it stood BEFORE the tap-group guard went
# into dwconv_bwd_weight_kernel (groups with grp*8 >= KW used to read their window past sU's rows): KW = 31 must not move a bit.
# The exact sums of this data are not fp32 numbers (asserted below), so the digest belongs to this kernel's order of additions.
_DW_KW31_SHA256 = "74b53bcbc5180b3b9311737425a75873026f2c588601441e56e1f2530b93ef90"


@gpu
def test_dwconv_weight_gradient_kw31_bits_unchanged(lib):
    B, T, C, KW = 3, 129, 72, 31
    dZ, U = _bits_input(B * T * C, 1).view(B * T, C), _bits_input(B * T * C, 2).view(B * T, C)
    nws = lib.ea_dwconv_wgrad_workspace_bytes(B, T, C, KW) // 4
    bdZ, bU, bdw, bws = inp(dZ), inp(U), out((C, KW), F32, torch.zeros(C, KW)), out((nws,), F32)
    assert lib.ea_dwconv_bwd_weight(bdZ.p, bU.p, bdw.p, bws.p, B, T, C, KW, _st()) == 0
    _sync()
    assert bdw.intact() and bws.intact()
    dwr, dwmag = R.dwconv_wgrad(dZ, U, B, T, KW)
    _check("dw", bdw.cpu(), dwr, B * T * 2.0 ** -24 * dwmag)
    inexact = dwr.float().double() != dwr
    print("elements of the exact dw that fp32 cannot hold:", int(inexact.sum()), "of", dwr.numel())
    assert int(inexact.sum()) > dwr.numel() // 4 and not torch.equal(bdw.cpu().double(), dwr)  # the digest is not the exact result's
    digest = hashlib.sha256(bdw.cpu().contiguous().numpy().tobytes()).hexdigest()
    print("dw sha256:", digest)
    assert digest == _DW_KW31_SHA256


@gpu
def test_glu_dwconv_return_codes(lib):
    """odd C and an uninstantiated KW are refused (-2), an empty batch is a no-op (0): nothing is written either way"""
    B, T, C, KW = 2, 5, 64, 7
    g = _gen(11)
    bY, bw, bdZ = inp(_utts(g, B, T, 2 * (C + 2))), inp(torch.randn(C + 2, 8, generator=g)), inp(_utts(g, B, T, C + 2))
    for (b, t, c, kw, want) in ((B, T, C + 1, KW, -2), (B, T, C, 5, -2), (0, T, C, KW, 0), (B, 0, C, KW, 0)):
        bU, bZ, bst = out((B * T, C + 2), BF), out((B * T, C + 2), BF), out((2 * C + 4,), F64)
        assert lib.ea_glu_dwconv_fwd(bY.p, bw.p, bU.p, bZ.p, bst.p, b, t, c, kw, _st()) == want, (b, t, c, kw)
        bdY, bdw, bws = out((B * T, 2 * C + 4), BF), out((C + 2, 8), F32), out((4 * (C + 2) * 8,), F32)
        assert lib.ea_glu_dwconv_bwd(bdZ.p, bY.p, bdZ.p, bw.p, bdY.p, bdw.p, bws.p, b, t, c, kw, _st()) == want, (b, t, c, kw)
        if c % 2 == 0:  # (the weight gradient alone has no vector access to refuse an odd C for)
            assert lib.ea_dwconv_bwd_weight(bdZ.p, bdZ.p, bdw.p, bws.p, b, t, c, kw, _st()) == want, (b, t, c, kw)
        _sync()
        for o in (bU, bZ, bst, bdY, bdw, bws):
            assert o.untouched(), (b, t, c, kw)


# ------------------------------------------------------------------ BatchNorm + activation
def _bn_inputs(M, C, seed, device="cpu"):
    """Z with per-channel mean in [0.5, 1.5) and deviation in [0.5, 2) (variance >= 0.05 also in small batches; running means are
    positive too, so the running-mean update has no cancellation and a relative bound is meaningful)"""
    g = torch.Generator(device=device).manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g, device=device)
    randn = lambda *s: torch.randn(*s, generator=g, device=device)
    Z = (randn(M, C) * (0.5 + 1.5 * rand(C)) + 0.5 + rand(C)).to(BF)
    rowscale = 0.5 * 4.0 ** rand(M, 1)
    dH = (randn(M, C) * rowscale).to(BF)
    return dict(Z=Z, dH=dH, gamma=1 + 0.3 * randn(C), beta=0.3 * randn(C), rm=0.2 + rand(C), rv=0.5 + rand(C))


def _exact_stats(Z):
    Zd = Z.double()
    return torch.cat([Zd.sum(0), (Zd * Zd).sum(0)])


REL = 8 * 2.0 ** -23


def _bn_forward(lib, d, M, C, act, training, fused):
    """BatchNorm statistics -> mean / rstd (+ running statistics) -> H, by the two-launch route or ea_bn_act_fwd_train; every
    output against fp64.  Returns the kernel's mean_rstd."""
    Z, gamma, beta, rm, rv = d["Z"], d["gamma"], d["beta"], d["rm"], d["rv"]
    bZ, bg, bb = inp(Z), inp(gamma), inp(beta)
    bmr, bH = out((2 * C,), F32), out((M, C), BF)
    tag = "fwd_train" if fused else ("finalize+fwd" if training else "from_running+fwd")
    if training:
        stats = _exact_stats(Z)
        bst, brm, brv = inp(stats), out((C,), F32, rm), out((C,), F32, rv)
        if fused:
            zero_n = 2 * C + 40
            bzn = out((zero_n,), F64, torch.full((zero_n,), 3.5, dtype=F64))
            assert lib.ea_bn_act_fwd_train(bZ.p, bst.p, bmr.p, brm.p, brv.p, bg.p, bb.p, bH.p, M, C, act, float(M), EPS, MOM, bzn.p,
                                           zero_n, _st()) == 0
            _sync()
            assert bzn.intact() and bool((bzn.t == 0).all()), "zero_next not cleared over all zero_n doubles (or past them)"
        else:
            assert lib.ea_bn_finalize(bst.p, bmr.p, brm.p, brv.p, C, float(M), EPS, MOM, _st()) == 0
            assert lib.ea_bn_act_fwd(bZ.p, bmr.p, bg.p, bb.p, bH.p, M, C, act, _st()) == 0
            _sync()
        assert brm.intact() and brv.intact()
        mean, rstd, rmn, rvn = R.bn_finalize(stats[:C], stats[C:], M, EPS, MOM, rm, rv)
        if M > 1:
            assert float((stats[C:] / M - mean * mean).min()) >= 0.05
        _check_rel(tag + " running_mean", brm.cpu(), rmn.cpu(), REL)  # (updated exactly once: twice is far outside)
        _check_rel(tag + " running_var", brv.cpu(), rvn.cpu(), REL)
    else:
        brm, brv = inp(rm), inp(rv)
        assert lib.ea_bn_from_running(brm.p, brv.p, bmr.p, C, EPS, _st()) == 0
        assert lib.ea_bn_act_fwd(bZ.p, bmr.p, bg.p, bb.p, bH.p, M, C, act, _st()) == 0
        _sync()
        mean, rstd = R.f64(rm), 1.0 / torch.sqrt(R.f64(rv) + EPS)
    assert bmr.intact() and bH.intact()
    mr = bmr.t.detach().to(Z.device)
    _check_rel(tag + " mean", mr[:C], mean, REL)
    _check_rel(tag + " rstd", mr[C:], rstd, REL)
    Hr, hmag = R.bn_act(Z, mr[:C], mr[C:], gamma, beta, act)
    _check_bf16(tag + " H", bH.t.detach().to(Z.device), Hr, 2.0 ** -20 * hmag)
    return mr


def _red_checks(tag, red, ref, M, C, one_row=True):
    tol0, tol1 = (M * 2.0 ** -24 + 2.0 ** -20) * ref["mag_dy"], (M * 2.0 ** -24 + 2.0 ** -20) * ref["mag_dy_xhat"]
    _check(tag + " red[0] = sum dy", red[:C], ref["sum_dy"], tol0)
    _check(tag + " red[1] = sum dy*xhat", red[C:], ref["sum_dy_xhat"], tol1)
    if one_row:
        _sees_one_row(tag + " red[0]", tol0, ref["mag_dy"], M)
        _sees_one_row(tag + " red[1]", tol1, ref["mag_dy_xhat"], M)


def _bn_backward(lib, d, mr, M, C, act, training, fused=False, prefill=False, one_row=True):
    """ea_bn_act_bwd (or _fused) against fp64: red, dgamma / dbeta, dZ.  Returns the output buffers."""
    Z, dH, gamma, beta = d["Z"], d["dH"], d["gamma"], d["beta"]
    g = torch.Generator().manual_seed(M + C)
    dg0 = torch.randn(C, generator=g) if prefill else torch.zeros(C)
    db0 = torch.randn(C, generator=g) if prefill else torch.zeros(C)
    bZ, bdH, bmr, bg, bb = inp(Z), inp(dH), inp(mr), inp(gamma), inp(beta)
    bred, bdZ, bdg, bdb = out((2 * C,), F32, torch.zeros(2 * C)), out((M, C), BF), out((C,), F32, dg0), out((C,), F32, db0)
    tag = "bwd_fused" if fused else "bwd"
    if fused:
        zero_n = 2 * C + 40
        bzn = out((zero_n,), F32, torch.full((zero_n,), 3.5))
        assert lib.ea_bn_act_bwd_fused(bZ.p, bdH.p, bmr.p, bg.p, bb.p, bred.p, bdZ.p, bdg.p, bdb.p, M, C, act, int(training), bzn.p,
                                       zero_n, _st()) == 0
        _sync()
        assert bzn.intact() and bool((bzn.t == 0).all()), "zero_next not cleared over all zero_n floats (or past them)"
    else:
        assert lib.ea_bn_act_bwd(bZ.p, bdH.p, bmr.p, bg.p, bb.p, bred.p, bdZ.p, bdg.p, bdb.p, M, C, act, int(training), _st()) == 0
        _sync()
    assert bred.intact() and bdZ.intact() and bdg.intact() and bdb.intact()
    red = bred.t.detach().to(Z.device)
    ref = R.bn_act_bwd(Z, dH, mr[:C], mr[C:], gamma, beta, act, training, red=(red[:C], red[C:]))
    _red_checks(tag, red, ref, M, C, one_row)
    # the parameter gradients are `+=` of exactly those sums: one fp32 addition each, reproduced bit for bit
    assert torch.equal(bdb.cpu(), db0 + bred.cpu()[:C]) and torch.equal(bdg.cpu(), dg0 + bred.cpu()[C:]), tag + ": dgamma / dbeta != prefill + red"
    _check_bf16(tag + " dZ", bdZ.t.detach().to(Z.device), ref["dZ"], 2.0 ** -20 * ref["dZ_mag"])
    return dict(red=bred, dZ=bdZ, dgamma=bdg, dbeta=bdb, dg0=dg0, db0=db0)


BN_SHAPES = [(387, 64), (387, 72),  # nch = 9: TCH = 16 with idle chunk lanes
             (100, 8),              # TCH = 1, 256 row lanes, one short block
             (45, 520),             # TCH = 128, 2 row lanes: the 4-row unrolled loop plus its tail
             (1, 64),               # n = 1: no unbiased factor
             (2051, 256)]


@gpu
@pytest.mark.parametrize("M,C", BN_SHAPES)
@pytest.mark.parametrize("training", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("act", [0, 1, 2], ids=["identity", "relu", "silu"])
def test_batchnorm_activation_forward_and_backward(lib, act, training, M, C):
    d = _bn_inputs(M, C, seed=17 * M + C)
    mr = _bn_forward(lib, d, M, C, act, training, fused=False).cpu()
    if training:  # the one-launch route on the same inputs: both against fp64 (1/n as a product there: not bitwise the same)
        _bn_forward(lib, d, M, C, act, training, fused=True)
    _bn_backward(lib, d, mr, M, C, act, training)


@gpu
@pytest.mark.parametrize("M,C", [(387, 64), (100, 8), (45, 520), (387, 72), (2051, 256)])
@pytest.mark.parametrize("training", [1, 0], ids=["train", "eval"])
def test_batchnorm_backward_fused_equals_three_launches(lib, training, M, C):
    """ea_bn_act_bwd_fused == ea_bn_act_bwd: same two kernels, so dZ is bitwise equal whenever the two reduce passes left the same
    sums — always, for the first three shapes (at most two row blocks add onto the zeroed sums: fp32 addition commutes); with more
    row blocks the order of the fp32 atomics is free and `red` may differ in its last bits.  Parameter gradients are added onto
    pre-filled dgamma / dbeta; ea_bn_param_grad after a call with dgamma = dbeta = NULL gives the same."""
    act = 2
    d = _bn_inputs(M, C, seed=5 * M + C)
    mr = _bn_forward(lib, d, M, C, act, training, fused=False).cpu()
    a = _bn_backward(lib, d, mr, M, C, act, training, fused=False, prefill=True)
    b = _bn_backward(lib, d, mr, M, C, act, training, fused=True, prefill=True)
    same_red = torch.equal(a["red"].bits(), b["red"].bits())
    if (M, C) in ((387, 64), (100, 8), (45, 520)):
        assert same_red
    if same_red:
        assert torch.equal(a["dZ"].bits(), b["dZ"].bits()), "dZ of the fused call differs bitwise"
        assert torch.equal(a["dgamma"].bits(), b["dgamma"].bits()) and torch.equal(a["dbeta"].bits(), b["dbeta"].bits())
    bZ, bdH, bmr, bg, bb = inp(d["Z"]), inp(d["dH"]), inp(mr), inp(d["gamma"]), inp(d["beta"])
    # The same comparison where the sums cannot differ, at every shape: `red` starts at 2^60, half an ulp of which (2^35) is above
    # every partial sum of this data, so each atomic leaves it unchanged in any order — both apply passes read one fixed `red`.
    # (In eval mode the apply pass multiplies the sums by zero: the plain comparison above would do as well.)
    big, fixed = torch.full((2 * C,), 2.0 ** 60), []
    assert float(R.f64(d["dH"]).abs().sum(0).max()) * 4 * float(R.f64(d["Z"]).abs().max() * mr[C:].max() + 4) < 2.0 ** 35
    for fused in (False, True):
        bredf, bdZf, bdgf, bdbf = out((2 * C,), F32, big), out((M, C), BF), out((C,), F32, a["dg0"]), out((C,), F32, a["db0"])
        if fused:
            assert lib.ea_bn_act_bwd_fused(bZ.p, bdH.p, bmr.p, bg.p, bb.p, bredf.p, bdZf.p, bdgf.p, bdbf.p, M, C, act, training, None, 0, _st()) == 0
        else:
            assert lib.ea_bn_act_bwd(bZ.p, bdH.p, bmr.p, bg.p, bb.p, bredf.p, bdZf.p, bdgf.p, bdbf.p, M, C, act, training, _st()) == 0
        _sync()
        assert bredf.intact() and bdZf.intact() and bdgf.intact() and bdbf.intact()
        assert torch.equal(bredf.cpu(), big) and bool(torch.isfinite(bdZf.t.float()).all())
        fixed.append((bdZf, bdgf, bdbf))
    for x, y in zip(*fixed):
        assert torch.equal(x.bits(), y.bits()), "fused and unfused apply passes differ bitwise on the same sums"
    # zero_next = NULL is accepted
    bred, bdZ = out((2 * C,), F32, torch.zeros(2 * C)), out((M, C), BF)
    bdg, bdb = out((C,), F32, a["dg0"]), out((C,), F32, a["db0"])
    assert lib.ea_bn_act_bwd_fused(bZ.p, bdH.p, bmr.p, bg.p, bb.p, bred.p, bdZ.p, bdg.p, bdb.p, M, C, act, training, None, 0, _st()) == 0
    _sync()
    assert bred.intact() and bdZ.intact() and bdg.intact() and bdb.intact()
    if torch.equal(bred.bits(), a["red"].bits()):
        assert torch.equal(bdZ.bits(), a["dZ"].bits())
    assert torch.equal(bdg.cpu(), a["dg0"] + bred.cpu()[C:]) and torch.equal(bdb.cpu(), a["db0"] + bred.cpu()[:C])
    # dgamma = dbeta = NULL, then ea_bn_param_grad on the sums
    bred3, bdZ3 = out((2 * C,), F32, torch.zeros(2 * C)), out((M, C), BF)
    bdg3, bdb3 = out((C,), F32, a["dg0"]), out((C,), F32, a["db0"])
    assert lib.ea_bn_act_bwd(bZ.p, bdH.p, bmr.p, bg.p, bb.p, bred3.p, bdZ3.p, None, None, M, C, act, training, _st()) == 0
    _sync()
    assert torch.equal(bdg3.cpu(), a["dg0"]) and torch.equal(bdb3.cpu(), a["db0"])
    assert lib.ea_bn_param_grad(bred3.p, bdg3.p, bdb3.p, C, _st()) == 0
    _sync()
    assert bred3.intact() and bdZ3.intact() and bdg3.intact() and bdb3.intact()
    assert torch.equal(bdg3.cpu(), a["dg0"] + bred3.cpu()[C:]) and torch.equal(bdb3.cpu(), a["db0"] + bred3.cpu()[:C])
    if torch.equal(bred3.bits(), a["red"].bits()):
        assert torch.equal(bdZ3.bits(), a["dZ"].bits()) and torch.equal(bdg3.bits(), a["dgamma"].bits())


def _integer_bn_inputs(M, C, seed):
    """Z in {1, 2, 3} * sign, dH in {1, 2} * sign, mean 0, rstd 1, gamma 1, beta 0, identity activation: every term of both backward
    sums is a non-zero integer and every partial sum stays below 2^24, so fp32 adds them exactly in any order"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ri = lambda lo, hi: torch.randint(lo, hi, (M, C), generator=g, device=DEV)
    Z = (ri(1, 4) * (2 * ri(0, 2) - 1)).to(BF)
    dH = (ri(1, 3) * (2 * ri(0, 2) - 1)).to(BF)
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    return dict(Z=Z, dH=dH, gamma=one, beta=zero), torch.cat([zero, one])


@gpu
@pytest.mark.parametrize("M,C", [(33000, 512),   # > 8192 * 256 chunks: the grid-stride loops of the forward and apply kernels take a second trip
                                 (530000, 64)])  # want > rpb in launch_bn_bwd_reduce: the sub-sampler's regime
def test_batchnorm_large_grids(lib, M, C):
    """(fp64 reference evaluated with torch on the GPU.)  At these row counts the table's bound for the backward sums, M 2^-24 sum
    |term|, is far above one row's share — so the sums are ALSO taken on integer data, where fp32 is exact in any order and the
    kernel must return the integer sums themselves: one dropped or duplicated row is off by at least 1."""
    nch = C // 8
    tch = 1 << (nch - 1).bit_length()                  # launch_bn_bwd_reduce restated: chunks per block row, row lanes, rows per block
    lanes, gx = 256 // tch, (nch + tch - 1) // tch
    rpb, want = max(8 * lanes, 32), -(-M // (2048 // gx))
    if (M, C) == (33000, 512):
        assert M * nch > 8192 * 256                    # more chunks than the capped grid has threads: a second grid-stride trip
    else:
        assert want > rpb and M * nch > 8192 * 256     # the reduce's blocks take `want` rows each, rounded up to the row lanes
    d = _bn_inputs(M, C, seed=M + C, device=DEV)
    mr = _bn_forward(lib, d, M, C, 2, 1, fused=False)
    _bn_forward(lib, d, M, C, 2, 1, fused=True)
    _bn_backward(lib, d, mr, M, C, 2, 1, fused=True, one_row=False)
    del d
    di, mri = _integer_bn_inputs(M, C, seed=M)
    o = _bn_backward(lib, di, mri, M, C, 0, 1, fused=False, one_row=False)
    Zd, dHd = di["Z"].double(), di["dH"].double()
    assert float((Zd * dHd).abs().sum(0).max()) < 2.0 ** 24
    red = o["red"].t.double()
    assert torch.equal(red[:C], dHd.sum(0)) and torch.equal(red[C:], (dHd * Zd).sum(0)), "integer sums not exact: a row was dropped or taken twice"


@gpu
def test_batchnorm_return_codes(lib):
    """C % 8 != 0 is refused (-2), M = 0 is a no-op (0): nothing is written either way"""
    M, C = 20, 64
    d = _bn_inputs(M, C, seed=1)
    bZ, bdH, bg, bb = inp(d["Z"]), inp(d["dH"]), inp(d["gamma"]), inp(d["beta"])
    bmr, bst = inp(torch.cat([d["rm"], d["rv"]])), inp(_exact_stats(d["Z"]))
    for (m, c, want) in ((M, C - 4, -2), (M, C - 2, -2), (0, C, 0)):
        outs = [out((M, C), BF), out((2 * C,), F32), out((C,), F32), out((C,), F32), out((2 * C,), F32), out((2 * C + 40,), F64),
                out((2 * C + 40,), F32)]
        bH, bmro, ba, bb2, bred, bz64, bz32 = outs
        assert lib.ea_bn_act_fwd(bZ.p, bmr.p, bg.p, bb.p, bH.p, m, c, 2, _st()) == want
        assert lib.ea_bn_act_fwd_train(bZ.p, bst.p, bmro.p, ba.p, bb2.p, bg.p, bb.p, bH.p, m, c, 2, float(M), EPS, MOM, bz64.p, 2 * C + 40,
                                       _st()) == want
        assert lib.ea_bn_act_bwd(bZ.p, bdH.p, bmr.p, bg.p, bb.p, bred.p, bH.p, ba.p, bb2.p, m, c, 2, 1, _st()) == want
        assert lib.ea_bn_act_bwd_fused(bZ.p, bdH.p, bmr.p, bg.p, bb.p, bred.p, bH.p, ba.p, bb2.p, m, c, 2, 1, bz32.p, 2 * C + 40, _st()) == want
        _sync()
        for o in outs:
            assert o.untouched(), (m, c)


# ------------------------------------------------------------------ the module's middle, stage by stage
@gpu
def test_conv_module_middle_composition(lib):
    """glu_dwconv_fwd -> bn_finalize -> bn_act_fwd, then bn_act_bwd -> glu_dwconv_bwd (functional.conv_module's middle) at a width
    and tap count no model-level test reaches; each stage's fp64 reference is fed from the previous kernel's own stored output"""
    B, T, C, KW, act = 3, 70, 72, 15, 2
    M = B * T
    g = _gen(23)
    w = torch.randn(C, KW, generator=g)
    Y, w = _utts(g, B, T, 2 * C), (w / w.norm(dim=1, keepdim=True)).float()  # unit-norm filters: every channel of Z keeps U's variance
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    rm, rv = torch.zeros(C), torch.ones(C)  # a fresh BatchNorm1d
    bY, bw, bg, bb = inp(Y), inp(w), inp(gamma), inp(beta)
    bU, bZ, bst = out((M, C), BF), out((M, C), BF), out((2 * C,), F64, torch.zeros(2 * C, dtype=F64))
    bmr, brm, brv, bH = out((2 * C,), F32), out((C,), F32, rm), out((C,), F32, rv), out((M, C), BF)
    assert lib.ea_glu_dwconv_fwd(bY.p, bw.p, bU.p, bZ.p, bst.p, B, T, C, KW, _st()) == 0
    assert lib.ea_bn_finalize(bst.p, bmr.p, brm.p, brv.p, C, float(M), EPS, MOM, _st()) == 0
    assert lib.ea_bn_act_fwd(bZ.p, bmr.p, bg.p, bb.p, bH.p, M, C, act, _st()) == 0
    _sync()
    for o in (bU, bZ, bst, bmr, brm, brv, bH):
        assert o.intact()
    U, Z, stats, mr = bU.cpu(), bZ.cpu(), bst.cpu(), bmr.cpu()
    _check_bf16("U", U, R.glu(Y))
    Zr, zmag = R.dwconv(U, w, B, T, KW)
    _check_bf16("Z", Z, Zr, KW * 2.0 ** -23 * zmag)
    s, q, sabs = R.bn_stats(Z)
    _check("stats.sum", stats[:C], s, 2.0 ** -18 * sabs)
    _check("stats.sumsq", stats[C:], q, 2.0 ** -18 * q)
    mean, rstd, rmn, rvn = R.bn_finalize(stats[:C], stats[C:], M, EPS, MOM, rm, rv)
    assert float((stats[C:] / M - mean * mean).min()) >= 0.05
    _check_rel("mean", mr[:C], mean, REL)
    _check_rel("rstd", mr[C:], rstd, REL)
    _check_rel("running_mean", brm.cpu(), rmn, REL)
    _check_rel("running_var", brv.cpu(), rvn, REL)
    Hr, hmag = R.bn_act(Z, mr[:C], mr[C:], gamma, beta, act)
    _check_bf16("H", bH.cpu(), Hr, 2.0 ** -20 * hmag)
    # backward
    dH = _utts(g, B, T, C)
    bZi, bUi, bdH, bmri = inp(Z), inp(U), inp(dH), inp(mr)
    bred, bdZ, bdg, bdb = out((2 * C,), F32, torch.zeros(2 * C)), out((M, C), BF), out((C,), F32, torch.zeros(C)), out((C,), F32, torch.zeros(C))
    nws = lib.ea_dwconv_wgrad_workspace_bytes(B, T, C, KW) // 4
    bdY, bdw, bws = out((M, 2 * C), BF), out((C, KW), F32, torch.zeros(C, KW)), out((nws,), F32)
    assert lib.ea_bn_act_bwd(bZi.p, bdH.p, bmri.p, bg.p, bb.p, bred.p, bdZ.p, bdg.p, bdb.p, M, C, act, 1, _st()) == 0
    _sync()
    dZ = bdZ.cpu()
    bdZi = inp(dZ)
    assert lib.ea_glu_dwconv_bwd(bdZi.p, bY.p, bUi.p, bw.p, bdY.p, bdw.p, bws.p, B, T, C, KW, _st()) == 0
    _sync()
    for o in (bred, bdZ, bdg, bdb, bdY, bdw, bws):
        assert o.intact()
    red = bred.cpu()
    ref = R.bn_act_bwd(Z, dH, mr[:C], mr[C:], gamma, beta, act, True, red=(red[:C], red[C:]))
    _red_checks("bwd", red, ref, M, C)
    assert torch.equal(bdb.cpu(), red[:C]) and torch.equal(bdg.cpu(), red[C:])
    _check_bf16("dZ", dZ, ref["dZ"], 2.0 ** -20 * ref["dZ_mag"])
    dYr, dymag = R.glu_dwconv_bwd(dZ, Y, w, B, T, KW)
    _check_bf16("dY", bdY.cpu(), dYr, KW * 2.0 ** -23 * dymag)
    dwr, dwmag = R.dwconv_wgrad(dZ, U, B, T, KW)
    _check("dw", bdw.cpu(), dwr, M * 2.0 ** -24 * dwmag)
    _sees_one_row("dw", M * 2.0 ** -24 * dwmag, dwmag, M)
