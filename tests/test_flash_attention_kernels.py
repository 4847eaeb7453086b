"""The fused attention kernels (espresso_amd/csrc/flash_relpos.hip: forward, backward-Q, backward-KV and the keep-bit kernel; the
general kernels of flash_attention.hip) per element against the plain fp64 restatement in tests/flash_attention_ref.py, through
the C ABI and with the engine's strides: k / v are views into one [B*T][3C] buffer, dq / dk / dv the thirds of another,
ldq = ldo = ldpp = C + 8, ldt = C + 16, ld_bd = Rp + 8, H = 2, B = 3.

Every device tensor is a view into a larger allocation with guard rows on both sides and (where the pitch leaves one) a gap behind
every row: NaN around and between input rows (a row or column consumed outside the tensor poisons the output), a sentinel bit
pattern around and between output rows (checked afterwards), NaN inside outputs (an element nobody wrote fails).  Key / value rows
j >= klen[b] hold finite values 64 times larger than the valid ones; utterances and heads are drawn at different scales (query
scale 0.35: peaked softmax, 0.1: flat), so a leaked padded key or a read of the neighbouring utterance or head moves the result
far beyond any bound.  The dropout keep decisions come from oracle/dropout_ref.py, never from a device kernel.

Staging and bounds.  u = 2^-8 (one bf16 rounding), e = 2^-24 (one fp32 rounding), x = 2^-20 (the project's allowance for a
hardware transcendental, on the term it enters), ulp(r) = the bf16 step at |r| (tests.gpu_checks._bf_ulp_ok's), nt = ceil(S/64).
None is measured; the counts are read off the kernels:
  score error  es[i][j] = e (130 sum_d(|qu||k| + |qv||pp|) + 5 max(max_j |S[i][j]|, |lse[i]|))
                                                       128 products accumulated in fp32 on the MFMA pipe, the band add, and
                                                       exp2(fma(s, LOG2E, -m LOG2E)): the rounding of m LOG2E, of the fma, of LOG2E
                                                       (general kernels: s - m, then __expf's own multiply: no more than that)
  lse   vs fp64 on the bf16 inputs    sum_j P es + x (nt + 2 + log l) + e (17 nt + 2 + 2|lse| + |m|)
                                                       x on every exp2 (P-weighted: once), on each of the <= nt rescales of the running
                                                       sum, on v_log's log l; 16 + 1 fp32 additions per tile, 2 across lanes, m + log l
        rl = sum_j P es + x (nt + 1) + e (17 nt + 2)   (the relative error of the row sum l, used below)
  out   vs fp64 on the bf16 inputs    ulp(ref) + sum_j Pd|v| (u + es + x) + sum_j Pd|v| (rl + e (S + 2 nt + 4))
                                                       bf16 rounding of every Pd, its exp2 and score error; the division by l; fp32
                                                       sum over S keys, nt rescales of the accumulator, 1/(1-p), 1/l; one bf16 store
  D     vs fp64 on the kernel's out   18 e sum_d |out dout|                    16 products per lane + 2 steps across lanes
  dS    (with the kernel's lse, D)    eds = P ((es + x + 2 e) |dPd keep/(1-p) - D| + 65 e keep/(1-p) sum_d |dout||v|)
                                                       P's exp2 and score error, the subtraction and the product; dPd = fp32 sum of 64
                                                       products and its multiplication by 1/(1-p);   E = u |dS| + eds once rounded to bf16
  t1    ulp(ref) + |scaling| (sum_j E|k| + e (S + 2) sum_j |dS||k|)            fp32 sum over keys, scaling, one bf16 store
  t2    the same over the band of pp;   dq: ulp(ref of t1 + t2) + both sums + e (S + 3) (...): summed BEFORE rounding
  dBD   inside the band: ulp(ref) + eds (one bf16 store of dS); outside, up to ld_bd: zero bit for bit
  dK    ulp(ref) + sum_i E|qu| + e (T + 2) sum_i |dS||qu|                       fp32 sum over query rows, one bf16 store
  dV    ulp(ref) + sum_i Pd (u + es + x + e) |dout| + e (T + 2) sum_i Pd|dout|
  dK, dV rows j >= klen[b]: exactly zero, and written
No element is excluded from any comparison.

The first two tests need no GPU: the reference against torch's own operators and autograd in float64, and the proof that these
bounds discriminate: nine planted faults (tests/flash_attention_ref.FAULTS), each evaluated through the reference, rounded the way
the kernels store and compared under the bounds above, fail at least one element in every case they can occur in, while the sound
reference rounded the same way passes everywhere."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import dropout_ref as DR
from tests import flash_attention_ref as R
from tests import gpu_checks as G

gpu = pytest.mark.gpu
DEV = "cuda:0"
BF, F32, F64, I16 = torch.bfloat16, torch.float32, torch.float64, torch.int16
_INT = {BF: torch.int16, F32: torch.int32, I16: torch.int16}
_SENTINEL = {BF: 0x5AA5, F32: 0x5AA55AA5, I16: 0x5AA5}
_NAN16 = 0x7FC0
GUARD = 128
H, B, DH = 2, 3, 64
C = H * DH
U8, E24, XT = 2.0 ** -8, 2.0 ** -24, 2.0 ** -20
SEED = (0x9E37 << 32) | 0x1234567  # non-zero high word


# ------------------------------------------------------------------ the reference against torch's operators (CPU)
@pytest.mark.parametrize("p", [0.0, 0.3], ids=["nodrop", "drop"])
@pytest.mark.parametrize("with_klen", [False, True], ids=["full", "klen"])
@pytest.mark.parametrize("T", [1, 5, 65])
@pytest.mark.parametrize("form", ["relpos", "causal", "cross"])
def test_reference_matches_torch_operators_in_float64(form, T, with_klen, p):
    """tests/flash_attention_ref.py == gather -> masked_fill -> torch.softmax -> dropout multiplier -> matmul in float64: forward
    values and every autograd gradient (dpp = sum dBD^T qv among them) within 1e-11 of each tensor's scale"""
    Bt, Ht, dh, sc = 2, 2, 8, 0.7
    S = T + 3 if form == "cross" else T
    g = torch.Generator().manual_seed(1000 * T + len(form))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    qu, k, v, dout = rnd(Bt, T, Ht, dh).requires_grad_(), rnd(Bt, S, Ht, dh).requires_grad_(), rnd(Bt, S, Ht, dh).requires_grad_(), rnd(Bt, T, Ht, dh)
    qv = pp = None
    if form == "relpos":
        qv, pp = rnd(Bt, T, Ht, dh).requires_grad_(), rnd(2 * T - 1, Ht, dh).requires_grad_()
    klen = [S + 4, max(1, S // 2)] if with_klen else None  # the first is clamped
    x = R.problem(qu, k, v, qv, pp, klen, form == "causal", p, SEED, sc)
    s = torch.einsum("bihd,bjhd->hbij", qu, k)
    if qv is not None:
        s = s + torch.einsum("bihd,rhd->hbir", qv, pp).gather(3, R.band_index(T, S).expand(Ht, Bt, T, S))
    j, i = torch.arange(S)[None, :], torch.arange(T)[:, None]
    ok = torch.stack([(j < (min(klen[b], S) if klen else S)) & ((j <= i + S - T) if form == "causal" else (j >= 0)) for b in range(Bt)])
    s = s.masked_fill(~ok[None], float("-inf"))
    mult = torch.ones(Ht, Bt, T, S, dtype=F64)
    if p > 0:
        mult = torch.from_numpy(DR.keep_mask(SEED, Ht * Bt * T * S, p).astype(np.float64)).view(Ht, Bt, T, S) * R.inv_keep(p)
    out = torch.einsum("hbij,bjhd->bihd", torch.softmax(s, -1) * mult, v)
    (out * dout).sum().backward()
    fw, bw = R.forward(x), R.backward(x, dout)
    # (the floor: with one valid key P = 1 and dS = dPd - D is the difference of two equal sums of unit-scale terms, exactly 0 in torch)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-11 * max(float(b.abs().max()), 1e-3)
    pairs = [("out", fw.out, out.detach()), ("lse", fw.lse, s.detach().exp().sum(-1).log()), ("t1", bw.t1, sc * qu.grad),
             ("dK", bw.dK, k.grad), ("dV", bw.dV, v.grad)]
    if qv is not None:
        pairs += [("t2", bw.t2, sc * qv.grad), ("dq", bw.dq, sc * (qu.grad + qv.grad)),
                  ("dpp", torch.einsum("hbir,bihd->rhd", bw.dBD, x.qv), pp.grad)]
        assert bw.dBD.shape[-1] == 2 * T - 1 and bool((bw.dBD[~bw.band] == 0).all())
    for name, got, want in pairs:
        assert close(got, want), (name, float((got - want).abs().max()), float(want.abs().max()))


# ------------------------------------------------------------------ the bounds (shared by the CPU proof and the GPU tests)
def _ulp(ref):
    """the bf16 step at |ref| (the definition in tests.gpu_checks._bf_ulp_ok)"""
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -60))) - 7)


def _cmp(res, what, got, ref, tol, bf16=False):
    """|got - ref| <= tol at EVERY element (a non-finite `got` fails); records (bad elements, worst ratio, a listing of the worst)"""
    got = R.f64(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    tol = tol.expand_as(ref)
    diff = torch.where(torch.isfinite(got), (got - ref).abs(), torch.full_like(ref, float("inf")))
    bad = diff > tol
    ratio = float((diff / tol.clamp_min(1e-300)).max()) if ref.numel() else 0.0
    lines = []
    for flat in torch.argsort((diff - tol).reshape(-1), descending=True)[:4].tolist() if bool(bad.any()) else []:
        idx = tuple(int(n) for n in np.unravel_index(flat, ref.shape))
        lines.append(f"{idx}: got {float(got.reshape(-1)[flat])!r} fp64 {float(ref.reshape(-1)[flat])!r} bound {float(tol.reshape(-1)[flat]):.3e}")
    if bf16 and not bool(bad.any()):  # the project's own bf16-step check agrees
        assert G._bf_ulp_ok(got, ref, ulps=1.0, atol=(tol - _ulp(ref)).clamp_min(0).float()), what
    res[what] = (int(bad.sum()), ratio, lines)


def _eps_scores(S, smag, lse):
    arow = torch.maximum(torch.where(torch.isfinite(S), S.abs(), torch.zeros_like(S)).amax(-1), lse.abs())
    return E24 * (130 * smag + 5 * arow[..., None])


def _rows(t):  # [H][B][T] -> broadcastable against [B][T][H][64]
    return t.permute(1, 2, 0)[..., None]


def verify(x, dout, got, dbd_outside=0):
    """every tensor of `got` (a kernel's, or the rounded reference's) under the bounds of this file's docstring -> {tensor: (bad,
    worst ratio, listing)}.  lse and out against fp64 on the inputs, D on got's out, the gradients on got's lse and D."""
    res = {}
    nt = (x.S + 63) // 64
    dout = R.f64(dout)
    fw = R.forward(x)
    es = _eps_scores(fw.S, fw.smag, fw.lse)
    m = fw.S.amax(-1)
    pes = (fw.P * es).sum(-1)
    _cmp(res, "lse", got["lse"], fw.lse, pes + XT * (nt + 2 + (fw.lse - m)) + E24 * (17 * nt + 2 + 2 * fw.lse.abs() + m.abs()))
    rl = pes + XT * (nt + 1) + E24 * (17 * nt + 2)
    tol = _ulp(fw.out) + R.sum_keys(fw.Pd * (U8 + es + XT), x.v.abs()) + fw.out_mag * (_rows(rl) + E24 * (x.S + 2 * nt + 4))
    _cmp(res, "out", got["out"], fw.out, tol, bf16=True)
    D, dmag = R.row_dot(R.f64(got["out"]), dout)
    _cmp(res, "D", got["D"], D, 18 * E24 * dmag)
    lse_k, D_k = R.f64(got["lse"]), R.f64(got["D"])
    if not (bool(torch.isfinite(lse_k).all()) and bool(torch.isfinite(D_k).all())):
        return res  # already recorded above as failures of lse / D
    ld_bd = got["dBD"].shape[-1] if got.get("dBD") is not None else None
    bw = R.backward(x, dout, lse=lse_k, D=D_k, ld_bd=ld_bd)
    es = _eps_scores(bw.S, bw.smag, lse_k)
    eds = bw.P * ((es + XT + 2 * E24) * (bw.dPs - D_k[..., None]).abs() + 65 * E24 * bw.keep * bw.dp_mag)
    E = U8 * bw.dS.abs() + eds
    sc = abs(x.scaling)
    e1 = sc * R.sum_keys(E, x.k.abs())
    _cmp(res, "t1", got["t1"], bw.t1, _ulp(bw.t1) + e1 + E24 * (x.S + 2) * bw.t1_mag, bf16=True)
    if x.qv is not None:
        e2 = sc * R.sum_band(E, x.pp.abs(), x.T, x.S)
        _cmp(res, "t2", got["t2"], bw.t2, _ulp(bw.t2) + e2 + E24 * (x.S + 2) * bw.t2_mag, bf16=True)
        _cmp(res, "dq", got["dq"], bw.dq, _ulp(bw.dq) + e1 + e2 + E24 * (x.S + 3) * (bw.t1_mag + bw.t2_mag), bf16=True)
        inside = torch.where(bw.band, R.f64(got["dBD"]), torch.zeros_like(bw.dBD))  # (outside the band: the bit comparison below)
        _cmp(res, "dBD", inside, bw.dBD, _ulp(bw.dBD) + R.to_band(eds, x.T, x.S, ld_bd))
        wrong = got["dBD"].view(torch.int16)[~bw.band] != dbd_outside
        res["dBD outside the band"] = (int(wrong.sum()), float(wrong.any()), [f"{int(wrong.sum())} elements differ from bit pattern {dbd_outside:#06x}"] if bool(wrong.any()) else [])
    _cmp(res, "dK", got["dk"], bw.dK, _ulp(bw.dK) + R.sum_rows(E, x.qu.abs()) + E24 * (x.T + 2) * bw.dK_mag, bf16=True)
    _cmp(res, "dV", got["dv"], bw.dV, _ulp(bw.dV) + R.sum_rows(bw.Pd * (U8 + es + XT + E24), dout.abs()) + E24 * (x.T + 2) * bw.dV_mag, bf16=True)
    pad = torch.stack([torch.arange(x.S) >= n for n in R.key_limits(x)])  # [B][S]
    nz = sum(int((R.f64(got[n])[pad] != 0).sum()) for n in ("dk", "dv"))  # (NaN != 0: an unwritten element counts)
    res["dK, dV of padded keys"] = (nz, float(nz > 0), [f"{nz} elements of rows j >= klen[b] are not zero"] if nz else [])
    return res


def _assert_ok(res, label=""):
    for name, (bad, ratio, _) in res.items():  # recorded for the reader of the log, never asserted
        print(f"RATIO | {label} | {name} | {ratio:.4f}")
    failed = {n: r for n, r in res.items() if r[0]}
    assert not failed, label + "\n" + "\n".join(f"{n}: {r[0]} elements outside the bound (worst ratio {r[1]:.3g})\n  " + "\n  ".join(r[2]) for n, r in failed.items())


# ------------------------------------------------------------------ inputs
def _case(T, S=None, klen=None, relpos=True, causal=False, seed=0, qv_is_qu=False):
    """bf16 operands: utterances and heads at their own scales, padded key / value rows 64 times larger"""
    S = T if S is None else S
    g = torch.Generator().manual_seed(7919 * T + 31 * S + seed)
    per = lambda bs, hs: torch.tensor(bs).view(B, 1, 1, 1) * torch.tensor(hs).view(1, 1, H, 1)
    rnd = lambda n, bs, hs: torch.randn(B, n, H, DH, generator=g) * per(bs, hs)
    qu, qv = rnd(T, [0.35, 0.1, 0.2], [1.0, 0.7]), rnd(T, [0.35, 0.1, 0.2], [0.8, 1.0])
    k, v = rnd(S, [1.0, 0.6, 1.4], [1.0, 1.5]), rnd(S, [0.8, 1.5, 0.5], [1.3, 0.7])
    dout = rnd(T, [1.0, 0.5, 2.0], [0.6, 1.2])
    pp = torch.randn(2 * T - 1, H, DH, generator=g) * torch.tensor([0.5, 0.8]).view(1, H, 1)
    if klen is not None:
        for b in range(B):
            k[b, min(klen[b], S):] *= 64
            v[b, min(klen[b], S):] *= 64
    c = SimpleNamespace(T=T, S=S, klen=klen, relpos=relpos, causal=causal, qu=qu.to(BF), qv=qv.to(BF), k=k.to(BF), v=v.to(BF), dout=dout.to(BF),
                        pp=pp.to(BF), scaling=0.125)
    if qv_is_qu:
        c.qv = c.qu
    if not relpos:
        c.qv = c.pp = None
    return c


def _problem(c, p=0.0):
    return R.problem(c.qu, c.k, c.v, c.qv, c.pp, c.klen, c.causal, p, SEED, c.scaling)


def _ld_bd(T):
    return (2 * T - 1 + 7) // 8 * 8 + 8


# ------------------------------------------------------------------ the bounds discriminate (CPU)
def simulate(x, dout, fault=None, ld_bd=None):
    """what kernels with `fault` would store: the reference through every stage on its own earlier (rounded) results"""
    dout = R.f64(dout)
    fw = R.forward(x, fault)
    out, lse = fw.out.to(BF), fw.lse.to(F32)
    D = None if fault == "D_without_dropout" else R.row_dot(R.f64(out), dout)[0].to(F32).double()
    bw = R.backward(x, dout, lse=R.f64(lse), D=D, ld_bd=ld_bd, fault=fault)
    got = dict(out=out, lse=lse, D=bw.D.to(F32), t1=bw.t1.to(BF), dk=bw.dK.to(BF), dv=bw.dV.to(BF), t2=None, dq=None, dBD=None)
    if x.qv is not None:
        got.update(t2=bw.t2.to(BF), dq=bw.dq.to(BF), dBD=bw.dBD.to(BF))
    return got


def _applies(fault, x):
    if fault == "mask+1":
        return any(n < x.S for n in R.key_limits(x))
    if fault in ("pos-1", "pos+1", "dbd_band_shifted"):
        return x.qv is not None
    if fault in ("keep_z_swapped", "fwd_no_keep_scale", "D_without_dropout"):
        return x.p > 0
    return True


_PROOF_CASES = [(T, klen, p) for T, kl in ((65, (65, 64, 1)), (129, (129, 65, 63)), (257, (257, 128, 65))) for klen in (None, kl) for p in (0.0, 0.1)]


@pytest.mark.parametrize("T,klen,p", _PROOF_CASES, ids=[f"T{t}-{'klen' if k else 'full'}-p{p}" for t, k, p in _PROOF_CASES])
def test_bounds_see_every_planted_fault(T, klen, p):
    """a condition, not a measurement: the sound reference rounded as the kernels store passes everywhere, each planted fault fails"""
    c = _case(T, klen=klen)
    x = _problem(c, p)
    res = verify(x, c.dout, simulate(x, c.dout, ld_bd=_ld_bd(T)))
    assert not any(r[0] for r in res.values()), {n: r for n, r in res.items() if r[0]}
    for fault in R.FAULTS:
        if not _applies(fault, x):
            continue
        res = verify(x, c.dout, simulate(x, c.dout, fault, ld_bd=_ld_bd(T)))
        caught = {n: r[0] for n, r in res.items() if r[0]}
        print(f"T={T} klen={klen} p={p} {fault}: caught by", ", ".join(f"{n} ({k} elements)" for n, k in caught.items()) or "NOTHING")
        assert caught, f"{fault} passes every bound at T={T} klen={klen} p={p}"


# ------------------------------------------------------------------ device buffers
class Alloc:
    """[rows][ld] device allocation with GUARD rows before and after; tensors are column ranges of its rows (`region`), the rest of
    every row is the pitch gap.  Inputs: NaN everywhere outside the data.  Outputs: a sentinel bit pattern everywhere outside the
    regions (`intact()`), NaN inside them."""

    def __init__(self, rows, ld, dtype, out=False, guard=GUARD):
        self.rows, self.ld, self.dtype, self.out, self.g = rows, ld, dtype, out, guard
        self.full = torch.empty(rows + 2 * guard, ld, dtype=dtype, device=DEV)
        self.full.view(_INT[dtype]).fill_(_SENTINEL[dtype] if out else _NAN16 if dtype == I16 else 0)
        if not out and dtype != I16:
            self.full.fill_(float("nan"))
        self.claimed = torch.zeros(rows + 2 * guard, ld, dtype=torch.bool, device=DEV)

    def region(self, col0=0, width=None, data=None, fill_bits=None):
        width = self.ld - col0 if width is None else width
        t = self.full[self.g:self.g + self.rows, col0:col0 + width]
        self.claimed[self.g:self.g + self.rows, col0:col0 + width] = True
        if data is not None:
            t.copy_(data.reshape(self.rows, width).to(self.dtype))
        elif fill_bits is not None:
            t.view(_INT[self.dtype]).fill_(fill_bits - 65536 if fill_bits >= 32768 and self.dtype != F32 else fill_bits)
        elif self.dtype == I16:
            t.fill_(_NAN16)
        else:
            t.fill_(float("nan"))
        return t

    def ptr(self, col0=0, byte_off=0):
        return ctypes.c_void_p(self.full.data_ptr() + (self.g * self.ld + col0) * self.full.element_size() + byte_off)

    def intact(self):
        return self.out and bool(((self.full.view(_INT[self.dtype]) == _SENTINEL[self.dtype]) | self.claimed).all())


def _bits(t):
    return t.contiguous().view(_INT[t.dtype]).cpu()


@pytest.fixture
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from espresso_amd import _lib

    return _lib.lib()  # the HIP library is the thing under test: a missing one is an error, not a skip


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _expected_keep_bits(T, p):
    """the keep-bit buffer of flash_relpos.hip from oracle/dropout_ref.py: bits[((z nkt + kt) Tpad + i) 4 + g], bit jt*4 + r = key
    kt*64 + jt*16 + g*4 + r of row i; rows and keys >= T are zero"""
    Z, nkt = H * B, (T + 63) // 64
    Tp = nkt * 64
    keep = np.zeros((Z, Tp, Tp), dtype=np.int64)
    keep[:, :T, :T] = DR.keep_mask(SEED, Z * T * T, p).reshape(Z, T, T)
    k6 = keep.reshape(Z, Tp, nkt, 4, 4, 4)  # z, i, kt, jt, g, r
    w = (1 << (np.arange(4)[:, None, None] * 4 + np.arange(4)[None, None, :]))  # [jt][1][r]
    pieces = (k6 * w[None, None, None]).sum(axis=(3, 5))  # z, i, kt, g
    return torch.from_numpy(pieces.transpose(0, 2, 1, 3).reshape(-1).astype(np.uint16).view(np.int16).copy())


class Harness:
    """the buffers of one case and the two argument lists (mutable: the argument checks change single entries)"""

    def __init__(self, lib, c, p=0.0, use_bits=True, dbd_fill=None):
        self.lib, self.c, self.p = lib, c, p
        T, S = c.T, c.S
        self.M, self.Mk = B * T, B * S
        self.thr, self.scale = DR.drop_threshold(p), R.inv_keep(p)
        self.ldq, self.ldt, self.ld_bd = C + 8, C + 16, _ld_bd(T)
        self.ldkv = 3 * C if T == S else 2 * C  # the encoder's / decoder's packed qkv, the cross attention's packed kv

        def inp(rows, ld, data):
            a = Alloc(rows, ld, BF)
            a.region(0, C, data)
            return a

        self.qu = inp(self.M, self.ldq, c.qu)
        self.qv = None if c.qv is None else (self.qu if c.qv is c.qu else inp(self.M, self.ldq, c.qv))
        self.kv = Alloc(self.Mk, self.ldkv, BF)
        self.kcol = self.ldkv - 2 * C
        self.kv.region(self.kcol, C, c.k)
        self.kv.region(self.kcol + C, C, c.v)
        self.pp = None if c.pp is None else inp(2 * T - 1, self.ldq, c.pp)
        self.klen = None if c.klen is None else torch.tensor(c.klen, dtype=torch.int32, device=DEV)
        self.dout = inp(self.M, self.ldq, c.dout)
        self.bits = None
        if p > 0 and use_bits and c.qv is not None:
            self.bits = Alloc(int(lib.ea_flash_keep_bits_bytes(H, B, T)) // 2, 1, I16, out=True, guard=256)
            self.t_bits = self.bits.region()
        # forward outputs
        self.out = Alloc(self.M, self.ldq, BF, out=True)
        self.t_out = self.out.region(0, C)
        self.lse = Alloc(H * B * T, 1, F32, out=True, guard=256)
        self.t_lse = self.lse.region()
        # backward outputs
        self.D = Alloc(H * B * T, 1, F32, out=True, guard=256)
        self.t_D = self.D.region()
        self.t1, self.t2 = Alloc(self.M, self.ldt, BF, out=True), Alloc(self.M, self.ldt, BF, out=True)
        self.t_t1 = self.t1.region(0, C)
        self.t_t2 = self.t2.region(0, C) if c.qv is not None else None
        self.dqkv = Alloc(self.Mk, 3 * C, BF, out=True)
        self.t_dq = self.dqkv.region(0, C) if c.qv is not None else None
        self.t_dk, self.t_dv = self.dqkv.region(C, C), self.dqkv.region(2 * C, C)
        self.dbd = None
        if c.qv is not None:
            self.dbd = Alloc(H * B * T, self.ld_bd, BF, out=True)
            self.t_dbd = self.dbd.region(fill_bits=dbd_fill)
        self.outs_fwd = [self.out, self.lse]
        self.outs_bwd = [a for a in (self.D, self.t1, self.t2, self.dqkv, self.dbd) if a is not None]

    def _p(self, a, col0=0):
        return None if a is None else a.ptr(col0)

    def fwd_args(self, flags=0):
        c = self.c
        return [self.qu.ptr(), self._p(self.qv), self.ldq, self.kv.ptr(self.kcol), self.kv.ptr(self.kcol + C), self.ldkv, self._p(self.pp),
                self.ldq if self.pp is not None else 0, None if self.klen is None else ctypes.c_void_p(self.klen.data_ptr()), self.out.ptr(), self.ldq,
                self.lse.ptr(), H, B, c.T, c.S, DH, int(c.causal) | flags, SEED, self.thr, self.scale, self._p(self.bits), _st()]

    def bwd_args(self, flags=0):
        """`out` and `lse` as inputs of their own: copies of the forward's results between NaN guards and gaps"""
        c = self.c
        self.out_in = Alloc(self.M, self.ldq, BF)
        self.out_in.region(0, C, self.t_out)
        self.lse_in = Alloc(H * B * c.T, 1, F32, guard=256)
        self.lse_in.region(data=self.t_lse)
        rel = c.qv is not None
        return [self.qu.ptr(), self._p(self.qv), self.ldq, self.kv.ptr(self.kcol), self.kv.ptr(self.kcol + C), self.ldkv, self._p(self.pp),
                self.ldq if rel else 0, None if self.klen is None else ctypes.c_void_p(self.klen.data_ptr()), self.out_in.ptr(), self.dout.ptr(), self.ldq,
                self.lse_in.ptr(), self.D.ptr(), self.t1.ptr(), self.t2.ptr() if rel else None, self.ldt, self._p(self.dbd), self.ld_bd if rel else 0,
                self.dqkv.ptr(C), self.dqkv.ptr(2 * C), 3 * C, H, B, c.T, c.S, DH, int(c.causal) | flags, c.scaling, SEED, self.thr, self.scale,
                self._p(self.bits), self.dqkv.ptr(0) if rel else None, 3 * C if rel else 0, _st()]

    def intact(self, allocs):
        return all(a.intact() for a in allocs) and (self.bits is None or self.bits.intact())

    def unwritten(self, allocs):
        """guards and gaps intact AND every claimed element still holds what it was filled with (NaN)"""
        return self.intact(allocs) and all(bool(torch.isnan(a.full[a.claimed]).all()) for a in allocs)

    def run(self, fwd_flags=0, bwd_flags=0, prefill_bits=False):
        lib, c = self.lib, self.c
        if prefill_bits:
            assert lib.ea_flash_keep_bits(self.bits.ptr(), H, B, c.T, SEED, self.thr, _st()) == 0
        assert lib.ea_flash_attention_fwd(*self.fwd_args(fwd_flags)) == 0
        torch.cuda.synchronize()
        assert self.intact(self.outs_fwd), "forward: a store outside out / lse / the keep bits"
        assert lib.ea_flash_attention_bwd(*self.bwd_args(bwd_flags)) == 0
        torch.cuda.synchronize()
        assert self.intact(self.outs_bwd), "backward: a store outside the gradients"
        v4 = lambda t, n: None if t is None else t.cpu().reshape(B, n, H, DH)
        z3 = lambda t: t.cpu().reshape(H, B, c.T)
        return dict(out=v4(self.t_out, c.T), lse=z3(self.t_lse), D=z3(self.t_D), t1=v4(self.t_t1, c.T), t2=v4(self.t_t2, c.T), dq=v4(self.t_dq, c.T),
                    dk=v4(self.t_dk, c.S), dv=v4(self.t_dv, c.S), dBD=None if self.dbd is None else self.t_dbd.cpu().reshape(H, B, c.T, self.ld_bd))


def _same_bits(a, b, what):
    for n in a:
        if a[n] is not None:
            assert torch.equal(_bits(a[n]), _bits(b[n])), f"{what}: {n} differs"


def _check_case(lib, c, p=0.0, label="", **kw):
    h = Harness(lib, c, p, **kw)
    got = h.run()
    _assert_ok(verify(_problem(c, p), c.dout, got), label)
    return h, got


# ------------------------------------------------------------------ flash_relpos.hip
@gpu
@pytest.mark.parametrize("T", [1, 15, 16, 17, 63, 64, 65, 127, 129, 193, 257])  # one row; a wave -1/+0/+1; a tile -1/+0/+1; two tiles -1, +1 (a
def test_relpos_row_wave_and_tile_edges(lib, T):                                 # one-row third); four key tiles; five: the ring of three is reused
    _check_case(lib, _case(T), label=f"relpos T={T}")


_KLEN = {65: (65, 64, 1), 129: (129, 65, 63), 257: (257, 128, 65)}


@gpu
@pytest.mark.parametrize("T,klen", [(65, _KLEN[65]), (129, _KLEN[129]), (257, _KLEN[257]), (257, (300, 200, 1))],
                         ids=["T65", "T129", "T257-skipped-tiles", "T257-clamped"])
def test_relpos_key_lengths(lib, T, klen):
    """klen on a tile boundary, one past it, one key; whole trailing key tiles skipped; klen > T clamped"""
    _check_case(lib, _case(T, klen=klen), label=f"relpos T={T} klen={klen}")


@gpu
@pytest.mark.parametrize("T,with_klen,p", [(65, False, 0.1), (65, True, 0.1), (129, False, 0.1), (129, True, 0.1), (257, False, 0.1), (257, True, 0.1),
                                           (129, True, 0.5)])
def test_relpos_dropout_and_keep_bits_on_the_side(lib, T, with_klen, p):
    """dropout against oracle/dropout_ref.py (seed with a non-zero high word), the keep-bit buffer bit for bit, and forward flag
    bit 4 (keep bits already evaluated by ea_flash_keep_bits): every output identical to the run that evaluates them itself"""
    c = _case(T, klen=_KLEN[T] if with_klen else None)
    h, got = _check_case(lib, c, p, label=f"relpos T={T} klen={c.klen} p={p}")
    assert torch.equal(h.t_bits.cpu().reshape(-1), _expected_keep_bits(T, p)), "keep bits differ from oracle/dropout_ref.py"
    h2 = Harness(lib, c, p)
    got2 = h2.run(fwd_flags=4, prefill_bits=True)
    _same_bits(got, got2, "keep bits evaluated beforehand (causal | 4)")


@gpu
def test_relpos_backward_with_dbd_prezeroed(lib):
    """backward flag bit 2: onto zeros the result is bit-identical to the plain run; onto the sentinel everything outside the band
    is untouched and everything inside it is written"""
    c = _case(129, klen=_KLEN[129])
    _, plain = _check_case(lib, c, label="relpos T=129 klen")
    _same_bits(plain, Harness(lib, c, dbd_fill=0).run(bwd_flags=2), "dBD pre-zeroed (causal | 2)")
    c = _case(129)
    _same_bits(Harness(lib, c).run(), Harness(lib, c, dbd_fill=0).run(bwd_flags=2), "dBD pre-zeroed (causal | 2), no klen")
    got = Harness(lib, c, dbd_fill=_SENTINEL[BF]).run(bwd_flags=2)
    _assert_ok(verify(_problem(c), c.dout, got, dbd_outside=_SENTINEL[BF]), "relpos T=129 dBD onto the sentinel")


@gpu
def test_relpos_qv_is_qu_with_an_unprojected_table(lib):
    """the engine's pos_mode == 1 call: qv and qu are the same buffer"""
    _check_case(lib, _case(129, klen=_KLEN[129], qv_is_qu=True, seed=5), label="relpos T=129 qv == qu")


# ------------------------------------------------------------------ flash_attention.hip (the general kernels)
@gpu
@pytest.mark.parametrize("T,p", [(65, 0.0), (129, 0.0), (65, 0.1), (129, 0.1)])
def test_general_kernels_relpos_form(lib, T, p):
    """ea_set_flash_relpos(0); with dropout the kernels re-evaluate the hash themselves (keep_bits = NULL)"""
    prev = lib.ea_set_flash_relpos(0)
    try:
        _check_case(lib, _case(T, klen=_KLEN[T], seed=2), p, label=f"general relpos T={T} p={p}", use_bits=False)
    finally:
        lib.ea_set_flash_relpos(prev)


@gpu
@pytest.mark.parametrize("T,p", [(65, 0.0), (129, 0.0), (129, 0.1)])
def test_general_kernels_absolute_position_causal(lib, T, p):
    h, _ = _check_case(lib, _case(T, relpos=False, causal=True, seed=3), p, label=f"causal T={T} p={p}")
    assert h.t2.intact() and bool((_bits(h.dqkv.full[:, :C]) == _SENTINEL[BF]).all()), "t2 / dq written without qv"


@gpu
@pytest.mark.parametrize("T,S,klen", [(17, 130, (130, 65, 1)), (130, 17, (17, 16, 1)), (64, 65, (65, 64, 63))])
def test_general_kernels_cross_attention(lib, T, S, klen):
    """t1 is the query gradient; t2, dBD and dq are NULL"""
    _check_case(lib, _case(T, S, klen=klen, relpos=False, seed=4), label=f"cross T={T} S={S}")


# ------------------------------------------------------------------ argument checks
@gpu
def test_rejected_calls_return_minus_two_and_write_nothing(lib):
    c = _case(17)
    h = Harness(lib, c)
    every = h.outs_fwd + h.outs_bwd
    FWD = dict(ldq=2, qu=0, dh=16)
    BWD = dict(ldq=2, qu=0, qv=1, ld_bd=18, dh=26, dq=33)

    def fwd(**ch):
        a = h.fwd_args()
        for n, val in ch.items():
            a[FWD[n]] = val
        return lib.ea_flash_attention_fwd(*a)

    def bwd(**ch):
        a = h.bwd_args()
        for n, val in ch.items():
            a[BWD[n]] = val
        return lib.ea_flash_attention_bwd(*a)

    assert fwd(ldq=h.ldq + 4) == -2 and bwd(ldq=h.ldq + 4) == -2, "ldq % 8 != 0"
    assert fwd(qu=h.qu.ptr(byte_off=2)) == -2 and bwd(qu=h.qu.ptr(byte_off=2)) == -2, "qu not 16-byte aligned"
    assert (2 * c.T - 2) % 8 == 0 and bwd(ld_bd=2 * c.T - 2) == -2, "ld_bd < 2T - 1"
    assert fwd(dh=32) == -2 and bwd(dh=32) == -2, "dh != 64"
    torch.cuda.synchronize()
    assert h.unwritten(every), "a rejected call wrote something"
    # dq without qv: the absolute-position form, with a dq pointer
    c2 = _case(17, relpos=False)
    h2 = Harness(lib, c2)
    assert lib.ea_flash_attention_fwd(*h2.fwd_args()) == 0
    a = h2.bwd_args()
    a[BWD["dq"]], a[BWD["dq"] + 1] = h2.dqkv.ptr(0), 3 * C
    assert lib.ea_flash_attention_bwd(*a) == -2, "dq without qv"
    torch.cuda.synchronize()
    assert h2.unwritten(h2.outs_bwd), "a rejected call wrote something"
    # T <= 0: nothing to do
    a, b = h.fwd_args(), h.bwd_args()
    a[14], b[24] = 0, 0
    assert lib.ea_flash_attention_fwd(*a) == 0 and lib.ea_flash_attention_bwd(*b) == 0
    torch.cuda.synchronize()
    assert h.unwritten(every), "a call with T = 0 wrote something"
