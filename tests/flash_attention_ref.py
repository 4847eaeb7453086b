"""TEST INFRASTRUCTURE ONLY — the fused attention of espresso_amd/csrc/flash_relpos.hip and flash_attention.hip restated plainly
in float64 on the CPU: no tiling, no online softmax, the backward pass written out by hand (not autograd).

  S[i][j] = qu_i . k_j + qv_i . pp[T-1-i+j]       (the positional term only with qv); keys j >= min(klen[b], S) are -inf, with
                                                   the causal flag keys j > i + (S - T) as well
  P = softmax(S), lse = logsumexp(S), Pd = P * keep / (1-p), out = Pd V
  keep = oracle.dropout_ref at element ((h*B + b)*T + i)*S + j; 1/(1-p) is the fp32 value the kernels are handed
  D = sum_d out dout, dPd = dout V^T, dS = P * (dPd * keep/(1-p) - D)
  t1 = scaling dS K, t2 = scaling dS PP_band, dq = t1 + t2, dBD[z][i][T-1-i+j] = dS[i][j] (zero elsewhere, up to ld_bd)
  dK = dS^T Qu, dV = Pd^T dout

Layouts: qu / qv / out / dout / t1 / t2 / dq [B][T][H][64]; k / v / dK / dV [B][S][H][64]; pp [2T-1][H][64]; everything per
(head, sentence, row[, key]) is [H][B][T]([S]); dBD [H][B][T][ld_bd].  Every stage takes the earlier stages' results as optional
arguments, so that a later stage can be evaluated on a kernel's own lse / D / out; every stage also returns the magnitude sums
an error bound needs.  `fault` plants one deliberate mistake (tests/test_flash_attention_kernels.py proves that its bounds see each)."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import dropout_ref as DR

F64 = torch.float64
FAULTS = ("mask-1", "mask+1", "pos-1", "pos+1", "keep_z_swapped", "fwd_no_keep_scale", "D_without_dropout", "kv_last_row_twice",
          "dbd_band_shifted")


def f64(x):
    return x.detach().cpu().to(F64)


def inv_keep(p):
    """1/(1-p) as the fp32 number the kernels receive (oracle.dropout_ref.scale_mask's)"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def problem(qu, k, v, qv=None, pp=None, klen=None, causal=False, p=0.0, seed=0, scaling=1.0):
    """the operands (bf16 or anything else) cast to float64; H, B, T, S from their shapes"""
    B, T, H, dh = qu.shape
    return SimpleNamespace(qu=f64(qu), k=f64(k), v=f64(v), qv=None if qv is None else f64(qv), pp=None if pp is None else f64(pp),
                           klen=None if klen is None else [int(n) for n in klen], causal=bool(causal), p=float(p), seed=int(seed),
                           scaling=float(scaling), B=B, T=T, H=H, S=k.shape[1], dh=dh)


def band_index(T, S, shift=0):
    """r[i][j] = T-1-i+j: the row of the positional table (and the column of dBD) that pairs query i with key j"""
    r = (T - 1) - torch.arange(T)[:, None] + torch.arange(S)[None, :] + shift
    return r.clamp(0, T + S - 2)


def key_limits(x, fault=None):
    kl = [min(n, x.S) for n in x.klen] if x.klen is not None else [x.S] * x.B
    if fault == "mask-1":  # the last valid key masked (where that leaves one)
        kl = [n - 1 if n >= 2 else n for n in kl]
    if fault == "mask+1":  # the first padded key admitted
        kl = [n + 1 if n < x.S else n for n in kl]
    return kl


def valid_mask(x, fault=None):
    """[B][T][S] bool"""
    j = torch.arange(x.S)
    ok = torch.stack([(j < n)[None, :].expand(x.T, x.S) for n in key_limits(x, fault)])
    if x.causal:
        ok = ok & (j[None, :] <= torch.arange(x.T)[:, None] + (x.S - x.T))[None]
    return ok


def keep_scale(x, fault=None, scaled=True):
    """[H][B][T][S]: 0 or 1/(1-p)"""
    if x.p <= 0:
        return torch.ones(x.H, x.B, x.T, x.S, dtype=F64)
    m = torch.from_numpy(DR.keep_mask(x.seed, x.H * x.B * x.T * x.S, x.p).astype(np.float64))
    if fault == "keep_z_swapped":  # the mask read with z = b*H + h
        m = m.view(x.B, x.H, x.T, x.S).transpose(0, 1).contiguous()
    return m.view(x.H, x.B, x.T, x.S) * (inv_keep(x.p) if scaled else 1.0)


def sum_keys(W, k):
    """sum_j W[h][b][i][j] k[b][j][h][d] -> [B][T][H][64]"""
    return torch.einsum("hbij,bjhd->bihd", W, k)


def sum_rows(W, q):
    """sum_i W[h][b][i][j] q[b][i][h][d] -> [B][S][H][64]"""
    return torch.einsum("hbij,bihd->bjhd", W, q)


def to_band(W, T, S, ld_bd, shift_rows=None):
    """[H][B][T][S] -> [H][B][T][ld_bd] with W[i][j] at column T-1-i+j, zero elsewhere"""
    r = band_index(T, S)
    if shift_rows is not None:
        r = r.clone()
        r[shift_rows[0]:shift_rows[1]] += 1
    out = torch.zeros(*W.shape[:3], ld_bd, dtype=W.dtype)
    return out.scatter_(3, r.expand(*W.shape[:2], T, S), W)


def sum_band(W, pp, T, S):
    """sum_j W[h][b][i][j] pp[T-1-i+j][h][d] -> [B][T][H][64]"""
    return torch.einsum("hbir,rhd->bihd", to_band(W, T, S, T + S - 1), pp)


def scores(x, fault=None):
    """S [H][B][T][S] with -inf at the masked keys, and sum_d |qu||k| + sum_d |qv||pp| of every score"""
    s = torch.einsum("bihd,bjhd->hbij", x.qu, x.k)
    mag = torch.einsum("bihd,bjhd->hbij", x.qu.abs(), x.k.abs())
    if x.qv is not None:
        assert x.T == x.S
        r = band_index(x.T, x.S, {"pos-1": -1, "pos+1": 1}.get(fault, 0)).expand(x.H, x.B, x.T, x.S)
        s = s + torch.einsum("bihd,rhd->hbir", x.qv, x.pp).gather(3, r)
        mag = mag + torch.einsum("bihd,rhd->hbir", x.qv.abs(), x.pp.abs()).gather(3, r)
    return s.masked_fill(~valid_mask(x, fault)[None], float("-inf")), mag


def softmax(s, lse=None):
    """P and lse; with `lse` given (a kernel's), P = exp(S - lse) as the backward kernels recompute it"""
    if lse is None:
        lse = torch.logsumexp(s, dim=-1)
    return torch.exp(s - lse[..., None]), lse


def forward(x, fault=None):
    s, smag = scores(x, fault)
    P, lse = softmax(s)
    ks = keep_scale(x, fault, scaled=fault != "fwd_no_keep_scale")
    Pd = P * ks
    return SimpleNamespace(S=s, smag=smag, P=P, lse=lse, Pd=Pd, out=sum_keys(Pd, x.v), out_mag=sum_keys(Pd, x.v.abs()))


def row_dot(out, dout):
    """D [H][B][T] = sum_d out dout, and sum_d |out dout|"""
    return (out * dout).sum(-1).permute(2, 0, 1), (out * dout).abs().sum(-1).permute(2, 0, 1)


def backward(x, dout, lse=None, D=None, out=None, ld_bd=None, fault=None):
    """dout [B][T][H][64].  lse / D / out: a kernel's own (float64 casts), else the reference's"""
    dout = f64(dout)
    s, smag = scores(x, fault)
    P, lse = softmax(s, lse)
    ks = keep_scale(x, fault)
    Pd = P * ks
    dPd = torch.einsum("bihd,bjhd->hbij", dout, x.v)
    dp_mag = torch.einsum("bihd,bjhd->hbij", dout.abs(), x.v.abs())
    if D is None:
        if fault == "D_without_dropout":
            D = (P * dPd).sum(-1)
        else:
            D, _ = row_dot(sum_keys(Pd, x.v) if out is None else out, dout)
    dPs = dPd * ks
    dS = P * (dPs - D[..., None])
    r = SimpleNamespace(S=s, smag=smag, P=P, lse=lse, Pd=Pd, keep=ks, dp_mag=dp_mag, dPs=dPs, D=D, dS=dS)
    r.t1, r.t1_mag = x.scaling * sum_keys(dS, x.k), abs(x.scaling) * sum_keys(dS.abs(), x.k.abs())
    dSk, Pdk = dS, Pd
    if fault == "kv_last_row_twice":  # what a clamped query row >= T adds if it is not masked
        w = torch.ones(x.T, dtype=F64)
        w[-1] = 2.0
        dSk, Pdk = dS * w[:, None], Pd * w[:, None]
    r.dK, r.dK_mag = sum_rows(dSk, x.qu), sum_rows(dS.abs(), x.qu.abs())
    r.dV, r.dV_mag = sum_rows(Pdk, dout), sum_rows(Pd, dout.abs())
    if x.qv is not None:
        ld_bd = x.T + x.S - 1 if ld_bd is None else ld_bd
        r.t2, r.t2_mag = x.scaling * sum_band(dS, x.pp, x.T, x.S), abs(x.scaling) * sum_band(dS.abs(), x.pp.abs(), x.T, x.S)
        r.dq = r.t1 + r.t2
        lo = 16 if x.T > 16 else 0
        r.dBD = to_band(dS, x.T, x.S, ld_bd, (lo, lo + 16) if fault == "dbd_band_shifted" else None)
        r.band = to_band(torch.ones_like(dS), x.T, x.S, ld_bd) > 0
    return r
