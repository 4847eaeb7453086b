"""Plain fp64 restatement of the LayerNorm kernels (espresso_amd/csrc/layernorm.hip; include/espresso_amd.h:150-205) and of the
streaming element-wise kernels (espresso_amd/csrc/elementwise.hip; include/espresso_amd.h:207-246).

Plain torch, no call into espresso_amd.  Operands are upcast exactly to fp64 and nothing is rounded on the way except where the
header rounds (the gradient between the two norms of the pair, the dx that the second output starts from, the casts).  Next to each
value the functions return `*_mag`, the same expression over the magnitudes of its terms, and the sensitivities an error bound of
the form `k * 2^-23 * mag` needs.

  LayerNorm      mean = sum_c x / C, rstd = 1 / sqrt(sum_c (x - mean)^2 / C + eps), y = ((x - mean) rstd gamma + beta) keep live
  its backward   xhat = (x - mean) rstd, dv = dy keep live, g = dv gamma, dx = rstd (g - mean_c g - xhat mean_c(g xhat)) + dx_add,
                 dgamma += sum_m dv xhat, dbeta += sum_m dv, out2 = a2 keep2 bf16(dx)          (mean, rstd: the kernel's inputs)
  keep(m, c) = oracle.dropout_ref at the element index m * C + c: 0 or 1 / (1 - p), the fp32 value the kernels multiply by
  live(m)    = 0 where row_zero[m], else 1

tests/test_layernorm_kernels.py and tests/test_elementwise_kernels.py prove this file against F.layer_norm, autograd, F.embedding,
torch.sum and .t() (CPU, float64)."""
import numpy as np
import torch

from oracle import dropout_ref
from tests.gemm_ref import bf16_rne, drop_params, f64  # noqa: F401 (re-exported)

F64 = torch.float64


def keep(seed, p, M, C, shift=0):
    """[M][C] fp64 keep-scales at the element index m * C + c + shift (shift != 0: only the mutation tests)"""
    n = M * C
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    k = dropout_ref.keep_mask(seed, n, p, idx0=shift).astype(np.float32) * inv
    return torch.from_numpy(k).view(M, C).to(F64)


def _keep_live(M, C, row_zero, drop, shift=0):
    k = torch.ones(M, C, dtype=F64) if drop is None else keep(drop[0], drop[1], M, C, shift)
    if row_zero is not None:
        k = k * (1.0 - (f64(row_zero) != 0).to(F64)).view(M, 1)
    return k


def f32_eps(eps):
    """the fp32 value the C ABI receives for `eps`"""
    return float(np.float32(eps))


def ln_fwd(x, gamma, beta, eps, row_zero=None, drop=None, drop_shift=0):
    """x [M][C], gamma, beta [C]; drop = (seed, p) or None -> dict: mean, rstd [M]; y, y_mag [M][C]; the sensitivities
    absd = |x - mean| [M][C], absmean = |mean|, a1 = mean_c |x|, w = variance + eps [M]; keep [M][C] (keep * live)"""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    M, C = x.shape
    mean = x.sum(1) / C
    d = x - mean.view(M, 1)
    w = (d * d).sum(1) / C + f32_eps(eps)
    rstd = 1.0 / torch.sqrt(w)
    k = _keep_live(M, C, row_zero, drop, drop_shift)
    r = rstd.view(M, 1)
    return dict(mean=mean, rstd=rstd, y=(d * r * gamma + beta) * k, y_mag=(d.abs() * r * gamma.abs() + beta.abs()) * k,
                absd=d.abs(), absmean=mean.abs(), a1=x.abs().sum(1) / C, w=w, keep=k)


def ln_bwd(x, dy, gamma, mean, rstd, row_zero=None, drop=None, dx_add=None, dgamma0=None, dbeta0=None, out2=None, rows=None):
    """mean, rstd [M]: the values the kernel is given.  out2 = (a2, (seed2, p2) or None).  rows: only these rows enter dgamma /
    dbeta (the mutation tests).  -> dict: dx, dx_mag [M][C] (dx unrounded, dx_add included); dgamma, dbeta, dgamma_mag, dbeta_mag
    [C] (pre-fill included); term_g, term_b [M][C], the rows' contributions; with out2: out2 [M][C] = a2 keep2 bf16(dx), keep2"""
    x, dy, gamma, mean, rstd = f64(x), f64(dy), f64(gamma), f64(mean), f64(rstd)
    M, C = x.shape
    r = rstd.view(M, 1)
    h = (x - mean.view(M, 1)) * r
    dv = dy * _keep_live(M, C, row_zero, drop)
    g = dv * gamma
    s1, s2 = g.sum(1, keepdim=True) / C, (g * h).sum(1, keepdim=True) / C
    m1, m2 = g.abs().sum(1, keepdim=True) / C, (g * h).abs().sum(1, keepdim=True) / C
    dx, mag = r * (g - s1 - h * s2), r * (g.abs() + m1 + h.abs() * m2)
    if dx_add is not None:
        dx, mag = dx + f64(dx_add), mag + f64(dx_add).abs()
    tg, tb = dv * h, dv
    sel = slice(None) if rows is None else rows
    out = dict(dx=dx, dx_mag=mag, term_g=tg, term_b=tb, dgamma=tg[sel].sum(0), dbeta=tb[sel].sum(0),
               dgamma_mag=tg[sel].abs().sum(0), dbeta_mag=tb[sel].abs().sum(0))
    for k, pre in (("dgamma", dgamma0), ("dbeta", dbeta0)):
        if pre is not None:
            out[k], out[k + "_mag"] = f64(pre) + out[k], f64(pre).abs() + out[k + "_mag"]
    if out2 is not None:
        a2, drop2 = out2
        out["keep2"] = _keep_live(M, C, None, drop2)
        out["out2"] = a2 * out["keep2"] * bf16_rne(dx)
    return out


def second_output(dx, a2, keep2):
    """out2 from a given (stored, or bounding) dx: a2 keep2 bf16(dx)"""
    return a2 * keep2 * bf16_rne(dx)


def ln_bwd_pair(x1, dy1, gamma1, mean1, rstd1, dx_add, x2, gamma2, mean2, rstd2, out2=None, rnd=bf16_rne):
    """the backward of two LayerNorms back to back: d = bf16(LNbwd1 + dx_add), dx = LNbwd2(d) (unrounded), out2 = a2 keep2 bf16(dx).
    rnd: the rounding of d (the identity: the CPU comparison with autograd).  -> (first norm's dict with d = rnd(dx), second's)"""
    b1 = ln_bwd(x1, dy1, gamma1, mean1, rstd1, dx_add=dx_add)
    b1["d"] = rnd(b1["dx"])
    return b1, ln_bwd(x2, b1["d"], gamma2, mean2, rstd2, out2=out2)


# ------------------------------------------------------------------ element-wise
def scale_dropout(x, y, a, b, keep_scale=None):
    """a x keep + b y (y None: read as +0, include/espresso_amd.h — the sign of a zero result follows) -> (value, mag)"""
    x = f64(x)
    k = torch.ones_like(x) if keep_scale is None else f64(keep_scale)
    y = torch.zeros_like(x) if y is None else f64(y)
    return a * x * k + b * y, abs(a) * x.abs() * k + abs(b) * y.abs()


def keep_flat(seed, p, n, shift=0):
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return torch.from_numpy(dropout_ref.keep_mask(seed, n, p, idx0=shift).astype(np.float32) * inv).to(F64)


def colsum(X, out0=None):
    """X [M][N] -> (out0 + column sums, mag)"""
    X = f64(X)
    v, mag = X.sum(0), X.abs().sum(0)
    if out0 is not None:
        v, mag = f64(out0) + v, f64(out0).abs() + mag
    return v, mag


def embedding_fwd(tok, position, W, pos, scale):
    """scale W[tok] + pos[position] (pos None: the first term alone) -> (value, mag)"""
    v = scale * f64(W)[tok.long()]
    mag = v.abs()
    if pos is not None:
        v, mag = v + f64(pos)[position.long()], mag + f64(pos)[position.long()].abs()
    return v, mag


def embedding_bwd(tok, dy, dW0, scale, pad_idx):
    """dW[tok[m]] += scale dy[m] for tok[m] != pad_idx -> (dW, mag, rows added per vocabulary row [V])"""
    dy = f64(dy)
    dW, mag = f64(dW0).clone(), f64(dW0).abs()
    hits = torch.zeros(dW.shape[0], dtype=torch.long)
    for m, t in enumerate(tok.tolist()):   # (plain: the restatement of a scatter with collisions)
        if t == pad_idx:
            continue
        dW[t] += scale * dy[m]
        mag[t] += abs(scale) * dy[m].abs()
        hits[t] += 1
    return dW, mag, hits


def transpose(X):
    return X.transpose(0, 1).contiguous()


def cast_f32_to_bf16_bits(x):
    """fp32 -> bf16 bit patterns (int16), round-to-nearest-even from the bit pattern, NaN kept (a quiet NaN of the same sign):
    b + 0x7fff + (bit 16 of b) >> 16"""
    b = x.detach().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    r = torch.where(nan, (b >> 16) | 0x0040, r) & 0xFFFF
    return torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)


def cast_bf16_to_f32_bits(bits16):
    """bf16 bit patterns (int16) -> fp32 bit patterns (int32): the pattern shifted up by 16"""
    b = (bits16.to(torch.int64) & 0xFFFF) << 16
    return torch.where(b >= 0x80000000, b - 0x100000000, b).to(torch.int32)
