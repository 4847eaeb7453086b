"""Plain fp64 restatement of ea_gemm_bf16 and ea_wgrad_group (include/espresso_amd.h:42-51, 81-86, 121-126; the kernels are
espresso_amd/csrc/gemm.hip, gemm_w8.hip, wgrad_w8.hip and the shared epilogue gemm_epilogue.h).

Plain torch, no call into espresso_amd.  The operands are taken as the kernels take them — a flat piece of memory, a base offset
per batch item, a row pitch and a layout flag — and upcast exactly to fp64; nothing is rounded on the way except where the header
rounds (the query split's first bf16 store).  Next to each value the functions return `mag`, the same expression taken over the
magnitudes of its terms, which an error bound of the form `k * 2^-23 * mag` needs.

  A(z; m, k) = A[(z / zdiv) * sA_hi + (z % zdiv) * sA_lo + (a_kstrided ? k * lda + m : m * lda + k)],  B likewise with n
  v = alpha * sum_k A(z; m, k) B(z; n, k) + bias[n]
  aux:          v = v * keep * act'(aux[z][m][n])
  two outputs:  C = v, C2 = keep * act(v)                                  (nothing else is applied)
  otherwise:    v = keep * act(v)
  v = v * out_scale + resid[z][m][n];   C = prefill + v (accumulate) or v
  query split:  q = bf16(alpha * acc + bias) for the columns n < qsplit_n, q_u = (q + pos_u[n]) * qscale, q_v likewise
keep(z, m, n) = oracle.dropout_ref at the element index (z * M + m) * N + n: 0 or 1 / (1 - p) (the fp32 value the kernels multiply by).

`mag` through an activation: ReLU and the identity pass it on unchanged (|relu(a) - relu(b)| <= |a - b|), SiLU multiplies it by
SILU_LIP = 1.1 (max |silu'| = 1.0998), act'(aux) multiplies it by |act'(aux)|.

tests/test_gemm_kernels.py proves this file against torch.bmm, F.silu, F.relu and autograd (CPU, float64)."""
import numpy as np
import torch

from oracle import dropout_ref

F64 = torch.float64
ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2
SILU_LIP = 1.1


def f64(x):
    return x.detach().to(F64)


def bf16_rne(x):
    """round-to-nearest-even onto the bf16 grid (8 significant bits), carried out in fp64: no double rounding through fp32"""
    x = f64(x)
    _, e = torch.frexp(x)                       # |x| = m 2^e, m in [0.5, 1): the bf16 step at |x| is 2^(e - 8)
    step = torch.exp2((e - 8).to(F64))
    return torch.where(x == 0, x, torch.round(x / step) * step)   # torch.round: halves to even


def operand(flat, rows, K, batch, zdiv, ld, kstrided, s_hi, s_lo):
    """-> [batch][rows][K] fp64: element (z; r, k) read from the flat memory at the header's address"""
    z = torch.arange(batch).view(batch, 1, 1)
    r = torch.arange(rows).view(1, rows, 1)
    k = torch.arange(K).view(1, 1, K)
    idx = (z // zdiv) * s_hi + (z % zdiv) * s_lo + ((k * ld + r) if kstrided else (r * ld + k))
    return f64(flat.reshape(-1))[idx]


def drop_params(p):
    """(threshold, fp32 keep-scale) as the callers of the library compute them"""
    return dropout_ref.drop_threshold(p), float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep(seed, p, batch, M, N):
    """[batch][M][N] fp64: 0 where element (z, m, n) — index (z * M + m) * N + n — is dropped, else 1 / (1 - p)"""
    return dropout_ref.scale_mask(seed, (batch, M, N), p).to(F64)


def act(v, kind):
    if kind == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if kind == ACT_SILU:
        return v / (1.0 + torch.exp(-v))
    return v


def dact(z, kind):
    if kind == ACT_RELU:
        return (z > 0).to(F64)
    if kind == ACT_SILU:
        s = 1.0 / (1.0 + torch.exp(-z))
        return s * (1.0 + z * (1.0 - s))
    return torch.ones_like(z)


def act_lip(kind):
    return SILU_LIP if kind == ACT_SILU else 1.0


def query(q_pre, pos, qscale):
    """the query split's second step on the unrounded q: (bf16(q) + pos[n]) * qscale (pos None: zeros)"""
    q = bf16_rne(q_pre)
    return (q if pos is None else q + f64(pos)) * qscale


def gemm(A, B, M, N, K, *, batch=1, zdiv=1, a_kstrided=False, b_kstrided=False, lda=None, ldb=None, sA=(0, 0), sB=(0, 0), alpha=1.0,
         bias=None, activation=ACT_NONE, keep_scale=None, aux=None, two_outputs=False, out_scale=1.0, resid=None, prefill=None,
         qsplit=None):
    """A, B: flat memory.  bias [N]; keep_scale, aux, resid, prefill: [batch][M][N] or None.  qsplit = (qsplit_n, pos_u, pos_v, qscale).
    -> dict of fp64 [batch][M][N] tensors (unrounded): C, C_mag; with two_outputs also C2, C2_mag; with qsplit also q_pre, q_pre_mag
    [batch][M][qsplit_n] (the unrounded q), q_u, q_v (columns < qsplit_n of C are not the library's to write)."""
    lda = lda if lda is not None else (M if a_kstrided else K)
    ldb = ldb if ldb is not None else (N if b_kstrided else K)
    a = operand(A, M, K, batch, zdiv, lda, a_kstrided, *sA)
    b = operand(B, N, K, batch, zdiv, ldb, b_kstrided, *sB)
    v = alpha * torch.matmul(a, b.transpose(1, 2))
    mag = abs(alpha) * torch.matmul(a.abs(), b.abs().transpose(1, 2))
    if bias is not None:
        v = v + f64(bias)
        mag = mag + f64(bias).abs()
    out = {}
    if qsplit is not None:
        qn, pos_u, pos_v, qscale = qsplit
        out["q_pre"], out["q_pre_mag"] = v[..., :qn].clone(), mag[..., :qn].clone()
        out["q_u"], out["q_v"] = query(out["q_pre"], pos_u, qscale), query(out["q_pre"], pos_v, qscale)
    kp = torch.ones_like(v) if keep_scale is None else f64(keep_scale)
    if aux is not None:
        d = dact(f64(aux), activation)
        v, mag = v * kp * d, mag * kp * d.abs()
    elif two_outputs:
        out.update(C=v, C_mag=mag, C2=kp * act(v, activation), C2_mag=kp * act_lip(activation) * mag)
        return out
    else:
        v, mag = kp * act(v, activation), kp * act_lip(activation) * mag
    v, mag = v * out_scale, mag * abs(out_scale)
    if resid is not None:
        v, mag = v + f64(resid), mag + f64(resid).abs()
    if prefill is not None:
        v, mag = f64(prefill) + v, f64(prefill).abs() + mag
    out.update(C=v, C_mag=mag)
    return out


def wgrad(dy, x, dW0=None, db0=None):
    """dy [M][N], x [M][K] -> (dW0 + dy^T x [N][K], db0 + colsum(dy) [N], mag of dW, mag of db)"""
    dy, x = f64(dy), f64(x)
    dW, wmag = torch.matmul(dy.t(), x), torch.matmul(dy.abs().t(), x.abs())
    db, bmag = dy.sum(0), dy.abs().sum(0)
    if dW0 is not None:
        dW, wmag = f64(dW0) + dW, f64(dW0).abs() + wmag
    if db0 is not None:
        db, bmag = f64(db0) + db, f64(db0).abs() + bmag
    return dW, db, wmag, bmag
