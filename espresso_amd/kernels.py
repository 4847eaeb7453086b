"""Thin, typed Python wrappers over the C ABI (include/espresso_amd.h).

Every function takes CUDA(=HIP) torch tensors, checks dtype/contiguity, and launches the HIP kernel
on torch's current stream.  torch is used here ONLY for device memory and streams.  Nothing in this
module computes on the host and nothing falls back to eager PyTorch: a missing library or a CPU
tensor raises.
"""
import ctypes
from typing import Optional

import torch

from . import _lib
from ._lib import EaGemmParams, check

ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2
_ACT = {None: 0, "none": 0, "relu": 1, "silu": 2, "swish": 2}


def _stream():
    """Raw handle of torch's current HIP stream on the current device (the C accessors: `torch.cuda.current_stream()` builds a
    Python Stream object through several device-index lookups, ~9 us per call — per kernel launch that was 12 % of the
    transducer beam search's host time)."""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("espresso_amd kernels need device tensors (no CPU path)")
    return ctypes.c_void_p(t.data_ptr())


def drop_params(p: float):
    """(threshold, keep-scale) for dropout probability p as the kernels expect them."""
    if p <= 0.0:
        return 0, 1.0
    thr = min(int(p * 4294967296.0), 4294967295)
    return thr, 1.0 / (1.0 - p)


def gemm(
    A: torch.Tensor,
    B: torch.Tensor,
    C: torch.Tensor,
    M: int,
    N: int,
    K: int,
    *,
    lda: int,
    ldb: int,
    ldc: int,
    a_kstrided: bool = False,
    b_kstrided: bool = False,
    batch: int = 1,
    zdiv: int = 1,
    sA=(0, 0),
    sB=(0, 0),
    sC=(0, 0),
    a_off: int = 0,
    b_off: int = 0,
    c_off: int = 0,
    bias: Optional[torch.Tensor] = None,
    act=None,
    alpha: float = 1.0,
    out_scale: float = 1.0,
    resid: Optional[torch.Tensor] = None,
    ldr: int = 0,
    sR=(0, 0),
    r_off: int = 0,
    C2: Optional[torch.Tensor] = None,
    ldc2: int = 0,
    aux: Optional[torch.Tensor] = None,
    ldaux: int = 0,
    sX=(0, 0),
    accumulate: bool = False,
    drop_p: float = 0.0,
    drop_seed: int = 0,
    splitk: int = 1,
    qsplit=None,
):
    """C[z][m][n] = epi(alpha * sum_k A(z;m,k) B(z;n,k)).  Offsets (a_off, ...) are in elements.
    qsplit = (q_u, q_v | None, pos_u | None, pos_v | None, n, ld_q, scale): columns [0, n) go to q_u / q_v as
    (q + pos) * scale instead of C (EaGemmParams.q_u in the header)."""
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16
    assert C.dtype in (torch.bfloat16, torch.float32)
    p = EaGemmParams()
    p.A = A.data_ptr() + 2 * a_off
    p.B = B.data_ptr() + 2 * b_off
    p.C = C.data_ptr() + C.element_size() * c_off
    p.C2 = (C2.data_ptr() + 2 * c_off) if C2 is not None else None
    if bias is not None:
        assert bias.dtype == torch.float32
        p.bias = bias.data_ptr()
    if resid is not None:
        assert resid.dtype in (torch.bfloat16, torch.float32)
        p.resid = resid.data_ptr() + resid.element_size() * r_off
        p.resid_f32 = 1 if resid.dtype == torch.float32 else 0
    if aux is not None:
        assert aux.dtype == torch.bfloat16
        p.aux = aux.data_ptr()
    p.M, p.N, p.K, p.batch, p.zdiv = M, N, K, batch, zdiv
    p.a_kstrided, p.b_kstrided = int(a_kstrided), int(b_kstrided)
    p.c_f32 = 1 if C.dtype == torch.float32 else 0
    p.accumulate = int(accumulate)
    p.act = _ACT[act] if not isinstance(act, int) else act
    p.lda, p.ldb, p.ldc, p.ldc2, p.ldr, p.ldaux = lda, ldb, ldc, ldc2, ldr, ldaux
    p.sA_hi, p.sA_lo = sA
    p.sB_hi, p.sB_lo = sB
    p.sC_hi, p.sC_lo = sC
    p.sR_hi, p.sR_lo = sR
    p.sX_hi, p.sX_lo = sX
    p.alpha, p.out_scale = alpha, out_scale
    thr, scale = drop_params(drop_p)
    p.drop_seed, p.drop_thr, p.drop_scale = drop_seed, thr, scale
    p.splitk = max(1, int(splitk))
    ws = None
    if p.splitk > 1:
        ws = torch.empty(p.splitk * batch * M * N, dtype=torch.float32, device=C.device)
        p.workspace = ws.data_ptr()
    if qsplit is not None:
        q_u, q_v, pos_u, pos_v, qn, ld_q, qscale = qsplit
        assert q_u.dtype == torch.bfloat16 and (q_v is None or q_v.dtype == torch.bfloat16)
        assert (pos_u is None or pos_u.dtype == torch.float32) and (pos_v is None or pos_v.dtype == torch.float32)
        p.q_u, p.q_v, p.pos_u, p.pos_v = _p(q_u), _p(q_v), _p(pos_u), _p(pos_v)
        p.qsplit_n, p.ld_q, p.qscale = int(qn), int(ld_q), float(qscale)
    check(_lib.lib().ea_gemm_bf16(ctypes.byref(p), _stream()), "ea_gemm_bf16")
    return C


def layernorm_fwd(x, gamma, beta, eps=1e-5, row_zero=None, drop_p=0.0, drop_seed=0, save_stats=True, out_f32=False):
    """out_f32: the output stays fp32 (an fp32 island of the reference's autocast run: the joint network's LayerNorms)."""
    M, C = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    y = torch.empty(M, C, dtype=torch.float32, device=x.device) if out_f32 else torch.empty_like(x)
    mean = torch.empty(M, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(M, dtype=torch.float32, device=x.device) if save_stats else None
    thr, scale = drop_params(drop_p)
    fn = _lib.lib().ea_layernorm_fwd_f32out if out_f32 else _lib.lib().ea_layernorm_fwd
    check(fn(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), M, C, eps, _p(row_zero), drop_seed, thr, scale, _stream()),
          "ea_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(x, dy, gamma, mean, rstd, dgamma, dbeta, row_zero=None, drop_p=0.0, drop_seed=0, dx_add=None):
    M, C = x.shape
    assert dy.is_contiguous() and dy.dtype in (torch.bfloat16, torch.float32)
    dx = torch.empty_like(x)
    thr, scale = drop_params(drop_p)
    ws = torch.empty(_lib.lib().ea_layernorm_bwd_workspace_bytes(M, C) // 4, dtype=torch.float32, device=x.device)
    fn = _lib.lib().ea_layernorm_bwd_f32dy if dy.dtype == torch.float32 else _lib.lib().ea_layernorm_bwd
    check(fn(_p(x), _p(dy), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dgamma), _p(dbeta), M, C, _p(row_zero), drop_seed, thr, scale,
             _p(dx_add), _p(ws), _stream()), "ea_layernorm_bwd")
    return dx


def cast_f32_to_bf16(src, dst=None):
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    check(_lib.lib().ea_cast_f32_to_bf16(_p(src), _p(dst), src.numel(), _stream()), "ea_cast_f32_to_bf16")
    return dst


def cast_f32_to_bf16_rows(src, ld_dst):
    """src fp32 [M][N] (row stride src.stride(0)) -> bf16 [M][ld_dst] buffer (columns N.. zero); returns the [M][N] view."""
    M, N = src.shape
    assert src.dtype == torch.float32 and src.stride(1) == 1 and ld_dst >= N
    dst = torch.empty(M, ld_dst, dtype=torch.bfloat16, device=src.device)
    check(_lib.lib().ea_cast_f32_to_bf16_rows(_p(src), src.stride(0), _p(dst), ld_dst, M, N, _stream()), "ea_cast_f32_to_bf16_rows")
    return dst if ld_dst == N else dst[:, :N]


def cast_bf16_to_f32(src, dst=None):
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    check(_lib.lib().ea_cast_bf16_to_f32(_p(src), _p(dst), src.numel(), _stream()), "ea_cast_bf16_to_f32")
    return dst


def scale_dropout(x, a=1.0, y=None, b=0.0, drop_p=0.0, drop_seed=0, out=None):
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    thr, scale = drop_params(drop_p)
    check(_lib.lib().ea_scale_dropout_bf16(_p(x), _p(y), _p(out), x.numel(), a, b, drop_seed, thr, scale, _stream()),
          "ea_scale_dropout_bf16")
    return out


def colsum(X, out, M, N, ld):
    """out[n] += sum_m X[m*ld + n]  (fp32 accumulate into `out`)."""
    assert X.dtype == torch.bfloat16 and out.dtype == torch.float32
    check(_lib.lib().ea_colsum_bf16(_p(X), _p(out), M, N, ld, _stream()), "ea_colsum_bf16")
    return out


def colsum_ptr(X_ptr: int, out, M, N, ld):
    check(_lib.lib().ea_colsum_bf16(ctypes.c_void_p(X_ptr), _p(out), M, N, ld, _stream()), "ea_colsum_bf16")
    return out


def zero_rows(x, row_zero):
    M, C = x.shape
    check(_lib.lib().ea_zero_rows_bf16(_p(x), _p(row_zero), M, C, _stream()), "ea_zero_rows_bf16")
    return x


def relpos_q_prep(qkv, ldq, u, v, M, C, scaling, want_qv=True):
    qu = torch.empty(M, C, dtype=torch.bfloat16, device=qkv.device)
    qv = torch.empty(M, C, dtype=torch.bfloat16, device=qkv.device) if want_qv else None
    check(_lib.lib().ea_relpos_q_prep(_p(qkv), ldq, _p(u), _p(v), _p(qu), _p(qv), M, C, scaling, _stream()),
          "ea_relpos_q_prep")
    return qu, qv


def relpos_softmax_fwd(ac, bd, key_len, attn_mask, H, B, T, S, ld_ac, ld_bd, ld_p, causal=False, drop_p=0.0,
                       drop_seed=0):
    P = torch.empty(H * B * T, ld_p, dtype=torch.bfloat16, device=ac.device)
    Pd = torch.empty_like(P) if drop_p > 0 else None
    thr, scale = drop_params(drop_p)
    check(
        _lib.lib().ea_relpos_softmax_fwd(_p(ac), _p(bd), _p(key_len), _p(attn_mask), _p(P), _p(Pd), H, B, T, S, ld_ac,
                                         ld_bd, ld_p, int(causal), drop_seed, thr, scale, _stream()),
        "ea_relpos_softmax_fwd",
    )
    return P, (Pd if Pd is not None else P)


def flash_attention_supported(dh, T, S, relpos):
    return bool(_lib.lib().ea_flash_attention_supported(dh, T, S, int(relpos)))


def flash_keep_bits_buffer(H, B, T, device):
    """Device buffer for the attention-dropout keep bits of the rel-pos encoder kernels (csrc/flash_relpos.hip)."""
    return torch.empty(int(_lib.lib().ea_flash_keep_bits_bytes(H, B, T)) // 2, dtype=torch.int16, device=device)


def flash_attention_fwd(qu, qv, k, v, pp, key_len, H, B, T, S, ldq, ldkv, ldpp=0, causal=False, drop_p=0.0, drop_seed=0,
                        want_lse=True, want_bits=False):
    """Fused attention forward.  qu/qv: [B*T][ldq] bf16; k, v: tensors (views allowed) whose data_ptr is head 0 of row 0,
    rows ldkv apart.  Returns (out [B*T][H*64] bf16, lse [H*B][T] fp32 or None); with want_bits also the keep-bit buffer
    the rel-pos encoder kernels filled (None when dropout is off or the general kernels ran): hand it to flash_attention_bwd."""
    dh = 64
    out = torch.empty(B * T, H * dh, dtype=torch.bfloat16, device=qu.device)
    lse = torch.empty(H * B, T, dtype=torch.float32, device=qu.device) if want_lse else None
    thr, scale = drop_params(drop_p)
    bits = None
    if want_bits and thr and qv is not None and T == S and not causal:
        bits = flash_keep_bits_buffer(H, B, T, qu.device)
    check(
        _lib.lib().ea_flash_attention_fwd(_p(qu), _p(qv), ldq, _p(k), _p(v), ldkv, _p(pp), ldpp, _p(key_len), _p(out),
                                          H * dh, _p(lse), H, B, T, S, dh, int(causal), drop_seed, thr, scale, _p(bits), _stream()),
        "ea_flash_attention_fwd",
    )
    return (out, lse, bits) if want_bits else (out, lse)


def flash_attention_bwd(qu, qv, k, v, pp, key_len, out, dout, lse, dk, dv, H, B, T, S, ldq, ldkv, lddkv, ldpp=0, causal=False,
                        scaling=1.0, drop_p=0.0, drop_seed=0, keep_bits=None, dq=None, lddq=0):
    """Fused attention backward.  dk / dv: destination views (row stride lddkv).  keep_bits: the buffer flash_attention_fwd
    returned with want_bits (None: the general kernels re-evaluate the dropout hash).  dq (rel-pos only): destination view for
    t1 + t2 (row stride lddq).  Returns (t1, t2, dBD)."""
    dh = 64
    C = H * dh
    relpos = qv is not None
    t1 = torch.empty(B * T, C, dtype=torch.bfloat16, device=qu.device)
    t2 = torch.empty_like(t1) if relpos else None
    Rp = (2 * T - 1 + 7) // 8 * 8
    dBD = torch.empty(H * B * T, Rp, dtype=torch.bfloat16, device=qu.device) if relpos else None
    D = torch.empty(H * B, T, dtype=torch.float32, device=qu.device)
    thr, scale = drop_params(drop_p)
    check(
        _lib.lib().ea_flash_attention_bwd(_p(qu), _p(qv), ldq, _p(k), _p(v), ldkv, _p(pp), ldpp, _p(key_len), _p(out), _p(dout),
                                          C, _p(lse), _p(D), _p(t1), _p(t2), C, _p(dBD), Rp, _p(dk), _p(dv), lddkv, H, B, T, S,
                                          dh, int(causal), scaling, drop_seed, thr, scale, _p(keep_bits), _p(dq), lddq,
                                          _stream()),
        "ea_flash_attention_bwd",
    )
    return t1, t2, dBD


def relpos_softmax_bwd(P, dPd, H, B, T, S, ld_p, ld_dp, ld_bd, want_bd=True, drop_p=0.0, drop_seed=0):
    dAC = torch.empty(H * B * T, ld_p, dtype=torch.bfloat16, device=P.device)
    dBD = torch.empty(H * B * T, ld_bd, dtype=torch.bfloat16, device=P.device) if want_bd else None
    thr, scale = drop_params(drop_p)
    check(
        _lib.lib().ea_relpos_softmax_bwd(_p(P), _p(dPd), _p(dAC), _p(dBD), H, B, T, S, ld_p, ld_dp, ld_bd, drop_seed,
                                         thr, scale, _stream()),
        "ea_relpos_softmax_bwd",
    )
    return dAC, dBD


def add2_strided(a, lda, b, ldb, out, ldo, M, C, out_off=0):
    check(
        _lib.lib().ea_add2_strided_bf16(_p(a), lda, _p(b), ldb, ctypes.c_void_p(out.data_ptr() + 2 * out_off), ldo, M,
                                        C, _stream()),
        "ea_add2_strided_bf16",
    )
    return out


def glu_dwconv_fwd(Y, w, B, T, C, KW, stats, causal=False):
    """causal: left padding KW-1, no look-ahead (ea_glu_dwconv_causal_fwd) instead of the symmetric (KW-1)/2."""
    U = torch.empty(B * T, C, dtype=torch.bfloat16, device=Y.device)
    Z = torch.empty(B * T, C, dtype=torch.bfloat16, device=Y.device)
    name = "ea_glu_dwconv_causal_fwd" if causal else "ea_glu_dwconv_fwd"
    check(getattr(_lib.lib(), name)(_p(Y), _p(w), _p(U), _p(Z), _p(stats), B, T, C, KW, _stream()), name)
    return U, Z


def bn_finalize(stats, C, n, eps, momentum, running_mean=None, running_var=None):
    mean_rstd = torch.empty(2, C, dtype=torch.float32, device=stats.device)
    check(_lib.lib().ea_bn_finalize(_p(stats), _p(mean_rstd), _p(running_mean), _p(running_var), C, float(n), eps,
                                    momentum, _stream()), "ea_bn_finalize")
    return mean_rstd


def bn_from_running(running_mean, running_var, eps):
    C = running_mean.numel()
    mean_rstd = torch.empty(2, C, dtype=torch.float32, device=running_mean.device)
    check(_lib.lib().ea_bn_from_running(_p(running_mean), _p(running_var), _p(mean_rstd), C, eps, _stream()),
          "ea_bn_from_running")
    return mean_rstd


def bn_act_fwd(Z, mean_rstd, gamma, beta, act):
    M, C = Z.shape
    H = torch.empty_like(Z)
    check(_lib.lib().ea_bn_act_fwd(_p(Z), _p(mean_rstd), _p(gamma), _p(beta), _p(H), M, C, _ACT[act], _stream()),
          "ea_bn_act_fwd")
    return H


def conv1_bn_bwd(X, Z, dH, mean_rstd, gamma, beta, dgamma, dbeta, dW, dbias, B, T, F, CO, sy, sx, act, training=True):
    """BatchNorm(+act) backward of the first sub-sampler layer fused with conv1's weight / bias gradient (no dZ tensor)."""
    from . import functional as _F

    red = _F._pool_zeros((2, CO), torch.float32, Z.device)
    check(_lib.lib().ea_conv1_bn_bwd(_p(X), _p(Z), _p(dH), _p(mean_rstd), _p(gamma), _p(beta), _p(red), _p(dgamma), _p(dbeta), _p(dW),
                                     _p(dbias), B, T, F, CO, sy, sx, _ACT[act], int(training), _stream()), "ea_conv1_bn_bwd")


def bn_act_bwd(Z, dH, mean_rstd, gamma, beta, dgamma, dbeta, act, training=True):
    M, C = Z.shape
    from . import functional as _F  # (zero pool: one fill per update step instead of one per call)

    red = _F._pool_zeros((2, C), torch.float32, Z.device)
    dZ = torch.empty_like(Z)
    check(
        _lib.lib().ea_bn_act_bwd(_p(Z), _p(dH), _p(mean_rstd), _p(gamma), _p(beta), _p(red), _p(dZ), _p(dgamma),
                                 _p(dbeta), M, C, _ACT[act], int(training), _stream()),
        "ea_bn_act_bwd",
    )
    return dZ


def glu_dwconv_bwd(dZ, Y, U, w, dw, B, T, C, KW, causal=False):
    dY = torch.empty(B * T, 2 * C, dtype=torch.bfloat16, device=Y.device)
    ws = torch.empty(int(_lib.lib().ea_dwconv_wgrad_workspace_bytes(B, T, C, KW)), dtype=torch.uint8, device=Y.device)
    name = "ea_glu_dwconv_causal_bwd" if causal else "ea_glu_dwconv_bwd"
    check(getattr(_lib.lib(), name)(_p(dZ), _p(Y), _p(U), _p(w), _p(dY), _p(dw), _p(ws), B, T, C, KW, _stream()), name)
    return dY


def conv1_fwd(X, W, bias, B, T, F, CO, sy, sx, stats):
    To, Fo = (T - 1) // sy + 1, (F - 1) // sx + 1
    Z = torch.empty(B * To * Fo, CO, dtype=torch.bfloat16, device=X.device)
    check(_lib.lib().ea_conv1_fwd(_p(X), _p(W), _p(bias), _p(Z), _p(stats), B, T, F, CO, sy, sx, _stream()),
          "ea_conv1_fwd")
    return Z


def conv1_wgrad(X, dZ, dW, dbias, B, T, F, CO, sy, sx):
    check(_lib.lib().ea_conv1_wgrad(_p(X), _p(dZ), _p(dW), _p(dbias), B, T, F, CO, sy, sx, _stream()), "ea_conv1_wgrad")


def conv3x3_fwd(X, W16, bias, B, T, F, Cin, Cout, sy, sx, stats=None):
    """Implicit-GEMM conv: X bf16 [B*T*F][Cin] (channels-last) -> Z bf16 [B*To*Fo][Cout]; W16 bf16 [Cout][9*Cin] (tap-major)."""
    To, Fo = (T - 1) // sy + 1, (F - 1) // sx + 1
    Z = torch.empty((B * To * Fo, Cout), dtype=torch.bfloat16, device=X.device)
    check(_lib.lib().ea_conv3x3_fwd(_p(X), _p(W16), _p(bias), _p(Z), _p(stats), B, T, F, Cin, Cout, sy, sx, _stream()), "ea_conv3x3_fwd")
    return Z


def conv3x3_dgrad(dZ, Wd16, B, T, F, Cin, Cout, sy, sx):
    """dX bf16 [B*T*F][Cin] from dZ bf16 [B*To*Fo][Cout]; Wd16 bf16 [Cin][9*Cout]."""
    dX = torch.empty((B * T * F, Cin), dtype=torch.bfloat16, device=dZ.device)
    check(_lib.lib().ea_conv3x3_dgrad(_p(dZ), _p(Wd16), _p(dX), B, T, F, Cin, Cout, sy, sx, _stream()), "ea_conv3x3_dgrad")
    return dX


def conv3x3_wgrad(X, dZ, dW, B, T, F, Cin, Cout, sy, sx, param_layout=False):
    """dW fp32 [Cout][9*Cin] += weight gradient of the 3x3 conv from X bf16 [B*T*F][Cin] and dZ bf16 [B*To*Fo][Cout];
    param_layout: dW is the parameter's gradient itself, [Cout][Cin][3][3]."""
    lib = _lib.lib()
    nb = lib.ea_conv3x3_wgrad_workspace_bytes(B, T, F, Cin, Cout, sy, sx)
    ws = torch.empty(nb, dtype=torch.uint8, device=X.device)
    fn = lib.ea_conv3x3_wgrad_param_layout if param_layout else lib.ea_conv3x3_wgrad
    check(fn(_p(X), _p(dZ), _p(dW), _p(ws), B, T, F, Cin, Cout, sy, sx, _stream()), "ea_conv3x3_wgrad")
    return dW


def im2col3x3(A, B, T, F, C, sy, sx):
    To, Fo = (T - 1) // sy + 1, (F - 1) // sx + 1
    col = torch.empty(B * To * Fo, 9 * C, dtype=torch.bfloat16, device=A.device)
    check(_lib.lib().ea_im2col3x3(_p(A), _p(col), B, T, F, C, sy, sx, _stream()), "ea_im2col3x3")
    return col


def col2im3x3(dcol, B, T, F, C, sy, sx):
    dA = torch.empty(B * T * F, C, dtype=torch.bfloat16, device=dcol.device)
    check(_lib.lib().ea_col2im3x3(_p(dcol), _p(dA), B, T, F, C, sy, sx, _stream()), "ea_col2im3x3")
    return dA


def colstats(X, stats):
    M, C = X.shape
    check(_lib.lib().ea_colstats_bf16(_p(X), _p(stats), M, C, _stream()), "ea_colstats_bf16")
    return stats


def log_softmax(x, M, V, ld):
    out = torch.empty(M, V, dtype=torch.float32, device=x.device)
    if x.dtype == torch.float32:
        check(_lib.lib().ea_log_softmax_f32(_p(x), ld, _p(out), M, V, _stream()), "ea_log_softmax_f32")
    else:
        assert x.dtype == torch.bfloat16
        check(_lib.lib().ea_log_softmax_bf16(_p(x), ld, _p(out), M, V, _stream()), "ea_log_softmax_bf16")
    return out


def ctc_loss_fwd(lprobs, targets, in_len, tgt_len, B, T, V, Lmax, blank, clean=False):
    """lprobs fp32 [B][T][V] -> (nll[B], workspace holding the gathered lattice + alpha + beta); with `clean` also
    nll_clean[B] = 0 where nll is infinite, else nll (the criterion's zero_infinity value): (nll, ws, nll_clean)."""
    assert lprobs.dtype == torch.float32 and lprobs.is_contiguous()
    assert targets.dtype == torch.int32 and in_len.dtype == torch.int32 and tgt_len.dtype == torch.int32
    assert targets.is_contiguous() and in_len.is_contiguous() and tgt_len.is_contiguous()
    assert targets.numel() >= B * Lmax and in_len.numel() >= B and tgt_len.numel() >= B
    dev = lprobs.device
    nll = torch.empty(B, dtype=torch.float32, device=dev)
    nll_clean = torch.empty(B, dtype=torch.float32, device=dev) if clean else None
    ws = torch.empty(int(_lib.lib().ea_ctc_workspace_bytes(B, T, Lmax)), dtype=torch.uint8, device=dev)
    check(
        _lib.lib().ea_ctc_loss_clean(_p(lprobs), _p(targets), _p(in_len), _p(tgt_len), _p(nll), _p(nll_clean), _p(ws), B, T, V,
                                     Lmax, blank, _stream()),
        "ea_ctc_loss_clean",
    )
    return (nll, ws, nll_clean) if clean else (nll, ws)


def ctc_targets(target, pad, eos):
    """target int64 [B][L] -> (int32 [B][L] copy, int32 [B] count of the entries that are neither pad nor eos), one launch."""
    assert target.dtype == torch.int64 and target.dim() == 2 and target.is_contiguous()
    B, L = target.shape
    tgt32 = torch.empty(B, L, dtype=torch.int32, device=target.device)
    tgt_len = torch.empty(B, dtype=torch.int32, device=target.device)
    check(_lib.lib().ea_ctc_targets(_p(target), _p(tgt32), _p(tgt_len), B, L, int(pad), int(eos), _stream()), "ea_ctc_targets")
    return tgt32, tgt_len


def subsample_lengths(src_lengths, total, Tp):
    """src_lengths int64 [B] -> (x_lengths int64 [B] = ceil(src / total), key_len int32 [B], padding_mask bool [B][Tp],
    row_zero uint8 [B*Tp]), one launch."""
    assert src_lengths.dtype == torch.int64 and src_lengths.dim() == 1 and src_lengths.is_contiguous()
    B, dev = src_lengths.numel(), src_lengths.device
    x_len = torch.empty(B, dtype=torch.int64, device=dev)
    key_len = torch.empty(B, dtype=torch.int32, device=dev)
    mask = torch.empty(B, Tp, dtype=torch.bool, device=dev)
    row_zero = torch.empty(B * Tp, dtype=torch.uint8, device=dev)
    check(_lib.lib().ea_subsample_lengths(_p(src_lengths), _p(x_len), _p(key_len), _p(mask), _p(row_zero), B, Tp, int(total),
                                          _stream()), "ea_subsample_lengths")
    return x_len, key_len, mask, row_zero


def stats_add4(stats, a0, loss, a2, a3):
    """stats[0:4] += (a0, loss[0], a2, a3) in fp32, one launch; `loss` is a one-element fp32 device tensor."""
    assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() >= 4
    assert loss.dtype == torch.float32 and loss.numel() == 1
    check(_lib.lib().ea_stats_add4(_p(stats), float(a0), _p(loss), float(a2), float(a3), _stream()), "ea_stats_add4")
    return stats


def transpose_pad(src, dst, rows, cols, ld_dst):
    """dst bf16 [cols][ld_dst]: dst[c][r] = src[r][c] for r < rows, zero for rows <= r < ld_dst (src dense [rows][cols])."""
    assert src.dtype == torch.bfloat16 and dst.dtype == torch.bfloat16 and src.is_contiguous() and dst.is_contiguous()
    assert src.numel() == rows * cols and dst.numel() == cols * ld_dst and ld_dst >= rows
    check(_lib.lib().ea_transpose_pad_bf16(_p(src), _p(dst), rows, cols, ld_dst, _stream()), "ea_transpose_pad_bf16")
    return dst


def permute_k(src, C, F, transposed=False):
    """bf16 [N][C*F] with the input axis in (c*F + f) order -> the same weight in (f*C + c) order; with `transposed` also its
    transpose [F*C][N] from the same launch: (permuted, transposed)."""
    assert src.dtype == torch.bfloat16 and src.is_contiguous() and src.dim() == 2 and src.shape[1] == C * F
    dst = torch.empty_like(src)
    dst_t = torch.empty(C * F, src.shape[0], dtype=torch.bfloat16, device=src.device) if transposed else None
    check(_lib.lib().ea_permute_k_bf16(_p(src), _p(dst), _p(dst_t), src.shape[0], C, F, _stream()), "ea_permute_k_bf16")
    return (dst, dst_t) if transposed else dst


def unpermute_k_add(src, dst, N, C, F):
    """dst fp32 [N][C*F] ((c*F + f) order) += src fp32 [N][F*C] ((f*C + c) order)."""
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous()
    assert src.numel() == N * C * F and dst.numel() == N * C * F
    check(_lib.lib().ea_unpermute_k_add_f32(_p(src), _p(dst), N, C, F, _stream()), "ea_unpermute_k_add_f32")
    return dst


def ctc_loss_grad(lprobs, ws, nll, targets, in_len, tgt_len, B, T, V, Lmax, blank, ld_out=None, grad_bf16=True,
                  grad_scale=1.0, grad_scale_dev=None, zero_infinity=True):
    ld_out = V if ld_out is None else ld_out
    dl = torch.empty(B * T, ld_out, dtype=torch.bfloat16 if grad_bf16 else torch.float32, device=lprobs.device)
    check(
        _lib.lib().ea_ctc_grad(_p(lprobs), _p(ws), _p(nll), _p(targets), _p(in_len), _p(tgt_len), _p(dl), ld_out,
                               int(grad_bf16), B, T, V, Lmax, blank, grad_scale, _p(grad_scale_dev),
                               int(zero_infinity), _stream()),
        "ea_ctc_grad",
    )
    return dl


SMOOTHING = {"uniform": 0, "unigram": 1, "temporal": 2}


def label_smoothed_ce(logits, ld, target, M, V, pad_idx, eps, want_grad=True, grad_bf16=True, grad_scale=1.0,
                      grad_ld=None, smoothing="uniform", prior=None, tgt_len=0):
    assert target.dtype == torch.int32
    dev = logits.device
    out = torch.zeros(2, dtype=torch.float32, device=dev)
    dl = None
    grad_ld = V if grad_ld is None else grad_ld
    if want_grad:
        dl = torch.zeros(M, grad_ld, dtype=torch.bfloat16 if grad_bf16 else torch.float32, device=dev)
    check(
        _lib.lib().ea_label_smoothed_ce(_p(logits), ld, int(logits.dtype == torch.bfloat16), _p(target), _p(out),
                                        _p(dl), grad_ld, int(grad_bf16), M, V, pad_idx, eps, grad_scale, SMOOTHING[smoothing],
                                        _p(prior), tgt_len, _stream()),
        "ea_label_smoothed_ce",
    )
    return out, dl


def fbank_batch(wav, offsets, B, tables, cmvn_mean, cmvn_std, Tmax, nmel=80, frame_len=400, frame_shift=160,
                preemph=0.97, log_floor=1.1920928955078125e-07, want_sum=True):
    dev = wav.device
    feat = torch.empty(B, Tmax, nmel, dtype=torch.float32, device=dev)
    utt_sum = torch.zeros(B, dtype=torch.float32, device=dev) if want_sum else None
    out_len = torch.empty(B, dtype=torch.int32, device=dev)
    assert wav.dtype in (torch.float32, torch.int16)
    fn = _lib.lib().ea_fbank_batch if wav.dtype == torch.float32 else _lib.lib().ea_fbank_batch_i16
    check(
        fn(_p(wav), _p(offsets), B, _p(tables["window"]), _p(tables["twiddle"]), _p(tables["mel_start"]), _p(tables["mel_len"]),
           _p(tables["mel_woff"]), _p(tables["mel_w"]), _p(cmvn_mean), _p(cmvn_std), _p(feat), _p(utt_sum), _p(out_len), Tmax, nmel,
           frame_len, frame_shift, preemph, log_floor, _stream()),
        "ea_fbank_batch",
    )
    return feat, out_len, utt_sum


def resample_batch(wav, in_offsets, out, out_offsets, B, taps, first, in_unit, max_out, in_base=None, out_base=None):
    """out[out_offsets[b] : out_offsets[b + 1]] = utterance b of `wav` (fp32 or int16) through the polyphase filter
    taps fp32 [phases][K] / first int32 [phases] (data/resample.py: ResamplePlan).  Bases int64 [B]: absolute index of the
    first sample held / first output wanted (None: 0, the offline case)."""
    assert wav.dtype in (torch.float32, torch.int16) and out.dtype == torch.float32
    assert taps.dtype == torch.float32 and taps.dim() == 2 and taps.is_contiguous() and first.dtype == torch.int32
    assert in_offsets.dtype == torch.int64 and out_offsets.dtype == torch.int64
    phases, Kt = taps.shape
    fn = _lib.lib().ea_resample_batch if wav.dtype == torch.float32 else _lib.lib().ea_resample_batch_i16
    check(
        fn(_p(wav), _p(in_offsets), _p(in_base), _p(out), _p(out_offsets), _p(out_base), B, _p(taps), _p(first), phases, Kt,
           in_unit, max_out, _stream()),
        "ea_resample_batch",
    )
    return out


def feature_stats(feat, lengths, acc):
    """acc fp64 [2*nmel+1] += (sum, sum of squares, frames) over the valid frames of feat fp32 [B][Tmax][nmel]."""
    B, Tmax, nmel = feat.shape
    assert acc.dtype == torch.float64 and acc.numel() == 2 * nmel + 1 and feat.dtype == torch.float32 and feat.is_contiguous()
    check(_lib.lib().ea_feature_stats(_p(feat), _p(lengths), _p(acc), B, Tmax, nmel, _stream()), "ea_feature_stats")
    return acc


def specaugment(feat, lengths, utt_sum, fmask, tmask, use_mean=True, mask_value=0.0):
    B, Tmax, nmel = feat.shape
    nf = fmask.shape[1] if fmask is not None else 0
    nt = tmask.shape[1] if tmask is not None else 0
    check(
        _lib.lib().ea_specaugment(_p(feat), _p(lengths), _p(utt_sum), _p(fmask), _p(tmask), nf, nt, B, Tmax, nmel,
                                  int(use_mean), mask_value, _stream()),
        "ea_specaugment",
    )
    return feat


def grad_sumsq(g, out):
    check(_lib.lib().ea_grad_sumsq(_p(g), g.numel(), _p(out), _stream()), "ea_grad_sumsq")
    return out


def clip_coef(sumsq, pre_scale, max_norm, coef, denom_dev=None):
    check(_lib.lib().ea_clip_coef(_p(sumsq), pre_scale, _p(denom_dev), max_norm, _p(coef), _stream()), "ea_clip_coef")
    return coef


def adam_step(p, g, m, v, p_bf16, coef, lr, beta1, beta2, eps, weight_decay, step, zero_grad=True):
    check(
        _lib.lib().ea_adam_step(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), p.numel(), _p(coef), lr, beta1, beta2, eps,
                                weight_decay, step, int(zero_grad), _stream()),
        "ea_adam_step",
    )


def clip_coef_clear(sumsq, pre_scale, max_norm, coef, denom_dev=None):
    """clip_coef that leaves sumsq[0] = 0 for the next grad_sumsq."""
    check(_lib.lib().ea_clip_coef_clear(_p(sumsq), pre_scale, _p(denom_dev), max_norm, _p(coef), _stream()), "ea_clip_coef_clear")
    return coef


def adam_step_capped(p, g, m, v, p_bf16, coef, lr, beta1, beta2, eps, weight_decay, step, max_blocks, stream, zero_grad=True):
    """adam_step from at most `max_blocks` workgroups on `stream` (a torch stream; not the current one: the caller orders it)."""
    check(
        _lib.lib().ea_adam_step_capped(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), p.numel(), _p(coef), lr, beta1, beta2, eps,
                                       weight_decay, step, int(zero_grad), int(max_blocks), ctypes.c_void_p(stream.cuda_stream)),
        "ea_adam_step_capped",
    )


def ctc_greedy_decode(x, in_len, B, T, V, blank, pad, ld=None, want_align=True):
    """x: [B*T][V] fp32/bf16 log-probs (batch-major).  Returns tokens [B][T] (pad filled), lengths [B], scores [B], align [B][T]."""
    dev = x.device
    ld = x.stride(0) if ld is None else ld
    best = torch.empty(B * T, dtype=torch.int32, device=dev)
    bestv = torch.empty(B * T, dtype=torch.float32, device=dev)
    tokens = torch.empty(B, T, dtype=torch.int32, device=dev)
    align = torch.zeros(B, T, dtype=torch.int32, device=dev) if want_align else None
    out_len = torch.empty(B, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    check(
        _lib.lib().ea_ctc_greedy_decode(_p(x), ld, int(x.dtype == torch.bfloat16), _p(in_len), _p(best), _p(bestv), _p(tokens),
                                        _p(align), _p(out_len), _p(score), B, T, V, blank, pad, _stream()),
        "ea_ctc_greedy_decode",
    )
    return tokens, out_len, score, align


def _finish_outputs(n, nbest, max_u, device):
    """The outputs of a finish: (tokens int32 [n][nbest][max_u], lengths int32 [n][nbest], scores fp32 [n][nbest], nhyp int32 [n])."""
    return (torch.empty(n, nbest, max_u, dtype=torch.int32, device=device), torch.empty(n, nbest, dtype=torch.int32, device=device),
            torch.empty(n, nbest, dtype=torch.float32, device=device), torch.empty(n, dtype=torch.int32, device=device))


def _partial_outputs(n, max_u, device):
    """The outputs of a streamed partial: (tokens int32 [n][max_u], lengths int32 [n], scores fp32 [n], stable_len int32 [n])."""
    return (torch.empty(n, max_u, dtype=torch.int32, device=device), torch.empty(n, dtype=torch.int32, device=device),
            torch.empty(n, dtype=torch.float32, device=device), torch.empty(n, dtype=torch.int32, device=device))


def _stream_state(bytes_fn, max_streams, max_frames, beam, device):
    """(state uint8 [max_streams][bytes per slot], zero-filled; bytes per slot) of a streamed search; bytes_fn: its
    ea_*_state_bytes entry."""
    nbytes = int(bytes_fn(max_frames, beam))
    assert nbytes > 0 and max_streams >= 1
    return torch.zeros(max_streams, nbytes, dtype=torch.uint8, device=device), nbytes


def _check_stream_state(state, bytes_fn, max_frames, beam):
    assert state.dtype == torch.uint8 and state.is_contiguous() and state.dim() == 2
    assert state.shape[1] == bytes_fn(max_frames, beam)


def _check_rnnt_step_args(logits, out, lm_rows, N, V, lm_no_blank):
    """The joint's logits fp32 [N][>= V], the triple a transducer step writes and its LM rows; returns the triple."""
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] == N and logits.shape[1] >= V
    parent, token, keep = out
    assert parent.numel() == token.numel() == keep.numel() == N
    assert parent.dtype == token.dtype == torch.int32 and keep.dtype == torch.uint8
    if lm_rows is not None:
        assert lm_rows.dtype == torch.float32 and lm_rows.stride(1) == 1 and lm_rows.shape == (N, V - 1 if lm_no_blank else V)
    return parent, token, keep


def ctc_prefix_beam_workspace(B, T, beam, device):
    """Workspace of the CTC prefix beam search (ea_ctc_prefix_beam_workspace_bytes): the beams and prefix tables of B utterances."""
    return torch.empty(int(_lib.lib().ea_ctc_prefix_beam_workspace_bytes(B, T, beam)), dtype=torch.uint8, device=device)


def ctc_prefix_beam_step(x, in_len, ws, B, T, V, beam, K, blank, t0, t1, lm_rows=None, lm_weight=0.0, ins_bonus=0.0, lm_out=None,
                         ld=None):
    """Frames [t0, t1) of the CTC prefix beam search over x [B*T][V] fp32/bf16 log-probs (batch-major).  With an LM: lm_rows
    fp32 [B*beam][V], t1 = t0 + 1 and lm_out = (parent int32, token int32, keep uint8), each [B*beam], written by the step."""
    ld = x.stride(0) if ld is None else ld
    assert x.dtype in (torch.float32, torch.bfloat16) and x.stride(-1) == 1 and x.shape[0] == B * T and x.shape[1] == V
    assert in_len.dtype == torch.int32 and in_len.numel() == B and ws.numel() >= _lib.lib().ea_ctc_prefix_beam_workspace_bytes(B, T, beam)
    parent, token, keep = lm_out if lm_out is not None else (None, None, None)
    if lm_rows is not None:
        assert lm_rows.dtype == torch.float32 and lm_rows.stride(1) == 1 and lm_rows.shape == (B * beam, V) and t1 == t0 + 1
        assert parent.numel() == token.numel() == keep.numel() == B * beam
        assert parent.dtype == token.dtype == torch.int32 and keep.dtype == torch.uint8
    check(_lib.lib().ea_ctc_prefix_beam_step(_p(x), ld, int(x.dtype == torch.bfloat16), _p(in_len), _p(ws), _p(lm_rows),
                                             lm_rows.stride(0) if lm_rows is not None else 0, _p(parent), _p(token), _p(keep), B, T,
                                             V, beam, K, blank, lm_weight, ins_bonus, t0, t1, _stream()), "ea_ctc_prefix_beam_step")


def ctc_prefix_beam_finish(ws, B, T, beam, nbest, pad, lm_rows=None, lm_weight=0.0, ins_bonus=0.0, eos=-1):
    """(tokens int32 [B][nbest][T] pad-filled, lengths int32 [B][nbest], scores fp32 [B][nbest], nhyp int32 [B]), best first."""
    dev = ws.device
    tokens, lengths, scores, nhyp = _finish_outputs(B, nbest, T, dev)
    check(_lib.lib().ea_ctc_prefix_beam_finish(_p(ws), _p(lm_rows), lm_rows.stride(0) if lm_rows is not None else 0, lm_weight,
                                               ins_bonus, eos, B, T, beam, nbest, pad, _p(tokens), _p(lengths), _p(scores),
                                               _p(nhyp), _stream()), "ea_ctc_prefix_beam_finish")
    return tokens, lengths, scores, nhyp


def _cg(graph, V=None):
    """(nodes, edges, root) device tables of a context graph -> the five table arguments of the bias calls."""
    nodes, edges, root = graph
    assert nodes.dtype == edges.dtype == root.dtype == torch.int32 and nodes.is_contiguous() and edges.is_contiguous() and root.is_contiguous()
    assert nodes.dim() == 2 and nodes.shape[1] == 4 and nodes.shape[0] >= 1 and tuple(edges.shape) == (nodes.shape[0] - 1, 4)
    assert root.dim() == 2 and root.shape[1] == 2 and (V is None or root.shape[0] == V), "context graph built for another vocabulary"
    return _p(nodes), (_p(edges) if edges.numel() else None), _p(root), nodes.shape[0], edges.shape[0]


def ctc_prefix_beam_bias_workspace(B, T, beam, device):
    """Workspace of the hotword-biased CTC prefix beam search (ea_ctc_prefix_beam_bias_workspace_bytes)."""
    return torch.empty(int(_lib.lib().ea_ctc_prefix_beam_bias_workspace_bytes(B, T, beam)), dtype=torch.uint8, device=device)


def ctc_prefix_beam_bias_step(x, in_len, ws, graph, B, T, V, beam, K, blank, t0, t1, lm_rows=None, lm_weight=0.0, ins_bonus=0.0,
                              lm_out=None, ld=None):
    """ctc_prefix_beam_step with a context graph (nodes, edges, root device tables of tools.context_graph.ContextGraph.cuda())."""
    ld = x.stride(0) if ld is None else ld
    assert x.dtype in (torch.float32, torch.bfloat16) and x.stride(-1) == 1 and x.shape[0] == B * T and x.shape[1] == V
    assert in_len.dtype == torch.int32 and in_len.numel() == B
    assert ws.numel() >= _lib.lib().ea_ctc_prefix_beam_bias_workspace_bytes(B, T, beam)
    parent, token, keep = lm_out if lm_out is not None else (None, None, None)
    if lm_rows is not None:
        assert lm_rows.dtype == torch.float32 and lm_rows.stride(1) == 1 and lm_rows.shape == (B * beam, V) and t1 == t0 + 1
        assert parent.numel() == token.numel() == keep.numel() == B * beam
        assert parent.dtype == token.dtype == torch.int32 and keep.dtype == torch.uint8
    check(_lib.lib().ea_ctc_prefix_beam_bias_step(_p(x), ld, int(x.dtype == torch.bfloat16), _p(in_len), _p(ws), _p(lm_rows),
                                                  lm_rows.stride(0) if lm_rows is not None else 0, _p(parent), _p(token), _p(keep),
                                                  *_cg(graph, V), B, T, V, beam, K, blank, lm_weight, ins_bonus, t0, t1, _stream()),
          "ea_ctc_prefix_beam_bias_step")


def ctc_prefix_beam_bias_finish(ws, graph, B, T, beam, nbest, pad, lm_rows=None, lm_weight=0.0, ins_bonus=0.0, eos=-1):
    """ctc_prefix_beam_finish of a biased search: the scores include the boosts of the completed phrases."""
    dev = ws.device
    tokens, lengths, scores, nhyp = _finish_outputs(B, nbest, T, dev)
    nodes, _, _, n_nodes, _ = _cg(graph)
    check(_lib.lib().ea_ctc_prefix_beam_bias_finish(_p(ws), _p(lm_rows), lm_rows.stride(0) if lm_rows is not None else 0, lm_weight,
                                                    ins_bonus, eos, nodes, n_nodes, B, T, beam, nbest, pad, _p(tokens), _p(lengths),
                                                    _p(scores), _p(nhyp), _stream()), "ea_ctc_prefix_beam_bias_finish")
    return tokens, lengths, scores, nhyp


def ctc_prefix_beam_stream_state(max_streams, max_frames, beam, device):
    """(state uint8 [max_streams][bytes per slot], zero-filled; bytes per slot) of the streamed CTC prefix beam search
    (ea_ctc_prefix_beam_stream_state_bytes)."""
    return _stream_state(_lib.lib().ea_ctc_prefix_beam_stream_state_bytes, max_streams, max_frames, beam, device)


def _cg_or_none(graph, V=None):
    return _cg(graph, V) if graph is not None else (None, None, None, 0, 0)


def ctc_prefix_beam_stream_reset(state, slots, max_frames, beam):
    """The slots int32 [n] (device) of `state` get the search state before frame 0 (ea_ctc_prefix_beam_stream_reset)."""
    _check_stream_state(state, _lib.lib().ea_ctc_prefix_beam_stream_state_bytes, max_frames, beam)
    assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.device == state.device
    check(_lib.lib().ea_ctc_prefix_beam_stream_reset(_p(state), _p(slots), slots.numel(), state.shape[0], max_frames, beam, _stream()),
          "ea_ctc_prefix_beam_stream_reset")


def ctc_prefix_beam_stream_step(x, meta, state, max_frames, V, beam, K, blank, j0=0, j1=None, graph=None, lm_rows=None, lm_weight=0.0,
                                ins_bonus=0.0, lm_out=None, ld=None):
    """The frames [j0, j1) of the pieces of every listed stream through the CTC prefix beam search (ea_ctc_prefix_beam_stream_step;
    j1 None: the whole pieces).  x [rows][V] fp32/bf16 log-probs packed stream by stream; meta int32 [3][n] = (slot, n_new,
    row_off) on the device; graph: the (nodes, edges, root) device tables of a context graph, the same for every call of a search.
    With an LM: lm_rows fp32 [n*beam][V], j1 = j0 + 1 and lm_out = (parent int32, token int32, keep uint8), each [n*beam], written
    by the step."""
    ld = x.stride(0) if ld is None else ld
    assert x.dtype in (torch.float32, torch.bfloat16) and x.dim() == 2 and x.stride(-1) == 1 and x.shape[1] == V
    assert meta.dtype == torch.int32 and meta.dim() == 2 and meta.shape[0] == 3 and meta.is_contiguous()
    _check_stream_state(state, _lib.lib().ea_ctc_prefix_beam_stream_state_bytes, max_frames, beam)
    n = meta.shape[1]
    j1 = max(x.shape[0], j0) if j1 is None else j1
    parent, token, keep = lm_out if lm_out is not None else (None, None, None)
    if lm_rows is not None:
        assert lm_rows.dtype == torch.float32 and lm_rows.stride(1) == 1 and lm_rows.shape == (n * beam, V) and j1 == j0 + 1
        assert parent.numel() == token.numel() == keep.numel() == n * beam
        assert parent.dtype == token.dtype == torch.int32 and keep.dtype == torch.uint8
    check(_lib.lib().ea_ctc_prefix_beam_stream_step(_p(x), ld, int(x.dtype == torch.bfloat16), x.shape[0], _p(meta[0]), _p(meta[1]),
                                                    _p(meta[2]), j0, j1, n, _p(state), _p(lm_rows),
                                                    lm_rows.stride(0) if lm_rows is not None else 0, _p(parent), _p(token), _p(keep),
                                                    *_cg_or_none(graph, V), state.shape[0], max_frames, V, beam, K, blank, lm_weight,
                                                    ins_bonus, _stream()), "ea_ctc_prefix_beam_stream_step")


def ctc_prefix_beam_stream_finish(state, slots, max_frames, beam, nbest, pad, max_u, graph=None, lm_rows=None, lm_weight=0.0,
                                  ins_bonus=0.0, eos=-1):
    """The finished hypotheses of the slots int32 [n] (device), the state left as it is (ea_ctc_prefix_beam_stream_finish);
    lm_rows fp32 [n*beam][V] in the order of `slots`.  Returns (tokens int32 [n][nbest][max_u] pad-filled, lengths int32
    [n][nbest], scores fp32 [n][nbest], nhyp int32 [n]), best first."""
    _check_stream_state(state, _lib.lib().ea_ctc_prefix_beam_stream_state_bytes, max_frames, beam)
    assert slots.dtype == torch.int32 and slots.is_contiguous() and 1 <= nbest <= beam
    n, dev = slots.numel(), state.device
    if lm_rows is not None:
        assert lm_rows.dtype == torch.float32 and lm_rows.dim() == 2 and lm_rows.stride(1) == 1 and lm_rows.shape[0] == n * beam
    tokens, lengths, scores, nhyp = _finish_outputs(n, nbest, max_u, dev)
    nodes, _, _, n_nodes, _ = _cg_or_none(graph)
    check(_lib.lib().ea_ctc_prefix_beam_stream_finish(_p(state), _p(slots), n, _p(lm_rows),
                                                      lm_rows.stride(0) if lm_rows is not None else 0, lm_weight, ins_bonus, eos, nodes,
                                                      n_nodes, state.shape[0], max_frames, beam, nbest, pad, max_u, _p(tokens),
                                                      _p(lengths), _p(scores), _p(nhyp), _stream()), "ea_ctc_prefix_beam_stream_finish")
    return tokens, lengths, scores, nhyp


def ctc_prefix_beam_stream_partial(state, slots, max_frames, beam, pad, max_u, lm_weight=0.0, ins_bonus=0.0, biased=False):
    """The best live hypothesis (by the in-beam score, with the running bias when `biased`) of the slots int32 [n] (device) and
    the length of the beam's common prefix (ea_ctc_prefix_beam_stream_partial).  Returns (tokens int32 [n][max_u] pad-filled,
    lengths int32 [n], scores fp32 [n], stable_len int32 [n])."""
    _check_stream_state(state, _lib.lib().ea_ctc_prefix_beam_stream_state_bytes, max_frames, beam)
    assert slots.dtype == torch.int32 and slots.is_contiguous()
    n, dev = slots.numel(), state.device
    tokens, lengths, scores, stable = _partial_outputs(n, max_u, dev)
    check(_lib.lib().ea_ctc_prefix_beam_stream_partial(_p(state), _p(slots), n, lm_weight, ins_bonus, int(bool(biased)), state.shape[0],
                                                       max_frames, beam, pad, max_u, _p(tokens), _p(lengths), _p(scores), _p(stable),
                                                       _stream()), "ea_ctc_prefix_beam_stream_partial")
    return tokens, lengths, scores, stable


def ctc_kws_state_bytes(K, Lmax, max_hits):
    """Bytes per slot of the keyword spotter's state (ea_ctc_kws_state_bytes; 0 for sizes it does not take)."""
    return int(_lib.lib().ea_ctc_kws_state_bytes(K, Lmax, max_hits))


def ctc_kws_state(max_streams, K, Lmax, max_hits, device):
    """(state uint8 [max_streams][bytes per slot], zero-filled; bytes per slot) of the keyword spotter."""
    nbytes = ctc_kws_state_bytes(K, Lmax, max_hits)
    assert nbytes > 0 and max_streams >= 1
    return torch.zeros(max_streams, nbytes, dtype=torch.uint8, device=device), nbytes


def _check_kws(state, keywords, max_hits):
    """keywords = (tokens int32 [K][Lmax], lengths int32 [K], tau fp32 [K]) on the device of `state`; returns (K, Lmax)."""
    tokens, lengths, tau = keywords
    assert tokens.dtype == lengths.dtype == torch.int32 and tau.dtype == torch.float32 and tokens.dim() == 2
    assert tokens.is_contiguous() and lengths.is_contiguous() and tau.is_contiguous()
    Kk, Lmax = tokens.shape
    assert lengths.numel() == tau.numel() == Kk and tokens.device == lengths.device == tau.device == state.device
    assert state.dtype == torch.uint8 and state.is_contiguous() and state.dim() == 2
    assert state.shape[1] == ctc_kws_state_bytes(Kk, Lmax, max_hits) > 0
    return Kk, Lmax


def ctc_kws_reset(state, slots, keywords, max_hits):
    """The slots int32 [n] (device) of `state` get the spotter's state before frame 0 (ea_ctc_kws_reset)."""
    Kk, Lmax = _check_kws(state, keywords, max_hits)
    assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.device == state.device
    check(_lib.lib().ea_ctc_kws_reset(_p(state), _p(slots), slots.numel(), state.shape[0], Kk, Lmax, max_hits, _stream()),
          "ea_ctc_kws_reset")


def ctc_kws_step(x, meta, state, keywords, max_hits, V, blank, hold, rowmax=None, ld=None):
    """The pieces of every listed stream through the keyword spotter (ea_ctc_kws_step).  x fp32 [rows][>= V] log-probs packed
    stream by stream; meta int32 [3][n] = (slot, n_new, row_off) on the device; keywords as `_check_kws` takes them; rowmax: fp32
    scratch [rows] (allocated when None).  Returns rowmax, the rows' maxima."""
    ld = x.stride(0) if ld is None else ld
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(-1) == 1 and x.shape[1] >= V and ld >= V
    assert meta.dtype == torch.int32 and meta.dim() == 2 and meta.shape[0] == 3 and meta.is_contiguous() and meta.device == x.device
    Kk, Lmax = _check_kws(state, keywords, max_hits)
    rows = x.shape[0]
    if rowmax is None:
        rowmax = torch.empty(max(rows, 1), dtype=torch.float32, device=x.device)
    assert rowmax.dtype == torch.float32 and rowmax.is_contiguous() and rowmax.numel() >= rows and rowmax.device == x.device
    tokens, lengths, tau = keywords
    check(_lib.lib().ea_ctc_kws_step(_p(x), ld, rows, _p(rowmax), _p(meta[0]), _p(meta[1]), _p(meta[2]), meta.shape[1], _p(state),
                                     _p(tokens), _p(lengths), _p(tau), state.shape[0], Kk, Lmax, max_hits, V, blank, int(hold),
                                     _stream()), "ea_ctc_kws_step")
    return rowmax


def ctc_kws_hits(state, slots, keywords, max_hits, flush=False, clear=False):
    """The hit lists of the slots int32 [n] (device), after emitting their open hits when `flush`; `clear` empties the lists
    afterwards (ea_ctc_kws_hits).  Returns (starts int32 [n][K][max_hits] -1-filled, ends likewise, scores fp32 [n][K][max_hits],
    counts int32 [n][K]) on the device."""
    Kk, Lmax = _check_kws(state, keywords, max_hits)
    assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.device == state.device
    n, dev = slots.numel(), state.device
    starts = torch.empty(n, Kk, max_hits, dtype=torch.int32, device=dev)
    ends = torch.empty_like(starts)
    scores = torch.empty(n, Kk, max_hits, dtype=torch.float32, device=dev)
    counts = torch.empty(n, Kk, dtype=torch.int32, device=dev)
    check(_lib.lib().ea_ctc_kws_hits(_p(state), _p(slots), n, int(bool(flush)), int(bool(clear)), state.shape[0], Kk, Lmax, max_hits,
                                     _p(starts), _p(ends), _p(scores), _p(counts), _stream()), "ea_ctc_kws_hits")
    return starts, ends, scores, counts


def ctc_kws_host(x, kw_tokens, kw_len, kw_tau, blank, hold, max_hits, V=None):
    """The keyword spotter over one utterance on the host (ea_ctc_kws_host; no device): x fp32 [T][ld] numpy log-probs (V: the
    columns that count, all by default), kw_tokens int32 [K][Lmax], kw_len int32 [K], kw_tau fp32 [K].  Returns numpy (starts
    int32 [K][max_hits], ends, scores fp32 [K][max_hits], counts int32 [K]), flushed at the end."""
    import numpy as np

    x = np.ascontiguousarray(x, dtype=np.float32)
    assert x.ndim == 2
    T, ld = x.shape
    V = ld if V is None else V
    tok = np.ascontiguousarray(kw_tokens, dtype=np.int32)
    assert tok.ndim == 2
    Kk, Lmax = tok.shape
    ln = np.ascontiguousarray(kw_len, dtype=np.int32)
    tau = np.ascontiguousarray(kw_tau, dtype=np.float32)
    assert ln.shape == tau.shape == (Kk,)
    starts = np.empty((Kk, max_hits), dtype=np.int32)
    ends = np.empty_like(starts)
    scores = np.empty((Kk, max_hits), dtype=np.float32)
    counts = np.empty(Kk, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(_lib.lib().ea_ctc_kws_host(vp(x), ld, T, V, vp(tok), vp(ln), vp(tau), Kk, Lmax, blank, int(hold), max_hits, vp(starts),
                                     vp(ends), vp(scores), vp(counts)), "ea_ctc_kws_host")
    return starts, ends, scores, counts


def rnnt_frame_beam_workspace(B, T, beam, device):
    """Workspace of the frame-synchronous transducer beam search (ea_rnnt_frame_beam_workspace_bytes): the beams, prefix tables
    and per-row candidates of B utterances of at most T frames."""
    return torch.empty(int(_lib.lib().ea_rnnt_frame_beam_workspace_bytes(B, T, beam)), dtype=torch.uint8, device=device)


def rnnt_frame_beam_step(logits, in_len, ws, out, B, T, V, beam, K, blank, t, eos=-1, temperature=1.0, lm_rows=None, lm_weight=0.0,
                         lm_no_blank=False):
    """Frame t of the frame-synchronous transducer beam search: logits fp32 [B*beam][>= V] (the joint's output for this frame, row
    b * beam + slot), in_len int32 [B], out = (parent int32, token int32, keep uint8), each [B*beam], written by the step.
    lm_rows fp32 [B*beam][V or V - 1 (lm_no_blank)]; eos >= 0: the model's eos is folded into blank."""
    assert in_len.dtype == torch.int32 and in_len.numel() == B  # (ws: rnnt_frame_beam_workspace(B, T, beam), checked by its owner)
    parent, token, keep = _check_rnnt_step_args(logits, out, lm_rows, B * beam, V, lm_no_blank)
    check(_lib.lib().ea_rnnt_frame_beam_step(_p(logits), logits.stride(0), _p(lm_rows), lm_rows.stride(0) if lm_rows is not None else 0,
                                             int(lm_no_blank), _p(in_len), _p(ws), _p(parent), _p(token), _p(keep), B, T, V, beam, K,
                                             blank, eos, temperature, lm_weight, t, _stream()), "ea_rnnt_frame_beam_step")


def rnnt_frame_beam_finish(ws, B, T, beam, nbest, pad, normalize=True):
    """(tokens int32 [B][nbest][T] pad-filled, lengths int32 [B][nbest], scores fp32 [B][nbest], nhyp int32 [B]), best first."""
    dev = ws.device
    tokens, lengths, scores, nhyp = _finish_outputs(B, nbest, T, dev)
    check(_lib.lib().ea_rnnt_frame_beam_finish(_p(ws), B, T, beam, nbest, pad, int(bool(normalize)), _p(tokens), _p(lengths),
                                               _p(scores), _p(nhyp), _stream()), "ea_rnnt_frame_beam_finish")
    return tokens, lengths, scores, nhyp


def rnnt_frame_beam_stream_state(max_streams, max_frames, beam, device):
    """(state uint8 [max_streams][bytes per slot], zero-filled; bytes per slot) of the streamed frame-synchronous transducer
    beam search (ea_rnnt_frame_beam_stream_state_bytes)."""
    return _stream_state(_lib.lib().ea_rnnt_frame_beam_stream_state_bytes, max_streams, max_frames, beam, device)


def rnnt_frame_beam_stream_reset(state, slots, max_frames, beam):
    """The slots int32 [n] (device) of `state` get the search state before frame 0 (ea_rnnt_frame_beam_stream_reset)."""
    _check_stream_state(state, _lib.lib().ea_rnnt_frame_beam_stream_state_bytes, max_frames, beam)
    assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.device == state.device
    check(_lib.lib().ea_rnnt_frame_beam_stream_reset(_p(state), _p(slots), slots.numel(), state.shape[0], max_frames, beam, _stream()),
          "ea_rnnt_frame_beam_stream_reset")


def rnnt_frame_beam_stream_step(logits, slot_idx, n_new, j, state, out, max_frames, V, beam, K, blank, eos=-1, temperature=1.0,
                                lm_rows=None, lm_weight=0.0, lm_no_blank=False):
    """The j-th new frame of the n listed streams through the frame-synchronous transducer beam search
    (ea_rnnt_frame_beam_stream_step): logits fp32 [n*beam][>= V], row b * beam + beam slot; slot_idx / n_new int32 [n] on the
    device; out = (parent int32, token int32, keep uint8), each [n*beam], written by the step (identity / blank / 1 for an entry
    with j >= n_new, a slot out of range or a full slot, whose state is left as it is)."""
    n = slot_idx.numel()
    assert slot_idx.dtype == n_new.dtype == torch.int32 and n_new.numel() == n and slot_idx.is_contiguous() and n_new.is_contiguous()
    _check_stream_state(state, _lib.lib().ea_rnnt_frame_beam_stream_state_bytes, max_frames, beam)
    parent, token, keep = _check_rnnt_step_args(logits, out, lm_rows, n * beam, V, lm_no_blank)
    check(_lib.lib().ea_rnnt_frame_beam_stream_step(_p(logits), logits.stride(0), _p(lm_rows),
                                                    lm_rows.stride(0) if lm_rows is not None else 0, int(lm_no_blank), _p(slot_idx),
                                                    _p(n_new), j, n, _p(state), _p(parent), _p(token), _p(keep), state.shape[0],
                                                    max_frames, V, beam, K, blank, eos, temperature, lm_weight, _stream()),
          "ea_rnnt_frame_beam_stream_step")


def rnnt_frame_beam_stream_finish(state, slots, max_frames, beam, nbest, pad, max_u, normalize=True):
    """The hypotheses of the slots int32 [n] (device) as if their streams ended now, the state left as it is
    (ea_rnnt_frame_beam_stream_finish).  Returns (tokens int32 [n][nbest][max_u] pad-filled, lengths int32 [n][nbest], scores
    fp32 [n][nbest], nhyp int32 [n]), best first."""
    _check_stream_state(state, _lib.lib().ea_rnnt_frame_beam_stream_state_bytes, max_frames, beam)
    assert slots.dtype == torch.int32 and slots.is_contiguous()
    n, dev = slots.numel(), state.device
    tokens, lengths, scores, nhyp = _finish_outputs(n, nbest, max_u, dev)
    check(_lib.lib().ea_rnnt_frame_beam_stream_finish(_p(state), _p(slots), n, state.shape[0], max_frames, beam, nbest, pad,
                                                      int(bool(normalize)), max_u, _p(tokens), _p(lengths), _p(scores), _p(nhyp),
                                                      _stream()), "ea_rnnt_frame_beam_stream_finish")
    return tokens, lengths, scores, nhyp


def rnnt_frame_beam_stream_partial(state, slots, max_frames, beam, pad, max_u):
    """The best live hypothesis (by the raw score the search prunes by) of the slots int32 [n] (device) and the length of the
    beam's common prefix (ea_rnnt_frame_beam_stream_partial).  Returns (tokens int32 [n][max_u] pad-filled, lengths int32 [n],
    scores fp32 [n], stable_len int32 [n])."""
    _check_stream_state(state, _lib.lib().ea_rnnt_frame_beam_stream_state_bytes, max_frames, beam)
    assert slots.dtype == torch.int32 and slots.is_contiguous()
    n, dev = slots.numel(), state.device
    tokens, lengths, scores, stable = _partial_outputs(n, max_u, dev)
    check(_lib.lib().ea_rnnt_frame_beam_stream_partial(_p(state), _p(slots), n, state.shape[0], max_frames, beam, pad, max_u,
                                                       _p(tokens), _p(lengths), _p(scores), _p(stable), _stream()),
          "ea_rnnt_frame_beam_stream_partial")
    return tokens, lengths, scores, stable


def rnnt_frame_beam_bias_workspace(B, T, beam, device):
    """Workspace of the hotword-biased frame-synchronous transducer beam search (ea_rnnt_frame_beam_bias_workspace_bytes)."""
    return torch.empty(int(_lib.lib().ea_rnnt_frame_beam_bias_workspace_bytes(B, T, beam)), dtype=torch.uint8, device=device)


def rnnt_frame_beam_bias_step(logits, in_len, ws, graph, out, B, T, V, beam, K, blank, t, eos=-1, temperature=1.0, lm_rows=None,
                              lm_weight=0.0, lm_no_blank=False):
    """rnnt_frame_beam_step with a context graph (nodes, edges, root device tables of tools.context_graph.ContextGraph.cuda());
    ws: rnnt_frame_beam_bias_workspace(B, T, beam)."""
    assert in_len.dtype == torch.int32 and in_len.numel() == B
    parent, token, keep = _check_rnnt_step_args(logits, out, lm_rows, B * beam, V, lm_no_blank)
    check(_lib.lib().ea_rnnt_frame_beam_bias_step(_p(logits), logits.stride(0), _p(lm_rows),
                                                  lm_rows.stride(0) if lm_rows is not None else 0, int(lm_no_blank), _p(in_len), _p(ws),
                                                  _p(parent), _p(token), _p(keep), *_cg(graph, V), B, T, V, beam, K, blank, eos,
                                                  temperature, lm_weight, t, _stream()), "ea_rnnt_frame_beam_bias_step")


def rnnt_frame_beam_bias_finish(ws, graph, B, T, beam, nbest, pad, normalize=True):
    """rnnt_frame_beam_finish of a biased search: the scores include the boosts of the completed phrases."""
    dev = ws.device
    tokens, lengths, scores, nhyp = _finish_outputs(B, nbest, T, dev)
    nodes, _, _, n_nodes, _ = _cg(graph)
    check(_lib.lib().ea_rnnt_frame_beam_bias_finish(_p(ws), nodes, n_nodes, B, T, beam, nbest, pad, int(bool(normalize)), _p(tokens),
                                                    _p(lengths), _p(scores), _p(nhyp), _stream()), "ea_rnnt_frame_beam_bias_finish")
    return tokens, lengths, scores, nhyp


def rnnt_frame_beam_stream_bias_state(max_streams, max_frames, beam, device):
    """(state uint8 [max_streams][bytes per slot], zero-filled; bytes per slot) of the streamed, hotword-biased frame-synchronous
    transducer beam search (ea_rnnt_frame_beam_stream_bias_state_bytes)."""
    return _stream_state(_lib.lib().ea_rnnt_frame_beam_stream_bias_state_bytes, max_streams, max_frames, beam, device)


def rnnt_frame_beam_stream_bias_reset(state, slots, max_frames, beam):
    """rnnt_frame_beam_stream_reset of a biased state: the empty hypothesis sits in the graph's root with bias 0."""
    _check_stream_state(state, _lib.lib().ea_rnnt_frame_beam_stream_bias_state_bytes, max_frames, beam)
    assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.device == state.device
    check(_lib.lib().ea_rnnt_frame_beam_stream_bias_reset(_p(state), _p(slots), slots.numel(), state.shape[0], max_frames, beam,
                                                          _stream()), "ea_rnnt_frame_beam_stream_bias_reset")


def rnnt_frame_beam_stream_bias_step(logits, slot_idx, n_new, j, state, graph, out, max_frames, V, beam, K, blank, eos=-1,
                                     temperature=1.0, lm_rows=None, lm_weight=0.0, lm_no_blank=False):
    """rnnt_frame_beam_stream_step with a context graph; state: rnnt_frame_beam_stream_bias_state."""
    n = slot_idx.numel()
    assert slot_idx.dtype == n_new.dtype == torch.int32 and n_new.numel() == n and slot_idx.is_contiguous() and n_new.is_contiguous()
    _check_stream_state(state, _lib.lib().ea_rnnt_frame_beam_stream_bias_state_bytes, max_frames, beam)
    parent, token, keep = _check_rnnt_step_args(logits, out, lm_rows, n * beam, V, lm_no_blank)
    check(_lib.lib().ea_rnnt_frame_beam_stream_bias_step(_p(logits), logits.stride(0), _p(lm_rows),
                                                         lm_rows.stride(0) if lm_rows is not None else 0, int(lm_no_blank),
                                                         _p(slot_idx), _p(n_new), j, n, _p(state), _p(parent), _p(token), _p(keep),
                                                         *_cg(graph, V), state.shape[0], max_frames, V, beam, K, blank, eos,
                                                         temperature, lm_weight, _stream()), "ea_rnnt_frame_beam_stream_bias_step")


def rnnt_frame_beam_stream_bias_finish(state, slots, graph, max_frames, beam, nbest, pad, max_u, normalize=True):
    """rnnt_frame_beam_stream_finish of a biased state: the scores include the boosts of the completed phrases."""
    _check_stream_state(state, _lib.lib().ea_rnnt_frame_beam_stream_bias_state_bytes, max_frames, beam)
    assert slots.dtype == torch.int32 and slots.is_contiguous()
    n, dev = slots.numel(), state.device
    tokens, lengths, scores, nhyp = _finish_outputs(n, nbest, max_u, dev)
    nodes, _, _, n_nodes, _ = _cg(graph)
    check(_lib.lib().ea_rnnt_frame_beam_stream_bias_finish(_p(state), _p(slots), n, state.shape[0], max_frames, beam, nodes, n_nodes,
                                                           nbest, pad, int(bool(normalize)), max_u, _p(tokens), _p(lengths), _p(scores),
                                                           _p(nhyp), _stream()), "ea_rnnt_frame_beam_stream_bias_finish")
    return tokens, lengths, scores, nhyp


def rnnt_frame_beam_stream_bias_partial(state, slots, max_frames, beam, pad, max_u):
    """rnnt_frame_beam_stream_partial of a biased state: the live hypothesis with the best score + running bias, and that value."""
    _check_stream_state(state, _lib.lib().ea_rnnt_frame_beam_stream_bias_state_bytes, max_frames, beam)
    assert slots.dtype == torch.int32 and slots.is_contiguous()
    n, dev = slots.numel(), state.device
    tokens, lengths, scores, stable = _partial_outputs(n, max_u, dev)
    check(_lib.lib().ea_rnnt_frame_beam_stream_bias_partial(_p(state), _p(slots), n, state.shape[0], max_frames, beam, pad, max_u,
                                                            _p(tokens), _p(lengths), _p(scores), _p(stable), _stream()),
          "ea_rnnt_frame_beam_stream_bias_partial")
    return tokens, lengths, scores, stable


# ---- time stamps for the four beam searches (the kTimes kernels of csrc/ctc_beam.hip and csrc/rnnt_beam.hip) -----------------
def _times_outputs(n, nbest, max_u, device):
    """(times int32 [n][nbest][max_u], vscores fp32 [n][nbest]) of a finish with time stamps."""
    return torch.empty(n, nbest, max_u, dtype=torch.int32, device=device), torch.empty(n, nbest, dtype=torch.float32, device=device)


def _check_times_state(tstate, bytes_fn, max_frames, beam, state):
    assert tstate.dtype == torch.uint8 and tstate.is_contiguous() and tstate.dim() == 2 and tstate.device == state.device
    assert tstate.shape == (state.shape[0], bytes_fn(max_frames, beam))


def ctc_prefix_beam_times_workspace(B, T, beam, device):
    """Times workspace of the CTC prefix beam search (ea_ctc_prefix_beam_times_workspace_bytes), beside its beam workspace."""
    return torch.empty(int(_lib.lib().ea_ctc_prefix_beam_times_workspace_bytes(B, T, beam)), dtype=torch.uint8, device=device)


def ctc_prefix_beam_times_step(x, in_len, ws, tws, B, T, V, beam, K, blank, t0, t1, graph=None, lm_rows=None, lm_weight=0.0,
                               ins_bonus=0.0, lm_out=None, ld=None):
    """ctc_prefix_beam_step (graph None; ws its workspace) or ctc_prefix_beam_bias_step (ws the bias workspace) that also follows
    every hypothesis' best alignment path in tws (ctc_prefix_beam_times_workspace)."""
    L = _lib.lib()
    ld = x.stride(0) if ld is None else ld
    assert x.dtype in (torch.float32, torch.bfloat16) and x.stride(-1) == 1 and x.shape[0] == B * T and x.shape[1] == V
    assert in_len.dtype == torch.int32 and in_len.numel() == B
    assert ws.numel() >= (L.ea_ctc_prefix_beam_workspace_bytes if graph is None else L.ea_ctc_prefix_beam_bias_workspace_bytes)(B, T, beam)
    assert tws.dtype == torch.uint8 and tws.numel() >= L.ea_ctc_prefix_beam_times_workspace_bytes(B, T, beam)
    parent, token, keep = lm_out if lm_out is not None else (None, None, None)
    if lm_rows is not None:
        assert lm_rows.dtype == torch.float32 and lm_rows.stride(1) == 1 and lm_rows.shape == (B * beam, V) and t1 == t0 + 1
        assert parent.numel() == token.numel() == keep.numel() == B * beam
        assert parent.dtype == token.dtype == torch.int32 and keep.dtype == torch.uint8
    check(L.ea_ctc_prefix_beam_times_step(_p(x), ld, int(x.dtype == torch.bfloat16), _p(in_len), _p(ws), _p(tws), _p(lm_rows),
                                          lm_rows.stride(0) if lm_rows is not None else 0, _p(parent), _p(token), _p(keep),
                                          *_cg_or_none(graph, V), B, T, V, beam, K, blank, lm_weight, ins_bonus, t0, t1, _stream()),
          "ea_ctc_prefix_beam_times_step")


def ctc_prefix_beam_times_finish(ws, tws, B, T, beam, nbest, pad, graph=None, lm_rows=None, lm_weight=0.0, ins_bonus=0.0, eos=-1):
    """ctc_prefix_beam_finish / _bias_finish and (times int32 [B][nbest][T], -1 after the hypothesis; vscores fp32 [B][nbest])."""
    dev = ws.device
    tokens, lengths, scores, nhyp = _finish_outputs(B, nbest, T, dev)
    times, vscores = _times_outputs(B, nbest, T, dev)
    nodes, _, _, n_nodes, _ = _cg_or_none(graph)
    check(_lib.lib().ea_ctc_prefix_beam_times_finish(_p(ws), _p(tws), _p(lm_rows), lm_rows.stride(0) if lm_rows is not None else 0,
                                                     lm_weight, ins_bonus, eos, nodes, n_nodes, B, T, beam, nbest, pad, _p(tokens),
                                                     _p(lengths), _p(scores), _p(nhyp), _p(times), _p(vscores), _stream()),
          "ea_ctc_prefix_beam_times_finish")
    return tokens, lengths, scores, nhyp, times, vscores


def ctc_prefix_beam_stream_times_state(max_streams, max_frames, beam, device):
    """(times state uint8 [max_streams][bytes per slot], bytes per slot) beside a ctc_prefix_beam_stream_state."""
    return _stream_state(_lib.lib().ea_ctc_prefix_beam_stream_times_state_bytes, max_streams, max_frames, beam, device)


def ctc_prefix_beam_stream_times_reset(state, tstate, slots, max_frames, beam):
    """ctc_prefix_beam_stream_reset of the slots and of their times slots (ea_ctc_prefix_beam_stream_times_reset)."""
    L = _lib.lib()
    _check_stream_state(state, L.ea_ctc_prefix_beam_stream_state_bytes, max_frames, beam)
    _check_times_state(tstate, L.ea_ctc_prefix_beam_stream_times_state_bytes, max_frames, beam, state)
    assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.device == state.device
    check(L.ea_ctc_prefix_beam_stream_times_reset(_p(state), _p(tstate), _p(slots), slots.numel(), state.shape[0], max_frames, beam,
                                                  _stream()), "ea_ctc_prefix_beam_stream_times_reset")


def ctc_prefix_beam_stream_times_step(x, meta, state, tstate, max_frames, V, beam, K, blank, j0=0, j1=None, graph=None, lm_rows=None,
                                      lm_weight=0.0, ins_bonus=0.0, lm_out=None, ld=None):
    """ctc_prefix_beam_stream_step that also follows every hypothesis' best alignment path in the streams' times slots."""
    L = _lib.lib()
    ld = x.stride(0) if ld is None else ld
    assert x.dtype in (torch.float32, torch.bfloat16) and x.dim() == 2 and x.stride(-1) == 1 and x.shape[1] == V
    assert meta.dtype == torch.int32 and meta.dim() == 2 and meta.shape[0] == 3 and meta.is_contiguous()
    _check_stream_state(state, L.ea_ctc_prefix_beam_stream_state_bytes, max_frames, beam)
    _check_times_state(tstate, L.ea_ctc_prefix_beam_stream_times_state_bytes, max_frames, beam, state)
    n = meta.shape[1]
    j1 = max(x.shape[0], j0) if j1 is None else j1
    parent, token, keep = lm_out if lm_out is not None else (None, None, None)
    if lm_rows is not None:
        assert lm_rows.dtype == torch.float32 and lm_rows.stride(1) == 1 and lm_rows.shape == (n * beam, V) and j1 == j0 + 1
        assert parent.numel() == token.numel() == keep.numel() == n * beam
        assert parent.dtype == token.dtype == torch.int32 and keep.dtype == torch.uint8
    check(L.ea_ctc_prefix_beam_stream_times_step(_p(x), ld, int(x.dtype == torch.bfloat16), x.shape[0], _p(meta[0]), _p(meta[1]),
                                                 _p(meta[2]), j0, j1, n, _p(state), _p(tstate), _p(lm_rows),
                                                 lm_rows.stride(0) if lm_rows is not None else 0, _p(parent), _p(token), _p(keep),
                                                 *_cg_or_none(graph, V), state.shape[0], max_frames, V, beam, K, blank, lm_weight,
                                                 ins_bonus, _stream()), "ea_ctc_prefix_beam_stream_times_step")


def ctc_prefix_beam_stream_times_finish(state, tstate, slots, max_frames, beam, nbest, pad, max_u, graph=None, lm_rows=None,
                                        lm_weight=0.0, ins_bonus=0.0, eos=-1):
    """ctc_prefix_beam_stream_finish and (times int32 [n][nbest][max_u], vscores fp32 [n][nbest]); frames count from the
    stream's first frame.  The states are read only."""
    L = _lib.lib()
    _check_stream_state(state, L.ea_ctc_prefix_beam_stream_state_bytes, max_frames, beam)
    _check_times_state(tstate, L.ea_ctc_prefix_beam_stream_times_state_bytes, max_frames, beam, state)
    assert slots.dtype == torch.int32 and slots.is_contiguous() and 1 <= nbest <= beam
    n, dev = slots.numel(), state.device
    if lm_rows is not None:
        assert lm_rows.dtype == torch.float32 and lm_rows.dim() == 2 and lm_rows.stride(1) == 1 and lm_rows.shape[0] == n * beam
    tokens, lengths, scores, nhyp = _finish_outputs(n, nbest, max_u, dev)
    times, vscores = _times_outputs(n, nbest, max_u, dev)
    nodes, _, _, n_nodes, _ = _cg_or_none(graph)
    check(L.ea_ctc_prefix_beam_stream_times_finish(_p(state), _p(tstate), _p(slots), n, _p(lm_rows),
                                                   lm_rows.stride(0) if lm_rows is not None else 0, lm_weight, ins_bonus, eos, nodes,
                                                   n_nodes, state.shape[0], max_frames, beam, nbest, pad, max_u, _p(tokens),
                                                   _p(lengths), _p(scores), _p(nhyp), _p(times), _p(vscores), _stream()),
          "ea_ctc_prefix_beam_stream_times_finish")
    return tokens, lengths, scores, nhyp, times, vscores


def ctc_prefix_beam_stream_endpoint(state, tstate, slots, max_frames, beam, silence_frames, empty_frames, segment_frames, lm_weight=0.0,
                                    ins_bonus=0.0, biased=False):
    """The endpoint probe of the slots int32 [n] (device) of a streamed search with times (ea_ctc_prefix_beam_stream_endpoint):
    int32 [n][4] = (rule, F, L, E) for the hypothesis ctc_prefix_beam_stream_partial reports with the same lm_weight, ins_bonus
    and biased.  A threshold <= 0 switches its rule off; a missing times state is refused by the entry point.  Read only."""
    L = _lib.lib()
    _check_stream_state(state, L.ea_ctc_prefix_beam_stream_state_bytes, max_frames, beam)
    if tstate is not None:
        _check_times_state(tstate, L.ea_ctc_prefix_beam_stream_times_state_bytes, max_frames, beam, state)
    assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.device == state.device
    n = slots.numel()
    out = torch.empty(n, 4, dtype=torch.int32, device=state.device)
    check(L.ea_ctc_prefix_beam_stream_endpoint(_p(state), _p(tstate), _p(slots), n, lm_weight, ins_bonus, int(bool(biased)),
                                               state.shape[0], max_frames, beam, int(silence_frames), int(empty_frames),
                                               int(segment_frames), _p(out), _stream()), "ea_ctc_prefix_beam_stream_endpoint")
    return out


def rnnt_frame_beam_times_workspace(B, T, beam, device):
    """Times workspace of the frame-synchronous transducer beam search (ea_rnnt_frame_beam_times_workspace_bytes)."""
    return torch.empty(int(_lib.lib().ea_rnnt_frame_beam_times_workspace_bytes(B, T, beam)), dtype=torch.uint8, device=device)


def rnnt_frame_beam_times_step(logits, in_len, ws, tws, out, B, T, V, beam, K, blank, t, graph=None, eos=-1, temperature=1.0,
                               lm_rows=None, lm_weight=0.0, lm_no_blank=False):
    """rnnt_frame_beam_step (graph None) or rnnt_frame_beam_bias_step (ws the bias workspace) that also follows every hypothesis'
    best alignment path in tws (rnnt_frame_beam_times_workspace)."""
    L = _lib.lib()
    assert in_len.dtype == torch.int32 and in_len.numel() == B
    assert tws.dtype == torch.uint8 and tws.numel() >= L.ea_rnnt_frame_beam_times_workspace_bytes(B, T, beam)
    parent, token, keep = _check_rnnt_step_args(logits, out, lm_rows, B * beam, V, lm_no_blank)
    check(L.ea_rnnt_frame_beam_times_step(_p(logits), logits.stride(0), _p(lm_rows), lm_rows.stride(0) if lm_rows is not None else 0,
                                          int(lm_no_blank), _p(in_len), _p(ws), _p(tws), _p(parent), _p(token), _p(keep),
                                          *_cg_or_none(graph, V), B, T, V, beam, K, blank, eos, temperature, lm_weight, t, _stream()),
          "ea_rnnt_frame_beam_times_step")


def rnnt_frame_beam_times_finish(ws, tws, B, T, beam, nbest, pad, graph=None, normalize=True):
    """rnnt_frame_beam_finish / _bias_finish and (times int32 [B][nbest][T], -1 after the hypothesis; vscores fp32 [B][nbest])."""
    dev = ws.device
    tokens, lengths, scores, nhyp = _finish_outputs(B, nbest, T, dev)
    times, vscores = _times_outputs(B, nbest, T, dev)
    nodes, _, _, n_nodes, _ = _cg_or_none(graph)
    check(_lib.lib().ea_rnnt_frame_beam_times_finish(_p(ws), _p(tws), nodes, n_nodes, B, T, beam, nbest, pad, int(bool(normalize)),
                                                     _p(tokens), _p(lengths), _p(scores), _p(nhyp), _p(times), _p(vscores), _stream()),
          "ea_rnnt_frame_beam_times_finish")
    return tokens, lengths, scores, nhyp, times, vscores


def rnnt_frame_beam_stream_times_state(max_streams, max_frames, beam, device):
    """(times state uint8 [max_streams][bytes per slot], bytes per slot) beside a rnnt_frame_beam_stream_state / _bias_state."""
    return _stream_state(_lib.lib().ea_rnnt_frame_beam_stream_times_state_bytes, max_streams, max_frames, beam, device)


def _rnnt_state_bytes_fn(biased):
    L = _lib.lib()
    return L.ea_rnnt_frame_beam_stream_bias_state_bytes if biased else L.ea_rnnt_frame_beam_stream_state_bytes


def rnnt_frame_beam_stream_times_reset(state, tstate, slots, max_frames, beam, biased=False):
    """rnnt_frame_beam_stream_reset (biased: _bias_reset) of the slots and of their times slots."""
    L = _lib.lib()
    _check_stream_state(state, _rnnt_state_bytes_fn(biased), max_frames, beam)
    _check_times_state(tstate, L.ea_rnnt_frame_beam_stream_times_state_bytes, max_frames, beam, state)
    assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.device == state.device
    check(L.ea_rnnt_frame_beam_stream_times_reset(_p(state), _p(tstate), _p(slots), slots.numel(), int(bool(biased)), state.shape[0],
                                                  max_frames, beam, _stream()), "ea_rnnt_frame_beam_stream_times_reset")


def rnnt_frame_beam_stream_times_step(logits, slot_idx, n_new, j, state, tstate, out, max_frames, V, beam, K, blank, graph=None, eos=-1,
                                      temperature=1.0, lm_rows=None, lm_weight=0.0, lm_no_blank=False):
    """rnnt_frame_beam_stream_step (graph None) or _bias_step (state a bias state) that also follows every hypothesis' best
    alignment path in the streams' times slots."""
    L = _lib.lib()
    n = slot_idx.numel()
    assert slot_idx.dtype == n_new.dtype == torch.int32 and n_new.numel() == n and slot_idx.is_contiguous() and n_new.is_contiguous()
    _check_stream_state(state, _rnnt_state_bytes_fn(graph is not None), max_frames, beam)
    _check_times_state(tstate, L.ea_rnnt_frame_beam_stream_times_state_bytes, max_frames, beam, state)
    parent, token, keep = _check_rnnt_step_args(logits, out, lm_rows, n * beam, V, lm_no_blank)
    check(L.ea_rnnt_frame_beam_stream_times_step(_p(logits), logits.stride(0), _p(lm_rows),
                                                 lm_rows.stride(0) if lm_rows is not None else 0, int(lm_no_blank), _p(slot_idx),
                                                 _p(n_new), j, n, _p(state), _p(tstate), _p(parent), _p(token), _p(keep),
                                                 *_cg_or_none(graph, V), state.shape[0], max_frames, V, beam, K, blank, eos, temperature,
                                                 lm_weight, _stream()), "ea_rnnt_frame_beam_stream_times_step")


def rnnt_frame_beam_stream_times_finish(state, tstate, slots, max_frames, beam, nbest, pad, max_u, graph=None, normalize=True):
    """rnnt_frame_beam_stream_finish / _bias_finish and (times int32 [n][nbest][max_u], vscores fp32 [n][nbest]); frames count
    from the stream's first frame.  The states are read only."""
    L = _lib.lib()
    _check_stream_state(state, _rnnt_state_bytes_fn(graph is not None), max_frames, beam)
    _check_times_state(tstate, L.ea_rnnt_frame_beam_stream_times_state_bytes, max_frames, beam, state)
    assert slots.dtype == torch.int32 and slots.is_contiguous()
    n, dev = slots.numel(), state.device
    tokens, lengths, scores, nhyp = _finish_outputs(n, nbest, max_u, dev)
    times, vscores = _times_outputs(n, nbest, max_u, dev)
    nodes, _, _, n_nodes, _ = _cg_or_none(graph)
    check(L.ea_rnnt_frame_beam_stream_times_finish(_p(state), _p(tstate), _p(slots), n, state.shape[0], max_frames, beam, nodes, n_nodes,
                                                   nbest, pad, int(bool(normalize)), max_u, _p(tokens), _p(lengths), _p(scores),
                                                   _p(nhyp), _p(times), _p(vscores), _stream()),
          "ea_rnnt_frame_beam_stream_times_finish")
    return tokens, lengths, scores, nhyp, times, vscores


def rnnt_frame_beam_stream_endpoint(state, tstate, slots, max_frames, beam, silence_frames, empty_frames, segment_frames, biased=False):
    """The endpoint probe of the slots int32 [n] (device) of a streamed search with times (ea_rnnt_frame_beam_stream_endpoint;
    biased: a bias state): int32 [n][4] = (rule, F, L, E) for the hypothesis rnnt_frame_beam_stream_partial / _bias_partial
    reports.  A threshold <= 0 switches its rule off; a missing times state is refused by the entry point.  Read only."""
    L = _lib.lib()
    _check_stream_state(state, _rnnt_state_bytes_fn(biased), max_frames, beam)
    if tstate is not None:
        _check_times_state(tstate, L.ea_rnnt_frame_beam_stream_times_state_bytes, max_frames, beam, state)
    assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.device == state.device
    n = slots.numel()
    out = torch.empty(n, 4, dtype=torch.int32, device=state.device)
    check(L.ea_rnnt_frame_beam_stream_endpoint(_p(state), _p(tstate), _p(slots), n, int(bool(biased)), state.shape[0], max_frames, beam,
                                               int(silence_frames), int(empty_frames), int(segment_frames), _p(out), _stream()),
          "ea_rnnt_frame_beam_stream_endpoint")
    return out


def context_graph_score(graph, tokens, lens):
    """Token rows int32 [N][L] (lens int32 [N]) replayed through a context graph on the device (ea_context_graph_score):
    (running bias fp32 [N][L], final bias fp32 [N], node int32 [N])."""
    assert tokens.dtype == lens.dtype == torch.int32 and tokens.is_contiguous() and tokens.dim() == 2 and lens.numel() == tokens.shape[0]
    N, L = tokens.shape
    running = torch.zeros(N, L, dtype=torch.float32, device=tokens.device)
    final = torch.empty(N, dtype=torch.float32, device=tokens.device)
    q = torch.empty(N, dtype=torch.int32, device=tokens.device)
    nodes, edges, root, n_nodes, n_edges = _cg(graph)
    check(_lib.lib().ea_context_graph_score(nodes, edges, root, n_nodes, n_edges, graph[2].shape[0], _p(tokens), _p(lens), N, L,
                                            _p(running), _p(final), _p(q), _stream()), "ea_context_graph_score")
    return running, final, q


def ctc_viterbi_align(x, targets, in_len, tgt_len, B, T, V, blank, ld=None):
    """Forced alignment of targets int32 [B][Lmax] to x [B*T][V] fp32/bf16 log-probs (batch-major, row pitch ld).  Returns
    (tok_start int32 [B][Lmax], tok_end int32 [B][Lmax], frame_label int32 [B][T], score fp32 [B]), all on the device."""
    ld = x.stride(0) if ld is None else ld
    assert x.dtype in (torch.float32, torch.bfloat16) and x.stride(-1) == 1 and x.shape[0] == B * T and x.shape[1] == V
    assert targets.dtype == torch.int32 and targets.is_contiguous() and targets.shape[0] == B
    assert in_len.dtype == tgt_len.dtype == torch.int32 and in_len.numel() == tgt_len.numel() == B
    Lmax = targets.shape[1]
    dev = x.device
    ws = torch.empty(max(1, int(_lib.lib().ea_ctc_viterbi_workspace_bytes(B, T, Lmax))), dtype=torch.uint8, device=dev)
    tok_start = torch.empty(B, Lmax, dtype=torch.int32, device=dev)
    tok_end = torch.empty(B, Lmax, dtype=torch.int32, device=dev)
    frame_label = torch.empty(B, T, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    check(_lib.lib().ea_ctc_viterbi_align(_p(x), ld, int(x.dtype == torch.bfloat16), _p(targets), _p(in_len), _p(tgt_len), _p(ws),
                                          _p(tok_start), _p(tok_end), _p(frame_label), _p(score), B, T, V, Lmax, blank, _stream()),
          "ea_ctc_viterbi_align")
    return tok_start, tok_end, frame_label, score


def ctc_viterbi_long_tile():
    """(frames, states) of one tile of ea_ctc_viterbi_long_align (compile-time constants of csrc/align_long.hip)."""
    frames, states = ctypes.c_int(0), ctypes.c_int(0)
    check(_lib.lib().ea_ctc_viterbi_long_tile(ctypes.byref(frames), ctypes.byref(states)), "ea_ctc_viterbi_long_tile")
    return frames.value, states.value


def _long_workspace(workspace_bytes, T, U, dev, refusal):
    """The uint8 workspace of a tiled (long-form) CTC entry point, or a ValueError made from `refusal` (a format string over need,
    free, T and U) when it is larger than the device's free memory."""
    need = int(workspace_bytes(T, U))
    free = int(torch.cuda.mem_get_info(dev)[0])
    if need > free:
        raise ValueError(refusal.format(need=need, free=free, T=T, U=U))
    return torch.empty(max(1, need), dtype=torch.uint8, device=dev)


def ctc_viterbi_align_long(x, targets, T, V, blank, ld=None):
    """Forced alignment of ONE sequence of any length: targets int32 [U] to x [T][V] fp32/bf16 log-probs (row pitch ld), tiled
    over the device (ea_ctc_viterbi_long_align).  Returns (tok_start int32 [U], tok_end int32 [U], frame_label int32 [T], frame_lp
    fp32 [T], score fp32 [1]), all on the device.  The backpointers take 2 bits per frame and state; a workspace larger than the
    device's free memory is refused with a ValueError (there is no banded or pruned search)."""
    if ld is None:
        ld = x.stride(0) if T > 1 else V  # (the strides of a tensor of no or one row say nothing)
    assert x.dtype in (torch.float32, torch.bfloat16) and x.dim() == 2 and x.shape[0] == T and x.shape[1] == V
    assert T == 0 or x.stride(-1) == 1
    assert targets.dtype == torch.int32 and targets.is_contiguous() and targets.dim() == 1
    U = targets.numel()
    dev = x.device
    ws = _long_workspace(_lib.lib().ea_ctc_viterbi_long_workspace_bytes, T, U, dev,
                         "long-form alignment of T = {T} frames to U = {U} tokens needs a workspace of {need} bytes, the device has "
                         "{free} bytes free (2 bits per frame and state; there is no banded search)")
    tok_start = torch.empty(U, dtype=torch.int32, device=dev)
    tok_end = torch.empty(U, dtype=torch.int32, device=dev)
    frame_label = torch.empty(T, dtype=torch.int32, device=dev)
    frame_lp = torch.empty(T, dtype=torch.float32, device=dev)
    score = torch.empty(1, dtype=torch.float32, device=dev)
    check(_lib.lib().ea_ctc_viterbi_long_align(_p(x), ld, int(x.dtype == torch.bfloat16), _p(targets) if U else None, _p(ws),
                                               _p(tok_start) if U else None, _p(tok_end) if U else None,
                                               _p(frame_label) if T else None, _p(frame_lp) if T else None, _p(score), T, V, U, blank,
                                               _stream()), "ea_ctc_viterbi_long_align")
    return tok_start, tok_end, frame_label, frame_lp, score


def rnnt_viterbi_align(lpb, lpy, logit_lengths, target_lengths):
    """Forced alignment over a transducer lattice lpb / lpy fp32 [B][T][U1] (ea_rnnt_scan's meaning).  Returns (emit_frame int32
    [B][U1 - 1], score fp32 [B]) on the device."""
    B, T, U1 = lpb.shape
    assert lpb.dtype == lpy.dtype == torch.float32 and lpb.is_contiguous() and lpy.is_contiguous() and lpy.shape == lpb.shape
    assert logit_lengths.dtype == target_lengths.dtype == torch.int32 and logit_lengths.numel() == target_lengths.numel() == B
    dev = lpb.device
    ws = torch.empty(max(1, int(_lib.lib().ea_rnnt_viterbi_workspace_bytes(B, T, U1))), dtype=torch.uint8, device=dev)
    emit_frame = torch.empty(B, U1 - 1, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    check(_lib.lib().ea_rnnt_viterbi_align(_p(lpb), _p(lpy), _p(logit_lengths), _p(target_lengths), _p(ws), _p(emit_frame),
                                           _p(score), B, T, U1, _stream()), "ea_rnnt_viterbi_align")
    return emit_frame, score


def ctc_prefix_posteriors(x, targets, utt, in_len, tgt_len, B, T, V, blank, ld=None, want_psi=False):
    """Per-token posteriors (ea_ctc_prefix_posteriors) of hypotheses targets int32 [N][Lmax] under x [B*T][V] fp32/bf16
    log-probs (batch-major, row pitch ld); hypothesis n reads utterance utt[n].  Returns (logc fp32 [N][Lmax + 1], total fp32
    [N]) and, with want_psi, psi fp32 [N][Lmax], all on the device."""
    ld = x.stride(0) if ld is None else ld
    assert x.dtype in (torch.float32, torch.bfloat16) and x.stride(-1) == 1 and x.shape[0] == B * T and x.shape[1] == V
    assert targets.dtype == torch.int32 and targets.is_contiguous() and targets.dim() == 2
    N, Lmax = targets.shape
    assert utt.dtype == tgt_len.dtype == in_len.dtype == torch.int32 and utt.numel() == tgt_len.numel() == N and in_len.numel() == B
    assert utt.is_contiguous() and tgt_len.is_contiguous() and in_len.is_contiguous()
    dev = x.device
    logc = torch.empty(N, Lmax + 1, dtype=torch.float32, device=dev)
    total = torch.empty(N, dtype=torch.float32, device=dev)
    psi = torch.empty(N, Lmax, dtype=torch.float32, device=dev) if want_psi else None
    check(_lib.lib().ea_ctc_prefix_posteriors(_p(x), ld, int(x.dtype == torch.bfloat16), _p(targets), _p(utt), _p(in_len),
                                              _p(tgt_len), _p(logc), _p(total), _p(psi), N, B, T, V, Lmax,
                                              blank, _stream()), "ea_ctc_prefix_posteriors")
    return (logc, total, psi) if want_psi else (logc, total)


def ctc_prefix_posteriors_long(x, targets, T, V, blank, ld=None, want_psi=False):
    """Per-token posteriors of ONE sequence of any length: targets int32 [U] under x [T][V] fp32/bf16 log-probs (row pitch ld),
    tiled over the device (ea_ctc_prefix_long_posteriors).  Returns (logc fp32 [U + 1], total fp32 [1]) and, with want_psi, psi
    fp32 [U], all on the device.  The workspace holds two scores per frame and state tile and no backpointers; one larger than
    the device's free memory is refused with a ValueError."""
    if ld is None:
        ld = x.stride(0) if T > 1 else V  # (the strides of a tensor of no or one row say nothing)
    assert x.dtype in (torch.float32, torch.bfloat16) and x.dim() == 2 and x.shape[0] == T and x.shape[1] == V
    assert T == 0 or x.stride(-1) == 1
    assert targets.dtype == torch.int32 and targets.is_contiguous() and targets.dim() == 1
    U = targets.numel()
    dev = x.device
    ws = _long_workspace(_lib.lib().ea_ctc_prefix_long_workspace_bytes, T, U, dev,
                         "long-form posteriors of U = {U} tokens over T = {T} frames need a workspace of {need} bytes, the device has "
                         "{free} bytes free (two scores per frame and tile of states)")
    logc = torch.empty(U + 1, dtype=torch.float32, device=dev)
    total = torch.empty(1, dtype=torch.float32, device=dev)
    psi = torch.empty(U, dtype=torch.float32, device=dev) if want_psi else None
    check(_lib.lib().ea_ctc_prefix_long_posteriors(_p(x), ld, int(x.dtype == torch.bfloat16), _p(targets) if U else None, _p(ws),
                                                   _p(logc), _p(total), _p(psi) if want_psi and U else None, T, V, U, blank,
                                                   _stream()), "ea_ctc_prefix_long_posteriors")
    return (logc, total, psi) if want_psi else (logc, total)


def rnnt_prefix_posteriors(lpb, lpy, logit_lengths, target_lengths, want_psi=False):
    """Per-token posteriors (ea_rnnt_prefix_posteriors) over transducer lattices lpb / lpy fp32 [B][T][U1] (ea_rnnt_scan's
    meaning).  Returns (logc fp32 [B][U1], total fp32 [B]) and, with want_psi, psi fp32 [B][U1 - 1], all on the device."""
    B, T, U1 = lpb.shape
    assert lpb.dtype == lpy.dtype == torch.float32 and lpb.is_contiguous() and lpy.is_contiguous() and lpy.shape == lpb.shape
    assert logit_lengths.dtype == target_lengths.dtype == torch.int32 and logit_lengths.numel() == target_lengths.numel() == B
    assert logit_lengths.is_contiguous() and target_lengths.is_contiguous()
    dev = lpb.device
    logc = torch.empty(B, U1, dtype=torch.float32, device=dev)
    total = torch.empty(B, dtype=torch.float32, device=dev)
    psi = torch.empty(B, U1 - 1, dtype=torch.float32, device=dev) if want_psi else None
    check(_lib.lib().ea_rnnt_prefix_posteriors(_p(lpb), _p(lpy), _p(logit_lengths), _p(target_lengths), _p(logc), _p(total),
                                               _p(psi), B, T, U1, _stream()), "ea_rnnt_prefix_posteriors")
    return (logc, total, psi) if want_psi else (logc, total)


def _lattice_views(ws, off_b, off_y, B, T, U1):
    n = B * T * U1
    return (ws[off_b:off_b + 4 * n].view(torch.float32).view(B, T, U1), ws[off_y:off_y + 4 * n].view(torch.float32).view(B, T, U1))


def joint_rnnt_lattice(ws, B, T, U1, V):
    """(lpb, lpy) fp32 [B][T][U1]: views of the lattice `joint_rnnt_loss_fwd` left in its workspace."""
    lib = _lib.lib()
    return _lattice_views(ws, lib.ea_joint_rnnt_lattice_offset(B, T, U1, V, 0), lib.ea_joint_rnnt_lattice_offset(B, T, U1, V, 1),
                          B, T, U1)


def rnnt_lattice(ws, B, T, U1):
    """(lpb, lpy) fp32 [B][T][U1]: views of the lattice `rnnt_loss_fwd` left in its workspace."""
    lib = _lib.lib()
    return _lattice_views(ws, lib.ea_rnnt_lattice_offset(B, T, U1, 0), lib.ea_rnnt_lattice_offset(B, T, U1, 1), B, T, U1)


def ngram_score(handle, ctx, words):
    """ln P(words[i] | ctx[i]) fp32 [N] from an uploaded n-gram handle (ea_ngram_score): ctx int32 [N][order - 1] oldest
    first, front-padded with -1; words int32 [N]."""
    N = words.numel()
    assert words.dtype == ctx.dtype == torch.int32 and ctx.is_contiguous() and words.is_contiguous() and ctx.shape[0] == N
    out = torch.empty(N, dtype=torch.float32, device=words.device)
    check(_lib.lib().ea_ngram_score(handle, _p(ctx) if ctx.numel() else None, _p(words), N, _p(out), _stream()), "ea_ngram_score")
    return out


NGRAM_ROW_LDS = 5120  # columns of a row that ea_ngram_token_rows_step stages in LDS (kNgRowLds); wider rows finish in global memory


class NgramTokenMap:
    """The uploaded (tok2word, word2tok) pair of a sub-word n-gram LM (ea_ngram_token_map_create): tok2word int32 [V] host
    values (>= 0 ARPA word id, -1 no ARPA entry, -2 always -inf), copied to `device` with its inverse."""

    def __init__(self, ngram_handle, tok2word, device):
        tok2word = torch.as_tensor(tok2word, dtype=torch.int32).contiguous().cpu()
        self.V, self._h = tok2word.numel(), ctypes.c_void_p()
        with torch.cuda.device(device):
            check(_lib.lib().ea_ngram_token_map_create(ngram_handle, ctypes.c_void_p(tok2word.data_ptr()), self.V,
                                                       ctypes.byref(self._h)), "ea_ngram_token_map_create")
        self.device = torch.device(device)

    @property
    def handle(self):
        return self._h

    def __del__(self):
        try:
            h, self._h = self._h, None
            if h is not None and h.value:
                _lib.lib().ea_ngram_token_map_destroy(h)
        except Exception:  # interpreter shutdown: the library may already be gone
            pass


def ngram_token_rows_start(handle, token_map, N, W, ld=None):
    """(ctx int32 [N][max(W, 1)], rows fp32 [N][V]) of N empty hypotheses: the context [-1, ..., -1, <s>] and
    ln P(. | <s>) over the dictionary (ea_ngram_token_rows_start).  W = order - 1; with W == 0 the one ctx column is unused."""
    V, dev = token_map.V, token_map.device
    ld = V if ld is None else ld
    ctx = torch.full((N, max(W, 1)), -1, dtype=torch.int32, device=dev)
    rows = torch.empty(N, ld, dtype=torch.float32, device=dev)
    check(_lib.lib().ea_ngram_token_rows_start(handle, token_map.handle, V, N, _p(ctx), _p(rows), ld, _stream()),
          "ea_ngram_token_rows_start")
    return ctx, rows[:, :V]


def ngram_token_rows_step(handle, token_map, ctx_in, parent, token, keep, ctx_out, rows=None, ld=None):
    """One frame of the n-gram LM for N rows in one launch (ea_ngram_token_rows_step): row i continues row parent[i] of ctx_in
    (keep[i]: unchanged, else token[i] appended), its context goes to ctx_out (a buffer other than ctx_in) and
    ln P(. | context) to rows fp32 [N][V] (allocated with row stride `ld` unless given).  Returns rows."""
    V, N = token_map.V, parent.numel()
    assert ctx_in.dtype == ctx_out.dtype == parent.dtype == token.dtype == torch.int32 and keep.dtype == torch.uint8
    assert ctx_in.is_contiguous() and ctx_out.is_contiguous() and ctx_in.shape == ctx_out.shape and ctx_in.shape[0] == N
    assert ctx_in.data_ptr() != ctx_out.data_ptr() and token.numel() == keep.numel() == N
    if rows is None:
        rows = torch.empty(N, V if ld is None else ld, dtype=torch.float32, device=parent.device)
    assert rows.dtype == torch.float32 and rows.stride(1) == 1 and rows.stride(0) >= V and rows.shape[0] == N
    check(_lib.lib().ea_ngram_token_rows_step(handle, token_map.handle, V, _p(ctx_in), _p(parent), _p(token), _p(keep), N,
                                              _p(ctx_out), _p(rows), rows.stride(0), _stream()), "ea_ngram_token_rows_step")
    return rows[:, :V]


def ngram_token_rows_host(handle, tok2word, ctx_in, parent, token, keep, W, ld=None):
    """The contract of `ngram_token_rows_step` on the host tables and numpy arrays (ea_ngram_token_rows_host; no device):
    returns (ctx_out int32 [N][W], rows fp32 [N][V]).  parent None: the N = ctx_in start rows (ctx_in is then a row count)."""
    import numpy as np

    t2w = np.ascontiguousarray(tok2word, dtype=np.int32)
    V = len(t2w)
    ld = V if ld is None else ld
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    if parent is None:
        N, args = int(ctx_in), (None, None, None, None)
    else:
        N = len(parent)
        keep_arrays = (np.ascontiguousarray(ctx_in, dtype=np.int32).reshape(N, W), np.ascontiguousarray(parent, dtype=np.int32),
                       np.ascontiguousarray(token, dtype=np.int32), np.ascontiguousarray(keep, dtype=np.uint8))
        args = tuple(vp(a) for a in keep_arrays)
    ctx_out = np.empty((N, W), dtype=np.int32)
    rows = np.full((N, ld), np.nan, dtype=np.float32)
    check(_lib.lib().ea_ngram_token_rows_host(handle, vp(t2w), V, *args, N, vp(ctx_out), vp(rows), ld), "ea_ngram_token_rows_host")
    return ctx_out, rows[:, :V]


def ctc_lexicon_beam_workspace(B, T, beam, device):
    """Workspace of the lexicon beam search (ea_ctc_lexicon_beam_workspace_bytes): the prefix tables of B utterances."""
    return torch.empty(int(_lib.lib().ea_ctc_lexicon_beam_workspace_bytes(B, T, beam)), dtype=torch.uint8, device=device)


def ctc_lexicon_beam_search(x, in_len, ws, ngram, trie, word_start, space, B, T, V, beam, K, blank, nbest, pad, lm_weight,
                            word_score, ins_bonus, ld=None):
    """The whole lexicon-constrained CTC prefix beam search with n-gram fusion over x [B*T][V] fp32/bf16 log-probs
    (batch-major), one call.  trie = (off, tok, child, word int32, smear fp32) device tensors; word_start uint8 [V] (space
    mode: None).  Returns (tokens int32 [B][nbest][T] pad-filled, lengths int32 [B][nbest], scores fp32 [B][nbest], nhyp
    int32 [B]), best first."""
    ld = x.stride(0) if ld is None else ld
    assert x.dtype in (torch.float32, torch.bfloat16) and x.stride(-1) == 1 and x.shape[0] == B * T and x.shape[1] == V
    assert in_len.dtype == torch.int32 and in_len.numel() == B
    assert ws.numel() >= _lib.lib().ea_ctc_lexicon_beam_workspace_bytes(B, T, beam)
    off, tok, child, word, smear = trie
    assert off.dtype == tok.dtype == child.dtype == word.dtype == torch.int32 and smear.dtype == torch.float32
    assert word_start is None or (word_start.dtype == torch.uint8 and word_start.numel() == V)
    dev = x.device
    tokens, lengths, scores, nhyp = _finish_outputs(B, nbest, T, dev)
    check(_lib.lib().ea_ctc_lexicon_beam_search(_p(x), ld, int(x.dtype == torch.bfloat16), _p(in_len), _p(ws), ngram, _p(off),
                                                _p(tok), _p(child), _p(word), _p(smear), _p(word_start), space, B, T, V, beam, K,
                                                blank, lm_weight, word_score, ins_bonus, nbest, pad, _p(tokens), _p(lengths),
                                                _p(scores), _p(nhyp), _stream()), "ea_ctc_lexicon_beam_search")
    return tokens, lengths, scores, nhyp


def ctc_lexicon_stream_state(max_streams, max_frames, beam, device):
    """(state uint8 [max_streams][bytes per slot], zero-filled; bytes per slot) of the streamed lexicon beam search
    (ea_ctc_lexicon_stream_state_bytes)."""
    return _stream_state(_lib.lib().ea_ctc_lexicon_stream_state_bytes, max_streams, max_frames, beam, device)


def ctc_lexicon_stream_reset(state, slots, ngram, max_frames, beam):
    """The slots int32 [n] (device) of `state` get the search state before frame 0 (ea_ctc_lexicon_stream_reset)."""
    _check_stream_state(state, _lib.lib().ea_ctc_lexicon_stream_state_bytes, max_frames, beam)
    assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.device == state.device
    check(_lib.lib().ea_ctc_lexicon_stream_reset(_p(state), _p(slots), slots.numel(), ngram, state.shape[0], max_frames, beam,
                                                 _stream()), "ea_ctc_lexicon_stream_reset")


def ctc_lexicon_stream_step(x, meta, state, ngram, trie, word_start, space, max_frames, V, beam, K, blank, lm_weight, word_score,
                            ins_bonus, ld=None):
    """The new frames of every ready stream through the lexicon beam search, one launch (ea_ctc_lexicon_stream_step).  x
    [rows][V] fp32/bf16 log-probs packed stream by stream; meta int32 [3][n] = (slot, n_new, row_off) on the device."""
    ld = x.stride(0) if ld is None else ld
    assert x.dtype in (torch.float32, torch.bfloat16) and x.stride(-1) == 1 and x.shape[1] == V
    assert meta.dtype == torch.int32 and meta.dim() == 2 and meta.shape[0] == 3 and meta.is_contiguous()
    _check_stream_state(state, _lib.lib().ea_ctc_lexicon_stream_state_bytes, max_frames, beam)
    off, tok, child, word, smear = trie
    assert off.dtype == tok.dtype == child.dtype == word.dtype == torch.int32 and smear.dtype == torch.float32
    assert word_start is None or (word_start.dtype == torch.uint8 and word_start.numel() == V)
    check(_lib.lib().ea_ctc_lexicon_stream_step(_p(x), ld, int(x.dtype == torch.bfloat16), x.shape[0], _p(meta[0]), _p(meta[1]),
                                                _p(meta[2]), meta.shape[1], _p(state), ngram, _p(off), _p(tok), _p(child),
                                                _p(word), _p(smear), _p(word_start), space, state.shape[0], max_frames, V, beam, K,
                                                blank, lm_weight, word_score, ins_bonus, _stream()), "ea_ctc_lexicon_stream_step")


def ctc_lexicon_stream_finish(state, slots, ngram, trie, max_frames, beam, nbest, pad, max_u, lm_weight, word_score, ins_bonus):
    """The finished hypotheses of the slots int32 [n] (device), the state left as it is (ea_ctc_lexicon_stream_finish).
    Returns (tokens int32 [n][nbest][max_u] pad-filled, lengths int32 [n][nbest], scores fp32 [n][nbest], nhyp int32 [n])."""
    _check_stream_state(state, _lib.lib().ea_ctc_lexicon_stream_state_bytes, max_frames, beam)
    assert slots.dtype == torch.int32 and slots.is_contiguous() and 1 <= nbest <= beam
    word, smear = trie[3], trie[4]
    assert word.dtype == torch.int32 and smear.dtype == torch.float32
    n, dev = slots.numel(), state.device
    tokens, lengths, scores, nhyp = _finish_outputs(n, nbest, max_u, dev)
    check(_lib.lib().ea_ctc_lexicon_stream_finish(_p(state), _p(slots), n, ngram, _p(word), _p(smear), state.shape[0], max_frames,
                                                  beam, lm_weight, word_score, ins_bonus, nbest, pad, max_u, _p(tokens),
                                                  _p(lengths), _p(scores), _p(nhyp), _stream()), "ea_ctc_lexicon_stream_finish")
    return tokens, lengths, scores, nhyp


def ctc_lexicon_stream_partial(state, slots, max_frames, beam, pad, max_u, ins_bonus):
    """The best live hypothesis of the slots int32 [n] (device) and the length of the beam's common prefix
    (ea_ctc_lexicon_stream_partial).  Returns (tokens int32 [n][max_u] pad-filled, lengths int32 [n], scores fp32 [n],
    stable_len int32 [n])."""
    _check_stream_state(state, _lib.lib().ea_ctc_lexicon_stream_state_bytes, max_frames, beam)
    assert slots.dtype == torch.int32 and slots.is_contiguous()
    n, dev = slots.numel(), state.device
    tokens, lengths, scores, stable = _partial_outputs(n, max_u, dev)
    check(_lib.lib().ea_ctc_lexicon_stream_partial(_p(state), _p(slots), n, state.shape[0], max_frames, beam, ins_bonus, pad, max_u,
                                                   _p(tokens), _p(lengths), _p(scores), _p(stable), _stream()),
          "ea_ctc_lexicon_stream_partial")
    return tokens, lengths, scores, stable


def embedding_fwd(tokens, positions, W, pos_table, scale):
    M, C = tokens.numel(), W.shape[1]
    out = torch.empty(M, C, dtype=torch.bfloat16, device=W.device)
    check(_lib.lib().ea_embedding_fwd(_p(tokens), _p(positions), _p(W), _p(pos_table), _p(out), M, C, scale, _stream()),
          "ea_embedding_fwd")
    return out


def embedding_bwd(tokens, dy, dW, scale, pad_idx):
    M, C = dy.shape
    check(_lib.lib().ea_embedding_bwd(_p(tokens), _p(dy), _p(dW), M, C, scale, pad_idx, _stream()), "ea_embedding_bwd")
    return dW


def decode_attention(q, Kc, Vc_off, kv_row, lens, N, H, dh, row_stride, ldkv, koff, voff, max_len):
    """One query per hypothesis.  q bf16 [N][C]; Kc: bf16 cache tensor holding K and V (offsets koff / voff)."""
    out = torch.empty_like(q)
    check(
        _lib.lib().ea_decode_attention(_p(q), _p(Kc), _p(Kc), _p(kv_row), _p(lens), _p(out), N, H, dh, q.stride(0), row_stride,
                                       ldkv, koff, voff, max_len, _stream()),
        "ea_decode_attention",
    )
    return out


def decode_attention_probs(q, Kc, Vc_off, kv_row, lens, N, H, dh, row_stride, ldkv, koff, voff, max_len):
    """decode_attention that also returns the fp32 attention weights [N][H][max_len] (0 past each row's length); the bf16
    output is bit-identical to decode_attention's."""
    out = torch.empty_like(q)
    probs = torch.empty(N, H, max_len, dtype=torch.float32, device=q.device)
    check(
        _lib.lib().ea_decode_attention_probs(_p(q), _p(Kc), _p(Kc), _p(kv_row), _p(lens), _p(out), N, H, dh, q.stride(0), row_stride,
                                             ldkv, koff, voff, max_len, _p(probs), max_len, _stream()),
        "ea_decode_attention_probs",
    )
    return out, probs


def attn_history_put(src, s_row, s_frame, s_head, N, H, S, dst, accumulate=False, div=1.0):
    """dst [N][>=S] fp32 (a slab of the alignment history) <- mean over the H heads of src (element strides s_row / s_frame /
    s_head), added to dst if `accumulate`, then divided by `div`."""
    check(_lib.lib().ea_attn_history_put(_p(src), s_row, s_frame, s_head, N, H, S, _p(dst), dst.stride(0), int(accumulate), float(div),
                                         _stream()), "ea_attn_history_put")
    return dst


def attn_backtrace(A, P, bbsz_idx, step, S):
    """A fp32 [steps][rows][S] slabs, P int32 [steps][rows] parents, bbsz_idx int64 [n] rows at `step` ->
    fp32 [n][S][step+1]: column k is the slab-k row of each hypothesis' ancestor at step k."""
    n = bbsz_idx.numel()
    out = torch.empty(n, S, step + 1, dtype=torch.float32, device=A.device)
    idx = bbsz_idx.contiguous()
    check(_lib.lib().ea_attn_backtrace(_p(A), A.stride(0), A.stride(1), _p(P), P.stride(0), _p(idx), n, step, S, _p(out), _stream()),
          "ea_attn_backtrace")
    return out


def kv_append_reorder(old_cache, new_cache, kv_new, parent, N, L, Lmax, W):
    check(_lib.lib().ea_kv_append_reorder(_p(old_cache), _p(new_cache), _p(kv_new), _p(parent), N, L, Lmax, W, _stream()),
          "ea_kv_append_reorder")
    return new_cache


def beam_mask_rows(lprobs, pad, unk, eos, unk_penalty=0.0, only_eos=False, forbid_eos=False, eos_factor=None):
    N, V = lprobs.shape
    assert lprobs.dtype == torch.float32 and lprobs.is_contiguous()
    check(
        _lib.lib().ea_beam_mask_rows(_p(lprobs), N, V, pad, unk, eos, unk_penalty, int(only_eos), int(forbid_eos),
                                     0.0 if eos_factor is None else float(eos_factor), int(eos_factor is not None), _stream()),
        "ea_beam_mask_rows",
    )
    return lprobs


def beam_topk(lprobs, prev_scores, bsz, beam, nbeam_used, k):
    V = lprobs.shape[1]
    dev = lprobs.device
    cs = torch.empty(bsz, k, dtype=torch.float32, device=dev)
    ct = torch.empty(bsz, k, dtype=torch.int32, device=dev)
    cb = torch.empty(bsz, k, dtype=torch.int32, device=dev)
    check(_lib.lib().ea_beam_topk(_p(lprobs), _p(prev_scores), bsz, beam, nbeam_used, V, k, _p(cs), _p(ct), _p(cb), _stream()),
          "ea_beam_topk")
    return cs, ct, cb


def _rnnt_pitch(logits):
    """(B, T, U1, V, ld) of a [B][T][U1][V] logits tensor that is contiguous or a column-slice view of rows with pitch ld."""
    B, T, U1, V = logits.shape
    assert logits.dtype in (torch.float32, torch.bfloat16) and logits.stride(3) == 1
    ld = logits.stride(2)
    assert ld >= V and logits.stride(1) == U1 * ld and logits.stride(0) == T * U1 * ld, "logits rows must be equally spaced"
    return B, T, U1, V, ld


def rnnt_loss_fwd(logits, targets, logit_lengths, target_lengths, blank):
    """logits fp32 or bf16 [B][T][U1][V] (rows may be padded: a [..., :V] view of a wider buffer); returns (loss [B], workspace)."""
    B, T, U1, V, ld = _rnnt_pitch(logits)
    Umax = targets.shape[1]
    assert U1 == Umax + 1
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    ws = torch.empty(int(_lib.lib().ea_rnnt_workspace_bytes(B, T, U1)), dtype=torch.uint8, device=logits.device)
    check(_lib.lib().ea_rnnt_loss(_p(logits), int(logits.dtype == torch.bfloat16), _p(targets), _p(logit_lengths), _p(target_lengths), _p(loss), _p(ws), B, T, U1, V,
                                  ld, Umax, blank, _stream()), "ea_rnnt_loss")
    return loss, ws


def rnnt_loss_grad(logits, targets, logit_lengths, target_lengths, loss, ws, blank, grad_scale_dev=None, grad_bf16=False):
    """Gradient with the logits' own row pitch (pad columns zero); returned as the [..., :V] view when the rows are padded."""
    B, T, U1, V, ld = _rnnt_pitch(logits)
    grad = torch.empty((B, T, U1, ld), dtype=torch.bfloat16 if grad_bf16 else torch.float32, device=logits.device)
    check(_lib.lib().ea_rnnt_grad(_p(logits), int(logits.dtype == torch.bfloat16), _p(targets), _p(logit_lengths), _p(target_lengths), _p(loss), _p(ws), _p(grad),
                                  int(grad_bf16), B, T, U1, V, ld, targets.shape[1], blank, 1.0, _p(grad_scale_dev), _stream()),
          "ea_rnnt_grad")
    return grad if ld == V else grad[..., :V]


def joint_rnnt_supported(Z, w16) -> bool:
    """Shapes the fused joint + RNN-T kernels take (csrc/joint_rnnt.hip): joint dim a multiple of 64, 16-byte aligned operands."""
    J = Z.shape[1]
    return (Z.is_cuda and Z.dtype == torch.bfloat16 and w16.dtype == torch.bfloat16 and J % 64 == 0 and Z.is_contiguous()
            and w16.is_contiguous() and Z.data_ptr() % 16 == 0 and w16.data_ptr() % 16 == 0 and Z.shape[0] * J < 2 ** 31)


def joint_rnnt_loss_fwd(Z, w16, bias, targets, logit_lengths, target_lengths, B, T, U1, blank):
    """Per-utterance RNN-T loss of logits = Z w16^T + bias WITHOUT materialising them (fp32 accumulators -> log-sum-exp per vocabulary
    tile -> alpha / beta).  Z bf16 [B*T*U1][J].  Returns (loss [B], workspace kept for joint_rnnt_loss_grad)."""
    V, J = w16.shape
    Umax = targets.shape[1]
    assert U1 == Umax + 1 and Z.shape[0] == B * T * U1
    loss = torch.empty(B, dtype=torch.float32, device=Z.device)
    ws = torch.empty(int(_lib.lib().ea_joint_rnnt_workspace_bytes(B, T, U1, V)), dtype=torch.uint8, device=Z.device)
    check(_lib.lib().ea_joint_rnnt_loss(_p(Z), _p(w16), _p(bias), _p(targets), _p(logit_lengths), _p(target_lengths), _p(loss), _p(ws),
                                        B, T, U1, V, J, Umax, blank, _stream()), "ea_joint_rnnt_loss")
    return loss, ws


def joint_rnnt_loss_grad(Z, w16, bias, targets, logit_lengths, target_lengths, loss, ws, B, T, U1, blank, ld, grad_scale_dev=None):
    """d loss / d logits as bf16 [B*T*U1][ld] (pad columns V .. ld - 1 zero), the logits recomputed tile by tile."""
    V, J = w16.shape
    dl = torch.empty(B * T * U1, ld, dtype=torch.bfloat16, device=Z.device)
    check(_lib.lib().ea_joint_rnnt_grad(_p(Z), _p(w16), _p(bias), _p(targets), _p(logit_lengths), _p(target_lengths), _p(loss), _p(ws),
                                        _p(dl), ld, B, T, U1, V, J, targets.shape[1], blank, 1.0, _p(grad_scale_dev), _stream()),
          "ea_joint_rnnt_grad")
    return dl


# ------------------------------------------------------------------------------------------------ LSTM
def lstm_cell_fwd(gates_pre, c_prev, c_out, h_f32, h_bf16, ldh, gates_act, B, H, keep_row=None, h_prev_f32=None, ldg=None,
                  frozen_out_zero=False):
    check(_lib.lib().ea_lstm_cell_fwd(_p(gates_pre), ldg if ldg is not None else 4 * H, _p(c_prev), _p(c_out), _p(h_f32), _p(h_bf16),
                                      ldh, _p(gates_act), _p(keep_row), _p(h_prev_f32), int(frozen_out_zero), B, H, _stream()),
          "ea_lstm_cell_fwd")


def lstm_cell_bwd(dh_bf16, ld_dh, dh_f32, dc_in, gates_act, c_prev, c, dgates, lddg, dc_prev, B, H, frozen=None):
    check(_lib.lib().ea_lstm_cell_bwd(_p(dh_bf16), ld_dh, _p(dh_f32), _p(dc_in), _p(gates_act), _p(c_prev), _p(c), _p(dgates), lddg,
                                      _p(dc_prev), _p(frozen), B, H, _stream()), "ea_lstm_cell_bwd")


def wgrad_group(problems):
    """ea_wgrad_group: for every problem (dy bf16 [M][ld_dy], x bf16 [M][ld_x], dW fp32 [N][ldw] accumulated in place, dbias fp32 [N]
    or None accumulated in place, M, N, K, ld_dy, ld_x, ldw) one grid computes dW += dy^T x and dbias += colsum(dy)."""
    import ctypes

    assert 0 < len(problems) <= 16
    grp = _lib.EaWgradGroup()
    grp.count = len(problems)
    for i, (dy, x, dW, db, M, N, Kk, ld_dy, ld_x, ldw) in enumerate(problems):
        q = grp.p[i]
        q.dy, q.x, q.dW, q.dbias = dy.data_ptr(), x.data_ptr(), dW.data_ptr(), (db.data_ptr() if db is not None else None)
        q.M, q.N, q.K, q.ld_dy, q.ld_x, q.ldw = M, N, Kk, ld_dy, ld_x, ldw
    check(_lib.lib().ea_wgrad_group(ctypes.byref(grp), _stream()), "ea_wgrad_group")


def lstm_seq_supported(B, H):
    return bool(_lib.lib().ea_lstm_seq_supported(int(B), int(H)))


def lstm_seq_fwd(gx, w_hh16, h0_16, c0, frozen, hs, cs, act, h_last, counter, B, U, H, reverse=False, frozen_out_zero=False):
    # the persistent kernels' contract (csrc/lstm_seq.hip): frozen steps emit zeros and start from the zero state
    assert frozen is None or (frozen_out_zero and h0_16 is None and c0 is None), "lstm_seq_fwd: frozen needs frozen_out_zero and no h0 / c0"
    check(_lib.lib().ea_lstm_seq_fwd(_p(gx), _p(w_hh16), _p(h0_16), _p(c0), _p(frozen), _p(hs), _p(cs), _p(act), _p(h_last),
                                     _p(counter), B, U, H, int(reverse), int(frozen_out_zero), _stream()), "ea_lstm_seq_fwd")


def lstm_seq_bwd(dhs, dh_last, dc_last, act, cs, c0, frozen, w_hhT16, dG, dh0, dc0, counter, B, U, H, reverse=False):
    check(_lib.lib().ea_lstm_seq_bwd(_p(dhs), _p(dh_last), _p(dc_last), _p(act), _p(cs), _p(c0), _p(frozen), _p(w_hhT16), _p(dG),
                                     _p(dh0), _p(dc0), _p(counter), B, U, H, int(reverse), _stream()), "ea_lstm_seq_bwd")


def bahdanau_fwd(qp, key, value, nv, bias, lens, T, B, ctx=None, ldc=None, kv_col=None, Bkv=0):
    A, Cv = qp.shape[1], value.shape[-1]
    p = torch.empty(T, B, dtype=torch.float32, device=qp.device)
    if ctx is None:
        ctx = torch.empty(B, Cv, dtype=torch.bfloat16, device=qp.device)
        ldc = Cv
    check(_lib.lib().ea_bahdanau_fwd(_p(qp), _p(key), _p(value), _p(nv), _p(bias), _p(lens), _p(p), _p(ctx), ldc, T, B, A, Cv,
                                     _p(kv_col), Bkv, _stream()), "ea_bahdanau_fwd")
    return p, ctx


def bahdanau_bwd(dctx, qp, key, value, nv, bias, lens, p, dkey_acc, dvalue_acc, dnv_acc, dbias_acc, T, B):
    A, Cv = qp.shape[1], value.shape[-1]
    dqp = torch.empty(B, A, dtype=torch.bfloat16, device=qp.device)
    check(_lib.lib().ea_bahdanau_bwd(_p(dctx), dctx.stride(0), _p(qp), _p(key), _p(value), _p(nv), _p(bias), _p(lens), _p(p), _p(dqp),
                                     _p(dkey_acc), _p(dvalue_acc), _p(dnv_acc), _p(dbias_acc), T, B, A, Cv, _stream()), "ea_bahdanau_bwd")
    return dqp


def gather_rows(src, parent, out=None):
    """out[n] = src[parent[n]] for a contiguous [N][...] fp32 / bf16 tensor; parent int32 on device."""
    assert src.is_contiguous() and src.element_size() in (2, 4)
    N = parent.numel()
    W = src.numel() // src.shape[0]
    if out is None:
        out = torch.empty((N,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    check(_lib.lib().ea_gather_rows(_p(src), _p(out), _p(parent), N, W, src.element_size(), _stream()), "ea_gather_rows")
    return out


def multilevel_lm_step(word_logits, sub_logits, prev_tok, prev_out, word_lp, cum, nodes, children, prev_subword, word_idx,
                       subword_weight, log_oov_penalty, open_vocab, word_eos, word_unk, sub_space, sub_eos, root_id):
    """One multi-level LM fusion step (ea_multilevel_lm_step): updates word_lp [N][Vw] / cum [N] / nodes [N] in place and
    returns the fused sub-word log-probs fp32 [N][Vs].  prev_out None = the first call (every row refreshes its word
    distribution and sits at the root)."""
    N, Vw = word_logits.shape
    Vs = sub_logits.shape[1]
    assert word_logits.dtype == sub_logits.dtype == torch.float32 and word_logits.stride(1) == 1 and sub_logits.stride(1) == 1
    assert prev_tok.dtype == nodes.dtype == torch.int32 and prev_tok.is_contiguous() and nodes.is_contiguous()
    assert word_lp.shape == (N, Vw) and word_lp.is_contiguous() and cum.shape == (N,) and cum.is_contiguous()
    assert prev_out is None or (prev_out.shape == (N, Vs) and prev_out.is_contiguous())
    out = torch.empty(N, Vs, dtype=torch.float32, device=sub_logits.device)
    check(_lib.lib().ea_multilevel_lm_step(_p(word_logits), word_logits.stride(0), _p(sub_logits), sub_logits.stride(0), _p(prev_tok),
                                           _p(prev_out), _p(word_lp), _p(cum), _p(nodes), _p(out), _p(children), _p(prev_subword),
                                           _p(word_idx), N, Vw, Vs, children.shape[1], subword_weight, log_oov_penalty,
                                           int(prev_out is None), int(open_vocab), word_eos, word_unk, sub_space, sub_eos, root_id,
                                           _stream()), "ea_multilevel_lm_step")
    return out


def joint_add_relu(E, D, B, T, U1):
    """Z [B*T*U1][J] bf16 = relu(E[b,t] + D[b,u]).  E, D fp32 (the model's path: sum and ReLU in fp32 as in the reference's
    autocast run, only Z is rounded) or both bf16."""
    J = E.shape[1]
    assert E.dtype == D.dtype and E.is_contiguous() and D.is_contiguous()
    Z = torch.empty(B * T * U1, J, dtype=torch.bfloat16, device=E.device)
    fn = _lib.lib().ea_joint_add_relu_f32 if E.dtype == torch.float32 else _lib.lib().ea_joint_add_relu
    check(fn(_p(E), _p(D), _p(Z), B, T, U1, J, _stream()), "ea_joint_add_relu")
    return Z


def joint_reduce(dZ, B, T, U1, out_f32=False):
    J = dZ.shape[1]
    dt = torch.float32 if out_f32 else torch.bfloat16
    dE = torch.empty(B * T, J, dtype=dt, device=dZ.device)
    dD = torch.empty(B * U1, J, dtype=dt, device=dZ.device)
    fn = _lib.lib().ea_joint_reduce_f32 if out_f32 else _lib.lib().ea_joint_reduce
    check(fn(_p(dZ), _p(dE), _p(dD), B, T, U1, J, _stream()), "ea_joint_reduce")
    return dE, dD


def stream_attention_supported(dh, chunk_size, left_chunks, C) -> bool:
    return bool(_lib.lib().ea_stream_attention_supported(dh, chunk_size, left_chunks, C))


def stream_kv_append(kv, ldkv, cache, meta, frames, B, C, chunk_size, left_chunks, total_rows):
    """cache bf16 [max_streams][(L+1)*cs][2C] <- rows of kv (k, v adjacent); meta int32 [3][B] = (slot_idx, n_new, row_off)."""
    assert meta.dtype == torch.int32 and meta.shape == (3, B) and meta.is_contiguous() and frames.dtype == torch.int32
    max_streams = cache.shape[0]
    assert cache.dtype == torch.bfloat16 and cache.is_contiguous() and cache.shape[1:] == ((left_chunks + 1) * chunk_size, 2 * C)
    check(_lib.lib().ea_stream_kv_append(_p(kv), ldkv, _p(cache), _p(meta[0]), _p(meta[1]), _p(meta[2]), _p(frames), B, C,
                                         chunk_size, left_chunks, max_streams, total_rows, _stream()), "ea_stream_kv_append")


def stream_attention(qu, qv, cache, pp, pp_center, meta, frames, B, H, dh, chunk_size, left_chunks, out=None):
    """Chunk attention over the ring cache (include/espresso_amd.h).  qu / qv bf16 [rows][C]; pp bf16 [R][C] or None."""
    rows, C = qu.shape
    assert C == H * dh and qu.dtype == torch.bfloat16 and qu.is_contiguous()
    assert meta.dtype == torch.int32 and meta.shape == (3, B) and meta.is_contiguous() and frames.dtype == torch.int32
    max_streams = cache.shape[0]
    assert cache.dtype == torch.bfloat16 and cache.is_contiguous() and cache.shape[1:] == ((left_chunks + 1) * chunk_size, 2 * C)
    assert frames.numel() >= max_streams
    if pp is not None:
        assert pp.dtype == torch.bfloat16 and pp.stride(1) == 1 and qv is not None and qv.shape == qu.shape and qv.is_contiguous()
    if out is None:
        out = torch.empty(rows, C, dtype=torch.bfloat16, device=qu.device)
    check(_lib.lib().ea_stream_attention(_p(qu), _p(qv) if pp is not None else None, C, _p(cache), _p(pp),
                                         pp.stride(0) if pp is not None else 0, pp_center, pp.shape[0] if pp is not None else 0,
                                         _p(meta[0]), _p(meta[1]), _p(meta[2]), _p(frames), _p(out), out.stride(0), B, H, dh,
                                         chunk_size, left_chunks, max_streams, rows, _stream()), "ea_stream_attention")
    return out


def stream_convmodule_supported(C, KW, chunk_size) -> bool:
    return bool(_lib.lib().ea_stream_convmodule_supported(C, KW, chunk_size))


def stream_glu_dwconv_bn_act(Y, w, mean_rstd, gamma, beta, carry, meta, B, chunk_size, want_z=False):
    """Streamed middle of a causal conv module for the new rows of B entries (include/espresso_amd.h).  Y bf16 [rows][2C];
    w fp32 [C][KW]; carry bf16 [max_streams][KW-1][C], updated in place; meta int32 [3][B] = (slot_idx, n_new, row_off).
    Returns H bf16 [rows][C], or (H, Z) with want_z."""
    rows, C = Y.shape[0], Y.shape[1] // 2
    KW = w.shape[1]
    assert Y.dtype == torch.bfloat16 and Y.is_contiguous() and Y.shape[1] == 2 * C
    assert w.dtype == torch.float32 and w.is_contiguous() and w.shape == (C, KW)
    assert mean_rstd.dtype == torch.float32 and mean_rstd.is_contiguous() and mean_rstd.numel() == 2 * C
    assert meta.dtype == torch.int32 and meta.shape == (3, B) and meta.is_contiguous()
    assert carry.dtype == torch.bfloat16 and carry.is_contiguous() and carry.shape[1:] == (KW - 1, C)
    H = torch.empty(rows, C, dtype=torch.bfloat16, device=Y.device)
    Z = torch.empty(rows, C, dtype=torch.bfloat16, device=Y.device) if want_z else None
    check(_lib.lib().ea_stream_glu_dwconv_bn_act(_p(Y), _p(w), _p(mean_rstd), _p(gamma), _p(beta), _p(carry), _p(meta[0]),
                                                 _p(meta[1]), _p(meta[2]), _p(H), _p(Z), B, C, KW, chunk_size, carry.shape[0], rows,
                                                 _stream()), "ea_stream_glu_dwconv_bn_act")
    return (H, Z) if want_z else H


def stream_advance(frames, meta, B, chunk_size):
    check(_lib.lib().ea_stream_advance(_p(frames), _p(meta[0]), _p(meta[1]), B, chunk_size, frames.numel(), _stream()),
          "ea_stream_advance")


LONGFORM_MAX_OVERLAP = 12288  # frames of one overlap that ea_longform_cuts holds in LDS


def _longform_args(logits, counts, V):
    assert logits.dim() == 3 and logits.is_contiguous() and logits.dtype in (torch.float32, torch.bfloat16)
    Nw, Tw, ld = logits.shape
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == Nw and counts.device == logits.device
    assert 1 <= V <= ld
    return Nw, Tw, ld, int(logits.dtype == torch.bfloat16)


def longform_cuts(logits, counts, V, Hf, blank, edge, guard):
    """Long-form junction cuts (include/espresso_amd.h, "Long-form recognition").  logits [Nw][Tw][ld >= V] bf16 or fp32, counts
    int32 [Nw] on the device -> (cuts int32 [Nw - 1], scores fp32 [Nw - 1])."""
    Nw, Tw, ld, is_bf16 = _longform_args(logits, counts, V)
    cuts = torch.empty(Nw - 1, dtype=torch.int32, device=logits.device)
    scores = torch.empty(Nw - 1, dtype=torch.float32, device=logits.device)
    check(_lib.lib().ea_longform_cuts(_p(logits), is_bf16, ld, _p(counts), Nw, Tw, V, Hf, blank, edge, guard, _p(cuts), _p(scores),
                                      _stream()), "ea_longform_cuts")
    return cuts, scores


def longform_stitch(logits, counts, cuts, V, Hf, T, out=None):
    """The stitched fp32 log-probs [T][V] of a recording (T = (Nw - 1) * Hf + the last window's frames, known to the caller):
    row t is the log-softmax of frame t's row in the window that owns it under `cuts`.  `out` ([T][ldo >= V] fp32, rows
    contiguous) is written in columns < V only."""
    Nw, Tw, ld, is_bf16 = _longform_args(logits, counts, V)
    assert Nw == 1 or (cuts.dtype == torch.int32 and cuts.is_contiguous() and cuts.numel() == Nw - 1)
    if out is None:
        out = torch.empty(T, V, dtype=torch.float32, device=logits.device)
    assert out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == T and out.stride(1) == 1 and out.shape[1] >= V
    check(_lib.lib().ea_longform_stitch(_p(logits), is_bf16, ld, _p(counts), _p(cuts) if Nw > 1 else None, Nw, Tw, V, Hf, T, _p(out),
                                        out.stride(0), _stream()), "ea_longform_stitch")
    return out


def longform_feature_cuts(x, counts, D, Hf, edge, guard):
    """Long-form junction cuts on encoder outputs (include/espresso_amd.h, "Long-form recognition for transducer models").
    x [Nw][Tw][ld >= D] bf16 or fp32, counts int32 [Nw] on the device -> (cuts int32 [Nw - 1], scores fp32 [Nw - 1], <= 0)."""
    Nw, Tw, ld, is_bf16 = _longform_args(x, counts, D)
    cuts = torch.empty(Nw - 1, dtype=torch.int32, device=x.device)
    scores = torch.empty(Nw - 1, dtype=torch.float32, device=x.device)
    check(_lib.lib().ea_longform_feature_cuts(_p(x), is_bf16, ld, _p(counts), Nw, Tw, D, Hf, edge, guard, _p(cuts), _p(scores),
                                              _stream()), "ea_longform_feature_cuts")
    return cuts, scores


def longform_stitch_rows(x, counts, cuts, D, Hf, T, out=None):
    """The stitched encoder outputs [T][D] of a recording, in x's element type: row t is the bit copy of frame t's row in the window
    that owns it under `cuts`.  `out` ([T][ldo >= D], x's dtype, rows contiguous) is written in columns < D only.  The kernel
    moves bytes: any dtype of 2 or 4 bytes per element."""
    assert x.dim() == 3 and x.is_contiguous() and x.element_size() in (2, 4)
    Nw, Tw, ld = x.shape
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == Nw and counts.device == x.device
    assert 1 <= D <= ld
    assert Nw == 1 or (cuts.dtype == torch.int32 and cuts.is_contiguous() and cuts.numel() == Nw - 1)
    if out is None:
        out = torch.empty(T, D, dtype=x.dtype, device=x.device)
    assert out.dtype == x.dtype and out.dim() == 2 and out.shape[0] == T and out.stride(1) == 1 and out.shape[1] >= D
    assert out.device == x.device
    check(_lib.lib().ea_longform_stitch_rows(_p(x), x.element_size(), ld, _p(counts), _p(cuts) if Nw > 1 else None, Nw, Tw, D, Hf, T,
                                             _p(out), out.stride(0), _stream()), "ea_longform_stitch_rows")
    return out
