"""Plain fp64 restatement of the Conformer convolution module's middle (espresso_amd/csrc/convmodule.hip):
GLU -> depthwise Conv1d -> BatchNorm1d (+ activation), forward and backward.

Plain torch, no call into espresso_amd.  Every function takes the tensors the kernel takes (bf16 activations, fp32 parameters and
statistics) and upcasts them exactly to fp64; nothing is rounded on the way, so a comparison against a kernel's output has only
that kernel's own arithmetic and its one bf16 store to tolerate.  A stage's reference is meant to be fed from the PREVIOUS kernel's
own stored output (its bf16 U, Z, dZ, its fp32 mean / rstd and sums) — those stores are the kernels' documented rounding points.

Next to each result the functions return the magnitude sums (sum of |term| of what was added up) that an error bound of the form
`k * 2^-24 * sum |term|` needs.  Activations are [B*T][C], row m = b*T + t; `act`: 0 identity, 1 ReLU, 2 SiLU.
tests/test_convmodule_kernels.py proves these functions against torch's own operators (CPU, float64, forward and autograd)."""
import torch


def f64(x):
    return x.detach().to(torch.float64)


def pad_of(KW):
    return (KW - 1) // 2


def glu(Y):
    """Y [M][2C] = (a | g)  ->  U = a * sigmoid(g)  [M][C]"""
    Y = f64(Y)
    C = Y.shape[-1] // 2
    return Y[..., :C] * torch.sigmoid(Y[..., C:])


def _shifted(X, B, T, s):
    """X [B*T][C] -> R with R[b,t] = X[b, t+s], zero where t+s leaves [0, T) of utterance b"""
    X3 = X.reshape(B, T, -1)
    R = torch.zeros_like(X3)
    lo, hi = max(0, -s), min(T, T - s)
    if lo < hi:
        R[:, lo:hi] = X3[:, lo + s:hi + s]
    return R.reshape(B * T, -1)


def dwconv(U, w, B, T, KW):
    """Z[b,t,c] = sum_k w[c,k] * U[b, t-PAD+k, c], zero outside [0,T) per utterance  ->  (Z, sum_k |w*u|)"""
    U, w = f64(U), f64(w)
    PAD = pad_of(KW)
    Z, mag = torch.zeros_like(U), torch.zeros_like(U)
    for k in range(KW):
        term = _shifted(U, B, T, k - PAD) * w[:, k]
        Z += term
        mag += term.abs()
    return Z, mag


def bn_stats(Z):
    """per-channel (sum, sum of squares, sum |z|) over the rows"""
    Z = f64(Z)
    return Z.sum(0), (Z * Z).sum(0), Z.abs().sum(0)


def bn_finalize(s, q, n, eps, momentum, rm, rv):
    """batch sums -> (mean, rstd, new running mean, new running var); biased variance clamped at 0 for rstd, times n/(n-1)
    (n > 1) for the running variance"""
    s, q, rm, rv = f64(s), f64(q), f64(rm), f64(rv)
    mean = s / n
    var = (q / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    unb = var * (n / (n - 1.0)) if n > 1 else var
    return mean, rstd, (1.0 - momentum) * rm + momentum * mean, (1.0 - momentum) * rv + momentum * unb


def _act(y, act):
    if act == 2:
        return y * torch.sigmoid(y)
    return y.clamp_min(0.0) if act == 1 else y


def _dact(y, act):
    if act == 2:
        sg = torch.sigmoid(y)
        return sg * (1.0 + y * (1.0 - sg))
    return (y > 0).to(y.dtype) if act == 1 else torch.ones_like(y)


def _dact_mag(y, act):
    """sum of the magnitudes of the terms act'(y) is made of: sg and y*sg*(1-sg) for SiLU (they cancel around y = -1.28, where
    the derivative crosses zero), |act'(y)| itself otherwise"""
    if act == 2:
        sg = torch.sigmoid(y)
        return sg + (y * sg * (1.0 - sg)).abs()
    return _dact(y, act).abs()


def bn_act(Z, mean, rstd, gamma, beta, act):
    """H = act((Z - mean) * rstd * gamma + beta)  ->  (H, |z*sc| + |sh|) with sc = rstd*gamma, sh = beta - mean*sc"""
    Z, mean, rstd, gamma, beta = f64(Z), f64(mean), f64(rstd), f64(gamma), f64(beta)
    sc = rstd * gamma
    sh = beta - mean * sc
    return _act(Z * sc + sh, act), (Z * sc).abs() + sh.abs()


def bn_act_bwd(Z, dH, mean, rstd, gamma, beta, act, training, red=None):
    """dy = dH * act'(y);  sum_dy, sum_dy_xhat over the rows (= dbeta, dgamma);
    dZ = rstd*gamma*(dy - sum_dy/M - xhat*sum_dy_xhat/M) in training mode, rstd*gamma*dy in eval mode.
    `red` = (sum_dy, sum_dy_xhat) as a kernel stored them: dZ is then formed from those instead of this function's own sums.
    Returns a dict with the sums, their magnitude sums, dZ and dZ's magnitude |dy| + |r0| + |xhat*r1| (times rstd*|gamma|), where
    |dy| stands for |dH| times the magnitude sum of act'(y)'s own terms (_dact_mag: equal to |dy| except where SiLU's derivative
    cancels)."""
    Z, dH, mean, rstd, gamma, beta = f64(Z), f64(dH), f64(mean), f64(rstd), f64(gamma), f64(beta)
    M = Z.shape[0]
    xh = (Z - mean) * rstd
    y = xh * gamma + beta
    dy = dH * _dact(y, act)
    out = {"sum_dy": dy.sum(0), "sum_dy_xhat": (dy * xh).sum(0), "mag_dy": dy.abs().sum(0), "mag_dy_xhat": (dy * xh).abs().sum(0)}
    if training:
        s0, s1 = (out["sum_dy"], out["sum_dy_xhat"]) if red is None else (f64(red[0]), f64(red[1]))
        r0, r1 = s0 / M, s1 / M
    else:
        r0 = r1 = torch.zeros_like(mean)
    out["dZ"] = rstd * gamma * (dy - r0 - xh * r1)
    out["dZ_mag"] = rstd * gamma.abs() * (dH.abs() * _dact_mag(y, act) + r0.abs() + (xh * r1).abs())
    return out


def glu_dwconv_bwd(dZ, Y, w, B, T, KW):
    """dU[t] = sum_k w[k] * dZ[t+PAD-k];  dY_a = dU*sigmoid(g),  dY_g = dU*a*sigmoid(g)*(1-sigmoid(g))
    -> (dY [M][2C], sum_k |w*dz| times the same factor)"""
    dZ, Y, w = f64(dZ), f64(Y), f64(w)
    C = dZ.shape[-1]
    PAD = pad_of(KW)
    dU, mag = torch.zeros_like(dZ), torch.zeros_like(dZ)
    for k in range(KW):
        term = _shifted(dZ, B, T, PAD - k) * w[:, k]
        dU += term
        mag += term.abs()
    a, sg = Y[:, :C], torch.sigmoid(Y[:, C:])
    fa, fg = sg, a * sg * (1.0 - sg)
    return torch.cat([dU * fa, dU * fg], 1), torch.cat([mag * fa.abs(), mag * fg.abs()], 1)


def dwconv_wgrad(dZ, U, B, T, KW):
    """dw[c,k] = sum_{b,t} dZ[b,t,c] * U[b, t-PAD+k, c]  ->  (dw [C][KW], sum |dz*u|)"""
    dZ, U = f64(dZ), f64(U)
    PAD = pad_of(KW)
    dw = torch.zeros(dZ.shape[-1], KW, dtype=torch.float64, device=dZ.device)
    mag = torch.zeros_like(dw)
    for k in range(KW):
        term = dZ * _shifted(U, B, T, k - PAD)
        dw[:, k] = term.sum(0)
        mag[:, k] = term.abs().sum(0)
    return dw, mag
