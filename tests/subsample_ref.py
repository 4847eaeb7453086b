"""Plain fp64 restatement of the Conv2d sub-sampling front-end's convolutions (espresso_amd/csrc/subsample.hip, conv_igemm.hip and
conv1_bn_bwd_wgrad_kernel of convmodule.hip): 3x3, padding 1, stride (sy, sx), channels-last.

Plain torch, no call into espresso_amd and no conv2d: every function is a loop over the nine taps with strided slices of a
zero-padded tensor and one matmul per tap.  The tensors are taken as the kernels take them (bf16 activations and weights, fp32
features / bias) and upcast exactly to fp64; nothing is rounded on the way.  Next to each result the functions return `mag`, the
same sum taken over the magnitudes of its terms, which an error bound of the form `k * 2^-23 * mag` needs.

  X [B][T][F][Cin]   W [Cout][3][3][Cin]   Z, dZ [B][To][Fo][Cout]   To = (T-1)//sy + 1, Fo = (F-1)//sx + 1
  Z[b,to,fo,:] = bias + sum_{ky,kx} W[:,ky,kx,:] X[b, to*sy+ky-1, fo*sx+kx-1, :]          (zero outside the plane)

The first layer (one input channel, fp32 features [B][T][F], W [CO][3][3]) is the same with Cin = 1: `first_layer` reshapes.
tests/test_subsample_kernels.py proves these functions against torch.nn.functional.conv2d and its autograd (CPU, float64)."""
import torch

F64 = torch.float64


def f64(x):
    return x.detach().to(F64)


def out_size(n, s):
    return (n - 1) // s + 1


def _tap_slices(T, F, sy, sx):
    """(ky, kx, time slice, frequency slice) of the padded plane [T+2][F+2] that tap (ky, kx) reads for the To x Fo outputs"""
    To, Fo = out_size(T, sy), out_size(F, sx)
    for ky in range(3):
        for kx in range(3):
            yield ky, kx, slice(ky, ky + (To - 1) * sy + 1, sy), slice(kx, kx + (Fo - 1) * sx + 1, sx)


def _padded(X):
    B, T, F, C = X.shape
    Xp = torch.zeros(B, T + 2, F + 2, C, dtype=F64)
    Xp[:, 1:T + 1, 1:F + 1] = X
    return Xp


def conv3x3(X, W, bias, sy, sx):
    """-> (Z [B][To][Fo][Cout], mag = |bias| + sum |x| |w|)"""
    X, W = f64(X), f64(W)
    B, T, F, _ = X.shape
    Cout = W.shape[0]
    Xp = _padded(X)
    Z = torch.zeros(B, out_size(T, sy), out_size(F, sx), Cout, dtype=F64)
    mag = torch.zeros_like(Z)
    if bias is not None:
        Z += f64(bias)
        mag += f64(bias).abs()
    for ky, kx, st, sf in _tap_slices(T, F, sy, sx):
        G, w = Xp[:, st, sf], W[:, ky, kx, :]
        Z += torch.matmul(G, w.t())
        mag += torch.matmul(G.abs(), w.abs().t())
    return Z, mag


def conv3x3_dgrad(dZ, W, T, F, sy, sx):
    """the adjoint of conv3x3 in X: every tap's dZ W scattered back onto the slice it was gathered from -> (dX [B][T][F][Cin], mag)"""
    dZ, W = f64(dZ), f64(W)
    B, Cin = dZ.shape[0], W.shape[3]
    dXp = torch.zeros(B, T + 2, F + 2, Cin, dtype=F64)
    magp = torch.zeros_like(dXp)
    for ky, kx, st, sf in _tap_slices(T, F, sy, sx):
        w = W[:, ky, kx, :]
        dXp[:, st, sf] += torch.matmul(dZ, w)
        magp[:, st, sf] += torch.matmul(dZ.abs(), w.abs())
    return dXp[:, 1:T + 1, 1:F + 1].contiguous(), magp[:, 1:T + 1, 1:F + 1].contiguous()


def conv3x3_wgrad(X, dZ, sy, sx):
    """-> (dW [Cout][3][3][Cin], dbias [Cout], mag of dW, mag of dbias)"""
    X, dZ = f64(X), f64(dZ)
    B, T, F, Cin = X.shape
    Cout = dZ.shape[3]
    Xp = _padded(X)
    d2 = dZ.reshape(-1, Cout)
    dW = torch.zeros(Cout, 3, 3, Cin, dtype=F64)
    mag = torch.zeros_like(dW)
    for ky, kx, st, sf in _tap_slices(T, F, sy, sx):
        G = Xp[:, st, sf].reshape(-1, Cin)
        dW[:, ky, kx, :] = torch.matmul(d2.t(), G)
        mag[:, ky, kx, :] = torch.matmul(d2.abs().t(), G.abs())
    return dW, d2.sum(0), mag, d2.abs().sum(0)


def first_layer(X, W=None):
    """fp32 features [B][T][F] -> [B][T][F][1]; W [CO][3][3] -> [CO][3][3][1]"""
    X = f64(X).unsqueeze(-1)
    return X if W is None else (X, f64(W).unsqueeze(-1))


def _gather_index(B, T, F, sy, sx):
    """[B*To*Fo][9] int64: the flat source position b*T*F + t*F + f of every (output position, tap), B*T*F where the tap is padding"""
    To, Fo = out_size(T, sy), out_size(F, sx)
    b = torch.arange(B).view(B, 1, 1, 1)
    t = (torch.arange(To) * sy).view(1, To, 1, 1) + (torch.arange(9) // 3 - 1).view(1, 1, 1, 9)
    f = (torch.arange(Fo) * sx).view(1, 1, Fo, 1) + (torch.arange(9) % 3 - 1).view(1, 1, 1, 9)
    ok = (t >= 0) & (t < T) & (f >= 0) & (f < F)
    idx = (b * T + t) * F + f
    return torch.where(ok, idx, torch.full_like(idx, B * T * F)).reshape(B * To * Fo, 9)


def im2col(A, sy, sx):
    """A [B][T][F][C] -> col [B*To*Fo][9*C], column (ky*3+kx)*C + c: a gather from the positions plus one row of zeros"""
    B, T, F, C = A.shape
    rows = torch.cat([A.reshape(B * T * F, C), torch.zeros(1, C, dtype=A.dtype)])
    idx = _gather_index(B, T, F, sy, sx)
    return rows[idx].reshape(idx.shape[0], 9 * C)


def col2im(dcol, B, T, F, sy, sx):
    """the adjoint of im2col: dcol [B*To*Fo][9*C] -> (dA [B][T][F][C], mag), every tap's block added back onto its slice"""
    dcol = f64(dcol)
    C = dcol.shape[1] // 9
    d5 = dcol.reshape(B, out_size(T, sy), out_size(F, sx), 9, C)
    dAp = torch.zeros(B, T + 2, F + 2, C, dtype=F64)
    magp = torch.zeros_like(dAp)
    for ky, kx, st, sf in _tap_slices(T, F, sy, sx):
        dAp[:, st, sf] += d5[:, :, :, ky * 3 + kx]
        magp[:, st, sf] += d5[:, :, :, ky * 3 + kx].abs()
    return dAp[:, 1:T + 1, 1:F + 1].contiguous(), magp[:, 1:T + 1, 1:F + 1].contiguous()


def colstats(X):
    """X [M][C] -> (sum_m x, sum_m x^2) in fp64"""
    X = f64(X)
    return X.sum(0), (X * X).sum(0)
