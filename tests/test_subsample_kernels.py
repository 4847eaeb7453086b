"""The Conv2d sub-sampler's convolution kernels (espresso_amd/csrc/subsample.hip, conv_igemm.hip, and conv1_bn_bwd_wgrad_kernel of
convmodule.hip) one kernel at a time against the plain fp64 restatement in tests/subsample_ref.py, through the C ABI.

Buffers are tests/test_convmodule_kernels.py's: every device tensor is a view into a larger allocation, NaN around inputs, a
sentinel bit pattern around outputs (checked after the call), NaN inside outputs (a missed store is a failure, not a stale match).
Utterances — and in one case per kernel channels as well — are drawn at scales a factor 16 apart.  No element is excluded from
any comparison.

EXACT cases.  Inputs, weights, bias and every pre-filled accumulator hold small integers (activations in {-1, 0, 1}, weights
sparse), so every product and every partial sum in any order is an integer below 2^24 and fp32 accumulation is exact whatever the
tiling or split: a bf16 output must be the round-to-nearest-even bf16 of the fp64 integer, an fp32 output the integer itself, the
BatchNorm sums the integer sums (asserted first: sum z^2 < 2^24 per channel).  All of it bit for bit.

REAL-VALUED cases.  Bounds derived from the arithmetic, none measured (ulp(x) = the bf16 step at |x|; mag = the reference's sum
taken over the magnitudes of its terms):
  Z, dX of the gather kernel  vs fp64 on the same bf16 operands    ulp(ref) + K 2^-23 mag     K = products per element: taps * C (+ 1: bias);
                                                                                              the data gradient's taps per parity class
  Z of conv1_fwd              vs fp64 on the fp32 operands         ulp(ref) + 10 2^-23 mag
  BatchNorm sums              vs fp64 on the kernel's own bf16 Z   2^-18 sum |z|, 2^-18 sum z^2   a chain of <= 64 fp32 additions (asserted per
                                                                   (+ 2^-48 of the fp64 total)    kernel below), then fp64 atomics onto the pre-fill
  dW of conv3x3_wgrad         vs fp64 on the bf16 operands + pre-fill   depth 2^-23 mag       depth = 64 chunks_per_wg + nsplit + 1
  dW, dbias of conv1_wgrad    vs fp64 on the kernel's inputs       depth 2^-23 mag            depth = 64 (a thread's run) + 3 (lane groups) + 3 (waves)
                                                                                              + one atomic per workgroup (2048 positions)
  dW, dbias of conv1_bn_bwd   vs fp64 on ea_bn_act_bwd's bf16 dZ   (depth 2^-23 + 2^-16) mag  depth = 64 per 32-position block of a wave (hi and lo
                                                                                              MFMA) + 3 (waves) + one atomic per workgroup
  col2im                      vs fp64 on the bf16 input            ulp(ref) + 9 2^-23 mag
`mag` of an accumulated output includes the pre-fill's magnitude (the last addition rounds at the total's size).  Chain lengths of
the BatchNorm sums: conv1_fwd 16 (a thread's run) + 3 + 3; the gather kernel 2 * 64 / RL rows per thread + RL row lanes (36 for 64
channels, 24 for 128); colstats rows_per_block / 8 + 8.  Every sum's bound (its own share, without the pre-fill's last-place
rounding) is also asserted to be below what one dropped or duplicated position would contribute (sum |term| / M).

The first test needs no GPU: it proves the reference itself against torch.nn.functional.conv2d and its autograd in float64."""
import pytest
import torch
import torch.nn.functional as TF

from tests import convmodule_ref as CR
from tests import subsample_ref as R
from tests.test_convmodule_kernels import (Buf, _bn_inputs, _check, _check_bf16, _gen, _red_checks, _sees_one_row, _st, _sync,  # noqa: F401
                                           _ulp, inp, out)

gpu = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 1e-5
STRIDES = [(1, 1), (2, 2), (1, 2), (2, 1)]
E23 = 2.0 ** -23


# ------------------------------------------------------------------ the reference against torch's operators (CPU, no GPU needed)
@pytest.mark.parametrize("sy,sx", STRIDES)
def test_reference_matches_torch_conv2d_in_float64(sy, sx):
    """tests/subsample_ref.py == F.conv2d(padding=1, stride=(sy, sx)) in float64: forward, the gradient with respect to input, weight
    and bias, T, F in {1, 2, 5, 8}, every tensor within 1e-11 of its scale; the first-layer form (Cin = 1); im2col @ W == conv;
    col2im == the autograd of the im2col gather, for an arbitrary dcol and for dcol = im2col(A)"""
    B, Cin, Cout = 2, 3, 4
    close = lambda a, b: a.shape == b.shape and float((a - b).abs().max()) <= 1e-11 * max(float(b.abs().max()), 1e-300)
    for T in (1, 2, 5, 8):
        for F in (1, 2, 5, 8):
            g = torch.Generator().manual_seed(1000 * sy + 100 * sx + 10 * T + F)
            rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
            for cin in (Cin, 1):
                X, W, bias = rnd(B, T, F, cin), rnd(Cout, 3, 3, cin), rnd(Cout)
                xt, wt, bt = X.permute(0, 3, 1, 2).requires_grad_(), W.permute(0, 3, 1, 2).requires_grad_(), bias.clone().requires_grad_()
                zt = TF.conv2d(xt, wt, bt, stride=(sy, sx), padding=1)
                To, Fo = R.out_size(T, sy), R.out_size(F, sx)
                assert zt.shape == (B, Cout, To, Fo)
                dZ = rnd(B, To, Fo, Cout)
                (zt * dZ.permute(0, 3, 1, 2)).sum().backward()
                if cin == 1:
                    Xr, Wr = R.first_layer(X[..., 0], W[..., 0])
                    assert torch.equal(Xr, X) and torch.equal(Wr, W)
                Z, zmag = R.conv3x3(X, W, bias, sy, sx)
                dX, dxmag = R.conv3x3_dgrad(dZ, W, T, F, sy, sx)
                dW, db, wmag, bmag = R.conv3x3_wgrad(X, dZ, sy, sx)
                tag = (T, F, cin)
                assert close(Z, zt.detach().permute(0, 2, 3, 1)), tag
                assert close(dX, xt.grad.permute(0, 2, 3, 1)), tag
                assert close(dW, wt.grad.permute(0, 2, 3, 1)), tag
                assert close(db, bt.grad), tag
                Z0, _ = R.conv3x3(X, W, None, sy, sx)
                assert close(Z0 + bias, Z), tag
                # the magnitude sums are the same sums over |terms|
                Za, _ = R.conv3x3(X.abs(), W.abs(), bias.abs(), sy, sx)
                dXa, _ = R.conv3x3_dgrad(dZ.abs(), W.abs(), T, F, sy, sx)
                dWa, dba, _, _ = R.conv3x3_wgrad(X.abs(), dZ.abs(), sy, sx)
                assert close(zmag, Za) and close(dxmag, dXa) and close(wmag, dWa) and close(bmag, dba), tag
                # im2col / col2im
                A = X.clone().requires_grad_()
                col = R.im2col(A, sy, sx)
                assert col.shape == (B * To * Fo, 9 * cin)
                assert close(torch.matmul(col.detach(), W.reshape(Cout, 9 * cin).t()).view(B, To, Fo, Cout), Z0), tag
                for dcol in (rnd(*col.shape), col.detach().clone()):
                    (gA,) = torch.autograd.grad(col, A, dcol, retain_graph=True)
                    dA, amag = R.col2im(dcol, B, T, F, sy, sx)
                    assert close(dA, gA), tag
                    assert close(amag, R.col2im(dcol.abs(), B, T, F, sy, sx)[0]), tag
            s, q = R.colstats(col.detach())
            assert close(s, col.detach().sum(0)) and close(q, (col.detach() ** 2).sum(0))


# ------------------------------------------------------------------ data
@pytest.fixture
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from espresso_amd import _lib

    return _lib.lib()  # the HIP library is the thing under test: a missing one is an error, not a skip


def _utt_scale(B):
    """utterance b at scale 16^(b % 3 - 1): neighbours are a factor 16 or 256 apart"""
    return torch.tensor([16.0 ** (b % 3 - 1) for b in range(B)])


def _chan_scale(C):
    """channel c at scale 16^((c // 8 + c) % 3 - 1): neighbouring channels and neighbouring 16-byte slots both differ"""
    c = torch.arange(C)
    return 16.0 ** ((c // 8 + c) % 3 - 1).float()


def _real(g, B, *rest, chan=False):
    """bf16 [B][...][C], utterance b (and, with `chan`, channel c) at its own scale"""
    x = torch.randn(B, *rest, generator=g) * _utt_scale(B).view(B, *([1] * len(rest)))
    if chan:
        x = x * _chan_scale(rest[-1])
    return x.to(BF)


def _ints(g, shape, lo, hi, density=1.0):
    v = torch.randint(lo, hi + 1, tuple(shape), generator=g)
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=g) < density)
    return v.double()


def _same_values(what, got, want):
    """exact cases: got == want bit for bit, every element (`want`: the exact integers, or their bf16 rounding, in any dtype that
    holds them; a sum of integers is never -0, so the bits of an exact zero are +0's in both)"""
    got = got.detach().cpu()
    want = want.detach().to(got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ints = {BF: torch.int16, F32: torch.int32, F64: torch.int64}[got.dtype]
    bad = got.contiguous().view(ints) != want.contiguous().view(ints)
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: got {float(got[idx])!r}, exact {float(want[idx])!r}")


def _bf_exact(ref):
    """the round-to-nearest-even bf16 of an fp64 tensor of integers below 2^24 (exact in fp32 on the way)"""
    assert float(ref.abs().max()) < 2.0 ** 24
    return ref.float().to(BF)


def _stats_check(tag, stats, Z, st0, M, exact):
    """BatchNorm sums against fp64 on the kernel's own stored Z [M][C], accumulated onto st0"""
    C = Z.shape[1]
    s, q = R.colstats(Z)
    sabs = CR.f64(Z).abs().sum(0)
    if exact:
        assert float(q.max()) < 2.0 ** 24, tag  # every fp32 partial sum of z and of z^2 is an integer below 2^24
        _same_values(tag + " stats", stats, st0 + torch.cat([s, q]))
        return
    tot = st0.abs() + torch.cat([sabs, q])
    _check(tag + " stats.sum", stats[:C], st0[:C] + s, 2.0 ** -18 * sabs + 2.0 ** -48 * tot[:C])
    _check(tag + " stats.sumsq", stats[C:], st0[C:] + q, 2.0 ** -18 * q + 2.0 ** -48 * tot[C:])
    _sees_one_row(tag + " stats.sum", 2.0 ** -18 * sabs, sabs, M)   # (the sums' own share of the bound: the pre-fill's last-place
    _sees_one_row(tag + " stats.sumsq", 2.0 ** -18 * q, q, M)        # rounding has nothing to do with the number of rows)


# ------------------------------------------------------------------ the gather kernel: forward and data gradient
# (B, T, F)
#   (1,1,1) (1,1,5) (1,5,1) (2,2,2): all-padding taps, at stride 2 an empty parity class    (3,7,9): 63 positions per utterance, one
#   128-row tile spans three    (2,16,8): exactly two full tiles    (2,37,21): ragged last tile, odd sizes    (1,10,26): even sizes
#           B  T   F   sy sx Cin  Cout bias   stats  chan
FWD_CASES = [(1, 1, 1, 1, 1, 64, 64, True, True, False),
             (1, 1, 5, 2, 2, 64, 128, False, True, False),
             (1, 5, 1, 2, 1, 128, 64, True, False, False),
             (2, 2, 2, 2, 2, 64, 64, True, True, False),
             (2, 2, 2, 1, 2, 192, 128, False, False, False),
             (3, 7, 9, 1, 1, 64, 128, True, True, False),
             (3, 7, 9, 2, 2, 128, 128, True, True, False),
             (2, 16, 8, 1, 1, 128, 64, False, True, False),
             (2, 37, 21, 1, 1, 192, 64, True, True, True),
             (2, 37, 21, 2, 2, 64, 128, True, True, False),
             (2, 37, 21, 1, 2, 128, 128, False, True, False),
             (1, 10, 26, 2, 1, 64, 64, True, True, False),
             (1, 10, 26, 2, 2, 192, 128, True, False, False)]
#             B  T   F   sy sx Cin  Cout chan
DGRAD_CASES = [(1, 1, 1, 1, 1, 64, 64, False),
               (1, 1, 5, 2, 2, 128, 64, False),
               (1, 5, 1, 2, 1, 64, 128, False),
               (2, 2, 2, 2, 2, 64, 192, False),
               (2, 2, 2, 1, 2, 128, 128, False),
               (3, 7, 9, 1, 1, 128, 64, False),
               (3, 7, 9, 2, 2, 64, 128, False),
               (2, 16, 8, 1, 1, 64, 192, False),
               (2, 37, 21, 1, 1, 64, 128, False),
               (2, 37, 21, 2, 2, 128, 192, True),
               (2, 37, 21, 2, 2, 64, 64, False),
               (2, 37, 21, 1, 2, 128, 64, False),
               (1, 10, 26, 2, 1, 64, 64, False),
               (1, 10, 26, 2, 2, 128, 128, False)]


def _id(c):
    return "-".join(str(int(v)) if not isinstance(v, bool) else "ft"[v] for v in c)


def _gather_stats_chain(N):
    RL = 256 // (N // 8)          # row lanes of the epilogue; a thread owns 2 * 64 / RL rows, then RL partial sums are folded
    return 2 * 64 // RL + RL


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("case", FWD_CASES, ids=_id)
def test_conv3x3_forward(lib, case, exact):
    B, T, F, sy, sx, Cin, Cout, has_bias, has_stats, chan = case
    To, Fo = R.out_size(T, sy), R.out_size(F, sx)
    M = B * To * Fo
    g = _gen(31 * T + F + Cin + 7 * sy + sx)
    if exact:
        X, W = _ints(g, (B, T, F, Cin), -1, 1).to(BF), _ints(g, (Cout, 3, 3, Cin), -1, 1, 0.125).to(BF)
        bias, st0 = _ints(g, (Cout,), -3, 3).float(), _ints(g, (2 * Cout,), 0, 1000)
    else:
        X = _real(g, B, T, F, Cin, chan=chan)
        W = torch.randn(Cout, 3, 3, Cin, generator=g) * (9 * Cin) ** -0.5
        if chan:
            W = W * _chan_scale(Cout).view(Cout, 1, 1, 1)
        W, bias, st0 = W.to(BF), torch.randn(Cout, generator=g), 10.0 * torch.randn(2 * Cout, generator=g).double()
    bX, bW, bb = inp(X.reshape(B * T * F, Cin)), inp(W.reshape(Cout, 9 * Cin)), inp(bias)
    bZ, bst = out((M, Cout), BF), out((2 * Cout,), F64, st0)
    assert lib.ea_conv3x3_fwd(bX.p, bW.p, bb.p if has_bias else None, bZ.p, bst.p if has_stats else None, B, T, F, Cin, Cout, sy, sx,
                              _st()) == 0
    _sync()
    assert bZ.intact() and bst.intact()
    Z = bZ.cpu()
    Zr, mag = R.conv3x3(X, W, bias if has_bias else None, sy, sx)
    Zr, mag = Zr.reshape(M, Cout), mag.reshape(M, Cout)
    if exact:
        _same_values("Z", Z, _bf_exact(Zr))
    else:
        _check_bf16("Z", Z, Zr, (9 * Cin + int(has_bias)) * E23 * mag)
    assert _gather_stats_chain(Cout) <= 64
    if has_stats:
        _stats_check("conv3x3_fwd", bst.cpu(), Z, st0, M, exact)
    else:
        _same_values("stats (not passed)", bst.cpu(), st0)
    # the other setting of `stats` leaves Z as it is, bit for bit
    bZ2, bst2 = out((M, Cout), BF), out((2 * Cout,), F64, st0)
    assert lib.ea_conv3x3_fwd(bX.p, bW.p, bb.p if has_bias else None, bZ2.p, None if has_stats else bst2.p, B, T, F, Cin, Cout, sy, sx,
                              _st()) == 0
    _sync()
    assert bZ2.intact() and bst2.intact()
    assert torch.equal(bZ2.bits(), bZ.bits()), "passing / not passing `stats` changed Z"
    if not has_stats:
        _stats_check("conv3x3_fwd", bst2.cpu(), Z, st0, M, exact)


def _dgrad_products(T, F, sy, sx, Cout):
    """products per element of dX: (taps that reach input row ti) * (taps that reach input column fi) * Cout — with stride 2 an
    even coordinate is reached by the centre tap alone, an odd one by the two outer taps"""
    def n(size, s):
        i = torch.arange(size)
        return torch.full((size,), 3.0, dtype=F64) if s == 1 else torch.where(i % 2 == 0, 1.0, 2.0).double()
    return (n(T, sy).view(T, 1) * n(F, sx).view(1, F) * Cout).view(1, T, F, 1)


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("case", DGRAD_CASES, ids=_id)
def test_conv3x3_data_gradient(lib, case, exact):
    B, T, F, sy, sx, Cin, Cout, chan = case
    To, Fo = R.out_size(T, sy), R.out_size(F, sx)
    g = _gen(17 * T + F + Cout + 5 * sy + sx)
    if exact:
        dZ, W = _ints(g, (B, To, Fo, Cout), -1, 1).to(BF), _ints(g, (Cout, 3, 3, Cin), -1, 1, 0.125).to(BF)
    else:
        dZ = _real(g, B, To, Fo, Cout, chan=chan)
        W = torch.randn(Cout, 3, 3, Cin, generator=g) * (9 * Cout) ** -0.5
        if chan:
            W = W * _chan_scale(Cin).view(1, 1, 1, Cin)
        W = W.to(BF)
    Wd = W.permute(3, 1, 2, 0).contiguous()  # [Cin][3][3][Cout]: the forward weight with its channel axes swapped
    bdZ, bWd, bdX = inp(dZ.reshape(B * To * Fo, Cout)), inp(Wd.reshape(Cin, 9 * Cout)), out((B * T * F, Cin), BF)
    assert lib.ea_conv3x3_dgrad(bdZ.p, bWd.p, bdX.p, B, T, F, Cin, Cout, sy, sx, _st()) == 0
    _sync()
    assert bdX.intact()
    dXr, mag = R.conv3x3_dgrad(dZ, W, T, F, sy, sx)
    if exact:
        _same_values("dX", bdX.cpu(), _bf_exact(dXr).reshape(B * T * F, Cin))
    else:
        K = _dgrad_products(T, F, sy, sx, Cout)
        _check_bf16("dX", bdX.cpu(), dXr.reshape(B * T * F, Cin), (K * E23 * mag).reshape(B * T * F, Cin))


# ------------------------------------------------------------------ the 3x3 weight gradient, both output layouts
def _wgrad_split(M, Cin, Cout):
    """conv_igemm.hip's wgrad_split and the reduce kernel's slab groups restated -> (nsplit, chunks_per_wg, reduce groups)"""
    chunks, blocks = (M + 63) // 64, (Cin // 64) * (Cout // 64)
    nsplit = max(1, min((256 + blocks - 1) // blocks, chunks // 8))
    n = Cout * 9 * Cin
    zg = max(1, min(1024 // ((n // 4 + 255) // 256), nsplit // 4))
    return nsplit, (chunks + nsplit - 1) // nsplit, zg


#              B  T   F   sy sx Cin  Cout  M     nsplit groups
WGRAD_CASES = [(1, 1, 1, 1, 1, 64, 64, 1, 1, 1),          # every tap but the centre is padding
               (2, 2, 2, 2, 2, 128, 64, 2, 1, 1),
               (3, 7, 9, 2, 2, 64, 64, 60, 1, 1),         # M < 64: one partial chunk
               (3, 7, 9, 2, 2, 192, 64, 60, 1, 1),
               (1, 8, 8, 1, 1, 64, 128, 64, 1, 1),        # M = 64
               (2, 16, 8, 2, 2, 64, 192, 64, 1, 1),
               (2, 37, 21, 2, 2, 64, 64, 418, 1, 1),      # nsplit = 1, a ragged last chunk
               (2, 37, 21, 2, 2, 64, 128, 418, 1, 1),
               (2, 37, 21, 1, 2, 192, 64, 814, 1, 1),
               (2, 37, 21, 2, 1, 128, 64, 798, 1, 1),
               (2, 26, 40, 1, 1, 64, 64, 2080, 4, 1),     # nsplit > 1 (33 chunks, 9 per workgroup: the last one takes 6), one reduce group
               (2, 26, 40, 1, 1, 192, 64, 2080, 4, 1),
               (2, 26, 40, 1, 1, 64, 192, 2080, 4, 1),
               (2, 52, 40, 1, 1, 64, 64, 4160, 8, 2),     # nsplit = 8, two reduce groups: fp32 atomics onto dW
               (2, 52, 40, 1, 1, 128, 64, 4160, 8, 2),
               (2, 52, 40, 1, 1, 64, 128, 4160, 8, 2),
               (2, 52, 40, 1, 1, 192, 64, 4160, 8, 2),
               (2, 52, 40, 1, 1, 64, 192, 4160, 8, 2)]


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=_id)
def test_conv3x3_weight_gradient_both_layouts(lib, case, exact):
    B, T, F, sy, sx, Cin, Cout, M, nsplit, groups = case
    To, Fo = R.out_size(T, sy), R.out_size(F, sx)
    assert M == B * To * Fo
    n = Cout * 9 * Cin
    ws_bytes = lib.ea_conv3x3_wgrad_workspace_bytes(B, T, F, Cin, Cout, sy, sx)
    assert ws_bytes % (n * 4) == 0 and ws_bytes // (n * 4) == nsplit, (ws_bytes // (n * 4), nsplit)  # the case still covers its path
    assert _wgrad_split(M, Cin, Cout)[0] == nsplit and _wgrad_split(M, Cin, Cout)[2] == groups
    cpw = _wgrad_split(M, Cin, Cout)[1]
    depth = 64 * cpw + nsplit + 1
    g = _gen(13 * T + F + Cin + 3 * Cout + sy)
    chan = (Cin, Cout, M) == (192, 64, 2080)
    if exact:
        X, dZ = _ints(g, (B, T, F, Cin), -1, 1).to(BF), _ints(g, (B, To, Fo, Cout), -1, 1, 0.25).to(BF)
        dW0 = _ints(g, (Cout, 3, 3, Cin), -3, 3)
    else:
        X, dZ = _real(g, B, T, F, Cin, chan=chan), _real(g, B, To, Fo, Cout, chan=chan)
        dW0 = 0.25 * torch.randn(Cout, 3, 3, Cin, generator=g).double()
    dWr, _, mag, _ = R.conv3x3_wgrad(X, dZ, sy, sx)
    want, tol = dW0.float().double() + dWr, depth * E23 * (mag + dW0.abs())
    if not exact:
        _sees_one_row("dW", depth * E23 * mag, mag, M)  # (the sum's own share of the bound, without the pre-fill's)
    bX, bdZ = inp(X.reshape(B * T * F, Cin)), inp(dZ.reshape(M, Cout))
    for param_layout in (False, True):
        perm = (lambda t: t.permute(0, 3, 1, 2).contiguous()) if param_layout else (lambda t: t)
        shape = (Cout * Cin, 9) if param_layout else (Cout * 9, Cin)
        bdW, bws = out(shape, F32, perm(dW0)), out((nsplit * Cout * 9, Cin), F32)
        fn = lib.ea_conv3x3_wgrad_param_layout if param_layout else lib.ea_conv3x3_wgrad
        assert fn(bX.p, bdZ.p, bdW.p, bws.p, B, T, F, Cin, Cout, sy, sx, _st()) == 0
        _sync()
        assert bdW.intact() and bws.intact()
        tag = "dW [Cout][Cin][3][3]" if param_layout else "dW [Cout][3][3][Cin]"
        if exact:
            assert float((mag + dW0.abs()).max()) < 2.0 ** 24
            _same_values(tag, bdW.cpu(), perm(want).reshape(shape))
        else:
            _check(tag, bdW.cpu(), perm(want).reshape(shape), perm(tol).reshape(shape))


# ------------------------------------------------------------------ the first layer: conv1_fwd, conv1_wgrad, conv1_bn_bwd
# positions: below one thread run (16 forward, 64 weight gradient), one run plus one (17, 65), one workgroup plus one (513, 2049);
# (40,2,5) at stride 2 has 3 positions per utterance: every run crosses several utterances; for the fused kernel 513, 1440 and 2049
# are no multiples of 32 and above 128 (waves take different 32-position blocks)
#              CO  B   T    F   sy sx npos
CONV1_CASES = [(64, 1, 3, 5, 1, 1, 15),
               (128, 1, 17, 1, 1, 1, 17),
               (64, 1, 13, 5, 1, 1, 65),
               (128, 40, 2, 5, 2, 2, 120),
               (64, 2, 7, 80, 2, 2, 320),
               (128, 3, 171, 1, 1, 1, 513),
               (64, 3, 113, 5, 2, 2, 513),
               (128, 2, 9, 80, 1, 1, 1440),
               (64, 3, 683, 1, 1, 1, 2049),
               (128, 1, 1, 80, 2, 2, 40),
               (64, 2, 37, 5, 2, 2, 114)]


def _conv1_inputs(g, B, T, F, CO, exact, chan=False):
    if exact:
        return _ints(g, (B, T, F), -2, 2).float(), _ints(g, (CO, 3, 3), -1, 1).float(), _ints(g, (CO,), -3, 3).float()
    X = torch.randn(B, T, F, generator=g) * _utt_scale(B).view(B, 1, 1)
    W = torch.randn(CO, 3, 3, generator=g) / 3.0
    if chan:
        W = W * _chan_scale(CO).view(CO, 1, 1)
    return X, W, torch.randn(CO, generator=g)


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("case", CONV1_CASES, ids=_id)
def test_conv1_forward(lib, case, exact):
    CO, B, T, F, sy, sx, npos = case
    To, Fo = R.out_size(T, sy), R.out_size(F, sx)
    assert npos == B * To * Fo
    g = _gen(npos + CO)
    X, W, bias = _conv1_inputs(g, B, T, F, CO, exact, chan=npos == 1440)
    st0 = _ints(g, (2 * CO,), 0, 1000) if exact else 10.0 * torch.randn(2 * CO, generator=g).double()
    bX, bW, bb = inp(X.reshape(B * T, F)), inp(W.reshape(CO, 9)), inp(bias)
    bZ, bst = out((npos, CO), BF), out((2 * CO,), F64, st0)
    assert lib.ea_conv1_fwd(bX.p, bW.p, bb.p, bZ.p, bst.p, B, T, F, CO, sy, sx, _st()) == 0
    _sync()
    assert bZ.intact() and bst.intact()
    Z = bZ.cpu()
    Zr, mag = R.conv3x3(*R.first_layer(X, W), bias, sy, sx)
    if exact:
        _same_values("Z", Z, _bf_exact(Zr).reshape(npos, CO))
    else:
        _check_bf16("Z", Z, Zr.reshape(npos, CO), 10 * E23 * mag.reshape(npos, CO))
    assert 16 + 3 + 3 <= 64  # a thread's run of 16 positions, three lane-group folds, the four waves
    _stats_check("conv1_fwd", bst.cpu(), Z, st0, npos, exact)
    # stats = NULL (eval): the same Z, bit for bit
    bZ2 = out((npos, CO), BF)
    assert lib.ea_conv1_fwd(bX.p, bW.p, bb.p, bZ2.p, None, B, T, F, CO, sy, sx, _st()) == 0
    _sync()
    assert bZ2.intact() and torch.equal(bZ2.bits(), bZ.bits())


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("case", CONV1_CASES, ids=_id)
def test_conv1_weight_gradient(lib, case, exact):
    CO, B, T, F, sy, sx, npos = case
    To, Fo = R.out_size(T, sy), R.out_size(F, sx)
    g = _gen(3 * npos + CO)
    X, _, _ = _conv1_inputs(g, B, T, F, CO, exact)
    if exact:
        dZ, dW0, db0 = _ints(g, (B, To, Fo, CO), -1, 1).to(BF), _ints(g, (CO, 3, 3), -3, 3), _ints(g, (CO,), -3, 3)
    else:
        dZ = _real(g, B, To, Fo, CO, chan=npos == 1440)
        dW0, db0 = 0.25 * torch.randn(CO, 3, 3, generator=g).double(), 0.25 * torch.randn(CO, generator=g).double()
    depth = 64 + 3 + 3 + (npos + 2047) // 2048
    dWr, dbr, mag, bmag = R.conv3x3_wgrad(R.first_layer(X), dZ, sy, sx)
    dWr, mag = dWr[..., 0], mag[..., 0]
    bX, bdZ = inp(X.reshape(B * T, F)), inp(dZ.reshape(npos, CO))
    bdW, bdb = out((CO, 9), F32, dW0), out((CO,), F32, db0)
    assert lib.ea_conv1_wgrad(bX.p, bdZ.p, bdW.p, bdb.p, B, T, F, CO, sy, sx, _st()) == 0
    _sync()
    assert bdW.intact() and bdb.intact()
    if exact:
        _same_values("dW", bdW.cpu(), (dW0 + dWr).reshape(CO, 9))
        _same_values("dbias", bdb.cpu(), db0 + dbr)
    else:
        wtol, btol = depth * E23 * (mag + dW0.abs()), depth * E23 * (bmag + db0.abs())
        _check("dW", bdW.cpu(), (dW0.float().double() + dWr).reshape(CO, 9), wtol.reshape(CO, 9))
        _check("dbias", bdb.cpu(), db0.float().double() + dbr, btol)
        _sees_one_row("dW", depth * E23 * mag, mag, npos)
        _sees_one_row("dbias", depth * E23 * bmag, bmag, npos)
    # dbias = NULL: dW alone, the same sums (one workgroup: the same bits)
    bdW2 = out((CO, 9), F32, dW0)
    assert lib.ea_conv1_wgrad(bX.p, bdZ.p, bdW2.p, None, B, T, F, CO, sy, sx, _st()) == 0
    _sync()
    assert bdW2.intact()
    if exact or npos <= 2048:
        assert torch.equal(bdW2.bits(), bdW.bits())


@gpu
@pytest.mark.parametrize("training", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("case", CONV1_CASES, ids=_id)
def test_conv1_fused_batchnorm_backward_weight_gradient(lib, case, training):
    """ea_conv1_bn_bwd: dW / dbias against the fp64 weight gradient taken on the bf16 dZ that ea_bn_act_bwd stores for the same
    inputs (the fused kernel forms the same bf16 dZ in registers); the BatchNorm sums and dgamma / dbeta held to
    tests/test_convmodule_kernels.py's bounds.  In training mode the bias gradient (sum of dZ) cancels: it is compared against
    its own bound, depth 2^-23 sum |dz|, not against zero."""
    CO, B, T, F, sy, sx, npos = case
    To, Fo = R.out_size(T, sy), R.out_size(F, sx)
    act = 1  # ReLU, the sub-sampler's
    g = _gen(7 * npos + CO)
    X, _, _ = _conv1_inputs(g, B, T, F, CO, False)
    d = _bn_inputs(npos, CO, seed=11 * npos + CO)
    d["dH"] = (d["dH"].float() * _utt_scale(B).repeat_interleave(To * Fo).view(npos, 1) * (_chan_scale(CO) if npos == 1440 else 1.0)).to(BF)
    Zd = CR.f64(d["Z"])
    if training:
        mean = Zd.mean(0)
        mr = torch.cat([mean, 1.0 / torch.sqrt((Zd * Zd).mean(0) - mean * mean + EPS)]).float()
    else:
        mr = torch.cat([d["rm"], 1.0 / torch.sqrt(d["rv"].double() + EPS).float()]).float()
    dW0, db0 = 0.25 * torch.randn(CO, 9, generator=g), 0.25 * torch.randn(CO, generator=g)
    dg0, dbe0 = torch.randn(CO, generator=g), torch.randn(CO, generator=g)
    bX, bZ, bdH, bmr, bg, bb = inp(X.reshape(B * T, F)), inp(d["Z"]), inp(d["dH"]), inp(mr), inp(d["gamma"]), inp(d["beta"])
    # ---- the separate kernels: red, dZ (bf16, stored)
    bred0, bdZ = out((2 * CO,), F32, torch.zeros(2 * CO)), out((npos, CO), BF)
    assert lib.ea_bn_act_bwd(bZ.p, bdH.p, bmr.p, bg.p, bb.p, bred0.p, bdZ.p, None, None, npos, CO, act, training, _st()) == 0
    _sync()
    assert bred0.intact() and bdZ.intact()
    dZ = bdZ.cpu()
    assert bool(torch.isfinite(dZ.float()).all())
    # ---- the fused kernel
    bred, bdg, bdbe = out((2 * CO,), F32, torch.zeros(2 * CO)), out((CO,), F32, dg0), out((CO,), F32, dbe0)
    bdW, bdb = out((CO, 9), F32, dW0), out((CO,), F32, db0)
    assert lib.ea_conv1_bn_bwd(bX.p, bZ.p, bdH.p, bmr.p, bg.p, bb.p, bred.p, bdg.p, bdbe.p, bdW.p, bdb.p, B, T, F, CO, sy, sx, act,
                               training, _st()) == 0
    _sync()
    for o in (bred, bdg, bdbe, bdW, bdb):
        assert o.intact()
    red = bred.cpu()
    ref = CR.bn_act_bwd(d["Z"], d["dH"], mr[:CO], mr[CO:], d["gamma"], d["beta"], act, bool(training), red=(red[:CO], red[CO:]))
    _red_checks("conv1_bn_bwd", red, ref, npos, CO)
    assert torch.equal(bdbe.cpu(), dbe0 + red[:CO]) and torch.equal(bdg.cpu(), dg0 + red[CO:]), "dgamma / dbeta != prefill + red"
    nb = min((npos + 127) // 128, 1024)
    bpw = -(-((npos + 31) // 32) // (4 * nb))    # 32-position blocks per wave
    depth = 64 * bpw + 3 + nb
    dWr, dbr, mag, bmag = R.conv3x3_wgrad(R.first_layer(X), dZ.view(B, To, Fo, CO), sy, sx)
    dWr, mag = dWr[..., 0].reshape(CO, 9), mag[..., 0].reshape(CO, 9)
    wtol = (depth * E23 + 2.0 ** -16) * (mag + dW0.double().abs())
    btol = (depth * E23 + 2.0 ** -16) * (bmag + db0.double().abs())
    _check("dW", bdW.cpu(), dW0.double() + dWr, wtol)
    _check("dbias", bdb.cpu(), db0.double() + dbr, btol)
    _sees_one_row("dW", (depth * E23 + 2.0 ** -16) * mag, mag, npos)
    _sees_one_row("dbias", (depth * E23 + 2.0 ** -16) * bmag, bmag, npos)
    # dbias = dgamma = dbeta = NULL are accepted and leave dW as it is (one workgroup: the same bits)
    bred2, bdW2 = out((2 * CO,), F32, torch.zeros(2 * CO)), out((CO, 9), F32, dW0)
    assert lib.ea_conv1_bn_bwd(bX.p, bZ.p, bdH.p, bmr.p, bg.p, bb.p, bred2.p, None, None, bdW2.p, None, B, T, F, CO, sy, sx, act,
                               training, _st()) == 0
    _sync()
    assert bred2.intact() and bdW2.intact()
    if nb == 1:
        assert torch.equal(bdW2.bits(), bdW.bits())
    else:
        _check("dW (dbias = NULL)", bdW2.cpu(), dW0.double() + dWr, wtol)


# ------------------------------------------------------------------ im2col / col2im
#               C   B  T   F   sy sx
COL_CASES = [(8, 1, 1, 1, 1, 1),
             (64, 1, 1, 5, 2, 2),
             (8, 1, 5, 1, 2, 1),
             (192, 1, 5, 1, 1, 2),
             (192, 2, 2, 2, 2, 2),
             (64, 2, 2, 2, 1, 2),
             (8, 2, 2, 2, 2, 1),
             (8, 2, 37, 21, 1, 1),
             (64, 2, 37, 21, 2, 2),
             (192, 2, 37, 21, 1, 2),
             (64, 2, 37, 21, 2, 1),
             (192, 2, 37, 21, 2, 2)]


@gpu
@pytest.mark.parametrize("case", COL_CASES, ids=_id)
def test_im2col_is_a_pure_copy(lib, case):
    """bitwise for any data: every bf16 of col is the bit pattern of its source element, +0 where the tap is padding"""
    C, B, T, F, sy, sx = case
    To, Fo = R.out_size(T, sy), R.out_size(F, sx)
    g = _gen(T + F + C)
    A = _real(g, B, T, F, C, chan=True)
    bA, bcol = inp(A.reshape(B * T * F, C)), out((B * To * Fo, 9 * C), BF)
    assert lib.ea_im2col3x3(bA.p, bcol.p, B, T, F, C, sy, sx, _st()) == 0
    _sync()
    assert bcol.intact()
    want = R.im2col(A, sy, sx)
    assert want.dtype == BF and torch.equal(bcol.bits(), want.view(torch.int16)), "col differs bitwise from the gather"


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("case", COL_CASES, ids=_id)
def test_col2im(lib, case, exact):
    C, B, T, F, sy, sx = case
    To, Fo = R.out_size(T, sy), R.out_size(F, sx)
    g = _gen(T + F + C + 1)
    if exact:  # sums of up to nine integers in [-60, 60]: beyond 256 the bf16 store rounds
        dcol = _ints(g, (B * To * Fo, 9 * C), -60, 60).to(BF)
    else:
        dcol = _real(g, B, To * Fo, 9 * C, chan=True).reshape(B * To * Fo, 9 * C)
    bdcol, bdA = inp(dcol), out((B * T * F, C), BF)
    assert lib.ea_col2im3x3(bdcol.p, bdA.p, B, T, F, C, sy, sx, _st()) == 0
    _sync()
    assert bdA.intact()
    dAr, mag = R.col2im(dcol, B, T, F, sy, sx)
    if exact:
        _same_values("dA", bdA.cpu(), _bf_exact(dAr).reshape(B * T * F, C))
    else:
        _check_bf16("dA", bdA.cpu(), dAr.reshape(B * T * F, C), 9 * E23 * mag.reshape(B * T * F, C))


# ------------------------------------------------------------------ colstats
@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("C", [64, 70, 192])  # 70: a partial 64-column block
def test_colstats(lib, C, M, exact):
    g = _gen(M + C)
    if exact:
        X, st0 = _ints(g, (M, C), -3, 3).to(BF), _ints(g, (2 * C,), 0, 1000)
    else:
        X = (torch.randn(M, C, generator=g) * _chan_scale(C) + 0.5).to(BF)
        st0 = 10.0 * torch.randn(2 * C, generator=g).double()
    rpb = max(64, (M + 1023) // 1024)
    assert rpb // 8 + 8 <= 64  # a thread's rows (every eighth of its block's), then the eight row lanes
    bX, bst = inp(X), out((2 * C,), F64, st0)
    assert lib.ea_colstats_bf16(bX.p, bst.p, M, C, _st()) == 0
    _sync()
    assert bst.intact()
    _stats_check("colstats", bst.cpu(), X, st0, M, exact)


# ------------------------------------------------------------------ return codes
@gpu
def test_subsample_return_codes(lib):
    """the documented refusals return -2, an empty problem (B, T or F <= 0, M = 0) returns 0: nothing is stored either way"""
    B, T, F, C = 2, 5, 4, 192
    g = _gen(5)
    bA = inp(_real(g, B * T * F, C))                       # any bf16 activation / gradient / col operand
    bW = inp(torch.randn(C, 9 * C, generator=g).to(BF))    # any bf16 weight
    bXf = inp(torch.randn(B * T, F, generator=g))          # fp32 features
    bf32 = inp(torch.randn(9 * C, generator=g))            # any fp32 vector: bias, conv1 weight, mean_rstd, gamma, beta

    def outs():
        return dict(Z=out((B * T * F, 9 * C), BF), st=out((2 * C,), F64), dW=out((C * 9, C), F32), ws=out((C * 9, C), F32),
                    db=out((C,), F32), red=out((2 * C,), F32), dg=out((C,), F32), dbe=out((C,), F32))

    def run(what, want, call):
        o = outs()
        assert call(o) == want, (what, want)
        _sync()
        for k, b in o.items():
            assert b.untouched(), (what, k)

    s = _st()
    fwd = lambda o, b, t, f, ci, co, sy=1, sx=1: lib.ea_conv3x3_fwd(bA.p, bW.p, bf32.p, o["Z"].p, o["st"].p, b, t, f, ci, co, sy, sx, s)
    dgr = lambda o, b, t, f, ci, co, sy=1, sx=1: lib.ea_conv3x3_dgrad(bA.p, bW.p, o["Z"].p, b, t, f, ci, co, sy, sx, s)
    c1f = lambda o, b, t, f, co, sy=1, sx=1: lib.ea_conv1_fwd(bXf.p, bf32.p, bf32.p, o["Z"].p, o["st"].p, b, t, f, co, sy, sx, s)
    c1w = lambda o, b, t, f, co, sy=1, sx=1: lib.ea_conv1_wgrad(bXf.p, bA.p, o["dW"].p, o["db"].p, b, t, f, co, sy, sx, s)
    c1b = lambda o, b, t, f, co, sy=1, sx=1: lib.ea_conv1_bn_bwd(bXf.p, bA.p, bA.p, bf32.p, bf32.p, bf32.p, o["red"].p, o["dg"].p, o["dbe"].p,
                                                                 o["dW"].p, o["db"].p, b, t, f, co, sy, sx, 1, 1, s)
    i2c = lambda o, b, t, f, c, sy=1, sx=1: lib.ea_im2col3x3(bA.p, o["Z"].p, b, t, f, c, sy, sx, s)
    c2i = lambda o, b, t, f, c, sy=1, sx=1: lib.ea_col2im3x3(bA.p, o["Z"].p, b, t, f, c, sy, sx, s)
    for name in ("ea_conv3x3_wgrad", "ea_conv3x3_wgrad_param_layout"):
        fn = getattr(lib, name)
        wg = lambda o, b, t, f, ci, co, ws=True, sy=1, sx=1: fn(bA.p, bA.p, o["dW"].p, o["ws"].p if ws else None, b, t, f, ci, co, sy, sx, s)
        run(name + " Cin % 64", -2, lambda o: wg(o, B, T, F, 96, 64))
        run(name + " Cout % 64", -2, lambda o: wg(o, B, T, F, 64, 96))
        run(name + " null workspace", -2, lambda o: wg(o, B, T, F, 64, 64, ws=False))
        for (b, t, f) in ((0, T, F), (B, 0, F), (B, T, 0), (B, T, -1)):
            run(name + " empty", 0, lambda o: wg(o, b, t, f, 64, 64, sy=2, sx=2))
    run("fwd Cin % 64", -2, lambda o: fwd(o, B, T, F, 96, 64))
    run("fwd Cout = 192", -2, lambda o: fwd(o, B, T, F, 64, 192))
    run("fwd Cout = 96", -2, lambda o: fwd(o, B, T, F, 64, 96))
    run("dgrad Cin = 192", -2, lambda o: dgr(o, B, T, F, 192, 64))
    run("dgrad Cout % 64", -2, lambda o: dgr(o, B, T, F, 64, 96))
    run("dgrad stride 3 in time", -2, lambda o: dgr(o, B, T, F, 64, 64, 3, 1))
    run("dgrad stride 3 in frequency", -2, lambda o: dgr(o, B, T, F, 64, 64, 1, 3))
    run("conv1_fwd CO % 64", -2, lambda o: c1f(o, B, T, F, 96))
    run("conv1_wgrad CO % 64", -2, lambda o: c1w(o, B, T, F, 96))
    run("conv1_bn_bwd CO % 64", -2, lambda o: c1b(o, B, T, F, 96))
    run("im2col C % 8", -2, lambda o: i2c(o, B, T, F, 12))
    run("col2im C % 8", -2, lambda o: c2i(o, B, T, F, 12))
    run("colstats odd C", -2, lambda o: lib.ea_colstats_bf16(bA.p, o["st"].p, B * T * F, 7, s))
    run("colstats M = 0", 0, lambda o: lib.ea_colstats_bf16(bA.p, o["st"].p, 0, 64, s))
    # B, T or F <= 0: nothing to do.  (F = 0 at stride 2: C division would make Fo = (0 - 1) / 2 + 1 = 1 position per row.)
    for (b, t, f) in ((0, T, F), (B, 0, F), (B, T, 0), (B, T, -1)):
        for sy, sx in ((1, 1), (2, 2)):
            run("fwd empty", 0, lambda o: fwd(o, b, t, f, 64, 64, sy, sx))
            run("dgrad empty", 0, lambda o: dgr(o, b, t, f, 64, 64, sy, sx))
            run("conv1_fwd empty", 0, lambda o: c1f(o, b, t, f, 64, sy, sx))
            run("conv1_wgrad empty", 0, lambda o: c1w(o, b, t, f, 64, sy, sx))
            run("conv1_bn_bwd empty", 0, lambda o: c1b(o, b, t, f, 64, sy, sx))
            run("im2col empty", 0, lambda o: i2c(o, b, t, f, 64, sy, sx))
            run("col2im empty", 0, lambda o: c2i(o, b, t, f, 64, sy, sx))
