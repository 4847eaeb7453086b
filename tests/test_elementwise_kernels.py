"""The streaming element-wise kernels (espresso_amd/csrc/elementwise.hip: the casts, scale + dropout, the column sum, zero-rows, the
embedding forward / backward and the batched transpose) one launch at a time against the plain restatement in tests/rowwise_ref.py,
through the C ABI, every element of every output.

BUFFERS.  As in tests/test_layernorm_kernels.py: every device tensor is a view into a larger allocation (Buf, or the pitched PBuf of
tests/test_gemm_kernels.py) with NaN around inputs — guards and pitch padding — and a sentinel bit pattern around outputs; an output
starts as NaN, or as known data where the call accumulates (the column sum, the embedding's weight gradient) or works in place
(zero-rows).

BIT FOR BIT, no tolerance: the casts (fp32 -> bf16 is round-to-nearest-even from the bit pattern, a NaN stays a NaN of its sign; bf16
-> fp32 is the pattern shifted up), the transpose, zero-rows (flagged rows +0, the others unchanged), and the EXACT cases of scale +
dropout and the column sum: operands small integers, a, b and the keep-scale powers of two (p = 0.5: threshold 2^31, keep-scale 2), so
that every product and every partial sum in any order is an exact dyadic fraction below 2^24 (asserted) whatever the compiler
contracts.

REAL-VALUED cases.  Bounds derived from the arithmetic, none measured; e = 2^-23 is charged per fp32 rounding (tests/
test_layernorm_kernels.py), ulp(x) = the bf16 step at |x|, mag = the expression over the magnitudes of its terms:
  scale + dropout   ulp(ref) + 4 e mag      scale_dropout_kernel, elementwise.hip:84, :96: a x, times keep, b y, the addition
  column sum        chain e mag, chain = ceil(rpb / 8) + 8 + ceil(M / rpb) + 1, rpb = max(64, ceil(M / 256))
                    colsum_kernel :112-131: a thread adds every eighth row of its block's rpb, 8 partial sums are folded, one atomic
                    per row block lands on the pre-fill (whose magnitude is part of mag) in any order; + 1: the first addition
  embedding forward ulp(ref) + 2 e mag      embedding_fwd_kernel :152-153: scale w, the addition of the position's row
  embedding backward (hits + 2) e mag       embedding_bwd_kernel :165: scale dy rounds once, one atomic per row that names the token
Every sum's bound is asserted to stay below one average row's share (_sees_one_row).

The first tests need no GPU: the reference against torch.sum, F.embedding and its autograd, .t() and torch's own bf16 conversion;
mutations that a correct output must not survive (a row left out of a sum, the mask drawn 8 elements off, a colliding row dropped from
the scatter, a pad row not skipped); every case of every GPU test built on the CPU."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import rowwise_ref as R
from tests.test_convmodule_kernels import _INT, _SENTINEL, DEV, Buf, _check, _check_bf16, _gen, _sees_one_row, _st, _sync, _ulp, inp, lib, out  # noqa: F401 (lib: the fixture)
from tests.test_gemm_kernels import PBuf
from tests.test_subsample_kernels import _bf_exact, _ints, _same_values

gpu = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
I16, I32 = torch.int16, torch.int32
E23 = 2.0 ** -23
EXACT = pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])


def _close(a, b):
    return a.shape == b.shape and float((a - b).abs().max()) <= 1e-11 * max(float(b.abs().max()), 1e-300)


def _scale16(n, shift=0):
    return 16.0 ** ((torch.arange(n) + shift) % 3 - 1).double()


def _dev_ints(v, dtype=I32):
    return torch.as_tensor(v, dtype=dtype).to(DEV)


def _dp(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------ the casts' inputs
# fp32 bit patterns: ties to even in both directions and their neighbours, the largest finite value (rounds to inf), the largest bf16,
# the tie above it, +-inf, quiet and signalling NaNs (one whose payload lies in the 16 bits that are cut off, one whose payload would
# carry), +-0, denormals around the tie of the smallest bf16 denormal, the largest denormals
SPECIAL_F32 = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F817FFF, 0x3F818001, 0xBF808000, 0xBF818000, 0x7F7FFFFF, 0x7F7F0000,
               0x7F7F7FFF, 0x7F7F8000, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F80FFFF, 0xFF800001,
               0x7FFFFFFF, 0x00000000, 0x80000000, 0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x807FFFFF,
               0x00800000, 0x80008001]


def _f32_patterns(n, seed):
    """fp32 [n] from bit patterns: the special ones first (as many as fit), then random patterns of every class and ordinary values"""
    g = _gen(seed)
    b = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64)
    half = torch.randn(n, generator=g).view(I32).to(torch.int64)
    b = torch.where(torch.arange(n) % 2 == 0, b, half)
    sp = torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in SPECIAL_F32], dtype=torch.int64)
    k = min(n, sp.numel())
    b[:k] = sp[:k] if n >= sp.numel() else sp[torch.arange(k) * 7 % sp.numel()]
    return b.to(I32).view(F32)


def _bf16_patterns(n, seed):
    """bf16 [n] from bit patterns: all 65536 of them where they fit, then random ones"""
    b = torch.randint(-2 ** 15, 2 ** 15, (n,), generator=_gen(seed), dtype=torch.int64)
    k = min(n, 65536)
    b[:k] = (torch.arange(k) * 40503 % 65536) - 32768 if n < 65536 else torch.arange(65536) - 32768
    return b.to(I16).view(BF)


def _same_cast(what, got_bits, src):
    """bf16 bit patterns against the restated conversion of fp32 `src`: bit for bit; where the source is a NaN, a NaN of its sign"""
    want = R.cast_f32_to_bf16_bits(src).reshape(-1).to(torch.int64) & 0xFFFF
    got = got_bits.reshape(-1).to(torch.int64) & 0xFFFF
    nan = (want & 0x7FFF) > 0x7F80
    assert bool(((got[nan] & 0x7FFF) > 0x7F80).all()) and bool(((got[nan] ^ want[nan]) & 0x8000 == 0).all()), f"{what}: a NaN did not stay a NaN of its sign"
    bad = (got != want) & ~nan
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ, first at {int(bad.nonzero()[0])}: got {int(got[bad][0]):#06x}, want {int(want[bad][0]):#06x}"


# ------------------------------------------------------------------ the reference against torch (CPU, no GPU needed)
def test_reference_matches_torch():
    """tests/rowwise_ref.py == torch's own fp32 -> bf16 conversion on every non-NaN pattern (the specials and 2^20 random ones) and on
    NaN-ness, == the bf16 -> fp32 conversion on all 65536 patterns; == torch.sum, .t(), F.embedding and its autograd with padding_idx,
    and the plain expression of scale + dropout, in float64 within 1e-11 of each tensor's scale"""
    src = _f32_patterns(1 << 20, 3)
    want = src.to(BF).view(I16)
    mine = R.cast_f32_to_bf16_bits(src)
    nan = torch.isnan(src)
    assert torch.equal(mine[~nan], want[~nan]) and bool(torch.isnan(mine[nan].view(BF)).all()) and int(nan.sum()) > 1000
    assert bool(((mine[nan].to(torch.int64) ^ (src[nan].view(I32).to(torch.int64) >> 16)) & 0x8000 == 0).all())
    assert set(v & 0xFFFFFFFF for v in src[:len(SPECIAL_F32)].view(I32).tolist()) == set(SPECIAL_F32)
    pat = _bf16_patterns(65536, 0)
    assert torch.equal(pat.view(I16).to(torch.int64).sort().values, torch.arange(65536) - 32768)
    up = R.cast_bf16_to_f32_bits(pat.view(I16))
    ok = ~torch.isnan(pat)
    assert torch.equal(up.view(F32)[ok], pat.float()[ok]) and bool(torch.isnan(up.view(F32)[~ok]).all())
    assert torch.equal(up.to(torch.int64) & 0xFFFF, torch.zeros(65536, dtype=torch.int64)) and torch.equal(up >> 16, pat.view(I16).to(I32))
    g = _gen(5)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    X, pre = rnd(9, 7), rnd(7)
    v, mag = R.colsum(X, pre)
    assert _close(v, pre + torch.sum(X, 0)) and _close(mag, pre.abs() + X.abs().sum(0))
    assert torch.equal(R.transpose(X), X.t().contiguous())
    x, y, kp = rnd(50), rnd(50), R.keep_flat(11, 0.3, 50)
    v, mag = R.scale_dropout(x, y, -0.7, 1.3, kp)
    flat = torch.from_numpy(R.dropout_ref.keep_mask(11, 50, 0.3))
    assert torch.equal(kp != 0, flat) and _close(v, -0.7 * x * flat * R.drop_params(0.3)[1] + 1.3 * y)
    assert _close(mag, 0.7 * x.abs() * kp + 1.3 * y.abs()) and _close(R.scale_dropout(x, None, 2.0, 9.0)[0], 2.0 * x)
    assert torch.equal(R.keep_flat(11, 0.3, 50, shift=8)[:-8], kp[8:])
    V, C, tok, position = 6, 10, torch.tensor([3, 1, 3, 0, 3]), torch.tensor([2, 0, 5, 2, 6])
    W, pos, dy, dW0 = rnd(V, C).requires_grad_(), rnd(7, C), rnd(5, C), rnd(V, C)
    o = 1.5 * TF.embedding(tok, W, padding_idx=1) + TF.embedding(position, pos)
    v, mag = R.embedding_fwd(tok, position, W, pos, 1.5)
    assert _close(v, o.detach()) and _close(mag, 1.5 * W.detach()[tok].abs() + pos[position].abs())
    assert _close(R.embedding_fwd(tok, None, W, None, 1.5)[0], 1.5 * W.detach()[tok])
    (o * dy).sum().backward()
    dW, mag, hits = R.embedding_bwd(tok, dy, dW0, 1.5, 1)
    assert _close(dW, dW0 + W.grad) and hits.tolist() == [1, 0, 0, 3, 0, 0] and torch.equal(dW[1], dW0[1])
    assert _close(mag[3], dW0[3].abs() + 1.5 * dy[[0, 2, 4]].abs().sum(0))


# ------------------------------------------------------------------ casts
@gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2048 + 5])
def test_cast_f32_to_bf16(lib, n):
    """cast_f32_bf16_kernel: less than a chunk, a whole one, one past it, a whole block and a scalar tail"""
    src = _f32_patterns(n, n)
    if lib is None:
        return
    bs, bd = inp(src), out((n,), BF)
    assert lib.ea_cast_f32_to_bf16(bs.p, bd.p, n, _st()) == 0
    _sync()
    assert bd.intact()
    _same_cast(f"cast {n}", bd.bits(), src)


@gpu
@pytest.mark.parametrize("n", [1, 4096 * 256 + 5])
def test_cast_bf16_to_f32(lib, n):
    """cast_bf16_f32_kernel: 4096 blocks of 256 elements and a second trip of the stride loop for five of them"""
    src = _bf16_patterns(n, n)
    if lib is None:
        return
    bs, bd = inp(src), out((n,), F32)
    assert lib.ea_cast_bf16_to_f32(bs.p, bd.p, n, _st()) == 0
    _sync()
    assert bd.intact()
    assert torch.equal(bd.bits(), R.cast_bf16_to_f32_bits(src.view(I16))), f"bf16 -> fp32 {n}"


def _pitched(rows, cols, ld):
    return torch.arange(rows).view(rows, 1) * ld + torch.arange(cols).view(1, cols)


ROWS_CASTS = [(3, 5004, 5004, 5008), (3, 5004, 5005, 5008), (3, 5004, 5008, 5016), (3, 5004, 5006, 5013), (3, 5, 8, 8), (1, 2049, 2052, 2056),
              (2, 4096, 4096, 4096)]


@gpu
@pytest.mark.parametrize("M,N,ld_src,ld_dst", ROWS_CASTS)
def test_cast_f32_to_bf16_rows(lib, M, N, ld_src, ld_dst):
    """cast_f32_bf16_rows_kernel: the vocabulary gradient's N = 5004 into pitch 5008 (the chunk 5000 .. 5007 straddles N, the pad is
    zero-filled), ld_src % 4 != 0 and an odd ld_dst (element by element), more than one column block, no pad at all"""
    src = _f32_patterns(M * N, N + ld_src).view(M, N)
    vec = ld_src % 4 == 0 and ld_dst % 8 == 0
    assert vec == ((M, N, ld_src, ld_dst) in (ROWS_CASTS[0], ROWS_CASTS[2], ROWS_CASTS[4], ROWS_CASTS[5], ROWS_CASTS[6])) and (ld_dst > 2048 or N == 5)
    if lib is None:
        return
    bs, bd = PBuf(_pitched(M, N, ld_src), F32, src), out((M, ld_dst), BF)
    assert lib.ea_cast_f32_to_bf16_rows(bs.p, ld_src, bd.p, ld_dst, M, N, _st()) == 0
    _sync()
    assert bd.intact()
    got = bd.bits()
    _same_cast(f"rows cast {M} {N}", got[:, :N], src)
    assert bool((got[:, N:] == 0).all()), "the pad columns N .. ld_dst - 1 are not +0"


@gpu
def test_cast_return_codes(lib):
    bs, bd = inp(torch.zeros(64)), out((64,), BF)
    s = _st()
    assert lib.ea_cast_f32_to_bf16_rows(bs.p, 8, bd.p, 7, 2, 8, s) == -2      # ld_dst < N
    assert lib.ea_cast_f32_to_bf16_rows(bs.p, 7, bd.p, 8, 2, 8, s) == -2      # ld_src < N
    assert lib.ea_cast_f32_to_bf16_rows(bs.p, 8, bd.p, 8, 65536, 8, s) == -2  # more rows than grid.y holds
    assert lib.ea_cast_f32_to_bf16_rows(bs.p, 8, bd.p, 8, 0, 8, s) == 0 and lib.ea_cast_f32_to_bf16_rows(bs.p, 8, bd.p, 8, 2, 0, s) == 0
    assert lib.ea_cast_f32_to_bf16(bs.p, bd.p, 0, s) == 0 and lib.ea_cast_bf16_to_f32(bd.p, bs.p, 0, s) == 0
    _sync()
    assert bd.untouched()


# ------------------------------------------------------------------ scale + dropout
BIG = 4096 * 2048 + 13   # 4097 blocks' worth of chunks on a grid clamped to 4096 (grid_for, elementwise.hip:170-175)
SD_CASES = [(n, y, p) for n in (5, 8, 2053) for y in (False, True) for p in (0.0, 0.1, 0.5)] + [(BIG, True, 0.5), (BIG, False, 0.1)]


def _sd_plan(n, with_y, p, exact):
    P = types.SimpleNamespace()
    g = _gen(n % 100003 + 7 * int(with_y) + int(100 * p) + int(exact))
    if exact:
        p = 0.5 if p else 0.0
        P.x, P.y = _ints(g, (n,), -8, 8).to(BF), _ints(g, (n,), -8, 8).to(BF)
        P.a, P.b = 2.0, -0.5
    else:
        sc = _scale16(n)
        P.x, P.y = (sc * torch.randn(n, generator=g).double()).to(BF), (_scale16(n, 1) * torch.randn(n, generator=g).double()).to(BF)
        P.a, P.b = float(np.float32(0.37)), float(np.float32(-1.3))
    P.p, P.seed = p, 0xC0FFEE1234567 + n
    P.thr, P.scale = R.drop_params(p) if p else (0, 1.0)
    if exact and p:
        assert P.thr == 2 ** 31 and P.scale == 2.0
    kp = R.keep_flat(P.seed, p, n) if p else None
    P.ref, P.mag = R.scale_dropout(P.x, P.y if with_y else None, P.a, P.b, kp)
    if exact:
        assert float(P.mag.max()) < 2.0 ** 24 and torch.equal(R.bf16_rne(P.ref), P.ref)
    return P


def _sd_compare(what, P, got, exact):
    if exact:
        _same_values(what, got, _bf_exact(P.ref))
    else:
        _check_bf16(what, got, P.ref, 4 * E23 * P.mag)


@gpu
@EXACT
@pytest.mark.parametrize("n,with_y,p", SD_CASES)
def test_scale_dropout(lib, n, with_y, p, exact):
    """scale_dropout_kernel: less than a chunk (the scalar tail alone), one chunk, a block and a tail of 5, and 4096 * 2048 + 13: the
    grid is clamped to 4096 blocks, block 0 walks on to the last chunk and the scalar tail of 5"""
    assert (BIG + 2047) // 2048 > 4096 and BIG % 8 == 5
    P = _sd_plan(n, with_y, p, exact)
    if lib is None:
        return
    bx, by, bo = inp(P.x), (inp(P.y) if with_y else None), out((n,), BF)
    rc = lib.ea_scale_dropout_bf16(bx.p, by.p if by else None, bo.p, n, P.a, P.b, P.seed, P.thr, P.scale, _st())
    _sync()
    assert rc == 0 and bo.intact()
    _sd_compare(f"scale_dropout {n} {with_y} {p}", P, bo.cpu(), exact)


# ------------------------------------------------------------------ the column sum
def _lds(N):
    """(an even pitch > N, an odd pitch > N)"""
    return (N + 2 - N % 2, N + 1 + N % 2)


COLSUM = [(M, N) for M in (1, 7, 64, 65) for N in (1, 63, 64, 65, 5004)] + [(16385 + 3, N) for N in (1, 63, 64, 65)]


def _colsum_chain(M):
    rpb = max(64, -(-M // 256))
    chain = -(-rpb // 8) + 8 + -(-M // rpb) + 1
    assert chain <= M + -(-M // rpb) + 16   # never wider than rows + partial sums + a small constant
    return chain


def _colsum_plan(M, N, ld, exact):
    P = types.SimpleNamespace()
    g = _gen(M * 7919 + N + ld + int(exact))
    if exact:
        P.X, P.pre = _ints(g, (M, N), -2, 2).to(BF), _ints(g, (N,), -9, 9).float()
    else:
        P.X = (_scale16(M).view(M, 1) * _scale16(N, 1).view(1, N) * torch.randn(M, N, generator=g).double()).to(BF)
        P.pre = (_scale16(N, 1) * torch.randn(N, generator=g).double()).float()
    P.ref, P.mag = R.colsum(P.X, P.pre)
    P.chain = _colsum_chain(M)
    if exact:
        assert float(P.mag.max()) < 2.0 ** 24
    else:
        _sees_one_row(f"colsum {M} {N}", P.chain * E23 * P.mag, P.mag, M + 1)
    return P


def _colsum_compare(what, P, got, exact):
    if exact:
        _same_values(what, got, P.ref)
    else:
        _check(what, got, P.ref, P.chain * E23 * P.mag)


@gpu
@EXACT
@pytest.mark.parametrize("M,N", COLSUM)
def test_colsum(lib, M, N, exact):
    """colsum_kernel: one column, a ragged / whole / just started second column block, 79 blocks; the paired 4-byte loads (even pitch)
    and the element-wise path (odd pitch; the last column of an odd N); one row, less than the 8 row lanes, a whole row block and one
    row more; 16388 rows: 65 rows per block, 253 row blocks; onto a pre-filled output"""
    assert _colsum_chain(16388) == 9 + 8 + 253 + 1 and _colsum_chain(65) == 8 + 8 + 2 + 1
    for ld in _lds(N):
        P = _colsum_plan(M, N, ld, exact)
        if lib is None:
            continue
        bX, bo = PBuf(_pitched(M, N, ld), BF, P.X), out((N,), F32, P.pre)
        rc = lib.ea_colsum_bf16(bX.p, bo.p, M, N, ld, _st())
        _sync()
        assert rc == 0 and bo.intact()
        _colsum_compare(f"colsum {M} {N} ld {ld}", P, bo.cpu(), exact)


# ------------------------------------------------------------------ zero-rows
@gpu
@pytest.mark.parametrize("C", [1, 255, 256, 257])
def test_zero_rows(lib, C):
    """zero_rows_kernel: flagged rows become +0, every other row keeps its bits (NaN patterns included); the first and the last row
    flagged, and none"""
    M = 7
    x = _bf16_patterns(M * C, C).view(M, C)
    for flags in ([1, 0, 0, 1, 1, 0, 1], [0] * M):
        if lib is None:
            continue
        bx, z = out((M, C), BF, x), _dev_ints(flags, torch.uint8)
        assert lib.ea_zero_rows_bf16(bx.p, _dp(z), M, C, _st()) == 0
        _sync()
        assert bx.intact()
        want = x.view(I16).clone()
        want[torch.tensor(flags, dtype=torch.bool)] = 0
        assert torch.equal(bx.bits(), want), f"zero_rows {C} {flags}"


# ------------------------------------------------------------------ the embedding
TOKENS, POSITIONS, PAD, VOCAB, NPOS = [3, 1, 3, 0, 3], [2, 0, 5, 2, 6], 1, 6, 7
EMB = [(M, C) for M in (1, 4, 5) for C in (2, 126, 128, 130)]


def _emb_plan(M, C):
    P = types.SimpleNamespace()
    g = _gen(1000 * M + C)
    P.tok, P.position = torch.tensor(TOKENS[:M], dtype=I32), torch.tensor(POSITIONS[:M], dtype=I32)
    P.W = (_scale16(VOCAB).view(VOCAB, 1) * torch.randn(VOCAB, C, generator=g).double()).float()
    P.pos = (_scale16(NPOS, 1).view(NPOS, 1) * torch.randn(NPOS, C, generator=g).double()).float()
    P.scale = float(np.float32(math.sqrt(C)))
    P.dy = (_scale16(M, 2).view(M, 1) * torch.randn(M, C, generator=g).double()).to(BF)
    P.dW0 = (_scale16(VOCAB).view(VOCAB, 1) * torch.randn(VOCAB, C, generator=g).double()).float()
    P.dW, P.dW_mag, P.hits = R.embedding_bwd(P.tok, P.dy, P.dW0, P.scale, PAD)
    P.tol_dW = (P.hits.view(VOCAB, 1) + 2) * E23 * P.dW_mag
    _sees_one_row(f"embedding {M} {C}", P.tol_dW, P.dW_mag, 4)   # (at most three rows and the pre-fill meet in one row of dW)
    return P


@gpu
@pytest.mark.parametrize("M,C", EMB)
def test_embedding_forward(lib, M, C):
    """embedding_fwd_kernel: one column pair, 63 lanes, all 64, one lane's second pair; less than a block of four rows, a whole one,
    one more; with and without the positional table"""
    P = _emb_plan(M, C)
    if lib is None:
        return
    bW, bp, tok, position = inp(P.W), inp(P.pos), _dev_ints(P.tok), _dev_ints(P.position)
    for with_pos in (True, False):
        bo = out((M, C), BF)
        rc = lib.ea_embedding_fwd(_dp(tok), _dp(position) if with_pos else None, bW.p, bp.p if with_pos else None, bo.p, M, C, P.scale, _st())
        _sync()
        assert rc == 0 and bo.intact()
        ref, mag = R.embedding_fwd(P.tok, P.position, P.W, P.pos if with_pos else None, P.scale)
        _check_bf16(f"embedding {M} {C} pos {with_pos}", bo.cpu(), ref, 2 * E23 * mag)


@gpu
@pytest.mark.parametrize("M,C", EMB)
def test_embedding_backward(lib, M, C):
    """embedding_bwd_kernel: token 3 three times (the rows collide in the scatter), the pad token's row skipped, onto a pre-filled dW"""
    P = _emb_plan(M, C)
    if lib is None:
        return
    bdy, tok, bdW = inp(P.dy), _dev_ints(P.tok), out((VOCAB, C), F32, P.dW0)
    rc = lib.ea_embedding_bwd(_dp(tok), bdy.p, bdW.p, M, C, P.scale, PAD, _st())
    _sync()
    assert rc == 0 and bdW.intact()
    _check(f"embedding backward {M} {C}", bdW.cpu(), P.dW, P.tol_dW)
    idle = P.hits == 0
    assert torch.equal(bdW.bits()[idle], P.dW0.view(I32)[idle]), "a row no token names (or the pad row) was written"


@gpu
def test_embedding_return_codes(lib):
    bW, bo, tok = inp(torch.zeros(VOCAB, 8)), out((4, 8), BF), _dev_ints(TOKENS[:4])
    assert lib.ea_embedding_fwd(_dp(tok), None, bW.p, None, bo.p, 4, 7, 1.0, _st()) == -2   # odd C: the kernel stores pairs
    assert lib.ea_embedding_fwd(_dp(tok), None, bW.p, None, bo.p, 0, 8, 1.0, _st()) == 0
    assert lib.ea_embedding_bwd(_dp(tok), bo.p, bW.p, 0, 8, 1.0, PAD, _st()) == 0
    _sync()
    assert bo.untouched()


# ------------------------------------------------------------------ the batched transpose
SHAPES = [(1, 1), (63, 130), (64, 64), (0, 65), (65, 63), (130, 1), (1, 130), (65, 0)]   # an empty matrix in the middle, one at the end


@gpu
@pytest.mark.parametrize("n", [8, 3, 1])
def test_transpose_batch(lib, n):
    """transpose_batch_kernel: rows and columns of 1, 63, 64, 65, 130 (one to nine 64 x 64 tiles, ragged in either direction); an empty
    matrix takes no tile and shifts no other matrix's; n = 0 and n = 9"""
    mats = [_bf16_patterns(r * c, 13 * r + c).view(r, c) for r, c in SHAPES[:n]]
    if lib is None:
        return
    src = [inp(m) if m.numel() else inp(torch.zeros(8, dtype=BF)) for m in mats]
    dst = [out((c, r), BF) if r * c else out((8,), BF) for r, c in SHAPES[:n]]
    pad = [None] * (9 - n)
    ps = (ctypes.c_void_p * 9)(*([b.p.value for b in src] + pad))
    pd = (ctypes.c_void_p * 9)(*([b.p.value for b in dst] + pad))
    rows, cols = (ctypes.c_int * 9)(*([r for r, _ in SHAPES[:n]] + [0] * (9 - n))), (ctypes.c_int * 9)(*([c for _, c in SHAPES[:n]] + [0] * (9 - n)))
    assert lib.ea_transpose_bf16_batch(ps, pd, rows, cols, 0, _st()) == 0
    assert lib.ea_transpose_bf16_batch(ps, pd, rows, cols, 9, _st()) == -2
    _sync()
    assert all(b.untouched() for b in dst)
    assert lib.ea_transpose_bf16_batch(ps, pd, rows, cols, n, _st()) == 0
    _sync()
    for i, (m, b) in enumerate(zip(mats, dst)):
        if m.numel() == 0:
            assert b.untouched(), f"the empty matrix {i} was written"
            continue
        assert b.intact()
        assert torch.equal(b.bits(), R.transpose(m.view(I16))), f"matrix {i} of {n}: {SHAPES[i]}"


# ------------------------------------------------------------------ mutations of the reference (CPU, no GPU needed)
def _fails(fn):
    with pytest.raises(AssertionError):
        fn()


def test_bounds_see_the_faults_they_are_for():
    """A correct output must fall outside the bounds of a reference with one row left out of a column sum (the real-valued and the
    exact case, 16388 rows), the dropout mask drawn 8 elements off, one of three colliding rows dropped from the scatter, the pad row
    not skipped; a conversion that truncates, or rounds ties away from zero, is not the restated one"""
    for exact in (True, False):
        for M, N in ((16388, 65), (65, 5004), (7, 63)):
            P = _colsum_plan(M, N, N + 1, exact)
            good = P.ref.float()
            _colsum_compare("unperturbed", P, good, exact)
            Q = _colsum_plan(M, N, N + 1, exact)
            keep_rows = torch.arange(M) != M // 2
            Q.ref, Q.mag = R.colsum(Q.X[keep_rows], Q.pre)
            _fails(lambda: _colsum_compare("one row left out", Q, good, exact))
        for n in (2053, 8):
            P = _sd_plan(n, True, 0.5, exact)
            good = R.bf16_rne(P.ref).to(BF)
            _sd_compare("unperturbed", P, good, exact)
            Q = _sd_plan(n, True, 0.5, exact)
            Q.ref, Q.mag = R.scale_dropout(Q.x, Q.y, Q.a, Q.b, R.keep_flat(Q.seed, Q.p, n, shift=8))
            _fails(lambda: _sd_compare("mask 8 elements off", Q, good, exact))
    P = _emb_plan(5, 126)
    good = P.dW.float()
    _check("unperturbed", good, P.dW, P.tol_dW)
    tok = P.tok.clone()
    tok[2] = PAD   # (the second of the three rows that name token 3 goes nowhere)
    dW, mag, hits = R.embedding_bwd(tok, P.dy, P.dW0, P.scale, PAD)
    _fails(lambda: _check("a colliding row dropped", good, dW, (hits.view(VOCAB, 1) + 2) * E23 * mag))
    dW, mag, hits = R.embedding_bwd(P.tok, P.dy, P.dW0, P.scale, -1)
    _fails(lambda: _check("the pad row not skipped", good, dW, (hits.view(VOCAB, 1) + 2) * E23 * mag))
    src = _f32_patterns(4096, 1)
    b = src.view(I32).to(torch.int64) & 0xFFFFFFFF
    _same_cast("unperturbed", R.cast_f32_to_bf16_bits(src), src)
    _fails(lambda: _same_cast("truncation", (b >> 16).to(I32).to(I16), src))
    _fails(lambda: _same_cast("ties away from zero", ((b + 0x8000) >> 16).to(I32).to(I16), src))
    _fails(lambda: _same_cast("NaN to inf", torch.where(torch.isnan(src), torch.tensor(0x7F80), R.cast_f32_to_bf16_bits(src).to(torch.int64)).to(I16), src))


# ------------------------------------------------------------------ every GPU case on the CPU first
_GPU_TESTS = {
    "test_cast_f32_to_bf16": [(n,) for n in (1, 7, 8, 9, 2053)],
    "test_cast_bf16_to_f32": [(1,), (4096 * 256 + 5,)],
    "test_cast_f32_to_bf16_rows": ROWS_CASTS,
    "test_scale_dropout": [c + (e,) for c in SD_CASES for e in (True, False)],
    "test_colsum": [c + (e,) for c in COLSUM for e in (True, False)],
    "test_zero_rows": [(C,) for C in (1, 255, 256, 257)],
    "test_embedding_forward": EMB,
    "test_embedding_backward": EMB,
    "test_transpose_batch": [(8,), (3,), (1,)],
}


@pytest.mark.parametrize("name,args", [(n, a) for n in sorted(_GPU_TESTS) for a in _GPU_TESTS[n]], ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_every_case_on_the_cpu_first(name, args):
    """Every case of every GPU test, built without a GPU (lib = None: data, the fp64 reference, no launch): mag < 2^24 and a
    bf16-exact result for the exact cases, every sum's bound below one row's share for the real-valued ones"""
    globals()[name](None, *args)


def test_the_cpu_table_lists_every_gpu_test():
    mine = {k for k, f in globals().items() if k.startswith("test_") and callable(f) and any(m.name == "gpu" for m in getattr(f, "pytestmark", []))}
    assert mine - set(_GPU_TESTS) == {"test_cast_return_codes", "test_embedding_return_codes"} and set(_GPU_TESTS) <= mine
