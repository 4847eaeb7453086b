"""The training step's bookkeeping kernels (ea_subsample_lengths, ea_ctc_targets, ea_ctc_loss_clean, ea_stats_add4) bit for bit
against the torch expressions they replace, and the output projection's data gradient with a k-contiguous, zero-padded weight copy
(ea_ctc_grad at a pitch of 64, ea_transpose_pad_bf16, _Linear.backward) against fp64.

Bounds.  Everything integer-valued or copied is compared bit for bit.  The real-valued data gradient uses the bound
tests/test_gemm_kernels.py derives for a bf16 output with K additions along k (its module docstring): ulp(ref) + (K + 4) 2^-23 mag,
mag = sum_k |dy| |W|, K = the reduction length the launch is given (the padded pitch on the new path: its zero terms add nothing,
the bound only gets looser by the count the kernel really performs)."""
import ctypes

import pytest
import torch

from espresso_amd.criterions.ctc_loss import targets_and_lengths
from espresso_amd.modules.speech_convolutions import ConvBNReLU
from tests.test_convmodule_kernels import DEV, _st, _sync, lib  # noqa: F401 (lib: the fixture)
from tests.test_gemm_kernels import _compare

BF, F32 = torch.bfloat16, torch.float32


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _bits_equal(what, got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.is_floating_point():
        view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
        got, want = got.contiguous().view(view), want.contiguous().view(view)
    assert bool((got == want).all()), f"{what}: got {got.tolist()} want {want.tolist()}"


# ------------------------------------------------------------------ A: sub-sampler lengths and masks
def _torch_lengths_and_masks(src_lengths, total, Tp):
    """the expressions of ConvBNReLU.forward / output_lengths and of the encoder before this kernel existed"""
    x_len = torch.div(src_lengths + (total - 1), total, rounding_mode="floor")
    mask = torch.arange(Tp, device=src_lengths.device).unsqueeze(0) >= x_len.unsqueeze(1)
    return x_len, x_len.to(torch.int32).contiguous(), mask, mask.reshape(-1).to(torch.uint8).contiguous()


@pytest.mark.gpu
def test_subsample_lengths_kernel(lib):
    from espresso_amd import kernels as K

    B, Tp, total = 3, 5, 4
    src = torch.tensor([0, 3, 20], dtype=torch.int64)  # -> 0, 1 and exactly T' = 5 output frames
    want = _torch_lengths_and_masks(src, total, Tp)
    assert want[0].tolist() == [0, 1, Tp]
    got = K.subsample_lengths(src.to(DEV), total, Tp)
    _sync()
    for name, g, w in zip(("x_lengths", "key_len", "padding_mask", "row_zero"), got, want):
        _bits_equal(name, g, w)
    # the same through the module (strides 2 x 2 in time), other lengths: every remainder of the division
    m = ConvBNReLU([4, 4], [3, 3], [2, 2])
    src = torch.tensor([17, 18, 19, 20, 1], dtype=torch.int64)
    want = _torch_lengths_and_masks(src, 4, 5)
    got = m.lengths_and_masks(src.to(DEV), 5)
    _sync()
    _bits_equal("module lengths", got[0], m.output_lengths(src))
    for name, g, w in zip(("x_lengths", "key_len", "padding_mask", "row_zero"), got, want):
        _bits_equal(name, g, w)


# ------------------------------------------------------------------ B: criterion bookkeeping
PAD, EOS = 1, 2


def _target_rows():
    return torch.tensor([[PAD] * 6,                      # all pad
                         [EOS, PAD, PAD, PAD, PAD, PAD],  # eos then pad
                         [5, 6, 7, 8, 9, 10],             # full, no pad
                         [11, PAD, PAD, PAD, PAD, PAD]],  # a single label
                        dtype=torch.int64)


def _parent_targets(target):
    """the criterion's expressions before the kernel existed"""
    pad_mask = (target != PAD) & (target != EOS)
    return target.to(torch.int32).contiguous(), pad_mask.sum(-1).to(torch.int32).contiguous(), pad_mask.sum(-1)


@pytest.mark.gpu
def test_ctc_targets_kernel(lib):
    target = _target_rows()
    t32, n32, n64 = _parent_targets(target)
    assert n64.tolist() == [0, 0, 6, 1]
    got_t, got_n = targets_and_lengths(target.to(DEV), PAD, EOS)
    _sync()
    _bits_equal("targets", got_t, t32)
    _bits_equal("target lengths", got_n, n32)
    assert got_n.cpu().to(torch.int64).tolist() == n64.tolist()  # exactly what pad_mask.sum(-1) gives


def _ctc_problem(B, T, V, targets, tgt_len, in_len, seed):
    from espresso_amd import kernels as K

    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B * T, V, generator=g).to(DEV)
    lprobs = K.log_softmax(logits, B * T, V, V)
    return lprobs, targets.to(torch.int32).to(DEV), torch.tensor(in_len, dtype=torch.int32, device=DEV), \
        torch.tensor(tgt_len, dtype=torch.int32, device=DEV)


@pytest.mark.gpu
def test_ctc_loss_clean_output(lib):
    B, T, V, Lmax, blank = 2, 4, 7, 5, 0
    targets = torch.tensor([[3, 4, 0, 0, 0], [1, 2, 3, 4, 5]])
    lprobs, tg, il, tl = _ctc_problem(B, T, V, targets, [2, 5], [4, 4], seed=3)  # utterance 1: 5 labels in 4 frames, infeasible
    nbytes = int(lib.ea_ctc_workspace_bytes(B, T, Lmax))
    ws0, ws1 = (torch.zeros(nbytes, dtype=torch.uint8, device=DEV) for _ in range(2))
    nan = float("nan")
    raw0, raw1, clean = (torch.full((B,), nan, device=DEV) for _ in range(3))
    assert lib.ea_ctc_loss(_p(lprobs), _p(tg), _p(il), _p(tl), _p(raw0), _p(ws0), B, T, V, Lmax, blank, _st()) == 0
    assert lib.ea_ctc_loss_clean(_p(lprobs), _p(tg), _p(il), _p(tl), _p(raw1), _p(clean), _p(ws1), B, T, V, Lmax, blank, _st()) == 0
    _sync()
    r0, r1, c = raw0.cpu(), raw1.cpu(), clean.cpu()
    print("raw", r0.tolist(), "clean", c.tolist())
    assert bool(torch.isfinite(r0[0])) and float(r0[0]) > 0 and float(r0[1]) == float("inf")
    _bits_equal("raw output, with and without the second output", r1, r0)
    _bits_equal("clean output", c, torch.where(torch.isinf(r0), torch.zeros_like(r0), r0))
    assert float(c[1]) == 0.0
    _bits_equal("clean output of the feasible utterance", c[:1], r0[:1])
    _bits_equal("lattice workspace", ws1, ws0)


# ------------------------------------------------------------------ C: the trainer's statistics
@pytest.mark.gpu
def test_stats_add4_kernel(lib):
    from espresso_amd import kernels as K

    calls = [(24.0, 1234.5678, 1093.0, 24.0), (17.0, 0.333333, 700.0, 17.0)]
    want = torch.zeros(6, dtype=F32)
    got = torch.zeros(6, dtype=F32, device=DEV)
    for a0, loss, a2, a3 in calls:
        lt = torch.tensor([loss], dtype=F32)
        want[0:1].add_(float(a0))
        want[1:2].add_(lt.reshape(1))
        want[2:3].add_(float(a2))
        want[3:4].add_(float(a3))
        K.stats_add4(got, a0, lt.to(DEV), a2, a3)
    _sync()
    _bits_equal("statistics after two calls", got, want)  # (slots 4.. untouched)


# ------------------------------------------------------------------ E: loss gradient at a pitch of 64, k-contiguous data gradient
@pytest.mark.gpu
def test_ctc_grad_zero_pad_columns(lib):
    B, T, V, Lmax, blank = 2, 4, 37, 3, 0
    targets = torch.tensor([[5, 36, 5], [7, 0, 0]])
    lprobs, tg, il, tl = _ctc_problem(B, T, V, targets, [3, 1], [4, 3], seed=5)
    ws = torch.empty(int(lib.ea_ctc_workspace_bytes(B, T, Lmax)), dtype=torch.uint8, device=DEV)
    nll = torch.empty(B, device=DEV)
    assert lib.ea_ctc_loss(_p(lprobs), _p(tg), _p(il), _p(tl), _p(nll), _p(ws), B, T, V, Lmax, blank, _st()) == 0
    outs = {}
    for ld in (40, 64):  # 40: the pitch before (a multiple of 8), 64: the pitch the data gradient reduces over
        dl = torch.full((B * T, ld), float("nan"), dtype=BF, device=DEV)
        assert lib.ea_ctc_grad(_p(lprobs), _p(ws), _p(nll), _p(tg), _p(il), _p(tl), _p(dl), ld, 1, B, T, V, Lmax, blank, 1.0, None, 1,
                               _st()) == 0
        outs[ld] = dl
    _sync()
    new, old = outs[64].cpu(), outs[40].cpu()
    assert bool(torch.isfinite(old[:, :V].float()).all()) and float(old[:, :V].float().abs().max()) > 0
    _bits_equal("columns 0..36", new[:, :V], old[:, :V])
    assert bool((new[:, V:].contiguous().view(torch.int16) == 0).all()), "columns 37..63 must be +0 in every row"


def _dgrad_operands(M, V, Kin, ld, exact, seed):
    g = torch.Generator().manual_seed(seed)
    if exact:
        dy = torch.randint(-1, 2, (M, V), generator=g).double()
        W = torch.randint(-1, 2, (V, Kin), generator=g).double()
    else:
        dy = (torch.randn(M, V, generator=g) * torch.tensor([16.0 ** (m % 3 - 1) for m in range(M)]).unsqueeze(1)).to(BF).double()
        W = (torch.randn(V, Kin, generator=g) * torch.tensor([16.0 ** (k % 3 - 1) for k in range(Kin)]).unsqueeze(0)).to(BF).double()
    dyp = torch.zeros(M, ld, dtype=BF)
    dyp[:, :V] = dy.to(BF)
    return dy, W, dyp.to(DEV), W.to(BF).contiguous().to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("M,V,Kin", [(130, 100, 64), (257, 200, 128)])
def test_output_projection_dgrad(lib, M, V, Kin, exact, monkeypatch):
    from espresso_amd import functional as F
    from espresso_amd import kernels as K

    ld = F._pad_dgrad(V)
    assert ld == {100: 128, 200: 256}[V]
    dy, W, dyp, w16 = _dgrad_operands(M, V, Kin, ld, exact, seed=M + V)
    ref = dy @ W
    mag = dy.abs() @ W.abs()
    wt = torch.full((Kin, ld), float("nan"), dtype=BF, device=DEV)
    K.transpose_pad(w16, wt, V, Kin, ld)
    _sync()
    _bits_equal("k-contiguous copy", wt.cpu()[:, :V], w16.cpu().t().contiguous())
    assert bool((wt.cpu()[:, V:].contiguous().view(torch.int16) == 0).all()), "pad columns of the copy must be +0"
    dx_new = torch.full((M, Kin), float("nan"), dtype=BF, device=DEV)
    dx_old = torch.full((M, Kin), float("nan"), dtype=BF, device=DEV)
    K.gemm(dyp, wt, dx_new, M, Kin, ld, lda=ld, ldb=ld, ldc=Kin)
    K.gemm(dyp, w16, dx_old, M, Kin, V, lda=ld, ldb=Kin, ldc=Kin, b_kstrided=True)
    _sync()
    _compare("k-contiguous path", dx_new, ref, mag, exact, chain=ld + 4)
    _compare("k-strided path", dx_old, ref, mag, exact, chain=V + 4)

    # the same through _Linear.backward: a tagged gradient and a current copy select the k-contiguous launch, anything else the
    # k-strided one, and both give the data gradient above
    seen = []
    real_gemm = K.gemm

    def recording_gemm(*a, **kw):
        seen.append(bool(kw.get("b_kstrided", False)) or bool(kw.get("a_kstrided", False)))
        return real_gemm(*a, **kw)

    monkeypatch.setattr(K, "gemm", recording_gemm)
    for tagged in (True, False):
        x = torch.zeros(M, Kin, dtype=BF, device=DEV, requires_grad=True)
        w = torch.zeros(V, Kin, device=DEV)  # (no gradient wanted: only the data gradient runs)
        y = F._Linear.apply(x, w, None, w16, False, wt, None)
        gbuf = dyp.clone()
        gview = gbuf[:, :V]
        if tagged:
            gview._ea_zero_pad = ld
        seen.clear()
        y.backward(gview)
        _sync()
        assert seen == [True, not tagged], (tagged, seen)  # (weight gradient first: k-strided operands; then the data gradient)
        _compare(f"_Linear.backward tagged={tagged}", x.grad, ref, mag, exact, chain=(ld if tagged else V) + 4)


# ------------------------------------------------------------------ D: fc0's input-axis permutation
@pytest.mark.gpu
def test_fc0_permutation_kernels(lib):
    from espresso_amd import kernels as K

    N, C, Fp = 70, 24, 5  # (more than one 64 x 64 tile either way, ragged in both)
    g = torch.Generator().manual_seed(9)
    w = torch.randn(N, C * Fp, generator=g).to(BF)
    want = w.view(N, C, Fp).permute(0, 2, 1).reshape(N, Fp * C)
    got = K.permute_k(w.to(DEV), C, Fp)
    got2, got_t = K.permute_k(w.to(DEV), C, Fp, transposed=True)
    dW = torch.randn(N, Fp * C, generator=g)
    acc0 = torch.randn(N, C * Fp, generator=g)
    acc = acc0.clone().to(DEV)
    K.unpermute_k_add(dW.to(DEV), acc, N, C, Fp)
    _sync()
    _bits_equal("permuted weight", got, want)
    _bits_equal("permuted weight (with the transposed copy)", got2, want)
    _bits_equal("transposed permuted weight", got_t, want.t().contiguous())
    _bits_equal("un-permuted gradient", acc, acc0 + dW.view(N, Fp, C).permute(0, 2, 1).reshape(N, C * Fp))


@pytest.mark.gpu
def test_linear_with_permuted_input_axis(lib, monkeypatch):
    """F.linear(x, w, k_perm=(C, F)) against the permuted-view formulation it replaces, on exact operands: output, data gradient
    (k-contiguous launch: N is a multiple of 64, no pad needed) and the weight gradient in the weight's own order."""
    from espresso_amd import functional as F
    from espresso_amd import kernels as K

    M, N, C, Fp = 130, 64, 8, 4
    Kin = C * Fp
    g = torch.Generator().manual_seed(21)
    w = torch.randint(-1, 2, (N, Kin), generator=g).double()
    x = torch.randint(-1, 2, (M, Kin), generator=g).double()   # (f*C + c) order
    dy = torch.randint(-1, 2, (M, N), generator=g).double()
    wp = w.view(N, C, Fp).permute(0, 2, 1).reshape(N, Kin)
    seen = []
    real_gemm = K.gemm
    monkeypatch.setattr(K, "gemm", lambda *a, **kw: (seen.append((bool(kw.get("a_kstrided")), bool(kw.get("b_kstrided")))), real_gemm(*a, **kw))[1])
    wd = w.float().to(DEV).requires_grad_(True)
    xd = x.to(BF).to(DEV).requires_grad_(True)
    y = F.linear(xd, wd, None, k_perm=(C, Fp))
    y.backward(dy.to(BF).to(DEV))
    _sync()
    assert seen == [(False, False), (True, True), (False, False)], seen  # forward, weight gradient, k-contiguous data gradient
    _bits_equal("y", y.detach(), (x @ wp.t()).to(BF))
    _bits_equal("dx", xd.grad, (dy @ wp).to(BF))
    _bits_equal("dW", wd.grad, (dy.t() @ x).view(N, Fp, C).permute(0, 2, 1).reshape(N, Kin).float())


# ------------------------------------------------------------------ CPU: the Python fallbacks
def test_python_fallbacks_on_cpu_tensors():
    m = ConvBNReLU([4, 4], [3, 3], [2, 2])
    m.eval()
    src_lengths = torch.tensor([0, 3, 20, 17], dtype=torch.int64)
    Tp = 5
    want = _torch_lengths_and_masks(src_lengths, 4, Tp)
    _bits_equal("output_lengths", m.output_lengths(src_lengths), want[0])
    x_len, key_len, mask, row_zero = m.lengths_and_masks(src_lengths, Tp)
    assert key_len is None  # (the encoder casts the lengths itself, as before)
    _bits_equal("x_lengths", x_len, want[0])
    _bits_equal("padding_mask", mask, want[2])
    _bits_equal("row_zero", row_zero, want[3])
    target = _target_rows()
    t32, n32, _ = _parent_targets(target)
    got_t, got_n = targets_and_lengths(target, PAD, EOS)
    _bits_equal("targets", got_t, t32)
    _bits_equal("target lengths", got_n, n32)
