"""ea_gemm_bf16 and ea_wgrad_group (espresso_amd/csrc/gemm.hip, gemm_w8.hip, wgrad_w8.hip, gemm_epilogue.h) one launch at a time
against the plain fp64 restatement in tests/gemm_ref.py, through the C ABI, every element of every output.

BUFFERS.  Every device operand is a view into a larger allocation (PBuf, a pitched variant of tests/test_convmodule_kernels.py's
Buf): a guard before and after it, and — because most tensors here have a row pitch larger than their width and batch items that
do not touch — pitch padding and gaps inside it.  All of that holds NaN around inputs (the columns K .. lda-1 of an operand, the
columns N .. ld_dy-1 / K .. ld_x-1 of the weight gradient's operands: whatever a kernel lets through to a stored element fails) and
a sentinel bit pattern around outputs (the columns N .. ld-1 of every row, the gaps, the guards: checked after the call).  An
output itself starts as NaN (a missed store is a failure), or as known data where the call accumulates onto it; the split-K
workspace starts as NaN.  No element is excluded from any comparison.
ONE EXCEPTION, the header's contract for a padded output pitch (include/espresso_amd.h:65-68): on the 8-wave ragged-N path
(N % 4 == 0, ldc >= roundup32(N), plain / bias / activation / dropout only) the library may overwrite the columns N .. ldc-1.
test_w8_ragged_n asserts the guards, the rows' pad beyond roundup32(N) and every column < N, and nothing about N .. roundup32(N)-1.

SCALES.  In the real-valued cases row m of A and row n of B are drawn at 16^(i % 3 - 1): neighbouring output rows and columns
differ by 16 or 256, a value that lands one row or one 8-column chunk off cannot pass.

PATHS.  The tuning hooks are process-global: `hooks` pins all seven for every launch and restores them in `finally`.  The library's
profile record (ea_gemm_profile_dump: bm64 = 0 / 1 for the 4-wave kernels' tile height, 100 + cfg for the 8-wave kernels, 108 for
the 8-wave weight gradient; the effective split-K count) is asserted for every launch.  Where the record does not tell two kernels
apart (register-staged / direct-to-LDS ring, FAST / general epilogue, register-staged / transposing weight gradient) the host's
eligibility rules are restated from gemm.hip (glds_eligible, fast_epilogue_ok, w8_ragged_ok, aligned_for) and asserted to select
the path the case is named after.

EXACT cases.  Operands are sparse integers in {-1, 0, 1}; bias, residual, pre-fill and pos_u / pos_v small integers or
half-integers; alpha, out_scale, qscale in {0.125, 0.5, 1, 2}; activation none or ReLU; dropout p = 0.5 (threshold 2^31, keep-scale
exactly 2).  `mag < 2^24` is asserted first; every fp32 partial sum is then an exact integer in any order and at any split, and
every later step an exact dyadic fraction: an fp32 output must equal the fp64 value, a bf16 output its round-to-nearest-even, the
query outputs the twice-rounded value, the keep pattern the oracle's — all bit for bit.

REAL-VALUED cases.  Bounds derived from the arithmetic, none measured (ulp(x) = the bf16 step at |x|; mag = the reference's
expression over the magnitudes of its terms; all references are fp64 on the same bf16 operands):
  bf16 output            ulp(ref) + (K + 4) 2^-23 mag           K fp32 additions along k (the MFMA's accumulation, at most one
                                                                rounding per product added), then alpha, bias, activation, keep,
                                                                out_scale, residual: <= 6 roundings of 2^-24 each = 3 2^-23 <= 4
  fp32 output            (K + 4 + splitk) 2^-23 mag             as above; the reduce pass adds `splitk` slabs (the effective number
                                                                of chunks) and the pre-fill, whose magnitude is part of mag
  query outputs          ulp(ref) + 2^-22 |ref|, ref taken at the bf16 roundings of q - e and q + e, e = (K + 4) 2^-23 mag: the kernel's
                         fp32 q may sit on the other side of a rounding tie than the fp64 q, nowhere else; (q + pos) * qscale rounds twice
  weight gradient dW     (M + 1) 2^-23 mag                      M additions along the reduction, one onto the pre-fill (in mag)
  bias gradient db       (chain + 1) 2^-23 mag                  chain read from the kernels: register-staged kernel — a thread adds
                         the 4 reduction rows of its staging block per k-tile, 4 ceil(M / 64) additions, then one thread folds the 16
                         partial sums (wgrad_group_kernel, `bsum`, `s += sC[q * BM_ + tid]`): chain = 4 ceil(M / 64) + 16; transposing
                         and 8-wave kernels — one more MFMA against a fragment of ones, the same chain as dW: chain = M
  SiLU (v_exp_f32, v_rcp_f32 — common.h:128-132, both specified to 1 ulp = 2^-23 relative).  s = rcp(1 + exp(-x)): __expf(-x) is
    v_exp_f32(-x log2 e); the argument's two roundings (the constant, the product) are 2^-23 of it together and move the result by
    |x| log2(e) ln(2) 2^-23 = |x| 2^-23 relative, the instruction adds 2^-23; through 1 / (1 + e) an error of e is damped by
    e / (1 + e) = 1 - s; the addition rounds by 2^-24, v_rcp_f32 adds 2^-23:  eps_s = (1 + |x|)(1 - s) 2^-23 + 1.5 2^-23.
    silu = x * s, one more rounding:  extra = ((1 + |x|)(1 - s) 2^-23 + 2^-22) |silu(x)|  (times keep and out_scale).
  SiLU' = s (1 + x (1 - s)).  With t = s (1 + |x| (1 - s)), the magnitude of the derivative's own terms (they cancel near
    x = -1.28):  extra = (eps_s t + s |x| (s eps_s + 2^-24) + 3 2^-24 t) |v keep|  — s's error through the outer factor; 1 - s
    inherits s's absolute error s eps_s and rounds once; x (1 - s), 1 + ..., s (...) round once each.
  Both extras are asserted to stay below 1/8 of a bf16 step of the reference in every case, the zero crossing of SiLU' included: the
    auxiliary operand is a bf16 value, the nearest to the crossing is -1.28125, where the extra is still below that limit.
Every fp32 sum's own bound is also asserted to be below one average term's contribution (_sees_one_row with K, or M for the weight
gradient): one dropped or duplicated k index shows.

The first tests need no GPU: they prove the reference against torch.bmm, F.silu, F.relu and autograd in float64; show that
dropping the last k-step, shifting one 8-column chunk by a row, skipping the bias in the tail columns or omitting one split-K
chunk each put a correct output outside these bounds; and build every case of every GPU test on the CPU (data, memory images,
fp64 reference, no launch), asserting mag < 2^24 for the exact ones, and for the real-valued ones that every sum's bound stays below
one term's share and the SiLU terms below 1/8 of a step."""
import contextlib
import ctypes
import os
import tempfile
import types
import zlib

import pytest
import torch
import torch.nn.functional as TF

from tests import gemm_ref as R
from tests.test_convmodule_kernels import _INT, _SENTINEL, DEV, Buf, _check, _check_bf16, _gen, _sees_one_row, _st, _sync, _ulp, inp, lib, out  # noqa: F401 (lib: the fixture)
from tests.test_subsample_kernels import _bf_exact, _ints, _same_values

gpu = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
E23, E24 = 2.0 ** -23, 2.0 ** -24
NAN = float("nan")
GUARD_EL = 4096      # guard elements on either side of a PBuf (a multiple of 8: a 16-byte aligned base stays aligned)
BK = 64
EXACT = pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])


# ------------------------------------------------------------------ the reference against torch's operators (CPU, no GPU needed)
def _close(a, b):
    return a.shape == b.shape and float((a - b).abs().max()) <= 1e-11 * max(float(b.abs().max()), 1e-300)


def _store(mat, ld, transposed):
    """[Z][rows][cols] -> flat memory of Z slabs, row pitch ld (transposed: the slab holds cols x rows), pads NaN; -> (flat, slab size)"""
    m = mat.transpose(1, 2) if transposed else mat
    Z, r, c = m.shape
    s = torch.full((Z, r, ld), NAN, dtype=mat.dtype)
    s[:, :, :c] = m
    return s.reshape(-1), r * ld


def test_reference_matches_torch_in_float64():
    """tests/gemm_ref.py == torch.bmm / F.relu / F.silu / autograd in float64, within 1e-11 of every tensor's scale: the four operand
    layouts with padded pitches, a batch of 6 with zdiv = 3 (distinct s_hi / s_lo, and one B shared by the inner index), alpha, bias,
    the three epilogue branches, out_scale, residual, accumulate, the query split, the dropout index, the Linear weight / bias
    gradients; `mag` equals the function applied to absolute values"""
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    M, N, K, batch, zdiv = 5, 7, 9, 6, 3
    A, Bh, bias = rnd(batch, M, K), rnd(batch // zdiv, N, K), rnd(N)
    Bfull = Bh.repeat_interleave(zdiv, 0)
    resid, pre, aux = rnd(batch, M, N), rnd(batch, M, N), rnd(batch, M, N)
    kp = R.keep(1234, 0.3, batch, M, N)
    flat_keep = torch.from_numpy(R.dropout_ref.keep_mask(1234, batch * M * N, 0.3)).view(batch, M, N)
    assert torch.equal(kp != 0, flat_keep) and 0 < int(flat_keep.sum()) < flat_keep.numel()
    assert R.drop_params(0.3)[0] == int(0.3 * 2 ** 32) and abs(R.drop_params(0.3)[1] - 1.0 / 0.7) < 1e-7
    assert torch.equal(kp[kp != 0], torch.full_like(kp[kp != 0], R.drop_params(0.3)[1]))
    acc = torch.bmm(A, Bfull.transpose(1, 2))
    for a_ks in (False, True):
        for b_ks in (False, True):
            lda, ldb = (M if a_ks else K) + 3, (N if b_ks else K) + 2
            fa, sa = _store(A, lda, a_ks)
            fb, sb = _store(Bh, ldb, b_ks)
            # A: item z at (z / 3) * 3 slabs + (z % 3) slabs; B: one slab per outer index, s_lo = 0
            kw = dict(batch=batch, zdiv=zdiv, a_kstrided=a_ks, b_kstrided=b_ks, lda=lda, ldb=ldb, sA=(zdiv * sa, sa), sB=(sb, 0))
            run = lambda **k: R.gemm(fa, fb, M, N, K, **kw, **k)
            absrun = lambda **k: R.gemm(fa.abs(), fb.abs(), M, N, K, **kw, **k)
            tag = (a_ks, b_ks)
            r = run()
            assert _close(r["C"], acc) and _close(r["C_mag"], absrun()["C"]), tag
            v = -0.25 * acc + bias
            for kind, fn in ((R.ACT_NONE, lambda t: t), (R.ACT_RELU, TF.relu), (R.ACT_SILU, TF.silu)):
                r = run(alpha=-0.25, bias=bias, activation=kind, keep_scale=kp, out_scale=0.5, resid=resid, prefill=pre)
                assert _close(r["C"], pre + (0.5 * kp * fn(v) + resid)), (tag, kind)
                ra = absrun(alpha=0.25, bias=bias.abs(), keep_scale=kp, out_scale=0.5, resid=resid.abs(), prefill=pre.abs())
                assert _close(r["C_mag"], pre.abs() + (R.act_lip(kind) * (ra["C"] - pre.abs() - resid.abs()) + resid.abs())), (tag, kind)
                if kind != R.ACT_SILU:  # relu(|x|) = |x|: literally the same function of the absolute values
                    assert _close(r["C_mag"], absrun(alpha=0.25, bias=bias.abs(), activation=kind, keep_scale=kp, out_scale=0.5,
                                                     resid=resid.abs(), prefill=pre.abs())["C"]), (tag, kind)
                r2 = run(alpha=-0.25, bias=bias, activation=kind, keep_scale=kp, two_outputs=True)
                assert _close(r2["C"], v) and _close(r2["C2"], kp * fn(v)), (tag, kind)
                assert _close(r2["C2_mag"], R.act_lip(kind) * kp * r2["C_mag"]), (tag, kind)
                z = aux.clone().requires_grad_()
                (dz,) = torch.autograd.grad(fn(z) if kind else z * 1.0, z, v * kp)  # backward through the activation
                r3 = run(alpha=-0.25, bias=bias, activation=kind, keep_scale=kp, aux=aux, out_scale=2.0, resid=resid)
                assert _close(r3["C"], 2.0 * dz + resid), (tag, kind)
                d = R.dact(aux, kind)
                assert _close(r3["C_mag"], 2.0 * (0.25 * absrun()["C"] + bias.abs()) * kp * d.abs() + resid.abs()), (tag, kind)
    # the query split: q rounded as torch rounds an fp32 value to bf16, then biased and scaled
    fa, _ = _store(A[:1], K, False)
    fb, _ = _store(Bh[:1], K, False)
    pos_u, pos_v = rnd(4), rnd(4)
    r = R.gemm(fa, fb, M, N, K, bias=bias, qsplit=(4, pos_u, pos_v, 0.125))
    v = (acc[:1] + bias)[..., :4]
    assert _close(r["q_pre"], v) and _close(r["C"], acc[:1] + bias)
    q = v.float().to(BF).double()
    assert torch.equal(R.bf16_rne(v.float().double()), q)
    assert torch.equal(R.query(v.float().double(), pos_u, 0.125), (q + pos_u) * 0.125)
    assert torch.equal(R.query(v.float().double(), None, 2.0), q * 2.0)
    ties = torch.tensor([1.00390625, 1.01171875, -3.0234375, 0.0, 2.0 ** -40 * 1.01171875], dtype=F64)  # halfway cases: to even
    assert torch.equal(R.bf16_rne(ties), ties.float().to(BF).double())
    # the Linear weight / bias gradients
    x, dy, W, b = rnd(11, K), rnd(11, N), rnd(N, K).requires_grad_(), rnd(N).requires_grad_()
    (TF.linear(x, W, b) * dy).sum().backward()
    dW0, db0 = rnd(N, K), rnd(N)
    dW, db, wmag, bmag = R.wgrad(dy, x, dW0, db0)
    assert _close(dW, dW0 + W.grad) and _close(db, db0 + b.grad)
    dWa, dba, _, _ = R.wgrad(dy.abs(), x.abs(), dW0.abs(), db0.abs())
    assert _close(wmag, dWa) and _close(bmag, dba)


# ------------------------------------------------------------------ bounds
def _silu_extra(x):
    """absolute error bound of silu_f(x) for an exact fp32 x (module docstring)"""
    s = 1.0 / (1.0 + torch.exp(-x))
    return ((1.0 + x.abs()) * (1.0 - s) * E23 + 2.0 ** -22) * (x * s).abs()


def _dsilu_terms(x):
    """(t, absolute error bound of dsilu_f(x)): t = s (1 + |x| (1 - s)), the magnitude of the derivative's own terms"""
    s = 1.0 / (1.0 + torch.exp(-x))
    eps = (1.0 + x.abs()) * (1.0 - s) * E23 + 1.5 * E23
    t = s * (1.0 + x.abs() * (1.0 - s))
    return t, eps * t + s * x.abs() * (s * eps + E24) + 3 * E24 * t


def _eighth_of_a_step(what, extra, of):
    assert bool((extra <= _ulp(of) / 8).all()), f"{what}: the transcendental term has grown past 1/8 of a bf16 step"


def _rounded(ref, dtype):
    """a correct output: the reference rounded as the kernel stores it"""
    return R.bf16_rne(ref).to(BF) if dtype == BF else ref.float()


def _compare(what, got, ref, mag, exact, chain, extra=None, rows=None):
    """one output against its reference.  exact: bit for bit.  real: ulp(ref) (bf16 outputs) + chain 2^-23 mag + extra"""
    if exact:
        assert float(mag.max()) < 2.0 ** 24, what
        _same_values(what, got, _bf_exact(ref) if got.dtype == BF else ref)
        return
    tol = chain * E23 * mag
    if rows:
        _sees_one_row(what, tol, mag, rows)
    if extra is not None:
        tol = tol + extra
    if got.dtype == BF:
        _check_bf16(what, got, ref, tol)
    else:
        _check(what, got, ref, tol)


# ------------------------------------------------------------------ mutations of the reference (CPU, no GPU needed)
@EXACT
@pytest.mark.parametrize("c_f32", [False, True], ids=["bf16", "f32"])
def test_bounds_see_the_faults_they_are_for(c_f32, exact):
    """A correct output (the unperturbed reference rounded as the kernel would) must fall outside the bound of a reference that
    drops the last k-step, shifts one 8-column chunk by one row, skips the bias in the tail columns, or omits one split-K chunk"""
    M, N, K, splitk = 130, 136, 200, 3
    g = _gen(99)
    if exact:
        A, B, bias = _ints(g, (M, K), -1, 1, 0.5).to(BF), _ints(g, (N, K), -1, 1, 0.25).to(BF), _ints(g, (N,), -6, 6) / 2
    else:
        A, B, bias = _real_operand(g, 1, M, K, 1.0), _real_operand(g, 1, N, K, K ** -0.5), torch.randn(N, generator=g).double() * _scale(N)
        A, B = A[0], B[0]
    chain = K + 4 + (splitk if c_f32 else 0)
    dtype = F32 if c_f32 else BF
    good = R.gemm(A, B, M, N, K, bias=bias)
    correct = _rounded(good["C"], dtype)[0]
    _compare("unperturbed", correct, good["C"][0], good["C_mag"][0], exact, chain, rows=K)  # the check passes what is right

    def fails(what, ref, mag):
        with pytest.raises(AssertionError):
            _compare(what, correct, ref, mag, exact, chain)

    r = R.gemm(A, B, M, N, (K - 1) // BK * BK, lda=K, ldb=K, bias=bias)
    fails("last k-step dropped", r["C"][0], r["C_mag"][0])
    ref, mag = good["C"][0].clone(), good["C_mag"][0].clone()
    ref[64:M, 40:48], mag[64:M, 40:48] = good["C"][0][63:M - 1, 40:48], good["C_mag"][0][63:M - 1, 40:48]
    fails("one 8-column chunk one row off", ref, mag)
    tail = bias.clone()
    tail[N // 8 * 8 - 8:] = 0   # (N = 136: the last whole chunk of the ragged 128-column tile)
    r = R.gemm(A, B, M, N, K, bias=tail)
    fails("bias skipped in the tail columns", r["C"][0], r["C_mag"][0])
    chunk = (K + splitk - 1) // splitk
    chunk = (chunk + BK - 1) // BK * BK
    A2 = A.clone()
    A2[:, chunk:2 * chunk] = 0
    r = R.gemm(A2, B, M, N, K, bias=bias)
    fails("one split-K chunk omitted", r["C"][0], r["C_mag"][0])


_LAYOUT_LIST = [(False, False), (False, True), (True, False), (True, True)]
_KIND_LIST = ["plain", "bias_relu", "qsplit", "qsplit_no_v", "qsplit_no_pos_u", "act2", "aux", "resid"]
# every parametrisation (without `exact`) of the GPU tests below that build their cases through run_case / run_wgrad
_GPU_TESTS = {
    "test_register_staged_kernel": [(a, b, v) for (a, b) in _LAYOUT_LIST for v in (1, 2)],
    "test_batched_with_zdiv": [(a, b, v) for (a, b) in _LAYOUT_LIST for v in (1, 2)],
    "test_xcd_remap": [(b, M, s) for (b, M) in ((16, 256), (13, 320)) for s in (0, 3)],
    "test_general_epilogue": [(M, N, K, pads) for (M, N, K) in ((200, 136, 72), (130, 36, 64)) for pads in ("scalar", "vector")],
    "test_fast_epilogue": [(k, v) for k in _KIND_LIST for v in (1, 2)],
    "test_fast_epilogue_non_temporal_stores": [(k,) for k in ("plain", "qsplit", "act2", "resid")],
    "test_direct_to_lds_ring": [(st, v) for st in (2, 3, 4) for v in (1, 2)],
    "test_direct_to_lds_ring_batched_and_automatic": [(1,), (2,)],
    "test_w8_tiles": [(cfg, k) for cfg in (2, 3, 4, 5) for k in _KIND_LIST],
    "test_w8_ragged_n": [(2,), (3,), (4,), (5,)],
    "test_split_k": [(False,), (True,)],
    "test_wgrad_register_staged_kernel": [(1,), (2,)],
    "test_wgrad_transposing_kernel": [(1,), (2,)],
    "test_wgrad_transposing_kernel_falls_back_to_64_rows": [()],
    "test_wgrad_w8_kernel": [()],
    "test_wgrad_group_of_sixteen": [("reg",), ("tr",), ("w8",)],
}


@EXACT
@pytest.mark.parametrize("name,args", [(n, a) for n in sorted(_GPU_TESTS) for a in _GPU_TESTS[n]], ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_every_case_on_the_cpu_first(name, args, exact):
    """Every case of every GPU test below, built without a GPU (lib = None: geometry, data, memory images, the fp64 reference, no
    launch).  Exact cases: every reference satisfies mag < 2^24.  Real-valued cases: every sum's bound stays below one average
    term's share (_sees_one_row with K, or M), the SiLU / SiLU' term below 1/8 of a bf16 step of the reference.  Every case reaches
    the path it is named after by the restated host rules."""
    globals()[name](None, *args, exact)


def test_the_cpu_table_lists_every_gpu_test():
    """_GPU_TESTS names every GPU test of this file but the two return-code tests, which build no case"""
    mine = {k for k, f in globals().items() if k.startswith("test_") and callable(f) and any(m.name == "gpu" for m in getattr(f, "pytestmark", []))}
    assert mine - set(_GPU_TESTS) == {"test_gemm_return_codes", "test_wgrad_return_codes"} and set(_GPU_TESTS) <= mine


# ------------------------------------------------------------------ buffers, hooks, records
def _blank(n, dtype, out):
    if out:
        return torch.full((n,), _SENTINEL[dtype], dtype=_INT[dtype]).view(dtype)
    return torch.full((n,), NAN, dtype=dtype)


def _image(idx, dtype, data=None, out=False, span=None):
    """the CPU image of `span` elements of memory: the elements `idx` hold `data` (or NaN), the rest NaN (inputs) or the sentinel (outputs)"""
    idx = idx.reshape(-1)
    span = int(idx.max()) + 1 if span is None else int(span)
    assert int(idx.min()) >= 0 and int(idx.max()) < span
    flat = _blank(span, dtype, out)
    flat[idx] = torch.full((idx.numel(),), NAN, dtype=dtype) if data is None else data.reshape(-1).to(dtype)
    return flat


class PBuf(Buf):
    """The pitched variant of Buf: `span` elements of memory between two guards of GUARD_EL elements, of which the elements `idx`
    (an index tensor of the tensor's logical shape) are the tensor.  Everything else — pitch padding, the gaps between batch items,
    `lead` elements that misalign the base pointer, the guards — holds NaN (inputs) or the sentinel (outputs); the tensor holds
    `data`, or NaN.  `flat` is the CPU image of the span as uploaded (what a reference that addresses memory reads)."""

    def __init__(self, idx, dtype, data=None, out=False, lead=0, span=None):
        self.shape, self.dtype, self.out = tuple(idx.shape), dtype, out
        self.idx = idx.reshape(-1)
        self.flat = _image(idx, dtype, data, out, span)
        self.span = self.flat.numel()
        self.g = GUARD_EL + lead
        self.full = torch.cat([_blank(self.g, dtype, out), self.flat, _blank(GUARD_EL, dtype, out)]).to(DEV)
        self.t = self.full[self.g:self.g + self.span]

    def intact(self, also=None):
        """every element that is not the tensor's (nor one of `also`, flat indices the library may overwrite) still holds the sentinel"""
        v = self.full.view(_INT[self.dtype]).cpu()
        rest = torch.ones(v.numel(), dtype=torch.bool)
        rest[self.g + self.idx] = False
        if also is not None:
            rest[self.g + also.reshape(-1)] = False
        return self.out and bool((v[rest] == _SENTINEL[self.dtype]).all())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.cpu()).all())

    def cpu(self):
        return self.t.cpu()[self.idx].view(self.shape)

    def bits(self):
        return self.cpu().view(_INT[self.dtype])


def _idx(batch, zdiv, rows, cols, ld, s_hi, s_lo, transposed=False):
    """flat position of element (z; r, c): (z / zdiv) * s_hi + (z % zdiv) * s_lo + (transposed ? c * ld + r : r * ld + c)"""
    z = torch.arange(batch).view(batch, 1, 1)
    r = torch.arange(rows).view(1, rows, 1)
    c = torch.arange(cols).view(1, 1, cols)
    return (z // zdiv) * s_hi + (z % zdiv) * s_lo + ((c * ld + r) if transposed else (r * ld + c))


_HOOKS = {"variant": "ea_set_gemm_variant", "glds": "ea_set_gemm_glds", "w8": "ea_set_gemm_w8", "swizzle": "ea_set_gemm_xcd_swizzle",
          "nt": "ea_set_gemm_nt_store_min_bytes", "wgrad_tr": "ea_set_wgrad_transposing_reads", "wgrad_w8": "ea_set_wgrad_w8"}
_PINNED = dict(variant=1, glds=0, w8=0, swizzle=3, nt=0, wgrad_tr=0, wgrad_w8=0)


@contextlib.contextmanager
def hooks(lib, **kw):
    """pins ALL process-global tuning hooks (those not named: the register-staged 128-row kernels) and restores them afterwards"""
    assert set(kw) <= set(_PINNED), kw
    want, old = dict(_PINNED, **kw), {}
    try:
        for k, v in want.items():
            old[k] = getattr(lib, _HOOKS[k])(v)
        yield
    finally:
        for k, v in old.items():
            getattr(lib, _HOOKS[k])(v)


def _recorded(lib, call):
    """runs `call` with the library's launch profile on -> (return code, records [(M, N, K, batch, a_ks, b_ks, splitk, bm64, epi)])"""
    lib.ea_gemm_profile_enable(1)
    try:
        rc = call()
        _sync()
        fd, path = tempfile.mkstemp(suffix=".txt")
        os.close(fd)
        try:
            n = lib.ea_gemm_profile_dump(path.encode())
            with open(path) as f:
                recs = [tuple(int(t) for t in line.split()[:9]) for line in f if line.strip()]
        finally:
            os.unlink(path)
        assert n == len(recs)
    finally:
        lib.ea_gemm_profile_enable(1)  # (clears the records and their events)
        lib.ea_gemm_profile_enable(0)
    return rc, recs


def _scale(n):
    """index i at 16^(i % 3 - 1): neighbours are a factor 16 or 256 apart"""
    return 16.0 ** (torch.arange(n) % 3 - 1).double()


def _real_operand(g, Z, rows, K, s):
    """bf16 [Z][rows][K], row r at scale s * 16^(r % 3 - 1)"""
    return (torch.randn(Z, rows, K, generator=g).double() * (s * _scale(rows)).view(1, rows, 1)).to(BF)


def _rc_scaled(g, batch, M, N):
    return torch.randn(batch, M, N, generator=g).double() * _scale(M).view(1, M, 1) * _scale(N).view(1, 1, N)


# ------------------------------------------------------------------ one GEMM launch, described, run and compared
_DEFAULTS = dict(batch=1, zdiv=1, a_ks=False, b_ks=False, pad_a=0, pad_b=0, lead_a=0, lead_b=0, shared_b=False, bias=False, alpha=1.0,
                 act=R.ACT_NONE, drop=False, aux=False, c2=False, out_scale=1.0, resid="", c_f32=False, accumulate=False, splitk=1,
                 pad_c=8, pad_c2=16, pad_r=8, pad_x=8, q=None, ragged=False,
                 variant=1, glds=0, w8=0, swizzle=3, nt=0, path="reg", fast=None)


class Case:
    """(M, N, K) and everything else about one ea_gemm_bf16 launch.  pad_*: row pitch minus the natural width; lead_*: elements by
    which an operand's base is misaligned; shared_b: sB_lo = 0; resid: "" | "bf16" | "f32"; q = (qsplit_n, with q_v, with pos_u);
    path: the kernel the case is about ("reg" | "glds" | "w8"); fast: whether it must (True) / must not (False) take the FAST epilogue"""

    def __init__(self, M, N, K, **kw):
        assert set(kw) <= set(_DEFAULTS), set(kw) - set(_DEFAULTS)
        self.__dict__.update(_DEFAULTS, M=M, N=N, K=K, **kw)
        self.kw = kw

    def __repr__(self):
        return f"Case({self.M}, {self.N}, {self.K}, " + ", ".join(f"{k}={v!r}" for k, v in sorted(self.kw.items())) + ")"

    def but(self, **kw):
        return Case(self.M, self.N, self.K, **dict(self.kw, **kw))


def _split(K, splitk):
    """the library's rounding of a split-K request (gemm.hip ea_gemm_bf16) -> (k per chunk, effective chunks)"""
    if splitk <= 1:
        return K, 1
    chunk = ((K + splitk - 1) // splitk + BK - 1) // BK * BK
    return chunk, (K + chunk - 1) // chunk


def _selected_path(c, L):
    """gemm.hip's host rules restated -> (path, fast, expected bm64 of the record)"""
    kchunk, eff = _split(c.K, c.splitk)
    m8 = lambda *v: all(x % 8 == 0 for x in v)
    fast = (not c.c_f32 and eff == 1 and c.batch == 1 and c.resid != "f32" and c.N % 128 == 0 and m8(L["ldc"], L["sC_hi"], L["sC_lo"])
            and (not c.aux or m8(L["ldaux"])) and (not c.resid or m8(L["ldr"])) and (not c.c2 or m8(L["ldc2"])) and (not c.q or m8(L["ld_q"])))
    # (fast_epilogue_ok; every base pointer here is 16-byte aligned unless lead_* says otherwise)
    kc_ok = (not c.a_ks and not c.b_ks and c.K % BK == 0 and kchunk % BK == 0 and m8(L["lda"], L["ldb"], *L["sA"], *L["sB"])
             and c.lead_a == 0 and c.lead_b == 0)  # glds_eligible
    ragged = (not c.c_f32 and eff == 1 and c.batch == 1 and not c.resid and not c.aux and not c.c2 and not c.q and c.N % 4 == 0
              and L["ldc"] % 8 == 0 and L["ldc"] >= (c.N + 31) // 32 * 32)  # w8_ragged_ok
    if c.w8 >= 2 and kc_ok and (fast or ragged):
        kind_ok = not (c.q and (c.aux or c.c2 or c.resid or c.drop or c.act or c.out_scale != 1.0)) and not (c.c2 and (c.aux or c.resid)) \
            and not (c.aux and c.resid)  # w8_kind
        if kind_ok:
            return "w8", fast, 100 + c.w8
    bm64 = {1: 0, 2: 1}[c.variant]
    if c.glds and kc_ok:
        nst = c.glds
        if nst == 1:
            blocks = -(-c.N // 128) * -(-c.M // (64 if bm64 else 128)) * c.batch * eff
            nst = 3 if (blocks <= 512 and kchunk // BK >= 4) else (2 if kchunk // BK >= 16 else 0)
        if nst:
            return "glds", fast, bm64
    return "reg", fast and not c.a_ks and not c.b_ks, bm64


def _plan(c, exact):
    """Everything about a case that needs no GPU: geometry, the path the host rules select, the data, the memory images of A and B,
    the fp64 reference and the bound's parts.  The magnitudes of the exact cases and the transcendental terms of the real-valued ones
    are asserted here, so that they can be checked for every case before anything is launched."""
    M, N, K, batch, zdiv = c.M, c.N, c.K, c.batch, c.zdiv
    P = types.SimpleNamespace()
    g = _gen(zlib.crc32(repr(c).encode()) + int(exact))
    # ---- geometry: pitches, and batch strides that leave a gap after every item
    P.lda, P.ldb = (M if c.a_ks else K) + c.pad_a, (N if c.b_ks else K) + c.pad_b
    slab_a, slab_b = (K if c.a_ks else M) * P.lda, (K if c.b_ks else N) * P.ldb
    P.sA = (zdiv * slab_a + 16, slab_a)
    P.sB = (slab_b + 16, 0) if c.shared_b else (zdiv * slab_b + 16, slab_b)
    P.ldc, P.ldc2, P.ldr, P.ldaux = N + c.pad_c, N + c.pad_c2, N + c.pad_r, N + c.pad_x
    gap = 8 if P.ldc % 8 == 0 else 5
    sC_lo = M * max(P.ldc, P.ldc2 if c.c2 else 0) + gap
    P.sC = (zdiv * sC_lo + gap, sC_lo)
    P.sR, P.sX = (zdiv * (M * P.ldr + 8) + 8, M * P.ldr + 8), (zdiv * (M * P.ldaux + 8) + 8, M * P.ldaux + 8)
    P.qn, P.with_v, with_pos_u = c.q if c.q else (0, False, False)
    P.ld_q = P.qn + 8
    L = dict(lda=P.lda, ldb=P.ldb, ldc=P.ldc, ldc2=P.ldc2, ldr=P.ldr, ldaux=P.ldaux, ld_q=P.ld_q, sA=P.sA, sB=P.sB, sC_hi=P.sC[0], sC_lo=P.sC[1])
    P.path, P.fast, P.bm64 = _selected_path(c, L)
    assert P.path == c.path, (c, "takes", P.path)
    assert c.fast is None or P.fast == c.fast, (c, "FAST epilogue", P.fast)
    P.eff = _split(K, c.splitk)[1]
    # ---- data
    nb = -(-batch // zdiv) if c.shared_b else batch
    if exact:
        P.A, P.B = _ints(g, (batch, M, K), -1, 1, 0.5).to(BF), _ints(g, (nb, N, K), -1, 1, 0.25).to(BF)
        P.bias = (_ints(g, (N,), -6, 6) / 2).float()
        small = lambda: _ints(g, (batch, M, N), -8, 8) / 2
        P.aux, pos = _ints(g, (batch, M, N), -2, 2).to(BF), lambda: (_ints(g, (P.qn,), -6, 6) / 2).float()
        P.p_drop = 0.5
    else:
        P.A, P.B = _real_operand(g, batch, M, K, 1.0), _real_operand(g, nb, N, K, K ** -0.5)
        P.bias = (torch.randn(N, generator=g).double() * _scale(N)).float()
        small = lambda: _rc_scaled(g, batch, M, N)
        P.aux = (1.5 * torch.randn(batch, M, N, generator=g)).to(BF)
        pos = lambda: (torch.randn(P.qn, generator=g).double() * _scale(P.qn)).float()
        P.p_drop = 0.1
    if c.shared_b:  # item z reads the B of its outer index: the same memory for every inner index
        P.B = P.B.repeat_interleave(zdiv, 0)[:batch]
    P.iA, P.iB = _idx(batch, zdiv, M, K, P.lda, *P.sA, transposed=c.a_ks), _idx(batch, zdiv, N, K, P.ldb, *P.sB, transposed=c.b_ks)
    P.pre = small().float() if c.accumulate else None
    P.res = small().to(BF if c.resid == "bf16" else F32) if c.resid else None
    P.pos_u, P.pos_v = (pos() if with_pos_u else None, pos()) if c.q else (None, None)
    P.seed = 0x9E3779B97F4A7C15 ^ zlib.crc32(repr(c).encode())
    # ---- the reference, from the memory images the kernel will read
    kw = dict(batch=batch, zdiv=zdiv, a_kstrided=c.a_ks, b_kstrided=c.b_ks, lda=P.lda, ldb=P.ldb, sA=P.sA, sB=P.sB, alpha=c.alpha)
    if c.bias:
        kw["bias"] = P.bias
    imgA, imgB = _image(P.iA, BF, P.A), _image(P.iB, BF, P.B)
    v = R.gemm(imgA, imgB, M, N, K, **kw)["C"]  # alpha acc + bias
    kw.update(activation=c.act, out_scale=c.out_scale, two_outputs=c.c2, prefill=P.pre, resid=P.res)
    kp = torch.ones_like(v)
    if c.drop:
        kp = kw["keep_scale"] = R.keep(P.seed, P.p_drop, batch, M, N)
    if c.aux:
        kw["aux"] = P.aux
    if c.q:
        kw["qsplit"] = (P.qn, P.pos_u, P.pos_v, 0.125)
    P.ref = R.gemm(imgA, imgB, M, N, K, **kw)
    P.chain = K + 4 + (P.eff if c.c_f32 else 0)
    P.extra = None
    if exact:
        assert c.act != R.ACT_SILU
        for k in ("C_mag", "C2_mag", "q_pre_mag"):
            assert k not in P.ref or float(P.ref[k].max()) < 2.0 ** 24, (c, k)
    else:
        _sees_one_row(repr(c), P.chain * E23 * P.ref["C_mag"], P.ref["C_mag"], K)
        if c.act == R.ACT_SILU:
            assert not c.resid, "SiLU cases add no residual: the extra term is held against the step of the reference itself"
            if c.aux:
                P.extra = _dsilu_terms(R.f64(P.aux))[1] * (v * kp).abs() * abs(c.out_scale)
            else:
                P.extra = _silu_extra(v) * kp * abs(c.out_scale)
            _eighth_of_a_step(repr(c), P.extra, P.ref["C2"] if c.c2 else P.ref["C"])
    return P


def run_case(lib, c, exact):
    """lib = None: the CPU part alone (_plan)"""
    M, N, K, batch, zdiv = c.M, c.N, c.K, c.batch, c.zdiv
    P = _plan(c, exact)
    if lib is None:
        return
    qn = P.qn
    bA, bB = PBuf(P.iA, BF, P.A, lead=c.lead_a), PBuf(P.iB, BF, P.B, lead=c.lead_b)
    bC = PBuf(_idx(batch, zdiv, M, N, P.ldc, *P.sC), F32 if c.c_f32 else BF, P.pre, out=True)
    p = _params()
    p.A, p.B, p.C = bA.p.value, bB.p.value, bC.p.value
    p.M, p.N, p.K, p.batch, p.zdiv = M, N, K, batch, zdiv
    p.a_kstrided, p.b_kstrided, p.c_f32, p.accumulate, p.act = int(c.a_ks), int(c.b_ks), int(c.c_f32), int(c.accumulate), c.act
    p.lda, p.ldb, p.ldc = P.lda, P.ldb, P.ldc
    p.sA_hi, p.sA_lo, p.sB_hi, p.sB_lo, p.sC_hi, p.sC_lo = *P.sA, *P.sB, *P.sC   # (zdiv = 1: z % zdiv = 0, the outer stride alone is used)
    p.alpha, p.out_scale, p.splitk = c.alpha, c.out_scale, c.splitk
    outs = {"C": bC}
    if c.bias:
        bb = inp(P.bias)
        p.bias = bb.p.value
    if c.drop:
        p.drop_seed = P.seed
        p.drop_thr, p.drop_scale = R.drop_params(P.p_drop)
        if exact:
            assert p.drop_thr == 2 ** 31 and p.drop_scale == 2.0
    if c.aux:
        bX = PBuf(_idx(batch, zdiv, M, N, P.ldaux, *P.sX), BF, P.aux)
        p.aux, p.ldaux, p.sX_hi, p.sX_lo = bX.p.value, P.ldaux, *P.sX
    if c.resid:
        bR = PBuf(_idx(batch, zdiv, M, N, P.ldr, *P.sR), P.res.dtype, P.res)
        p.resid, p.ldr, p.sR_hi, p.sR_lo, p.resid_f32 = bR.p.value, P.ldr, *P.sR, int(c.resid == "f32")
    if c.c2:
        outs["C2"] = PBuf(_idx(batch, zdiv, M, N, P.ldc2, *P.sC), BF, out=True)
        p.C2, p.ldc2 = outs["C2"].p.value, P.ldc2
    if c.splitk > 1:
        nws = lib.ea_gemm_splitk_workspace_bytes(M, N, batch, c.splitk) // 4
        assert nws == c.splitk * batch * M * N
        outs["workspace"] = out((nws,), F32)
        p.workspace = outs["workspace"].p.value
    if c.q:
        outs["q_u"] = PBuf(_idx(1, 1, M, qn, P.ld_q, 0, 0), BF, out=True)
        p.q_u, p.ld_q, p.qsplit_n, p.qscale = outs["q_u"].p.value, P.ld_q, qn, 0.125
        if P.with_v:
            outs["q_v"] = PBuf(_idx(1, 1, M, qn, P.ld_q, 0, 0), BF, out=True)
            p.q_v = outs["q_v"].p.value
        bpu, bpv = (inp(P.pos_u) if P.pos_u is not None else None), inp(P.pos_v)
        p.pos_u, p.pos_v = (bpu.p.value if bpu else None), bpv.p.value
    # ---- the launch
    with hooks(lib, variant=c.variant, glds=c.glds, w8=c.w8, swizzle=c.swizzle, nt=c.nt):
        rc, recs = _recorded(lib, lambda: lib.ea_gemm_bf16(ctypes.byref(p), _st()))
    assert rc == 0, (c, rc)
    assert len(recs) == 1 and recs[0][:7] == (M, N, K, batch, int(c.a_ks), int(c.b_ks), P.eff), (c, recs)
    assert recs[0][7] == P.bm64, (c, "profile record bm64", recs[0][7], "expected", P.bm64)
    # ---- nothing outside the outputs was written
    pad_ok = None
    if c.ragged:  # the header's contract for a padded pitch (include/espresso_amd.h:65-68): N .. roundup32(N) - 1 may be overwritten
        assert P.path == "w8" and not P.fast
        n32 = (N + 31) // 32 * 32
        pad_ok = _idx(1, 1, M, n32 - N, P.ldc, 0, 0) + N
    for k, b in outs.items():
        assert b.intact(pad_ok) if k == "C" else b.intact(), (c, k, "stored outside the tensor")
    # ---- every element against fp64
    assert torch.equal(bA.flat.view(torch.int16), _image(P.iA, BF, P.A).view(torch.int16))  # the reference read what was uploaded
    ref, chain, extra, tag = P.ref, P.chain, P.extra, repr(c)
    got, want, mag = bC.cpu(), ref["C"], ref["C_mag"]
    if c.q:  # the library does not write the query columns of C
        assert bool(torch.isnan(got[..., :qn]).all()), (c, "columns < qsplit_n of C were written")
        got, want, mag = got[..., qn:], want[..., qn:], mag[..., qn:]
        for name, posv in (("q_u", P.pos_u), ("q_v", P.pos_v)):
            if name not in outs:
                continue
            gq = outs[name].cpu()
            if exact:
                _same_values(tag + " " + name, gq, _bf_exact(ref[name]))
            else:
                e = chain * E23 * ref["q_pre_mag"]
                lo, hi = R.query(ref["q_pre"] - e, posv, 0.125), R.query(ref["q_pre"] + e, posv, 0.125)
                mid, half = (lo + hi) / 2, (hi - lo).abs() / 2
                big = torch.maximum(lo.abs(), hi.abs())
                _check(tag + " " + name, gq, mid, half + _ulp(big) + 2.0 ** -22 * big)
    if got.numel():
        if c.c2:
            _compare(tag + " C (pre-activation)", got, want, mag, exact, chain)
            _compare(tag + " C2", outs["C2"].cpu(), ref["C2"], ref["C2_mag"], exact, chain, extra)
        else:
            _compare(tag + " C", got, want, mag, exact, chain, extra)


def _params():
    from espresso_amd import _lib

    p = _lib.EaGemmParams()
    p.zdiv, p.batch, p.alpha, p.out_scale, p.splitk, p.qscale = 1, 1, 1.0, 1.0, 1, 1.0
    return p


def _kinds(N, exact):
    """the six epilogue kinds of the layer GEMMs (tests.gpu_checks.check_gemm_w8's), SiLU where the case is real-valued"""
    act = R.ACT_RELU if exact else R.ACT_SILU
    qn = 256 if N >= 384 else 128
    return {"plain": {}, "bias_relu": dict(bias=True, act=R.ACT_RELU), "qsplit": dict(bias=True, q=(qn, True, True)),
            "qsplit_no_v": dict(bias=True, q=(qn, False, True)), "qsplit_no_pos_u": dict(q=(qn, True, False)),
            "act2": dict(bias=True, act=act, drop=True, c2=True), "aux": dict(aux=True, act=act, drop=True),
            "resid": dict(bias=True, drop=True, out_scale=0.5, resid="bf16")}


KINDS = _KIND_LIST
LAYOUTS = pytest.mark.parametrize("a_ks,b_ks", _LAYOUT_LIST, ids=["nt", "nn", "tt", "tn"])
VARIANTS = pytest.mark.parametrize("variant", [1, 2], ids=["bm128", "bm64"])


# ------------------------------------------------------------------ the register-staged kernel
# (M, N, K): one element; one 64-row / one 128-row whole tile (FAST epilogue when both operands are k-contiguous); one past a tile in
# every dimension; less than a tile with K < 64; ragged everything over two row blocks / two column blocks / two k-tiles
REG_SHAPES = [(1, 1, 1), (64, 128, 64), (128, 128, 128), (129, 130, 65), (77, 40, 16), (200, 136, 72), (257, 190, 100)]


@gpu
@EXACT
@VARIANTS
@LAYOUTS
def test_register_staged_kernel(lib, a_ks, b_ks, variant, exact):
    for i, (M, N, K) in enumerate(REG_SHAPES):
        run_case(lib, Case(M, N, K, a_ks=a_ks, b_ks=b_ks, variant=variant, pad_c=(8, 5, 0)[i % 3]), exact)
    # misaligned operands: odd pitches (K = 70 at pitch 71 / the k-strided pitch M + 1 or N + 1), a base one element off
    run_case(lib, Case(130, 72, 70, a_ks=a_ks, b_ks=b_ks, variant=variant, pad_a=1 if not a_ks else 3, pad_b=1 if not b_ks else 3), exact)
    run_case(lib, Case(130, 72, 70, a_ks=a_ks, b_ks=b_ks, variant=variant, pad_a=2 if not a_ks else 6, pad_b=2 if not b_ks else 0,
                       lead_a=1, lead_b=1), exact)
    if a_ks:  # a k-strided A whose pitch is the odd M itself
        run_case(lib, Case(133, 72, 70, a_ks=True, b_ks=b_ks, variant=variant, pad_a=0), exact)


@gpu
@EXACT
@VARIANTS
@LAYOUTS
def test_batched_with_zdiv(lib, a_ks, b_ks, variant, exact):
    """batch 6, zdiv 3: distinct s_hi / s_lo for A and C, and sB_lo = 0 (one B shared by the inner index)"""
    run_case(lib, Case(129, 130, 65, batch=6, zdiv=3, a_ks=a_ks, b_ks=b_ks, variant=variant, shared_b=True, bias=True), exact)
    run_case(lib, Case(77, 40, 16, batch=6, zdiv=3, a_ks=a_ks, b_ks=b_ks, variant=variant, pad_c=3, resid="bf16", out_scale=0.5), exact)


@gpu
@EXACT
@pytest.mark.parametrize("swizzle", [0, 3])
@pytest.mark.parametrize("batch,M", [(16, 256), (13, 320)], ids=["64wg", "65wg"])
def test_xcd_remap(lib, batch, M, swizzle, exact):
    """launch_gemm remaps workgroups onto tiles when `(g_xcd_swizzle & 2) && grid.x <= 16 && grid.x * grid.y * grid.z >= 64`: 64-row
    tiles, one column tile, batch * M / 64 = 64 and 65 workgroups (a count not divisible by 8); mask 0: the same launch unmapped"""
    assert batch * (M // 64) in (64, 65)
    run_case(lib, Case(M, 128, 64, batch=batch, variant=2, swizzle=swizzle, bias=True), exact)


# ------------------------------------------------------------------ the general epilogue, term by term
def _terms(exact):
    t = {"bias": dict(bias=True), "alpha": dict(alpha=0.125), "relu": dict(act=R.ACT_RELU), "dropout": dict(drop=True),
         "aux_relu": dict(aux=True, act=R.ACT_RELU), "two_outputs": dict(c2=True, bias=True, act=R.ACT_RELU),
         "scale_resid": dict(out_scale=0.5, resid="bf16"), "f32": dict(c_f32=True), "f32_accumulate": dict(c_f32=True, accumulate=True),
         "f32_resid_f32": dict(c_f32=True, resid="f32", bias=True),
         "layer_act2": dict(bias=True, act=R.ACT_RELU, drop=True, c2=True), "layer_aux": dict(aux=True, act=R.ACT_RELU, drop=True, alpha=0.5),
         "layer_resid": dict(bias=True, drop=True, out_scale=0.5, resid="bf16"),
         "everything_f32": dict(bias=True, alpha=2.0, act=R.ACT_RELU, drop=True, out_scale=0.5, resid="f32", c_f32=True, accumulate=True)}
    if not exact:
        t.update({"silu": dict(act=R.ACT_SILU, bias=True), "aux_silu": dict(aux=True, act=R.ACT_SILU),
                  "layer_act2_silu": dict(bias=True, act=R.ACT_SILU, drop=True, c2=True), "layer_aux_silu": dict(aux=True, act=R.ACT_SILU, drop=True)})
    return t


@gpu
@EXACT
@pytest.mark.parametrize("pads", ["scalar", "vector"])
@pytest.mark.parametrize("M,N,K", [(200, 136, 72), (130, 36, 64)])
def test_general_epilogue(lib, M, N, K, pads, exact):
    """each term alone and the layers' combinations; `scalar`: ldc, ldc2, ldr, ldaux not multiples of 8 (element-wise loads and stores),
    64-row tiles; `vector`: multiples of 8 (16-byte accesses in the whole chunks, element-wise in the ragged last one), 128-row tiles"""
    r8 = -N % 8
    pad = dict(pad_c=r8 + 3, pad_c2=r8 + 5, pad_r=r8 + 1, pad_x=r8 + 7, variant=2) if pads == "scalar" else \
        dict(pad_c=r8 + 8, pad_c2=r8 + 16, pad_r=r8 + 24, pad_x=r8, variant=1)
    for name, kw in _terms(exact).items():
        run_case(lib, Case(M, N, K, fast=False, **pad, **kw), exact)
    run_case(lib, Case(M, N, K, fast=False, batch=2, **pad, **_terms(exact)["layer_resid"]), exact)
    run_case(lib, Case(M, N, K, fast=False, batch=2, **pad, **_terms(exact)["layer_aux"]), exact)


# ------------------------------------------------------------------ the FAST epilogue
@gpu
@EXACT
@VARIANTS
@pytest.mark.parametrize("kind", KINDS)
def test_fast_epilogue(lib, kind, variant, exact):
    """fast_epilogue_ok: bf16 output, batch 1, N % 128 == 0, every pitch a multiple of 8, every base 16-byte aligned.  The prefetch of the
    residual / auxiliary rows clamps at M - 1: M = 1, 63, 65, 130 end inside the first, the last and a middle 16-row pass"""
    for N in (128, 384):
        for M in (1, 63, 65, 130):
            run_case(lib, Case(M, N, 96, variant=variant, fast=True, pad_r=16, pad_x=24, **_kinds(N, exact)[kind]), exact)


@gpu
@EXACT
@pytest.mark.parametrize("kind", ["plain", "qsplit", "act2", "resid"])
def test_fast_epilogue_non_temporal_stores(lib, kind, exact):
    """ea_set_gemm_nt_store_min_bytes(1): every bf16 output of the FAST epilogue leaves through the non-temporal store"""
    run_case(lib, Case(130, 384, 96, nt=1, fast=True, **_kinds(384, exact)[kind]), exact)
    run_case(lib, Case(65, 128, 128, nt=1, fast=True, glds=2, path="glds", **_kinds(128, exact)[kind]), exact)


# ------------------------------------------------------------------ the direct-to-LDS ring
@gpu
@EXACT
@VARIANTS
@pytest.mark.parametrize("stages", [2, 3, 4])
def test_direct_to_lds_ring(lib, stages, variant, exact):
    """K = 64 .. 320: 1 .. 5 k-tiles — fewer than the ring is deep, exactly as many, more.  M = 1, 65, 130: rows past M are clamped to
    the last valid row.  N = 128 (FAST epilogue), 136, 40 (general; operand rows past N clamped)"""
    for K in (64, 128, 192, 256, 320):
        for j, (M, N) in enumerate([(M, N) for M in (1, 65, 130) for N in (128, 136, 40)]):
            kw = [{}, dict(bias=True, act=R.ACT_RELU), dict(bias=True, drop=True, out_scale=0.5, resid="bf16")][(j + K // 64) % 3]
            run_case(lib, Case(M, N, K, glds=stages, variant=variant, path="glds", fast=N == 128, **kw), exact)


@gpu
@EXACT
@VARIANTS
def test_direct_to_lds_ring_batched_and_automatic(lib, variant, exact):
    run_case(lib, Case(130, 136, 192, batch=6, zdiv=3, shared_b=True, glds=3, variant=variant, path="glds", bias=True), exact)
    run_case(lib, Case(256, 128, 64, batch=16, glds=2, variant=2, path="glds", swizzle=1, bias=True), exact)  # the ring kernel's XCD remap
    # automatic depth: `blocks <= 512 && nkt >= 4` -> three stages
    run_case(lib, Case(130, 136, 1024, glds=1, variant=variant, path="glds", bias=True, act=R.ACT_RELU), exact)
    run_case(lib, Case(65, 128, 1024, glds=1, variant=variant, path="glds", fast=True), exact)


# ------------------------------------------------------------------ the 8-wave tiles
@gpu
@EXACT
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg", [2, 3, 4, 5])
def test_w8_tiles(lib, cfg, kind, exact):
    """forced tile configuration (256 x 256 / 128 x 128 / 256 x 128 / 128 x 256), against fp64 and the exact integers, not against the
    4-wave kernel; the record's bm64 = 100 + cfg proves which kernel ran.  K = 64 is shorter than every ring"""
    for M, N, K in [(M, N, K) for M in (1, 130, 257) for N in (128, 384, 640) for K in (64, 192, 512)]:
        run_case(lib, Case(M, N, K, w8=cfg, path="w8", fast=True, pad_r=16, pad_x=24, **_kinds(N, exact)[kind]), exact)


@gpu
@EXACT
@pytest.mark.parametrize("cfg", [2, 3, 4, 5])
def test_w8_ragged_n(lib, cfg, exact):
    """w8_ragged_ok: N % 4 == 0, ldc >= roundup32(N), plain / bias / activation / dropout only.  THE ONE EXCEPTION to the pad check:
    the kernel stores whole 32-column groups, the columns N .. roundup32(N) - 1 are padding it may overwrite (module docstring)"""
    act = R.ACT_RELU if exact else R.ACT_SILU
    for M, N, K, ldc in ((130, 132, 128, 160), (257, 36, 64, 64), (130, 132, 128, 176)):  # (176 > roundup32(132): pad the kernel must leave)
        for kw in ({}, dict(bias=True, act=act, drop=True), dict(bias=True, alpha=0.5)):
            run_case(lib, Case(M, N, K, w8=cfg, path="w8", fast=False, ragged=True, pad_c=ldc - N, **kw), exact)


# ------------------------------------------------------------------ split-K
@gpu
@EXACT
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
def test_split_k(lib, accumulate, exact):
    """fp32 output, NaN workspace (intact around it afterwards).  (130,200,520) at 3 and 7 (7 -> 128 per chunk -> 5 chunks);
    (64,72,130) at 7 -> 3 chunks; (64,64,64) at 4 -> one chunk, no reduce pass: the plain epilogue honours `accumulate`;
    k-contiguous (128,128,640) at 5 on the ring kernel; N and ldc multiples of 4 (float4 reduce) and not (scalar reduce); batch 2"""
    kw = dict(c_f32=True, accumulate=accumulate)
    assert _split(520, 3)[1] == 3 and _split(520, 7)[1] == 5 and _split(130, 7)[1] == 3 and _split(64, 4)[1] == 1 and _split(640, 5) == (128, 5)
    for variant in (1, 2):
        for pad_c in (0, 4, 3):
            run_case(lib, Case(130, 200, 520, a_ks=True, b_ks=True, splitk=3, variant=variant, pad_c=pad_c, **kw), exact)
            run_case(lib, Case(130, 200, 520, a_ks=True, b_ks=True, splitk=7, variant=variant, pad_c=pad_c, **kw), exact)
        run_case(lib, Case(64, 72, 130, a_ks=True, b_ks=True, splitk=7, variant=variant, pad_c=0, **kw), exact)
        run_case(lib, Case(64, 70, 130, a_ks=True, b_ks=True, splitk=7, variant=variant, pad_c=2, **kw), exact)
        run_case(lib, Case(64, 64, 64, a_ks=True, b_ks=True, splitk=4, variant=variant, **kw), exact)
        run_case(lib, Case(128, 128, 640, splitk=5, variant=variant, **kw), exact)
        run_case(lib, Case(128, 128, 640, splitk=5, glds=2, path="glds", variant=variant, **kw), exact)
        run_case(lib, Case(130, 200, 520, a_ks=True, b_ks=True, splitk=3, batch=2, variant=variant, pad_c=4, **kw), exact)
        run_case(lib, Case(64, 70, 130, a_ks=True, b_ks=False, splitk=7, batch=2, variant=variant, pad_c=1, **kw), exact)


# ------------------------------------------------------------------ return codes
@gpu
def test_gemm_return_codes(lib):
    """the documented refusals (-2, -4) and empty problems (0): no launch (no profile record), every output untouched"""
    M, N, K = 64, 128, 64
    g = _gen(3)
    bA, bB = inp(_ints(g, (M, K), -1, 1).to(BF)), inp(_ints(g, (N, K), -1, 1).to(BF))
    bf32 = inp(torch.randn(N, generator=g))

    def run(what, want, **kw):
        o = dict(C=out((2 * M, N), BF), C32=out((2 * M, N), F32), q_u=out((M, N), BF), q_v=out((M, N), BF), ws=out((4 * M, N), F32))
        p = _params()
        p.A, p.B, p.M, p.N, p.K, p.lda, p.ldb, p.ldc = bA.p.value, bB.p.value, M, N, K, K, K, N
        p.sA_hi, p.sC_hi = 0, M * N
        special = dict(q=False, ws=True, bias=False)
        special.update({k: kw.pop(k) for k in list(kw) if k in special})
        for k, v in kw.items():
            setattr(p, k, v)
        p.C = (o["C32"] if p.c_f32 else o["C"]).p.value
        if special["q"]:
            p.q_u, p.q_v, p.qscale = o["q_u"].p.value, o["q_v"].p.value, 0.125
        if p.splitk > 1 and special["ws"]:
            p.workspace = o["ws"].p.value
        if special["bias"]:
            p.bias = bf32.p.value
        with hooks(lib):
            rc, recs = _recorded(lib, lambda: lib.ea_gemm_bf16(ctypes.byref(p), _st()))
        assert rc == want, (what, rc, want)
        assert recs == [], (what, "launched")
        for k, b in o.items():
            assert b.untouched(), (what, k)

    run("M = 0", 0, M=0)
    run("M < 0", 0, M=-1)
    run("N = 0", 0, N=0)
    run("N < 0", 0, N=-1)
    run("batch = 0", 0, batch=0)
    run("batch < 0", 0, batch=-2)
    run("K = 0", -2, K=0)
    run("K < 0", -2, K=-5)
    run("zdiv = 0", -2, zdiv=0)
    ok = dict(q=True, qsplit_n=128, ld_q=128)
    run("qsplit_n % 128", -4, **dict(ok, qsplit_n=64))
    run("qsplit_n > N", -4, **dict(ok, qsplit_n=256, ld_q=256))
    run("query split, N % 8", -4, **dict(ok, N=132, ldc=132, qsplit_n=128))
    run("query split, batch 2", -4, **dict(ok, batch=2))
    run("query split, c_f32", -4, **dict(ok, c_f32=1))
    run("ld_q < qsplit_n", -4, **dict(ok, ld_q=120))
    sk = dict(splitk=2, c_f32=1)
    run("split-K, bf16 output", -4, splitk=2)
    run("split-K, bias", -4, bias=True, **sk)
    run("split-K, activation", -4, act=R.ACT_RELU, **sk)
    run("split-K, null workspace", -4, ws=False, **sk)


@gpu
def test_wgrad_return_codes(lib):
    from espresso_amd import _lib

    g = _gen(4)
    bdy, bx = inp(_ints(g, (64, 64), -1, 1).to(BF)), inp(_ints(g, (64, 64), -1, 1).to(BF))

    def run(what, want, count, **kw):
        o = dict(dW=out((64, 64), F32), db=out((64,), F32))
        grp = _lib.EaWgradGroup()
        grp.count = count
        for i in range(min(max(count, 1), 16)):
            q = grp.p[i]
            q.dy, q.x, q.dW, q.dbias, q.M, q.N, q.K, q.ld_dy, q.ld_x, q.ldw = bdy.p.value, bx.p.value, o["dW"].p.value, o["db"].p.value, 64, 64, 64, 64, 64, 64
        for k, v in kw.items():
            setattr(grp.p[0], k, v)
        for tr in (0, 1):
            with hooks(lib, wgrad_tr=tr, wgrad_w8=1):
                rc, recs = _recorded(lib, lambda: lib.ea_wgrad_group(ctypes.byref(grp), _st()))
            assert rc == want and recs == [], (what, rc, recs)
        for k, b in o.items():
            assert b.untouched(), (what, k)

    run("count 0", 0, 0)
    run("count 17", -2, 17)
    run("null dW", -2, 1, dW=None)
    run("M = 0", -2, 1, M=0)


# ------------------------------------------------------------------ the grouped weight gradient
def _tr_aligned_for(probs, bm):
    """ea_wgrad_group's aligned_for: whole tiles inside the row pitches, 16-byte aligned rows (the bases here always are)"""
    return all(-(-N // bm) * bm <= N + pdy and -(-K // 128) * 128 <= K + px and (N + pdy) % 8 == 0 and (K + px) % 8 == 0
               for (M, N, K, pdy, px, pw, bias) in probs)


def run_wgrad(lib, probs, exact, kernel, variant, seed=0, expect=None):
    """probs: [(M, N, K, ld_dy - N, ld_x - K, ldw - K, with bias)]; kernel: "reg" | "tr" | "w8"; variant: the tile height asked for;
    expect: the profile record's bm64 the caller claims.  lib = None: the CPU part alone (data, references, their assertions)"""
    g = _gen(1000 * len(probs) + seed + int(exact))
    bm64 = variant == 2
    if kernel == "tr":  # the preferred height first, then the other one
        if not _tr_aligned_for(probs, 64 if bm64 else 128):
            bm64 = not bm64
            assert _tr_aligned_for(probs, 64 if bm64 else 128), "the group does not reach the transposing kernel"
    elif kernel == "w8":
        assert all((N + pdy) % 8 == 0 and (K + px) % 8 == 0 and N + pdy >= 8 and K + px >= 8 for (M, N, K, pdy, px, pw, bias) in probs)
    want_bm64 = 108 if kernel == "w8" else int(bm64)
    assert expect is None or expect == want_bm64, (expect, want_bm64)
    data = []
    for i, (M, N, K, pdy, px, pw, bias) in enumerate(probs):
        if exact:
            dy, x = _ints(g, (1, M, N), -1, 1, 0.25).to(BF), _ints(g, (1, M, K), -1, 1).to(BF)
            dW0, db0 = _ints(g, (N, K), -3, 3).float(), _ints(g, (N,), -3, 3).float()
        else:
            dy = (torch.randn(1, M, N, generator=g).double() * _scale(N).view(1, 1, N)).to(BF)
            x = (torch.randn(1, M, K, generator=g).double() * _scale(K).view(1, 1, K)).to(BF)
            dW0 = (torch.randn(N, K, generator=g).double() * _scale(N).view(N, 1) * _scale(K).view(1, K)).float()
            db0 = (torch.randn(N, generator=g).double() * _scale(N)).float()
        dW, db, wmag, bmag = R.wgrad(dy[0], x[0], dW0, db0)
        chain_b = (4 * -(-M // 64) + 16 if kernel == "reg" else M) + 1
        tag = f"problem {i} {(M, N, K)}"
        if exact:
            assert float(wmag.max()) < 2.0 ** 24 and float(bmag.max()) < 2.0 ** 24, tag
        else:  # (the sums' own share of the bound, without the pre-fill's)
            own_w, own_b = wmag - dW0.double().abs(), bmag - db0.double().abs()
            _sees_one_row(tag + " dW", (M + 1) * E23 * own_w, own_w, M)
            _sees_one_row(tag + " db", chain_b * E23 * own_b, own_b, M)
        data.append((dy, x, dW0, db0, dW, db, wmag, bmag, chain_b, tag))
    if lib is None:
        return
    from espresso_amd import _lib

    grp = _lib.EaWgradGroup()
    grp.count = len(probs)
    bufs = []
    for i, ((M, N, K, pdy, px, pw, bias), (dy, x, dW0, db0, *_)) in enumerate(zip(probs, data)):
        bdy = PBuf(_idx(1, 1, M, N, N + pdy, 0, 0), BF, dy, span=M * (N + pdy))
        bx = PBuf(_idx(1, 1, M, K, K + px, 0, 0), BF, x, span=M * (K + px))
        bdW = PBuf(_idx(1, 1, N, K, K + pw, 0, 0), F32, dW0, out=True)
        bdb = out((N,), F32, db0)
        q = grp.p[i]
        q.dy, q.x, q.dW, q.dbias = bdy.p.value, bx.p.value, bdW.p.value, (bdb.p.value if bias else None)
        q.M, q.N, q.K, q.ld_dy, q.ld_x, q.ldw = M, N, K, N + pdy, K + px, K + pw
        bufs.append((bdy, bx, bdW, bdb))
    with hooks(lib, variant=variant, wgrad_tr=int(kernel != "reg"), wgrad_w8=2 if kernel == "w8" else 0):
        rc, recs = _recorded(lib, lambda: lib.ea_wgrad_group(ctypes.byref(grp), _st()))
    assert rc == 0
    assert len(recs) == 1 and recs[0][1] == len(probs) and recs[0][8] == 128, recs
    assert recs[0][7] == want_bm64, (recs, kernel, want_bm64)
    for (M, N, K, pdy, px, pw, bias), (dy, x, dW0, db0, dW, db, wmag, bmag, chain_b, tag), (bdy, bx, bdW, bdb) in zip(probs, data, bufs):
        assert bdW.intact() and bdb.intact(), tag
        _compare(tag + " dW", bdW.cpu()[0], dW, wmag, exact, M + 1)
        if bias:
            _compare(tag + " db", bdb.cpu(), db, bmag, exact, chain_b)
        else:
            _same_values(tag + " db (not passed)", bdb.cpu(), db0)


# (M, N, K, ld_dy - N, ld_x - K, ldw - K, bias): padded and unpadded pitches, bias off for two problems
WGRAD_REG = [(1, 1, 1, 0, 0, 0, True), (63, 129, 130, 7, 0, 3, True), (64, 136, 40, 8, 0, 0, False), (65, 200, 72, 0, 16, 4, True),
             (200, 64, 136, 3, 5, 1, False), (129, 128, 128, 0, 0, 8, True)]


@gpu
@EXACT
@VARIANTS
def test_wgrad_register_staged_kernel(lib, variant, exact):
    """transposing reads off, 8-wave kernel off: one group of six ragged and whole problems, then each problem as a group of one"""
    run_wgrad(lib, WGRAD_REG, exact, "reg", variant)
    for i, p in enumerate(WGRAD_REG):
        run_wgrad(lib, [p], exact, "reg", variant, seed=i + 1)


# whole-tile problems; ragged N / K inside a pitch that covers the tile (the pads hold NaN: they only reach rows / columns that are
# never stored)
WGRAD_TR = [(63, 128, 128, 0, 0, 0, True), (64, 256, 128, 8, 0, 4, True), (129, 128, 256, 0, 8, 0, False), (130, 100, 128, 28, 0, 0, True),
            (65, 128, 72, 0, 56, 3, True), (200, 100, 72, 28, 56, 0, False)]


@gpu
@EXACT
@VARIANTS
def test_wgrad_transposing_kernel(lib, variant, exact):
    """ea_wgrad_group's aligned_for holds for the asked height: the direct-to-LDS kernel with transposing reads, at that height (the
    record's bm64).  Rows past M come from the zero page: M = 63, 64, 65, 129, 130, 200"""
    assert _tr_aligned_for(WGRAD_TR, 128) and _tr_aligned_for(WGRAD_TR, 64)
    run_wgrad(lib, WGRAD_TR, exact, "tr", variant, expect=int(variant == 2))
    for i, p in enumerate(WGRAD_TR[:3]):
        run_wgrad(lib, [p], exact, "tr", variant, seed=i + 1)


@gpu
@EXACT
def test_wgrad_transposing_kernel_falls_back_to_64_rows(lib, exact):
    """N = 192 at pitch 192 = 3 x 64 has no whole 128-row tiling: asked for 128-row tiles the group must take the 64-row transposing
    kernel (bm64 = 1 in the record), not the register-staged one"""
    probs = [(130, 192, 128, 0, 0, 0, True), (65, 64, 256, 0, 0, 4, True)]
    assert not _tr_aligned_for(probs, 128) and _tr_aligned_for(probs, 64)
    run_wgrad(lib, probs, exact, "tr", 1, expect=1)


# small versions of tests.gpu_checks.check_wgrad_w8's shapes: M = 64 k - 1, 64 k + 1, N / K no multiples of 256, pitches shorter
# than the last 256-column tile (N = 296 at pitch 320, K = 130 at pitch 136)
WGRAD_W8 = [(63, 256, 256, 0, 0, 0, True), (65, 296, 128, 24, 0, 4, False), (257, 520, 130, 0, 6, 0, True), (130, 100, 384, 4, 8, 3, True)]


@gpu
@EXACT
def test_wgrad_w8_kernel(lib, exact):
    """ea_set_wgrad_w8(2): every 16-byte aligned group takes the 256 x 256 kernel (108 in the record)"""
    run_wgrad(lib, WGRAD_W8, exact, "w8", 1, expect=108)
    run_wgrad(lib, WGRAD_W8[2:3], exact, "w8", 1, seed=1)


@gpu
@EXACT
@pytest.mark.parametrize("kernel", ["reg", "tr", "w8"])
def test_wgrad_group_of_sixteen(lib, kernel, exact):
    """EA_WGRAD_MAX problems of mixed sizes: every start offset of the tile table"""
    probs = []
    for i in range(16):
        M, N, K = (63, 65, 130, 129)[i % 4], (128, 256, 64, 192)[(i // 2) % 4], (128, 256)[i % 2]
        if kernel == "reg":
            N, K = N + (i % 3), K - 5 * (i % 2)
        probs.append((M, N, K, {"reg": i % 2, "tr": 0, "w8": 8}[kernel], 0, (0, 4, 1)[i % 3], i % 5 != 0))
    run_wgrad(lib, probs, exact, kernel, 2)
