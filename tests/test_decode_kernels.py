"""The decode-step kernels of espresso_amd/csrc/decode.hip (ea_decode_attention / ea_decode_attention_probs: the vector and the
generic kernel; ea_kv_append_reorder; ea_beam_mask_rows; ea_beam_topk) one launch at a time against the plain restatement in
tests/recurrent_ref.py, through the C ABI, every element of every output.  (ea_attn_history_put / ea_attn_backtrace have their
exact test in tests/test_alignment_results.py.)

BUFFERS (tests/test_convmodule_kernels.py's Buf).  Every floating-point device tensor is a view into a larger allocation with
guards on both sides: NaN around inputs, a sentinel bit pattern around outputs (checked after the call).  Outputs start as NaN (a
missed store fails) or as known data (the new cache, the in-place lprobs).  Where a pitch exceeds the width (ldq > C, ldkv > 2C,
ldp > max_len) the gap holds NaN on input and the sentinel on output, checked after the call.  Integer inputs (kv_row, len,
parent) are plain tensors: a poisoned index would be an out-of-bounds access, not a finding.

SCALES.  q[n][h][c] ~ 0.35 N(0,1) s(h) s(c / 8), K ~ N(0,1) / (s(h) s(c / 8)), V ~ N(0,1) s(h + c / 8), s(i) = 16^(i % 3 - 1): the
scores stay O(sqrt(dh)) while a neighbouring head or 8-channel chunk of any operand is 16 or 256 times off.  Keys and values at
j >= len[row] are finite and 64 times larger than the valid ones.  Lengths differ per row and include 0.

DISPATCH (decode.hip:333-345).  decode_attention_vec_kernel<16 / 32 / 64>: "vec16", "vec32", "vec64" (all strides and offsets
multiples of 8, 16-byte aligned bases).  decode_attention_kernel: "gen8", "gen24", "gen40" (dh not in {16, 32, 64}) and "gen64off"
(dh = 64, koff = 4, voff = C + 4, ldkv = 2C + 8).  Every variant runs every max_len in {1, 15, 16, 17, 33, 64, 65, 157} with
(a) per-row len, interleaved K|V cache (ldkv = 2C, koff = 0, voff = C), N = 3, H = 3 (N H % 4 != 0), one empty row;
(b) len = NULL (fixed length), separate K and V allocations, N = 2, H = 8;
(c) per-row len, kv_row = [0, 1, 2, 3, 4, 1, 0] (seven hypotheses on five sentence rows, row 1 empty), ldq = C + 8, N = 7, H = 3.
Row 0 is full, row 1 empty; the other rows of (a) and (c) walk {1, 15, 16, 17, 31, 32, 33, max_len} (those <= max_len), so that every
variant meets every length.

BOUNDS.  Derived, none measured.  E = 2^-23 per fp32 rounding and per v_rcp_f32; ulp(x) = the bf16 step at |x|.
  score    tol_s = (dh / 4 + 6) E sum_d |q k|      the products of two bf16 values are exact in fp32; vector kernel: dh / 4 additions
           per lane and two shuffle steps (decode.hip:122-131); generic: the six steps of wave_sum (:50-51)
  e_j = __expf(s_j - m)                             rel_e = 2 max_j tol_s + (2 |s_j - m| + 1) E: the score's and the maximum's error,
           the subtraction's rounding (|s_j - m| E), and __expf as tests/test_gemm_kernels.py charges it: v_exp_f32 1 ulp, the two
           roundings of its argument |x| E of the result (:57-61, :144-148)
  sum      rel_sum = sum_j p_j rel_e_j + (ceil(max_len / 64) + 6) E     additions per lane, wave_sum (:60-62)
  probs    p (rel_e + rel_sum + 2 E)                the division (:25); exactly 0 from len to max_len; untouched up to ldp
  out      ulp(ref) + sum_j p |v| (rel_e + rel_sum) + (max_len + 4) E sum_j p |v|     fp32 sum over the keys (serially in the generic
           kernel, ceil(L / 16) per lane and four shuffle steps in the vector kernel), the reciprocal, the product (:65-68, :152-174)
The softmax and weighted-sum forms are those of tests/test_flash_attention_kernels.py.  |s_j - m| < 80 is asserted (no exponent
underflows), and every sum's bound is asserted to be below one average key's share (_sees_one_row).
The output with probs requested is bit-identical to the output without.  A row with len == 0 gives out = 0 and probs = 0 exactly
(the kernels used to divide by the zero sum there); that guard must not move a bit of any non-empty row:
test_decode_attention_bits_unchanged_by_empty_row_guard compares digests recorded from the kernels as they stood before it.

No output is compared through a rounding window (a reference re-rounded at both ends of a bound): a bf16 output takes
ulp(ref) + its fp32 bound directly, so no share of tie elements has to be capped.

ea_kv_append_reorder, ea_beam_mask_rows and ea_beam_topk are exact: data movement, single IEEE operations (the unk penalty, the
eos threshold eos_factor * max, lprobs + prev), comparisons.  They are compared bit for bit.

The first tests need no GPU: the reference against torch's softmax / topk / index_select in float64; six mutations that must land
outside the bounds (the neighbouring head, kv_row ignored, one key past len, koff and voff swapped, ties broken by the higher index,
the unk penalty applied after the maximum); every case of every GPU test built on the CPU with its preconditions asserted."""
import hashlib
import itertools
import math

import pytest
import torch

from tests import recurrent_ref as R
from tests.test_convmodule_kernels import _INT, _SENTINEL, DEV, Buf, _bits_input, _check, _check_bf16, _gen, _sees_one_row, _st, _sync, _ulp, inp, lib, out  # noqa: F401 (lib: the fixture)

gpu = pytest.mark.gpu
BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
E = R.E
INF = float("inf")
MAX_LENS = [1, 15, 16, 17, 33, 64, 65, 157]
LEN_SET = [1, 15, 16, 17, 31, 32, 33]
VARIANTS = {"vec16": (16, 0), "vec32": (32, 0), "vec64": (64, 0), "gen8": (8, 0), "gen24": (24, 0), "gen40": (40, 0), "gen64off": (64, 4)}
CONFIGS = "abc"
RATIOS = {}  # worst error / bound per kernel output so far, printed for the reader of the log (not a threshold)
KV_ROW = [0, 1, 2, 3, 4, 1, 0]


def _s16(i):
    return 16.0 ** (i % 3 - 1)


def _attn_case(variant, max_len, config, seed=0):
    """data, memory images (CPU tensors) and the fp64 reference of one decode-attention launch"""
    dh, off = VARIANTS[variant]
    N, H = {"a": (3, 3), "b": (2, 8), "c": (7, 3)}[config]
    C = H * dh
    g = _gen(1000 * max_len + 10 * dh + ord(config) + seed)
    kv_row = torch.tensor(KV_ROW, dtype=I32) if config == "c" else None
    rows = 5 if config == "c" else N
    Lmax = max_len + 3
    hsc = torch.tensor([_s16(h) for h in range(H)], dtype=F64).view(H, 1)
    csc = torch.tensor([_s16(c // 8) for c in range(dh)], dtype=F64).view(1, dh)
    vsc = torch.tensor([[_s16(h + c // 8) for c in range(dh)] for h in range(H)], dtype=F64)
    q = (torch.randn(N, H, dh, generator=g, dtype=F64) * 0.35 * hsc * csc).to(BF)
    K = torch.randn(rows, Lmax, H, dh, generator=g, dtype=F64) / (hsc * csc)
    V = torch.randn(rows, Lmax, H, dh, generator=g, dtype=F64) * vsc
    if config == "b":
        lens = None
    else:
        pool = [l for l in LEN_SET if l <= max_len] + [max_len]
        first = 4 * MAX_LENS.index(max_len) + (0 if config == "a" else 1)  # (a) and (c) together walk the pool, four draws per max_len
        lens = torch.tensor([pool[(first + max(r - 2, 0)) % len(pool)] for r in range(rows)], dtype=I32)
        lens[0], lens[1] = max_len, 0  # one full row, one empty row
        past = torch.arange(Lmax).view(1, Lmax, 1, 1) >= lens.view(rows, 1, 1, 1)
        K, V = torch.where(past, 64 * K, K), torch.where(past, 64 * V, V)
    K, V = K.to(BF), V.to(BF)
    ldq = C + 8 if config == "c" else C
    if config == "b":
        ldkv, koff, voff = C, 0, 0
        kimg, vimg = K.reshape(rows * Lmax, C), V.reshape(rows * Lmax, C)
    else:
        ldkv, koff, voff = 2 * C + 2 * off, off, C + off
        kimg = torch.full((rows * Lmax, ldkv), float("nan"), dtype=BF)
        kimg[:, koff:koff + C], kimg[:, voff:voff + C] = K.reshape(rows * Lmax, C), V.reshape(rows * Lmax, C)
        vimg = None
    qimg = torch.full((N, ldq), float("nan"), dtype=BF)
    qimg[:, :C] = q.reshape(N, C)
    ref = R.decode_attention(q, K, V, kv_row, lens, max_len)
    return dict(N=N, H=H, dh=dh, C=C, max_len=max_len, Lmax=Lmax, rows=rows, kv_row=kv_row, lens=lens, q=q, K=K, V=V, qimg=qimg, kimg=kimg,
                vimg=vimg, ldq=ldq, ldkv=ldkv, koff=koff, voff=voff, row_stride=Lmax * ldkv, ldp=max_len + 5, ref=ref,
                vector=(off == 0 and dh in (16, 32, 64)))


def _out_tol(ref):
    return _ulp(ref["out"]) + ref["tol_out"]


def _worst(got, ref, tol):
    return float(((got - ref).abs() / tol).max())


def _note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    print(f"{name}: worst error / bound {r:.3f} (so far {RATIOS[name]:.3f})")


# ------------------------------------------------------------------ CPU: the reference against torch, mutations, case construction
def test_reference_matches_torch_in_float64():
    g = _gen(5)
    N, H, dh, rows, Lmax, max_len = 5, 3, 8, 3, 12, 11
    q, K, V = (torch.randn(*s, generator=g, dtype=F64) for s in ((N, H, dh), (rows, Lmax, H, dh), (rows, Lmax, H, dh)))
    kv_row, lens = torch.tensor([0, 1, 2, 1, 0]), torch.tensor([11, 1, 7])
    ref = R.decode_attention(q, K, V, kv_row, lens, max_len)
    for n in range(N):
        r, L = int(kv_row[n]), int(lens[kv_row[n]])
        for h in range(H):
            p = torch.softmax(K[r, :L, h] @ q[n, h], 0)
            assert float((ref["probs"][n, h, :L] - p).abs().max()) <= 1e-11 and float(ref["probs"][n, h, L:].abs().sum()) == 0
            assert float((ref["out"][n, h] - p @ V[r, :L, h]).abs().max()) <= 1e-11 * float(V.abs().max())
    # topk (distinct values: no ties), gather, append
    lp, prev = torch.randn(2 * 4, 37, generator=g), torch.randn(2 * 4, generator=g)
    sc, tok, bm = R.beam_topk(lp, prev, 2, 4, 3, 37, 8)
    for s in range(2):
        v, i = torch.topk((lp.view(2, 4, 37)[s, :3] + prev.view(2, 4, 1)[s, :3]).reshape(-1), 8)
        assert torch.equal(sc[s], v) and torch.equal(tok[s].long(), i % 37) and torch.equal(bm[s].long(), i // 37)
    x, par = torch.randn(6, 7, generator=g), torch.tensor([5, 0, 0, 3, 2, 2])
    assert torch.equal(R.gather_rows(x, par), x.index_select(0, par))
    old, new, new0 = torch.randn(6, 9, 8, generator=g), torch.randn(6, 8, generator=g), torch.zeros(6, 9, 8)
    got = R.kv_append_reorder(old, new, par, 4, new0)
    assert torch.equal(got[:, :5], torch.cat([old.index_select(0, par)[:, :4], new[:, None]], 1)) and float(got[:, 5:].abs().max()) == 0
    # the row rules against a scalar restatement
    lp = torch.randn(3, 9, generator=g)
    lp[1, 4] = float("nan")
    got = R.beam_mask_rows(lp, 1, 3, 2, 0.5, 0, 0, 1.5, 1)
    for r in range(3):
        row = [(-INF if (v != v or c == 1) else v) for c, v in enumerate(lp[r].tolist())]
        row[3] = float(torch.tensor(row[3]) - torch.tensor(0.5))
        mx = max(row)
        if torch.tensor(row[2]) < torch.tensor(1.5) * torch.tensor(mx):
            row[2] = -INF
        assert got[r].tolist() == row


def test_mutations_land_outside_the_bounds():
    """each planted fault moves some element of a correct result by at least 8 times its tolerance (or, for the exact kernels,
    changes it)"""
    c = _attn_case("vec64", 33, "c")
    ref, tol = c["ref"], _out_tol(c["ref"])
    q, K, V, kv_row, lens, ml = c["q"], c["K"], c["V"], c["kv_row"], c["lens"], c["max_len"]
    muts = {
        "the neighbouring head": R.decode_attention(q.roll(1, 1), K, V, kv_row, lens, ml),
        "kv_row ignored": R.decode_attention(q, K[[0, 1, 2, 3, 4, 0, 1]], V[[0, 1, 2, 3, 4, 0, 1]], None, lens[[0, 1, 2, 3, 4, 0, 1]], ml),
        "one key past len": R.decode_attention(q, K, V, kv_row, (lens + 1).clamp(max=ml), ml),
        "koff and voff swapped": R.decode_attention(q, V, K, kv_row, lens, ml),
    }
    for name, m in muts.items():
        assert _worst(m["out"], ref["out"], tol) >= 8, name
    assert _worst(ref["out"], ref["out"], tol) == 0
    # ties: quantised scores, the higher flat index must change a token or a beam
    lp, prev = _topk_data(3, 4, 37, 0)
    lo, hi = R.beam_topk(lp, prev, 3, 4, 4, 37, 8), R.beam_topk(lp, prev, 3, 4, 4, 37, 8, lower_index_wins=False)
    assert torch.equal(lo[0], hi[0]) and not (torch.equal(lo[1], hi[1]) and torch.equal(lo[2], hi[2]))
    # the unk penalty applied after the maximum: unk holds the row maximum, eos sits between the two thresholds
    lp = torch.full((1, 9), -5.0)
    lp[0, 3], lp[0, 2], lp[0, 5] = -0.1, -0.9, -1.0
    good = R.beam_mask_rows(lp, 1, 3, 2, 2.0, 0, 0, 1.5, 1)  # max after the penalty: -0.9 (eos itself): kept
    bad = R.beam_mask_rows(lp, 1, 3, 2, 0.0, 0, 0, 1.5, 1)  # max before: -0.1 -> threshold -0.15: eos masked
    bad[0, 3] -= 2.0
    assert float(good[0, 2]) == pytest.approx(-0.9) and float(bad[0, 2]) == -INF and not torch.equal(good, bad)


def test_every_gpu_case_builds_on_the_cpu_with_its_preconditions():
    seen = {v: set() for v in VARIANTS}
    for variant, ml, cfg in itertools.product(VARIANTS, MAX_LENS, CONFIGS):
        c = _attn_case(variant, ml, cfg)
        ref = c["ref"]
        assert ref["max_arg"] < 80, (variant, ml, cfg)
        assert c["vector"] == (variant.startswith("vec")) and (c["ldq"] | c["row_stride"] | c["ldkv"]) % 8 == 0
        assert bool(torch.isfinite(ref["out"]).all()) and bool(torch.isfinite(ref["probs"]).all())
        _sees_one_row("out", ref["tol_out"], ref["out_mag"], ml)
        if c["lens"] is not None:
            seen[variant].update(int(l) for l in c["lens"])
            assert int(c["lens"].max()) <= ml  # the kernels size their LDS rows by max_len
            empty = ref["L"] == 0
            assert bool(empty.any()) and float(ref["out"][empty].abs().max()) == 0 and float(ref["probs"][empty].abs().max()) == 0
        # the neighbouring head, as the scales are meant to show it
        if ml > 1:
            m = R.decode_attention(c["q"].roll(1, 1), c["K"], c["V"], c["kv_row"], c["lens"], ml)
            assert _worst(m["out"], ref["out"], _out_tol(ref)) >= 8, (variant, ml, cfg)
    assert all(s >= set(LEN_SET) | {0} | set(MAX_LENS) for s in seen.values())
    for shape in TOPK_SHAPES:
        for mode in range(3):
            lp, prev = _topk_data(*shape[:3], mode)
            sc, tok, bm = R.beam_topk(lp, prev, shape[0], shape[1], shape[1], shape[2], shape[3])
            assert bool((sc[:, :-1] >= sc[:, 1:]).all())
            if mode == 0:  # exact ties among the winners: within a stride of 256, between neighbours, across beams
                flat = (bm.long() * shape[2] + tok.long())
                tie = (sc[:, 1:] == sc[:, :-1]) & (sc[:, 1:] > -INF)
                assert bool((flat[:, 1:][tie] > flat[:, :-1][tie]).all())
                if shape[2] * shape[1] > 600:
                    assert bool(tie.any())
                if shape == TOPK_SHAPES[-1]:  # ties of every kind among the winners of one sentence
                    top = flat[0][sc[0] == sc[0, 0]]
                    diff = (top.view(-1, 1) - top.view(1, -1))[torch.triu(torch.ones(len(top), len(top)), 1).bool()]
                    beams = (top // shape[2]).unique()
                    assert bool((diff % 256 == 0).any()), "no tie inside one thread's stride"
                    assert bool((diff % 256 != 0).any()), "no tie between two threads"
                    assert len(beams) > 1, "no tie across beams"
            if mode == 2:
                assert bool((sc == -INF).any())
    for V in MASK_V:
        lp, pad, unk, eos = _mask_data(V)
        if V > 600:
            assert len({pad // 256, unk // 256, eos // 256}) == 3 and min(pad, unk, eos) >= 256
        assert bool(torch.isnan(lp).any())
        # the eos threshold sees both sides: kept at the maximum and above eos_factor * max, masked below it
        want = R.beam_mask_rows(lp, pad, unk, eos, 0.5, 0, 0, 1.5, 1)
        assert float(want[0, eos]) == -0.25 and float(want[1, eos]) == -0.125 and float(want[2, eos]) == -INF and float(want[4, eos]) == -0.1875
        assert float(R.beam_mask_rows(lp, pad, -1, eos, 0.0, 0, 0, 1.5, 1)[4, eos]) == -INF  # (without the penalty unk's -0.05 masks eos)


# ------------------------------------------------------------------ GPU: decode attention
def _pitched_out(rows, W, ld, dtype):
    b = out((rows, ld), dtype)
    b.t.view(_INT[dtype])[:, W:] = _SENTINEL[dtype]
    return b


def _gap_intact(b, W):
    return b.intact() and bool((b.t.view(_INT[b.dtype])[:, W:] == _SENTINEL[b.dtype]).all())


def _launch_attn(lib, c, want_probs, bufs=None):
    N, H, dh, C, ml = c["N"], c["H"], c["dh"], c["C"], c["max_len"]
    if bufs is None:
        bk = inp(c["kimg"])
        bufs = dict(q=inp(c["qimg"]), k=bk, v=bk if c["vimg"] is None else inp(c["vimg"]),
                    kv_row=None if c["kv_row"] is None else c["kv_row"].to(DEV), lens=None if c["lens"] is None else c["lens"].to(DEV))
    bo = _pitched_out(N, C, c["ldq"], BF)
    bp = _pitched_out(N * H, ml, c["ldp"], F32) if want_probs else None
    ptr = lambda t: None if t is None else t.data_ptr()
    args = (bufs["q"].p, bufs["k"].p, bufs["v"].p, ptr(bufs["kv_row"]), ptr(bufs["lens"]), bo.p, N, H, dh, c["ldq"], c["row_stride"], c["ldkv"],
            c["koff"], c["voff"], ml)
    if want_probs:
        rc = lib.ea_decode_attention_probs(*args, bp.p, c["ldp"], _st())
    else:
        rc = lib.ea_decode_attention(*args, _st())
    assert rc == 0
    _sync()
    assert _gap_intact(bo, C) and (bp is None or _gap_intact(bp, ml))
    return bo, bp, bufs


def _check_attn(tag, c, bo, bp):
    N, H, dh, C, ml, ref = c["N"], c["H"], c["dh"], c["C"], c["max_len"], c["ref"]
    got = bo.cpu()[:, :C].reshape(N, H, dh)
    _check_bf16(tag + " out", got, ref["out"], ref["tol_out"])
    kern = "vec" if c.get("vector", c["dh"] in (16, 32, 64) and c["koff"] % 8 == 0) else "generic"
    _note(kern + " out", _worst(got.double(), ref["out"], _out_tol(ref)))
    empty = ref["L"] == 0
    assert bool((bo.bits()[:, :C].reshape(N, H, dh)[empty] == 0).all()), "an empty row's output is not +0"
    if bp is not None:
        probs = bp.cpu()[:, :ml].reshape(N, H, ml)
        _check(tag + " probs", probs, ref["probs"], ref["tol_probs"])
        _note(kern + " probs", _worst(probs.double(), ref["probs"], ref["tol_probs"].clamp_min(2.0 ** -140)))
        past = torch.arange(ml).view(1, 1, ml) >= ref["L"].view(N, 1, 1)
        assert bool((bp.bits()[:, :ml].reshape(N, H, ml)[past.expand(N, H, ml)] == 0).all()), "probs from len to max_len are not +0"


@gpu
@pytest.mark.parametrize("max_len", MAX_LENS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_decode_attention(lib, variant, max_len):
    for cfg in CONFIGS:
        c = _attn_case(variant, max_len, cfg)
        tag = f"{variant} L{max_len} {cfg}"
        bo, _, bufs = _launch_attn(lib, c, False)
        _check_attn(tag, c, bo, None)
        bo2, bp, _ = _launch_attn(lib, c, True, bufs)
        _check_attn(tag + " +probs", c, bo2, bp)
        assert torch.equal(bo.bits(), bo2.bits()), "the output changes when probs are requested"


def _digest_case(lib, variant):
    """(digest of out, digest of probs) over the NON-EMPTY rows of one launch on data made by integer arithmetic alone"""
    dh, off = VARIANTS[variant]
    N, H, ml = 3, 3, 33
    C, Lmax = H * dh, 36
    lens = torch.tensor([33, 0, 17], dtype=I32)
    q = (_bits_input(N * C, 3).double() / 16).to(BF).view(N, H, dh)
    K, V = _bits_input(N * Lmax * C, 4).view(N, Lmax, H, dh), _bits_input(N * Lmax * C, 5).view(N, Lmax, H, dh)
    ldkv, koff, voff = 2 * C + 2 * off, off, C + off
    kimg = torch.zeros(N * Lmax, ldkv, dtype=BF)
    kimg[:, koff:koff + C], kimg[:, voff:voff + C] = K.reshape(-1, C), V.reshape(-1, C)
    c = dict(N=N, H=H, dh=dh, C=C, max_len=ml, kv_row=None, lens=lens, qimg=q.reshape(N, C), kimg=kimg, vimg=None, ldq=C, ldkv=ldkv, koff=koff,
             voff=voff, row_stride=Lmax * ldkv, ldp=ml + 5, ref=R.decode_attention(q, K, V, None, lens, ml))
    bo, bp, _ = _launch_attn(lib, c, True)
    keep = torch.tensor([0, 2])
    o = bo.bits()[:, :C][keep].contiguous()
    p = bp.bits()[:, :ml].reshape(N, H, ml)[keep].contiguous()
    return c, bo, bp, hashlib.sha256(o.numpy().tobytes()).hexdigest(), hashlib.sha256(p.numpy().tobytes()).hexdigest()


# sha256 of out / probs of the rows with len > 0 in _digest_case, recorded from the kernels as they stood BEFORE the empty-row guard
# (`sum > 0 ? ... : 0`) went into decode_attention_kernel and decode_attention_vec_kernel: a non-empty row must not move a bit.
_PARENT_DIGESTS = {
    "vec64": ("36b11ee75f66fa68345813ccd8e3aa9a4dd98d3d22a429357e58607f0a193684", "be367adebbc44ea82cb7e4114c5e50da35552af76023b2a81e3d4ea870026010"),
    "vec16": ("55e093fdbb476ff55b452f5a467153acfa32d31497358671dd51d99b5619533d", "7182ecd20872f437760d3bfdd8065545c98b98025dbff5b8b63762931960668e"),
    "gen24": ("c61b7a5480a1ce6fc223a06b7c6e6755a420d11b53e72f8a647e1a3422f35f46", "23fc14370121310739bbcd578493d777420ccddef5e79fc1476076058c638f4c"),
    "gen64off": ("36b11ee75f66fa68345813ccd8e3aa9a4dd98d3d22a429357e58607f0a193684", "4cdec1be3ebfa88d9aa5a9decfd8c590054611601afb08690ba3760eeabc5d6f"),
}


@gpu
@pytest.mark.parametrize("variant", list(_PARENT_DIGESTS))
def test_decode_attention_bits_unchanged_by_empty_row_guard(lib, variant):
    c, bo, bp, d_out, d_probs = _digest_case(lib, variant)
    print(f"{variant}: out sha256 {d_out} probs sha256 {d_probs}")
    _check_attn(variant + " digest case", c, bo, bp)  # (and the empty row between them is exactly 0)
    inexact = c["ref"]["out"].float().double() != c["ref"]["out"]
    assert int(inexact.sum()) > inexact.numel() // 4  # the digest belongs to this kernel's arithmetic, not to an exact result
    assert (d_out, d_probs) == _PARENT_DIGESTS[variant]


@gpu
def test_decode_attention_return_codes(lib):
    """dh > 64, max_len <= 0, ldp < max_len: -2; LDS overflow (max_len > 4096): -3; N = 0: 0.  Nothing is written."""
    c = _attn_case("vec64", 17, "a")
    bq, bk = inp(c["qimg"]), inp(c["kimg"])
    lens = c["lens"].to(DEV)
    for (n, dh, ml, ldp, want) in ((3, 65, 17, 22, -2), (3, 64, 0, 22, -2), (3, 64, -1, 22, -2), (3, 64, 17, 16, -2), (3, 64, 4097, 4100, -3),
                                   (0, 64, 17, 22, 0)):
        bo, bp = out((3, c["ldq"]), BF), out((9, 22), F32)
        rc = lib.ea_decode_attention_probs(bq.p, bk.p, bk.p, None, lens.data_ptr(), bo.p, n, 3, dh, c["ldq"], c["row_stride"], c["ldkv"], 0,
                                           c["C"], ml, bp.p, ldp, _st())
        assert rc == want, (n, dh, ml, ldp, rc)
        if ldp >= ml:
            assert lib.ea_decode_attention(bq.p, bk.p, bk.p, None, lens.data_ptr(), bo.p, n, 3, dh, c["ldq"], c["row_stride"], c["ldkv"], 0,
                                           c["C"], ml, _st()) == want
        _sync()
        assert bo.untouched() and bp.untouched()


# ------------------------------------------------------------------ GPU: cache append + reorder
def _bf_bits(t):
    return t.view(torch.int16)


@gpu
@pytest.mark.parametrize("L,W", [(0, 8), (1, 8), (37, 8), (0, 1024), (1, 1024), (37, 1024), (130, 1024)])
def test_kv_append_reorder(lib, L, W):
    """bit for bit; L = 130, W = 1024: (L + 1) W / 8 = 16768 > 64 * 256 chunks, the capped grid makes a second trip"""
    N, Lmax = (2, L + 2) if L == 130 else (5, L + 3)
    assert L != 130 or (L + 1) * W // 8 > 64 * 256
    g = _gen(L * 7 + W)
    old = torch.randn(N, Lmax, W, generator=g).to(BF)
    old[:, L:] = float("nan")  # never copied
    new, new0 = torch.randn(N, W, generator=g).to(BF), torch.randn(N, Lmax, W, generator=g).to(BF)
    for parent in (None, torch.tensor(([1, 1] if N == 2 else [4, 0, 0, 2, 4]), dtype=I32)):
        bold, bnew = inp(old.view(N * Lmax, W)), inp(new)
        bc = out((N * Lmax, W), BF, new0.view(N * Lmax, W))
        par = None if parent is None else parent.to(DEV)
        assert lib.ea_kv_append_reorder(bold.p, bc.p, bnew.p, None if par is None else par.data_ptr(), N, L, Lmax, W, _st()) == 0
        _sync()
        assert bc.intact()
        want = R.kv_append_reorder(old, new, parent, L, new0)
        assert torch.equal(bc.bits().view(N, Lmax, W), _bf_bits(want)), (L, W, parent)


@gpu
def test_kv_append_reorder_return_codes(lib):
    g = _gen(3)
    old, new = inp(torch.randn(2 * 4, 16, generator=g).to(BF)), inp(torch.randn(2, 16, generator=g).to(BF))
    for (n, L, Lmax, W, want) in ((2, 1, 4, 12, -2), (2, 4, 4, 16, -2), (0, 1, 4, 16, 0)):
        bc = out((2 * 4, 16), BF)
        assert lib.ea_kv_append_reorder(old.p, bc.p, new.p, None, n, L, Lmax, W, _st()) == want, (n, L, Lmax, W)
        _sync()
        assert bc.untouched()


# ------------------------------------------------------------------ GPU: the row rules
MASK_V = [5, 256, 257, 1000]


def _mask_data(V):
    """six rows: the maximum at eos; elsewhere with eos above the eos_factor threshold; elsewhere with eos below it; NaN at eos;
    unk holding the maximum before the penalty; NaN scattered.  eos, pad, unk sit in different 256-strides where V allows."""
    pad, unk, eos = (300, 513, 800) if V > 800 else (1, 3, 2)
    g = _gen(V)
    lp = -0.5 - 3 * torch.rand(6, V, generator=g)
    other = 4 if V <= 5 else V - 2
    lp[0, eos] = -0.25
    lp[1, other], lp[1, eos] = -0.1, -0.125
    lp[2, other], lp[2, eos] = -0.1, -0.3
    lp[3, eos] = float("nan")
    lp[4, unk], lp[4, eos] = -0.05, -0.1875
    lp[5, torch.arange(0, V, 3)] = float("nan")
    return lp, pad, unk, eos


@gpu
@pytest.mark.parametrize("V", MASK_V)
def test_beam_mask_rows(lib, V):
    """every rule alone and in every combination, bit for bit, in place"""
    lp, pad, unk, eos = _mask_data(V)
    for pen, only_eos, forbid, use_f, with_pad in itertools.product((0.0, 0.5), (0, 1), (0, 1), (0, 1), (0, 1)):
        p_, u_ = (pad if with_pad else -1), (unk if pen else -1)
        b = out((6, V), F32, lp)
        assert lib.ea_beam_mask_rows(b.p, 6, V, p_, u_, eos, pen, only_eos, forbid, 1.5, use_f, _st()) == 0
        _sync()
        assert b.intact()
        want = R.beam_mask_rows(lp, p_, u_, eos, pen, only_eos, forbid, 1.5, use_f)
        assert not bool(torch.isnan(want).any())
        assert torch.equal(b.bits(), want.view(I32)), (V, pen, only_eos, forbid, use_f, with_pad)
    assert lib.ea_beam_mask_rows(None, 0, V, pad, unk, eos, 0.5, 0, 0, 1.5, 1, _st()) == 0


# ------------------------------------------------------------------ GPU: top-k over beam * V
TOPK_SHAPES = [(1, 1, 5, 2), (3, 4, 37, 8), (2, 5, 1000, 10), (1, 64, 300, 128)]


def _topk_data(bsz, beam, V, mode):
    """mode 0: scores on a grid of 0.25 (exact sums, many exact ties at every distance); 1: real-valued (the fp32 addition rounds);
    2: the grid with all but one entry of every sentence at -inf (fewer than k candidates)"""
    g = _gen(bsz * 1000 + beam * 10 + V + mode)
    if mode == 1:
        return torch.randn(bsz * beam, V, generator=g), torch.randn(bsz * beam, generator=g)
    lp = -0.25 * torch.randint(0, 12, (bsz * beam, V), generator=g).float()
    prev = -0.5 * torch.randint(0, 3, (bsz * beam,), generator=g).float()
    if mode == 2:
        keep = lp[:, V // 2].clone()
        lp[:] = -INF
        lp[::beam, V // 2] = keep[::beam]
    return lp, prev


@gpu
@pytest.mark.parametrize("shape", TOPK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_beam_topk(lib, shape):
    bsz, beam, V, k = shape
    for mode, with_prev, used in itertools.product(range(3), (True, False), sorted({beam, max(1, beam - 1)})):
        lp, prev = _topk_data(bsz, beam, V, mode)
        if used * V < 1:
            continue
        blp, bprev = inp(lp), inp(prev)
        bs, bt, bb = out((bsz * k,), F32), out((bsz * k,), F32), out((bsz * k,), F32)  # (tokens and beams: int32 in an fp32 Buf)
        assert lib.ea_beam_topk(blp.p, bprev.p if with_prev else None, bsz, beam, used, V, k, bs.p, bt.p, bb.p, _st()) == 0
        _sync()
        assert bs.intact() and bt.intact() and bb.intact()
        sc, tok, bm = R.beam_topk(lp, prev if with_prev else None, bsz, beam, used, V, k)
        tag = (shape, mode, with_prev, used)
        assert torch.equal(bs.bits().view(bsz, k), sc.view(I32)), tag
        assert torch.equal(bt.bits().view(bsz, k), tok), tag
        assert torch.equal(bb.bits().view(bsz, k), bm), tag


@gpu
def test_beam_topk_return_codes(lib):
    lp, prev = _topk_data(1, 2, 300, 0)
    blp, bprev = inp(lp), inp(prev)
    for (bsz, k, want) in ((1, 129, -2), (1, 0, -2), (0, 8, 0)):
        bs, bt, bb = out((130,), F32), out((130,), F32), out((130,), F32)
        assert lib.ea_beam_topk(blp.p, bprev.p, bsz, 2, 2, 300, k, bs.p, bt.p, bb.p, _st()) == want
        _sync()
        assert bs.untouched() and bt.untouched() and bb.untouched()
