"""The recurrent kernels (espresso_amd/csrc/lstm.hip: LSTM cell forward / backward, row gather, Bahdanau attention forward /
backward; espresso_amd/csrc/lstm_seq.hip: the persistent forward and backward recurrences) one launch at a time against the plain
fp64 restatement in tests/recurrent_ref.py, through the C ABI, every element of every output.

BUFFERS (tests/test_convmodule_kernels.py's Buf).  Every floating-point device tensor is a view into a larger allocation with
guards on both sides: NaN around inputs, a sentinel bit pattern around outputs (checked after the call).  An output starts as NaN
(a missed store fails) or as known non-zero data where the call accumulates (dkey_acc, dvalue_acc, dnv_acc, dbias_acc).  Every
pitch (ldg, ldh, ld_dh, lddg, ldc, ldd) is 8 wider than the dense row: the gap holds NaN on input and the sentinel on output,
checked after the call.  Row flags (keep_row, frozen) sit between guards of 0xff.  An output whose pointer is NULL is simply not
there: every other buffer of the call is compared in full, so a stray store through one of them fails.

DATA.  Gate pre-activations carry the offsets (0.5, 1.0, -0.3, -0.7) for (i, f, g, o), a pattern in the unit and in the row, and in
the first eight rows the values +-1e-4, +-30, +-100 in every gate (the saturation branches; nothing may become inf / inf).  Cell
states and gradients are drawn with a scale per row, lengths differ per row, keys / values / accumulators per sentence.

DISPATCH.  lstm_cell_*: one kernel each; B = 520, H = 1024 makes the grid-stride loop's second trip (B H > 2048 * 256).
lstm_seq_fwd_kernel<KS, MT, NG> and lstm_seq_bwd_kernel<KS, NG> (lstm_seq.hip:317-340): KS = H / 32 for H in {256, 320, 512, 640, 768,
800, 1024}, NG = 1 / 2 / 4 batch groups — 21 + 21 instantiations, each reached by a case of SEQ_CASES: NG = 2 at B = 17 for every H;
H = 256 and 800 at B = 1, 5, 16 (NG = 1), 33 (three groups on the four-group kernel), 64 (NG = 4); the other H at B = 3 (NG = 1) and
B = 49 (NG = 4).  Every case runs SEQ_COMBOS: both directions, h0 / c0 present / absent (also one alone), frozen (with
frozen_out_zero = 1 and the zero initial state: the contract, lstm_seq.hip header; frozen with frozen_out_zero = 0 is outside it
and not tested), dhs / dh_last / dc_last and dh0 / dc0 present / absent.

BOUNDS.  Derived from the arithmetic, none measured.  E = 2^-23 per fp32 rounding and per v_rcp_f32; TINY = 2^-126 where a result
underflows; ulp(x) = the bf16 step at |x| (every bf16 output: ulp(ref) + the fp32 bound, _check_bf16); s = sigmoid, t = tanh.
  sigmoid_f (lstm.hip:15)   RELATIVE ((1 + |x|)(1 - s) + 1.5) E: __expf(-x) as tests/test_gemm_kernels.py charges it (v_exp_f32 1 ulp, the
           two roundings of its argument |x| E of the result), damped by 1 - s through 1 / (1 + e); the addition and the division.
           At x = -100 exp overflows, the kernel gives 0 for 3.7e-44: TINY.
  tanh_f (lstm.hip:16-20, lstm_seq.hip:24-27)   1 - 2 / (e + 1), e = __expf(2x):
           E ((1 - t) ((1 + 2|x|)(1 + t) / 2 + 2) + |t|) — e is off by (1 + 2|x|) E of itself, which moves q = 2 / (e + 1) = 1 - t by
           e / (e + 1) = (1 + t) / 2 of that; the addition and the division add 2 E q; the subtraction rounds by E |t|.  ABSOLUTE near
           0 (2.5 E: a relative error of 3e-3 at |x| = 1e-4), relative to 1 - t in the positive tail up to the last rounding E |t|,
           4 E in the negative tail where q -> 2.  An argument off by d moves it by (1 - t^2 + 2 d) d.
  cell forward (lstm.hip:31-46)
    act    the two bounds above at the pre-activation
    c      |c_prev| tol_f + i tol_g + |g| tol_i + 2 E (|f c_prev| + |i g|)       two products and the addition
    h      o (tanh_f's bound at c, moved by tol_c) + |t(c)| tol_o + E |h|;  frozen rows: c = c_prev, h = h_prev or 0, exact
  cell backward (lstm.hip:59-77)
    dh     E (|dh_a| + |dh_b|)
    dc     tol_dc_in + go (1 - t^2) tol_dh + |dh| go (2 |t| tol_t + 2 E) + 2 E |term| + E (|dc_in| + |term|), term = dh o (1 - t^2)
    dG_i,f tol_dc |k| + 5 E |dG| (k = the factor of dc: three products and 1 - s);  dG_g: tol_dc |k| + |dc| i E + 3 E |dG| (1 - g^2 is
           off by E absolutely);  dG_o: tol_dh |k| + |dh| o (1 - o) tol_t + 5 E |dG|;  dc_prev: tol_dc f + E |dc_prev|
           frozen rows: dG = 0 and dc_prev = dc_in (0 without it), exact
  sequence forward, one step (lstm_seq.hip:104-147), on the kernel's own stored hs[prev] and cs[prev]:
    pre    (H + 1) E (|gx| + sum_k |w h|)      the fp32 MFMA sum of H bf16 products (tests/test_gemm_kernels.py: K additions, at most
           one rounding per product added) and the addition of gx; then the cell's bounds with the activations moved by that.
           It does not compound over the steps.
  sequence backward, one step (lstm_seq.hip:212-254), the recurrent term from the kernel's own stored dG of the step before:
    dh     (H + 4) E (|dhs| + sum_k |w dG|)    four per-gate MFMA sums of H products, three additions in LDS order, one onto dhs
    dc is carried in registers and never stored: the reference carries it in fp64 and its bound grows by one step's share per
    step, tol_dc[n] = tol_dc_prev[n+1] + (this step's dc terms above), tol_dc_prev = tol_dc f + E |dc_prev|.  For U = 3 walked
    n = 2, 1, 0:  tol_dc[2] = D2 (+ E |dc_last|),  tol_dc[1] = f2 tol_dc[2] + E |dc f2| + D1,  tol_dc[0] = f1 tol_dc[1] + E |dc f1| + D0,
    tol_dc0 = f0 tol_dc[0] + E |dc0|, Dn = the dc line of the cell backward at step n.  dh0: (H + 3) E sum_k |w dG|.
  Bahdanau forward (lstm.hip:108-141)
    score  sum_a |nv| (tanh_f at x, x off by 2 E (|qp| + |key| + |bias|)) + (ceil(A / 64) + 7) E sum_a |nv th|
    p      p (rel_e + rel_sum + 2 E), rel_e = 2 max_t tol_s + (2 |s - m| + 1) E, rel_sum = sum_t p rel_e + (ceil(T / 256) + 10) E
           (the forms of tests/test_flash_attention_kernels.py); exactly 0 from min(len, T) on, and for len = 0
    ctx    ulp(ref) + sum_t tol_p |v| + (L + 1) E sum_t p |v|
  Bahdanau backward (lstm.hip:161-207)
    dp (ceil(Cv / 64) + 6) E sum |dctx v|;  dot: sum p tol_dp + (ceil(T / 256) + 11) E sum p |dp|;  ds: p (tol_dp + tol_dot) + 2 E p (|dp| + |dot|)
    dvalue_acc  2 E (|pre-fill| + |p dctx|);  dkey_acc  tol_dpre + E (|pre-fill| + |dpre|),
    dpre = ds nv (1 - th^2): tol_ds |nv| (1 - th^2) + |ds nv| (2 |th| tol_th + 2 E) + 3 E |dpre|;  rows t >= len keep the pre-fill bit for bit
    dqp    ulp(ref) + sum_t tol_dpre + (ceil(L / 4) + 3) E sum_t |dpre|
    dnv_acc, dbias_acc   chain form of tests/test_layernorm_kernels.py: sum_b (the row's own bound) + B E (|pre-fill| + sum_b |row|):
           B atomic additions in any order; asserted with _sees_one_row to stay below one row's share
ea_gather_rows is data movement: bit for bit.  No output is compared through a rounding window (a reference re-rounded at both
ends of a bound): a bf16 output takes ulp(ref) + its fp32 bound directly, so no share of tie elements has to be capped.

The first tests need no GPU: the reference in float64 against torch.nn.LSTMCell, torch.nn.LSTM on packed ragged sequences in both
directions, and autograd (1e-11 relative); eleven mutations that must land outside the bounds; every GPU case built on the CPU with
the preconditions of its bounds asserted."""
import itertools
import math

import pytest
import torch

from tests import recurrent_ref as R
from tests.test_convmodule_kernels import _INT, _SENTINEL, DEV, Buf, _check, _check_bf16, _gen, _sees_one_row, _st, _sync, _ulp, inp, lib, out  # noqa: F401 (lib: the fixture)
from tests.test_decode_kernels import _gap_intact, _pitched_out

gpu = pytest.mark.gpu
BF, F32, F64, I32, U8 = torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.uint8
E = R.E
PAD = 8  # every pitch is this much wider than the dense row
SPECIALS = [1e-4, -1e-4, 30.0, -30.0, 100.0, -100.0]
GATE_OFF = torch.tensor([0.5, 1.0, -0.3, -0.7])
RATIOS = {}  # worst error / bound per kernel output so far, printed for the reader of the log (not a threshold)


def _ratio(name, got, ref, tol):
    got = R.f64(got)
    r = float(((got - ref).abs() / tol.expand_as(ref).clamp_min(2.0 ** -140)).max()) if ref.numel() else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    print(f"{name}: worst error / bound {r:.3f} (so far {RATIOS[name]:.3f})")


def _chk(name, got, ref, tol):
    _ratio(name, got, ref, tol)
    _check(name, got, ref, tol)


def _chk_bf16(name, got, ref, extra):
    _ratio(name, got, ref, _ulp(ref) + extra)
    _check_bf16(name, got, ref, extra)


def _moved(mut, ref, tol):
    """some element moved by at least 8 times its tolerance"""
    d = (R.f64(mut) - ref).abs()
    return bool(((d >= 8 * tol) & (d > 0)).any())


def _pitched_in(data, ld):
    img = torch.full((data.shape[0], ld), float("nan"), dtype=data.dtype)
    img[:, :data.shape[1]] = data
    return inp(img)


def _flags(t):
    """uint8 row flags between guards of 0xff"""
    full = torch.full((t.numel() + 256,), 255, dtype=U8, device=DEV)
    full[128:128 + t.numel()] = t.reshape(-1).to(U8)
    return full[128:128 + t.numel()]


def _p(b):
    return None if b is None else (b.data_ptr() if isinstance(b, torch.Tensor) else b.p)


def _rowscale(B):
    return torch.tensor([0.5 * 4.0 ** ((0.618 * b) % 1.0) for b in range(B)]).view(B, 1)


# ------------------------------------------------------------------ cases (built on the CPU; the GPU tests launch them)
CELL_SHAPES = [(1, 64), (5, 48), (3, 321), (17, 1024), (520, 1024)]
#               c_prev h_f32 h_bf16 act keep h_prev frozen_out_zero
FWD_CONFIGS = [(1, 1, 1, 1, 1, 1, 0), (1, 1, 1, 1, 1, 1, 1), (0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0), (0, 0, 1, 1, 1, 0, 1), (1, 0, 1, 0, 1, 0, 0),
               (0, 1, 0, 1, 0, 0, 0)]
#               dh_a dh_b dc_in c_prev frozen
BWD_CONFIGS = [(1, 1, 1, 1, 1), (1, 0, 0, 0, 0), (0, 1, 1, 1, 0), (1, 0, 0, 1, 1), (0, 1, 0, 0, 1), (0, 0, 1, 1, 0)]


def _gates(B, H, g):
    G = GATE_OFF.view(1, 4, 1) + 0.9 * torch.randn(B, 4, H, generator=g) + 0.25 * torch.sin(torch.arange(H).float()).view(1, 1, H) \
        + 0.2 * torch.cos(torch.arange(B).float()).view(B, 1, 1)
    for b in range(min(B, 8)):
        for gate in range(4):
            for i, s in enumerate(SPECIALS):
                G[b, gate, (b + gate + 7 * i) % H] = s
    return G.reshape(B, 4 * H)


def _cell_case(B, H):
    g = _gen(B * 10000 + H)
    G = _gates(B, H, g)
    rs = _rowscale(B)
    d = dict(B=B, H=H, G=G, c_prev=torch.randn(B, H, generator=g) * rs, h_prev=torch.randn(B, H, generator=g),
             keep=(torch.arange(B) % 3 == 1).to(U8), dh_a=(torch.randn(B, H, generator=g) * rs).to(BF), dh_b=torch.randn(B, H, generator=g) * rs,
             dc_in=torch.randn(B, H, generator=g) * rs)
    f = R.lstm_cell_fwd(G, d["c_prev"])
    d["act"], d["c"] = f["act"].float(), f["c"].float()
    return d


def _cell_fwd_ref(d, cfg):
    cp, _, _, _, keep, hp, fz0 = cfg
    return R.lstm_cell_fwd(d["G"], d["c_prev"] if cp else None, d["keep"] if keep else None, d["h_prev"] if hp else None, fz0)


def _cell_bwd_ref(d, cfg):
    a, b, dc, cp, fz = cfg
    return R.lstm_cell_bwd(d["dh_a"] if a else None, d["dh_b"] if b else None, d["dc_in"] if dc else None, d["act"], d["c_prev"] if cp else None,
                           d["c"], d["keep"] if fz else None)


HS = [256, 320, 512, 640, 768, 800, 1024]
SEQ_CASES = [(H, 17, 3) for H in HS] + [(H, B, 3) for H in (256, 800) for B in (1, 5, 16, 33, 64)] + \
            [(H, B, 3) for H in (320, 512, 640, 768, 1024) for B in (3, 49)] + [(256, 5, 1)]
#             reverse h0 c0 frozen | dhs dh_last dc_last dh0 dc0
SEQ_COMBOS = [(0, 0, 0, 0, 1, 1, 1, 1, 1), (1, 0, 0, 0, 1, 0, 0, 0, 0), (0, 1, 1, 0, 0, 1, 1, 1, 0), (1, 1, 1, 0, 1, 1, 0, 0, 1), (0, 0, 0, 1, 1, 1, 1, 1, 1),
              (1, 0, 0, 1, 1, 0, 1, 1, 1), (0, 1, 0, 0, 0, 0, 1, 0, 0), (1, 0, 1, 0, 0, 1, 0, 1, 1)]
GATE_W = torch.tensor([1.0, 0.5, 2.0, 1.0])


def _seq_case(H, B, U):
    g = _gen(H * 100 + B + 7 * U)
    w_hh = (torch.randn(4, H, H, generator=g) * GATE_W.view(4, 1, 1) / math.sqrt(H)).reshape(4 * H, H).to(BF)
    gx = torch.cat([_gates(B, H, g) for _ in range(U)], 0)
    rs = _rowscale(B)
    lens = torch.tensor([U if b == 0 else (1 if b == B - 1 else 1 + (b * 2) % U) for b in range(B)])
    frozen = (torch.arange(U).view(U, 1) >= lens.view(1, B)).to(U8)
    act = torch.cat([torch.sigmoid(_gates(B, H, g).view(B, 4, H)[:, :2]), torch.tanh(_gates(B, H, g).view(B, 4, H)[:, 2:3]),
                     torch.sigmoid(_gates(B, H, g).view(B, 4, H)[:, 3:])], 1).reshape(1, B, 4 * H).repeat(U, 1, 1)
    act = (act * (1 - 0.01 * torch.arange(U).view(U, 1, 1))).float()
    return dict(H=H, B=B, U=U, w_hh=w_hh, w_hhT=w_hh.t().contiguous(), gx=gx, h0=(0.5 * torch.randn(B, H, generator=g)).to(BF),
                c0=torch.randn(B, H, generator=g) * rs, frozen=frozen, lens=lens, act=act, cs=torch.randn(U, B, H, generator=g) * rs,
                dhs=(torch.randn(U * B, H, generator=g) * rs.repeat(U, 1)).to(BF), dh_last=torch.randn(B, H, generator=g) * rs,
                dc_last=torch.randn(B, H, generator=g) * rs)


BAH_CASES = [  # T, B, A, Cv, lens, bias, kv_col
    (1, 1, 64, 64, None, 1, None), (1, 1, 64, 64, [1], 0, None), (1, 1, 64, 64, [0], 1, None),
    (7, 3, 40, 72, [7, 1, 6], 1, None), (7, 3, 40, 72, [9, 0, 3], 0, None), (7, 3, 40, 72, None, 0, None),
    (130, 5, 320, 640, [130, 1, 129, 135, 0], 1, None), (130, 5, 320, 640, [129, 134], 0, [0, 1, 1, 0, 1]),
    (300, 2, 96, 200, [300, 299], 0, None), (300, 2, 96, 200, [1, 305], 1, None), (300, 3, 96, 200, [299], 1, [0, 0, 0]),
]


def _bah_case(T, B, A, Cv, lens, bias, kv_col):
    g = _gen(T * 1000 + B * 100 + A + Cv + (0 if lens is None else sum(lens)))
    Bkv = B if kv_col is None else max(kv_col) + 1
    ss = _rowscale(Bkv).view(1, Bkv, 1)  # a scale per sentence
    d = dict(T=T, B=B, A=A, Cv=Cv, Bkv=Bkv, qp=torch.randn(B, A, generator=g).to(BF), key=(torch.randn(T, Bkv, A, generator=g) * ss).to(BF),
             value=(torch.randn(T, Bkv, Cv, generator=g) * ss).to(BF), nv=torch.randn(A, generator=g) * 2 / A ** 0.5,
             bias=0.3 * torch.randn(A, generator=g) if bias else None, lens=None if lens is None else torch.tensor(lens, dtype=I32),
             kv_col=None if kv_col is None else torch.tensor(kv_col, dtype=I32), dctx=torch.randn(B, Cv, generator=g).to(BF))
    d["fwd"] = R.bahdanau_fwd(d["qp"], d["key"], d["value"], d["nv"], d["bias"], d["lens"], d["kv_col"])
    if kv_col is None:
        d["p"] = d["fwd"]["p"].float()
        d["pre"] = dict(dkey=torch.randn(T, B, A, generator=g), dvalue=torch.randn(T, B, Cv, generator=g), dnv=1 + torch.rand(A, generator=g),
                        dbias=1 + torch.rand(A, generator=g))
        d["bwd"] = R.bahdanau_bwd(d["dctx"], d["qp"], d["key"], d["value"], d["nv"], d["bias"], d["lens"], d["p"], d["pre"]["dkey"],
                                  d["pre"]["dvalue"], d["pre"]["dnv"], d["pre"]["dbias"] if bias else None)
    return d


# ------------------------------------------------------------------ CPU: the reference against torch
def test_lstm_reference_matches_torch_in_float64():
    g = _gen(1)
    B, I, H, U = 4, 5, 6, 4
    close = lambda a, b: float((a - b).abs().max()) <= 1e-11 * max(float(b.abs().max()), 1e-30)
    # ---- one cell against torch.nn.LSTMCell and autograd
    cell = torch.nn.LSTMCell(I, H).double()
    x, h0, c0 = (torch.randn(B, n, generator=g, dtype=F64) for n in (I, H, H))
    h0.requires_grad_(), c0.requires_grad_()
    G = (x @ cell.weight_ih.T + cell.bias_ih + h0 @ cell.weight_hh.T + cell.bias_hh).detach().requires_grad_()
    h1, c1 = cell(x, (h0, c0))
    r = R.lstm_cell_fwd(G, c0)
    assert close(r["h"], h1.detach()) and close(r["c"], c1.detach())
    dh, dc = torch.randn(B, H, generator=g, dtype=F64), torch.randn(B, H, generator=g, dtype=F64)
    # autograd through the same formula on G (gate order i, f, g, o)
    i_, f_, g_, o_ = G.view(B, 4, H).unbind(1)
    c_t = torch.sigmoid(f_) * c0 + torch.sigmoid(i_) * torch.tanh(g_)
    h_t = torch.sigmoid(o_) * torch.tanh(c_t)
    assert close(h_t.detach(), h1.detach())
    dG_t, dc0_t = torch.autograd.grad((h_t * dh).sum() + (c_t * dc).sum(), (G, c0))
    rb = R.lstm_cell_bwd(None, dh, dc, r["act"], c0, r["c"])
    assert close(rb["dG"], dG_t) and close(rb["dc_prev"], dc0_t)
    # ---- a 4-step ragged sequence in both directions against torch.nn.LSTM on packed sequences
    lstm = torch.nn.LSTM(I, H, bidirectional=True).double()
    lens = torch.tensor([4, 1, 3, 2])
    xs = torch.randn(U, B, I, generator=g, dtype=F64).requires_grad_()
    packed = torch.nn.utils.rnn.pack_padded_sequence(xs, lens, enforce_sorted=False)
    ys, (hn, cn) = lstm(packed)
    ys, _ = torch.nn.utils.rnn.pad_packed_sequence(ys, total_length=U)
    dys = torch.randn(U, B, 2 * H, generator=g, dtype=F64)
    frozen = (torch.arange(U).view(U, 1) >= lens.view(1, B)).to(U8)
    for d, sfx in ((0, ""), (1, "_reverse")):
        w_ih, w_hh = getattr(lstm, "weight_ih_l0" + sfx), getattr(lstm, "weight_hh_l0" + sfx)
        bias = getattr(lstm, "bias_ih_l0" + sfx) + getattr(lstm, "bias_hh_l0" + sfx)
        gx = (xs.reshape(U * B, I) @ w_ih.T + bias).detach().requires_grad_()
        f = R.lstm_seq_fwd(gx, w_hh.detach(), None, None, frozen, B, U, reverse=bool(d), frozen_out_zero=1, round_h=False)
        assert close(f["hs"], ys.detach()[:, :, d * H:(d + 1) * H]), ("hs", d)
        assert close(f["c_last"], cn.detach()[d]), ("c_last", d)
        (dgx_t,) = torch.autograd.grad((ys[:, :, d * H:(d + 1) * H] * dys[:, :, d * H:(d + 1) * H]).sum(), (xs,), retain_graph=True)
        b = R.lstm_seq_bwd(dys[:, :, d * H:(d + 1) * H].reshape(U * B, H), None, None, f["act"], f["cs"], None, frozen, w_hh.detach().T.contiguous(),
                           B, U, reverse=bool(d), round_dG=False)
        assert close((b["dG"].reshape(U * B, 4 * H) @ w_ih.detach()).view(U, B, I), dgx_t), ("dx", d)
    # ---- with an initial state and gradients of the final state, no padding: dh0, dc0 against autograd (one direction each)
    uni = torch.nn.LSTM(I, H).double()
    h0, c0 = (torch.randn(1, B, H, generator=g, dtype=F64).requires_grad_() for _ in range(2))
    ys, (hn, cn) = uni(xs, (h0, c0))
    dhn, dcn = torch.randn(B, H, generator=g, dtype=F64), torch.randn(B, H, generator=g, dtype=F64)
    dh0_t, dc0_t = torch.autograd.grad((ys * dys[:, :, :H]).sum() + (hn[0] * dhn).sum() + (cn[0] * dcn).sum(), (h0, c0))
    gx = (xs.reshape(U * B, I) @ uni.weight_ih_l0.T + uni.bias_ih_l0 + uni.bias_hh_l0).detach()
    f = R.lstm_seq_fwd(gx, uni.weight_hh_l0.detach(), h0[0].detach(), c0[0].detach(), None, B, U, round_h=False)
    assert close(f["hs"], ys.detach()) and close(f["h_last"], hn[0].detach()) and close(f["c_last"], cn[0].detach())
    b = R.lstm_seq_bwd(dys[:, :, :H].reshape(U * B, H), dhn, dcn, f["act"], f["cs"], c0[0].detach(), None, uni.weight_hh_l0.detach().T.contiguous(),
                       B, U, round_dG=False)
    assert close(b["dh0"], dh0_t[0]) and close(b["dc0"], dc0_t[0])


def test_bahdanau_reference_matches_autograd_in_float64():
    """tests/recurrent_ref.py against the float64 autograd restatement of oracle/torch_ref.py:bahdanau_attention"""
    g = _gen(2)
    T, B, A, Cv = 6, 3, 5, 7
    close = lambda a, b: float((a - b).abs().max()) <= 1e-11 * max(float(b.abs().max()), 1e-30)
    qp, key, value = (torch.randn(*s, generator=g, dtype=F64).requires_grad_() for s in ((B, A), (T, B, A), (T, B, Cv)))
    nv, bias = (torch.randn(A, generator=g, dtype=F64).requires_grad_() for _ in range(2))
    lens, dctx = torch.tensor([6, 2, 9]), torch.randn(B, Cv, generator=g, dtype=F64)
    mask = torch.arange(T).unsqueeze(1) >= lens.unsqueeze(0)
    scores = (nv * torch.tanh(qp.unsqueeze(0) + key + bias)).sum(2).masked_fill(mask, float("-inf"))
    a = torch.softmax(scores, 0)
    ctx = (a.unsqueeze(2) * value).sum(0)
    f = R.bahdanau_fwd(qp, key, value, nv, bias, lens)
    assert close(f["p"], a.detach()) and close(f["ctx"], ctx.detach())
    grads = torch.autograd.grad((ctx * dctx).sum(), (qp, key, value, nv, bias))
    pre = [torch.randn(*s, generator=g, dtype=F64) for s in ((T, B, A), (T, B, Cv), (A,), (A,))]
    b = R.bahdanau_bwd(dctx, qp, key, value, nv, bias, lens, a.detach(), *pre)
    for name, got, want in (("dqp", b["dqp"], grads[0]), ("dkey", b["dkey"] - pre[0], grads[1]), ("dvalue", b["dvalue"] - pre[1], grads[2]),
                            ("dnv", b["dnv"] - pre[2], grads[3]), ("dbias", b["dbias"] - pre[3], grads[4])):
        assert close(got, want), name
    # the beam-dedup addressing: hypotheses 0, 2 read sentence 1, hypothesis 1 reads sentence 0
    col = torch.tensor([1, 0, 1])
    f2 = R.bahdanau_fwd(qp, key[:, :2], value[:, :2], nv, bias, lens[:2], col)
    f3 = R.bahdanau_fwd(qp, key[:, col], value[:, col], nv, bias, lens[col])
    assert torch.equal(f2["p"], f3["p"]) and torch.equal(f2["ctx"], f3["ctx"])


# ------------------------------------------------------------------ CPU: mutations
def test_mutations_land_outside_the_bounds():
    d = _cell_case(5, 48)
    B, H = 5, 48
    cfg = (1, 1, 1, 1, 1, 1, 0)
    ref = _cell_fwd_ref(d, cfg)
    tol_h16 = _ulp(ref["h16"]) + ref["tol_h"]
    Gv = d["G"].view(B, 4, H)
    muts = {"two gates swapped": Gv[:, [1, 0, 2, 3]], "the neighbouring hidden unit": Gv.roll(1, 2), "the neighbouring batch row": Gv.roll(1, 0)}
    for name, Gm in muts.items():
        m = R.lstm_cell_fwd(Gm.reshape(B, 4 * H), d["c_prev"], d["keep"], d["h_prev"], 0)
        assert _moved(m["c"], ref["c"], ref["tol_c"]) and _moved(R.bf(m["h16"]), ref["h16"], tol_h16) and _moved(m["act"], ref["act"], ref["tol_act"]), name
    m = R.lstm_cell_fwd(d["G"], d["c_prev"], None, None, 0)
    assert _moved(m["c"], ref["c"], ref["tol_c"]) and _moved(m["h"], ref["h"], ref["tol_h"]), "a frozen row advanced"
    assert not _moved(R.bf(ref["h16"]), ref["h16"], tol_h16) and not _moved(ref["c"].float(), ref["c"], ref["tol_c"] + 2.0 ** -24 * ref["c"].abs())
    # the backward of the cell: dc not passed through a frozen step
    rb = _cell_bwd_ref(d, (1, 1, 1, 1, 1))
    fz = d["keep"].bool().view(B, 1)
    assert _moved(torch.where(fz, torch.zeros(B, H, dtype=F64), rb["dc_prev"]), rb["dc_prev"], rb["tol_dc_prev"]), "dc not passed through a frozen step"
    # the sequence: the wrong neighbour under reverse; dh_last / dc_last dropped
    s = _seq_case(256, 5, 3)
    U, B, H = 3, 5, 256
    f = R.lstm_seq_fwd(s["gx"], s["w_hh"], s["h0"], s["c0"], None, B, U, reverse=True)
    gx = s["gx"].view(U, B, 4 * H)
    good = R.lstm_seq_step_fwd(gx[1], s["w_hh"], f["hs"][2], f["cs"][2])
    bad = R.lstm_seq_step_fwd(gx[1], s["w_hh"], f["hs"][0], f["cs"][0])
    assert _moved(bad["c"], good["c"], good["tol_c"]) and _moved(bad["act"], good["act"], good["tol_act"]), "step t-1 read where t+1 is due"
    bw = lambda dh_last, dc_last: R.lstm_seq_bwd(s["dhs"], dh_last, dc_last, s["act"], s["cs"], s["c0"], None, s["w_hhT"], B, U)
    full = bw(s["dh_last"], s["dc_last"])
    tol_dG = _ulp(full["dG"]) + full["tol_dG"]
    for name, m in (("dh_last dropped", bw(None, s["dc_last"])), ("dc_last dropped", bw(s["dh_last"], None))):
        assert _moved(R.bf(m["dG"]), full["dG"], tol_dG) and _moved(m["dc0"], full["dc0"], full["tol_dc0"]), name
    # Bahdanau: kv_col ignored, one key past len, dkey_acc overwritten
    c = _bah_case(130, 5, 320, 640, [129, 134], 0, [0, 1, 1, 0, 1])
    fw = c["fwd"]
    tol_ctx = _ulp(fw["ctx"]) + fw["tol_ctx"]
    m = R.bahdanau_fwd(c["qp"], c["key"], c["value"], c["nv"], c["bias"], c["lens"], torch.arange(5) % 2)
    assert _moved(m["p"], fw["p"], fw["tol_p"]) and _moved(R.bf(m["ctx"]), fw["ctx"], tol_ctx), "kv_col ignored"
    m = R.bahdanau_fwd(c["qp"], c["key"], c["value"], c["nv"], c["bias"], c["lens"] + 1, c["kv_col"])
    assert _moved(m["p"], fw["p"], fw["tol_p"]) and _moved(R.bf(m["ctx"]), fw["ctx"], tol_ctx), "one key past len"
    c = _bah_case(7, 3, 40, 72, [7, 1, 6], 1, None)
    b = c["bwd"]
    assert _moved(b["dpre"], b["dkey"], b["tol_dkey"]), "dkey_acc overwritten where it must accumulate"


# ------------------------------------------------------------------ CPU: every GPU case, with the preconditions of its bounds
def test_every_gpu_case_builds_on_the_cpu_with_its_preconditions():
    for B, H in CELL_SHAPES:
        d = _cell_case(B, H)
        for s in SPECIALS:
            assert bool((d["G"].view(B, 4, H)[:8] == s).any(2).all()), (B, H, s)  # every gate of the first rows meets every special value
        for cfg in FWD_CONFIGS:
            r = _cell_fwd_ref(d, cfg)
            assert all(bool(torch.isfinite(r[k]).all()) for k in r)
            assert float(r["tol_c"].max()) < 1e-4 and float(r["tol_h"].max()) < 1e-4 and float(r["tol_act"].max()) < 2.0 ** -18
        for cfg in BWD_CONFIGS:
            r = _cell_bwd_ref(d, cfg)
            assert all(bool(torch.isfinite(r[k]).all()) for k in r)
            if B > 1:  # the neighbouring row, as the row scales are meant to show it
                m = R.lstm_cell_bwd(d["dh_a"].roll(1, 0) if cfg[0] else None, d["dh_b"].roll(1, 0) if cfg[1] else None,
                                    d["dc_in"].roll(1, 0) if cfg[2] else None, d["act"], d["c_prev"] if cfg[3] else None, d["c"],
                                    d["keep"] if cfg[4] else None)
                assert _moved(m["dc_prev"], r["dc_prev"], r["tol_dc_prev"]) or _moved(R.bf(m["dG"]), r["dG"], _ulp(r["dG"]) + r["tol_dG"])
    assert 520 * 1024 > 2048 * 256
    fwd_inst, bwd_inst = set(), set()
    for H, B, U in SEQ_CASES:
        ng = (B + 15) // 16
        fwd_inst.add((H // 32, {1: 1, 2: 2}.get(ng, 4)))
        bwd_inst.add((H // 32, {1: 1, 2: 2}.get(ng, 4)))
    assert len(fwd_inst) == 21 and len(bwd_inst) == 21
    for H, B, U in SEQ_CASES:
        s = _seq_case(H, B, U)
        assert int(s["lens"][0]) == U and int(s["lens"][-1]) == min(1, U) or B == 1
        gx = s["gx"].view(U, B, 4 * H)
        r = R.lstm_seq_step_fwd(gx[0], s["w_hh"], s["h0"], s["c0"])
        hp, w = s["h0"].double(), s["w_hh"].double()
        mag = gx[0].double().abs() + hp.abs() @ w.abs().T
        _sees_one_row("pre", (H + 1) * E * mag, mag, H)
        m = R.lstm_seq_step_fwd(gx[0], s["w_hh"], s["h0"].roll(1, 1), s["c0"])  # the hidden state one unit off
        assert _moved(m["act"], r["act"], r["tol_act"])
        b = R.lstm_seq_bwd(s["dhs"], s["dh_last"], s["dc_last"], s["act"], s["cs"], s["c0"], s["frozen"], s["w_hhT"], B, U)
        assert all(bool(torch.isfinite(b[k]).all()) for k in b)
        if U == 3:  # the carried dc: its bound grows over the steps and still resolves a dropped dc_last
            m = R.lstm_seq_bwd(s["dhs"], s["dh_last"], None, s["act"], s["cs"], s["c0"], s["frozen"], s["w_hhT"], B, U)
            assert _moved(m["dc0"], b["dc0"], b["tol_dc0"])
    for case in BAH_CASES:
        c = _bah_case(*case)
        fw = c["fwd"]
        assert fw["max_arg"] < 80 and all(bool(torch.isfinite(fw[k]).all()) for k in ("p", "ctx", "tol_p", "tol_ctx"))
        _sees_one_row("ctx", fw["tol_ctx"], fw["ctx_mag"], case[0])
        if "bwd" in c:
            bw = c["bwd"]
            _sees_one_row("dnv", bw["tol_dnv"], bw["dnv_mag"], case[1])
            _sees_one_row("dbias", bw["tol_dbias"], bw["dbias_mag"], case[1])


# ------------------------------------------------------------------ GPU: the cell
def _run_cell_fwd(lib, d, cfg):
    B, H = d["B"], d["H"]
    cp, hf, hb, ac, keep, hp, fz0 = cfg
    ldg, ldh = 4 * H + PAD, H + PAD
    bG = _pitched_in(d["G"], ldg)
    bcp, bhp = (inp(d["c_prev"]) if cp else None), (inp(d["h_prev"]) if hp else None)
    fl = _flags(d["keep"]) if keep else None
    bc, bh = out((B, H), F32), (out((B, H), F32) if hf else None)
    bh16, bact = (_pitched_out(B, H, ldh, BF) if hb else None), (out((B, 4 * H), F32) if ac else None)
    assert lib.ea_lstm_cell_fwd(bG.p, ldg, _p(bcp), bc.p, _p(bh), _p(bh16), ldh, _p(bact), _p(fl), _p(bhp), fz0, B, H, _st()) == 0
    _sync()
    r = _cell_fwd_ref(d, cfg)
    assert bc.intact()
    _chk("cell_fwd c", bc.cpu(), r["c"], r["tol_c"])
    if hf:
        assert bh.intact()
        _chk("cell_fwd h_f32", bh.cpu(), r["h"], r["tol_h"])
    if hb:
        assert _gap_intact(bh16, H)
        _chk_bf16("cell_fwd h_bf16", bh16.cpu()[:, :H], r["h16"], r["tol_h"])
    if ac:
        assert bact.intact()
        _chk("cell_fwd act", bact.cpu(), r["act"], r["tol_act"])


def _run_cell_bwd(lib, d, cfg):
    B, H = d["B"], d["H"]
    a, b, dc, cp, fz = cfg
    ld_dh, lddg = H + PAD, 4 * H + PAD
    ba = _pitched_in(d["dh_a"], ld_dh) if a else None
    bb, bdc, bcp = (inp(d["dh_b"]) if b else None), (inp(d["dc_in"]) if dc else None), (inp(d["c_prev"]) if cp else None)
    bact, bc = inp(d["act"]), inp(d["c"])
    fl = _flags(d["keep"]) if fz else None
    bdG, bdcp = _pitched_out(B, 4 * H, lddg, BF), out((B, H), F32)
    assert lib.ea_lstm_cell_bwd(_p(ba), ld_dh, _p(bb), _p(bdc), bact.p, _p(bcp), bc.p, bdG.p, lddg, bdcp.p, _p(fl), B, H, _st()) == 0
    _sync()
    assert _gap_intact(bdG, 4 * H) and bdcp.intact()
    r = _cell_bwd_ref(d, cfg)
    _chk_bf16("cell_bwd dG", bdG.cpu()[:, :4 * H], r["dG"], r["tol_dG"])
    _chk("cell_bwd dc_prev", bdcp.cpu(), r["dc_prev"], r["tol_dc_prev"])


@gpu
@pytest.mark.parametrize("B,H", CELL_SHAPES)
def test_lstm_cell_forward_and_backward(lib, B, H):
    d = _cell_case(B, H)
    big = B * H > 2048 * 256  # the grid-stride loop's second trip: two forward and two backward launches are enough there
    for cfg in (FWD_CONFIGS[:1] + FWD_CONFIGS[4:5] if big else FWD_CONFIGS):
        _run_cell_fwd(lib, d, cfg)
    for cfg in (BWD_CONFIGS[:2] if big else BWD_CONFIGS):
        _run_cell_bwd(lib, d, cfg)


@gpu
def test_lstm_cell_empty_batch_touches_nothing(lib):
    d = _cell_case(5, 48)
    bG, bc, bh, bh16, bact = inp(d["G"]), out((5, 48), F32), out((5, 48), F32), out((5, 48), BF), out((5, 192), F32)
    assert lib.ea_lstm_cell_fwd(bG.p, 192, None, bc.p, bh.p, bh16.p, 48, bact.p, None, None, 0, 0, 48, _st()) == 0
    bdG, bdc = out((5, 192), BF), out((5, 48), F32)
    assert lib.ea_lstm_cell_bwd(None, 48, bc.p, None, bG.p, None, bG.p, bdG.p, 192, bdc.p, None, 0, 48, _st()) == 0
    _sync()
    assert all(o.untouched() for o in (bc, bh, bh16, bact, bdG, bdc))


@gpu
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("W", [1, 7, 640])
def test_gather_rows(lib, W, dtype):
    g = _gen(W)
    x = torch.randn(6, W, generator=g).to(dtype)
    parent = torch.tensor([5, 0, 0, 3, 2, 2, 4], dtype=I32)
    bx, bo, par = inp(x), out((7, W), dtype), parent.to(DEV)
    assert lib.ea_gather_rows(bx.p, bo.p, par.data_ptr(), 7, W, x.element_size(), _st()) == 0
    _sync()
    assert bo.intact() and torch.equal(bo.bits(), R.gather_rows(x, parent).view(_INT[dtype]))
    bo2 = out((7, W), dtype)
    assert lib.ea_gather_rows(bx.p, bo2.p, par.data_ptr(), 7, W, 8, _st()) == -2
    assert lib.ea_gather_rows(bx.p, bo2.p, par.data_ptr(), 0, W, x.element_size(), _st()) == 0
    _sync()
    assert bo2.untouched()


# ------------------------------------------------------------------ GPU: the persistent recurrence
def _counter():
    return out((2,), F32)


def _run_seq_fwd(lib, s, combo):
    H, B, U = s["H"], s["B"], s["U"]
    reverse, h0, c0, frozen = combo[:4]
    gx = s["gx"].view(U, B, 4 * H)
    bgx, bw = inp(s["gx"]), inp(s["w_hh"])
    bh0, bc0 = (inp(s["h0"]) if h0 else None), (inp(s["c0"]) if c0 else None)
    fl = _flags(s["frozen"]) if frozen else None
    bhs, bcs, bact, bhl, cnt = out((U * B, H), BF), out((U * B, H), F32), out((U * B, 4 * H), F32), out((B, H), F32), _counter()
    assert lib.ea_lstm_seq_fwd(bgx.p, bw.p, _p(bh0), _p(bc0), _p(fl), bhs.p, bcs.p, bact.p, bhl.p, cnt.p, B, U, H, reverse, 1 if frozen else 0,
                               _st()) == 0
    _sync()
    assert all(o.intact() for o in (bhs, bcs, bact, bhl, cnt)), "rows b >= B of the last batch group (or the guards) were written"
    assert int(cnt.bits()[1]) == 0, "the grid barrier gave up"
    hs, cs, act = bhs.cpu().view(U, B, H), bcs.cpu().view(U, B, H), bact.cpu().view(U, B, 4 * H)
    for n in range(U):
        t = U - 1 - n if reverse else n
        tp = t + 1 if reverse else t - 1
        hp, cp = ((s["h0"] if h0 else None), (s["c0"] if c0 else None)) if n == 0 else (hs[tp], cs[tp])
        r = R.lstm_seq_step_fwd(gx[t], s["w_hh"], hp, cp, s["frozen"][t] if frozen else None, 1)
        _chk("seq_fwd act", act[t], r["act"], r["tol_act"])
        _chk("seq_fwd cs", cs[t], r["c"], r["tol_c"])
        _chk_bf16("seq_fwd hs", hs[t], r["h16"], r["tol_h"])
        if n == U - 1:
            _chk("seq_fwd h_last", bhl.cpu(), r["h"], r["tol_h"])


def _run_seq_bwd(lib, s, combo):
    H, B, U = s["H"], s["B"], s["U"]
    reverse, _, c0, frozen, dhs, dhl, dcl, dh0, dc0 = combo
    bact, bcs, bwT = inp(s["act"].view(U * B, 4 * H)), inp(s["cs"].view(U * B, H)), inp(s["w_hhT"])
    bdhs, bdhl, bdcl = (inp(s["dhs"]) if dhs else None), (inp(s["dh_last"]) if dhl else None), (inp(s["dc_last"]) if dcl else None)
    bc0 = inp(s["c0"]) if c0 else None
    fl = _flags(s["frozen"]) if frozen else None
    bdG, cnt = out((U * B, 4 * H), BF), _counter()
    bdh0, bdc0 = (out((B, H), F32) if dh0 else None), (out((B, H), F32) if dc0 else None)
    assert lib.ea_lstm_seq_bwd(_p(bdhs), _p(bdhl), _p(bdcl), bact.p, bcs.p, _p(bc0), _p(fl), bwT.p, bdG.p, _p(bdh0), _p(bdc0), cnt.p, B, U, H,
                               reverse, _st()) == 0
    _sync()
    assert all(o.intact() for o in (bdG, cnt, bdh0, bdc0) if o is not None)
    assert int(cnt.bits()[1]) == 0, "the grid barrier gave up"
    dG = bdG.cpu()
    r = R.lstm_seq_bwd(s["dhs"] if dhs else None, s["dh_last"] if dhl else None, s["dc_last"] if dcl else None, s["act"], s["cs"],
                       s["c0"] if c0 else None, s["frozen"] if frozen else None, s["w_hhT"], B, U, reverse=bool(reverse), dG_stored=dG)
    _chk_bf16("seq_bwd dG", dG.view(U, B, 4 * H), r["dG"], r["tol_dG"])
    if dh0:
        _chk("seq_bwd dh0", bdh0.cpu(), r["dh0"], r["tol_dh0"])
    if dc0:
        _chk("seq_bwd dc0", bdc0.cpu(), r["dc0"], r["tol_dc0"])


@gpu
@pytest.mark.parametrize("H,B,U", SEQ_CASES)
def test_lstm_seq_forward_and_backward(lib, H, B, U):
    assert lib.ea_lstm_seq_supported(B, H) == 1  # on this device that is the contract
    s = _seq_case(H, B, U)
    for combo in SEQ_COMBOS:
        _run_seq_fwd(lib, s, combo)
        _run_seq_bwd(lib, s, combo)


@gpu
def test_lstm_seq_refused_shapes_touch_nothing(lib):
    """H = 384, B = 65, counter = NULL: -2; U = 0: 0"""
    B, H, U = 5, 256, 2
    z = lambda *shape: inp(torch.zeros(*shape))
    gx, w, act, cs = z(U * 65, 4 * 384), inp(torch.zeros(4 * 384, 384).to(BF)), z(U * 65, 4 * 384), z(U * 65, 384)
    for (b, u, h, with_counter, want) in ((B, U, 384, 1, -2), (65, U, H, 1, -2), (B, U, H, 0, -2), (B, 0, H, 1, 0)):
        bhs, bcs, bact, bhl, cnt = out((U * 65, 384), BF), out((U * 65, 384), F32), out((U * 65, 4 * 384), F32), out((65, 384), F32), _counter()
        c = cnt.p if with_counter else None
        assert lib.ea_lstm_seq_fwd(gx.p, w.p, None, None, None, bhs.p, bcs.p, bact.p, bhl.p, c, b, u, h, 0, 0, _st()) == want, (b, u, h)
        bdG, bdh0, bdc0 = out((U * 65, 4 * 384), BF), out((65, 384), F32), out((65, 384), F32)
        assert lib.ea_lstm_seq_bwd(None, cs.p, cs.p, act.p, cs.p, None, None, w.p, bdG.p, bdh0.p, bdc0.p, c, b, u, h, 0, _st()) == want, (b, u, h)
        _sync()
        assert all(o.untouched() for o in (bhs, bcs, bact, bhl, cnt, bdG, bdh0, bdc0)), (b, u, h)


# ------------------------------------------------------------------ GPU: Bahdanau attention
@gpu
@pytest.mark.parametrize("case", BAH_CASES, ids=lambda c: f"T{c[0]}-B{c[1]}-A{c[2]}-Cv{c[3]}-{'full' if c[4] is None else 'len' + '_'.join(map(str, c[4]))}"
                                                          f"{'-bias' if c[5] else ''}{'-kvcol' if c[6] else ''}")
def test_bahdanau_forward_and_backward(lib, case):
    T, B, A, Cv = case[:4]
    d = _bah_case(*case)
    ldc = ldd = Cv + PAD
    bqp, bkey, bval, bnv = inp(d["qp"]), inp(d["key"].view(-1, A)), inp(d["value"].view(-1, Cv)), inp(d["nv"])
    bbias = inp(d["bias"]) if d["bias"] is not None else None
    lens = None if d["lens"] is None else d["lens"].to(DEV)
    col = None if d["kv_col"] is None else d["kv_col"].to(DEV)
    bp, bctx = out((T, B), F32), _pitched_out(B, Cv, ldc, BF)
    assert lib.ea_bahdanau_fwd(bqp.p, bkey.p, bval.p, bnv.p, _p(bbias), _p(lens), bp.p, bctx.p, ldc, T, B, A, Cv, _p(col), d["Bkv"], _st()) == 0
    _sync()
    assert bp.intact() and _gap_intact(bctx, Cv)
    fw = d["fwd"]
    _chk("bahdanau_fwd p", bp.cpu(), fw["p"], fw["tol_p"])
    _chk_bf16("bahdanau_fwd ctx", bctx.cpu()[:, :Cv], fw["ctx"], fw["tol_ctx"])
    assert bool((bp.bits()[fw["p"] == 0] == 0).all()), "p is not +0 from min(len, T) on"
    if "bwd" not in d:
        return
    pre, bw = d["pre"], d["bwd"]
    bdctx, bpin = _pitched_in(d["dctx"], ldd), inp(d["p"])
    bdq = out((B, A), BF)
    bdk, bdv = out((T * B, A), F32, pre["dkey"]), out((T * B, Cv), F32, pre["dvalue"])
    bdn, bdb = out((A,), F32, pre["dnv"]), (out((A,), F32, pre["dbias"]) if d["bias"] is not None else None)
    assert lib.ea_bahdanau_bwd(bdctx.p, ldd, bqp.p, bkey.p, bval.p, bnv.p, _p(bbias), _p(lens), bpin.p, bdq.p, bdk.p, bdv.p, bdn.p, _p(bdb), T, B, A,
                               Cv, _st()) == 0
    _sync()
    assert all(o.intact() for o in (bdq, bdk, bdv, bdn, bdb) if o is not None)
    _chk_bf16("bahdanau_bwd dqp", bdq.cpu(), bw["dqp"], bw["tol_dqp"])
    _chk("bahdanau_bwd dkey_acc", bdk.cpu().view(T, B, A), bw["dkey"], bw["tol_dkey"])
    _chk("bahdanau_bwd dvalue_acc", bdv.cpu().view(T, B, Cv), bw["dvalue"], bw["tol_dvalue"])
    past = ~bw["mask"]
    assert torch.equal(bdk.bits().view(T, B, A)[past], pre["dkey"].view(I32)[past]), "dkey_acc rows t >= len moved"
    assert torch.equal(bdv.bits().view(T, B, Cv)[past], pre["dvalue"].view(I32)[past]), "dvalue_acc rows t >= len moved"
    _sees_one_row("dnv", bw["tol_dnv"], bw["dnv_mag"], B)
    _chk("bahdanau_bwd dnv_acc", bdn.cpu(), bw["dnv"], bw["tol_dnv"])
    if bdb is not None:
        _sees_one_row("dbias", bw["tol_dbias"], bw["dbias_mag"], B)
        _chk("bahdanau_bwd dbias_acc", bdb.cpu(), bw["dbias"], bw["tol_dbias"])


@gpu
def test_bahdanau_refuses_a_time_axis_beyond_lds(lib):
    """forward: T floats above 48 KB; backward: T + 8 A floats above 60 KB: -2, nothing written; an empty batch: 0"""
    z, nv = inp(torch.zeros(4, 64).to(BF)), inp(torch.zeros(64))
    for (Tf, Tb, B, want) in ((12289, 14849, 1, -2), (5, 5, 0, 0)):
        bp, bctx, bdq, bacc = out((4, 4), F32), out((4, 64), BF), out((4, 64), BF), out((4, 64), F32)
        assert lib.ea_bahdanau_fwd(z.p, z.p, z.p, nv.p, None, None, bp.p, bctx.p, 64, Tf, B, 64, 64, None, 0, _st()) == want
        assert lib.ea_bahdanau_bwd(z.p, 64, z.p, z.p, z.p, nv.p, None, None, nv.p, bdq.p, bacc.p, bacc.p, bacc.p, None, Tb, B, 64, 64, _st()) == want
        _sync()
        assert all(o.untouched() for o in (bp, bctx, bdq, bacc))
