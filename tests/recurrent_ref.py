"""Plain fp64 restatements of the recurrent and decoding kernels (espresso_amd/csrc/lstm.hip, lstm_seq.hip, decode.hip), element
by element and with the kernels' storage points (bf16 where a kernel stores bf16, fp32 state otherwise), for
tests/test_lstm_kernels.py and tests/test_decode_kernels.py.  CPU, plain torch, no device code.

Every function that restates arithmetic returns its values together with the bound of the kernel's error on each of them,
derived from the kernel's own operations (the derivations are in the two test modules' docstrings).  E = 2^-23 is charged per
fp32 rounding and per v_rcp_f32, TINY = 2^-126 where a result may be flushed or underflow to zero."""
import math

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
E = 2.0 ** -23
TINY = 2.0 ** -126
INF = float("inf")


def f64(x):
    return x.detach().to("cpu").to(F64)


def bf(x):
    """the bf16 rounding of an fp64 tensor, as fp64 (through fp32, as the kernels round)"""
    return x.to(F32).to(BF).to(F64)


def _z(x, like):
    return torch.zeros_like(like) if x is None else f64(x)


# ------------------------------------------------------------------ the two activations and their bounds
def sig_tol(x, tol_x=0.0):
    """sigmoid_f (lstm.hip:15, lstm_seq.hip:23) = 1 / (1 + __expf(-x)): relative ((1 + |x|)(1 - s) + 1.5) E (the charge of
    tests/test_gemm_kernels.py for SiLU's sigmoid), TINY where exp overflows or the quotient is subnormal; an argument off by
    tol_x moves it by s (1 - s) tol_x (+ tol_x^2 for the curvature)"""
    s, oms = torch.sigmoid(x), torch.sigmoid(-x)
    return ((1 + x.abs()) * oms + 1.5) * E * s + TINY + (s * oms + tol_x) * tol_x


def tanh_tol(x, tol_x=0.0):
    """tanh_f (lstm.hip:16-20, lstm_seq.hip:24-27) = 1 - 2 / (e + 1), e = __expf(2x).  e is off by (1 + 2|x|) E of itself, which
    moves q = 2 / (e + 1) by e / (e + 1) = (1 + t) / 2 of that; the addition and the division add 2 E of q; q = 1 - t; the final
    subtraction rounds by E |t|.  ABSOLUTE near 0 (2.5 E), relative to 1 - t in the positive tail (+ E |t|, the last rounding),
    3 E + E |t| in the negative tail where q -> 2."""
    t = torch.tanh(x)
    omt = 2 * torch.sigmoid(-2 * x)  # 1 - t without cancellation
    opt_half = torch.sigmoid(2 * x)  # (1 + t) / 2
    return E * (omt * ((1 + 2 * x.abs()) * opt_half + 2) + t.abs()) + TINY + (omt * 2 * opt_half + 2 * tol_x) * tol_x


def one_minus_sq_tanh(x):
    """1 - tanh(x)^2 without cancellation"""
    return 2 * torch.sigmoid(-2 * x) * 2 * torch.sigmoid(2 * x)


# ------------------------------------------------------------------ LSTM cell (lstm.hip:22-79)
def lstm_cell_fwd(G, c_prev=None, keep_row=None, h_prev=None, frozen_out_zero=0, tol_G=None):
    """G [B][4H] pre-activations in gate order i, f, g, o.  Returns a dict: act [B][4H], c, h (fp32 outputs), h16 (the value whose
    bf16 rounding h_bf16 holds) and tol_* for each.  Frozen rows (keep_row != 0): c = c_prev, h = h_prev (0 without it), both exact;
    h16 = 0 with frozen_out_zero."""
    G = f64(G)
    B, H = G.shape[0], G.shape[1] // 4
    tG = torch.zeros_like(G) if tol_G is None else tol_G.expand_as(G)
    (pi, pf, pg, po), (ti, tf, tg, to) = G.view(B, 4, H).unbind(1), tG.reshape(B, 4, H).unbind(1)
    gi, gf, gg, go = torch.sigmoid(pi), torch.sigmoid(pf), torch.tanh(pg), torch.sigmoid(po)
    tgi, tgf, tgg, tgo = sig_tol(pi, ti), sig_tol(pf, tf), tanh_tol(pg, tg), sig_tol(po, to)
    cp = _z(c_prev, gi)
    c = gf * cp + gi * gg
    tol_c = cp.abs() * tgf + gi * tgg + gg.abs() * tgi + tgi * tgg + 2 * E * ((gf * cp).abs() + (gi * gg).abs())
    tc = torch.tanh(c)
    ttc = tanh_tol(c, tol_c)
    h = go * tc
    tol_h = go * ttc + tc.abs() * tgo + tgo * ttc + E * h.abs()
    h16 = h.clone()
    if keep_row is not None:
        fz = keep_row.to("cpu").bool().view(B, 1).expand(B, H)
        c, tol_c = torch.where(fz, cp, c), torch.where(fz, torch.zeros_like(c), tol_c)
        h, tol_h = torch.where(fz, _z(h_prev, c), h), torch.where(fz, torch.zeros_like(c), tol_h)
        h16 = torch.where(fz, torch.zeros_like(h), h) if frozen_out_zero else h.clone()
    return dict(act=torch.cat([gi, gf, gg, go], 1), tol_act=torch.cat([tgi, tgf, tgg, tgo], 1), c=c, tol_c=tol_c, h=h, tol_h=tol_h,
                h16=h16)


def lstm_cell_bwd(dh_a, dh_b, dc_in, act, c_prev, c, frozen=None, tol_dh=None, tol_dc_in=None):
    """dh = dh_a (bf16) + dh_b (fp32); returns dG [B][4H] (the value whose bf16 rounding is stored), dc_prev and their bounds.
    tol_dh: what dh_b already carries (the recurrent sum of the sequence kernel); tol_dc_in: what the carried dc carries.
    A frozen row gives zero gate gradients and passes dc_in through."""
    act, c = f64(act), f64(c)
    B, H = c.shape
    gi, gf, gg, go = act.view(B, 4, H).unbind(1)
    a, b_ = _z(dh_a, c), _z(dh_b, c)
    dh = a + b_
    tdh = E * (a.abs() + b_.abs()) + (0.0 if tol_dh is None else tol_dh)
    tc, tt = torch.tanh(c), tanh_tol(c)
    s = one_minus_sq_tanh(c)
    tol_s = 2 * tc.abs() * tt + 2 * E
    term = dh * go * s
    tol_term = go * s * tdh + dh.abs() * go * tol_s + tdh * go * tol_s + 2 * E * term.abs()
    dci = _z(dc_in, c)
    tdci = torch.zeros_like(c) if tol_dc_in is None else tol_dc_in
    dc = dci + term
    tdc = tdci + tol_term + E * (dci.abs() + term.abs())
    cp = _z(c_prev, c)
    ki, kf, kg = gg * gi * (1 - gi), cp * gf * (1 - gf), gi * (1 - gg * gg)
    d_i, d_f, d_g = dc * ki, dc * kf, dc * kg
    ko = tc * go * (1 - go)
    d_o = dh * ko
    # (TINY: a saturated gate is 0 or subnormal in fp32, and so are the products it enters)
    t_i = tdc * ki.abs() + 5 * E * d_i.abs() + TINY
    t_f = tdc * kf.abs() + 5 * E * d_f.abs() + TINY
    t_g = tdc * kg.abs() + (dc.abs() + tdc) * gi * E + 3 * E * d_g.abs() + TINY
    t_o = tdh * ko.abs() + (dh.abs() + tdh) * go * (1 - go) * tt + 5 * E * d_o.abs() + TINY
    dcp = dc * gf
    tdcp = tdc * gf + E * dcp.abs() + TINY
    dG, tdG = torch.cat([d_i, d_f, d_g, d_o], 1), torch.cat([t_i, t_f, t_g, t_o], 1)
    if frozen is not None:
        fz = frozen.to("cpu").bool().view(B, 1)
        dG, tdG = torch.where(fz, torch.zeros_like(dG), dG), torch.where(fz, torch.zeros_like(dG), tdG)
        dcp, tdcp = torch.where(fz, dci, dcp), torch.where(fz, tdci, tdcp)
    return dict(dG=dG, tol_dG=tdG, dc_prev=dcp, tol_dc_prev=tdcp, dh=dh)


# ------------------------------------------------------------------ one step of the persistent recurrence (lstm_seq.hip)
def lstm_seq_step_fwd(gx_t, w_hh, h_prev16, c_prev, frozen_t=None, frozen_out_zero=1):
    """pre = gx[t] + h_prev W_hh^T: the fp32 MFMA sum of H bf16 products plus one addition, (H + 1) E of the magnitudes
    (lstm_seq.hip:104-132); then the cell.  A frozen row keeps c and emits h = 0 (:136-140).  Returns lstm_cell_fwd's dict:
    act[t], c = cs[t], h16 -> hs[t], h -> h_last."""
    gx_t, w = f64(gx_t), f64(w_hh)
    H = w.shape[1]
    if h_prev16 is None:
        pre, tol = gx_t, torch.zeros_like(gx_t)
    else:
        hp = f64(h_prev16)
        pre = gx_t + hp @ w.T
        tol = (H + 1) * E * (gx_t.abs() + hp.abs() @ w.abs().T)
    return lstm_cell_fwd(pre, c_prev, keep_row=frozen_t, h_prev=None, frozen_out_zero=frozen_out_zero, tol_G=tol)


def lstm_seq_fwd(gx, w_hh, h0, c0, frozen, B, U, reverse=False, frozen_out_zero=1, round_h=True):
    """the whole recurrence on the reference's own state (round_h: hs stored as bf16 between the steps, as the kernel does)"""
    gx = f64(gx).view(U, B, -1)
    H = gx.shape[2] // 4
    act, cs, hs = torch.zeros(U, B, 4 * H, dtype=F64), torch.zeros(U, B, H, dtype=F64), torch.zeros(U, B, H, dtype=F64)
    h, c, h_last = (None if h0 is None else f64(h0)), (None if c0 is None else f64(c0)), None
    for n in range(U):
        t = U - 1 - n if reverse else n
        r = lstm_seq_step_fwd(gx[t], w_hh, h, c, None if frozen is None else frozen[t], frozen_out_zero)
        act[t], cs[t], hs[t] = r["act"], r["c"], (bf(r["h16"]) if round_h else r["h16"])
        h, c, h_last = hs[t], cs[t], r["h"]
    return dict(act=act, cs=cs, hs=hs, h_last=h_last, c_last=c)


def lstm_seq_step_bwd(dhs_t, dG_src16, w_hhT, dh_last, dcs, tol_dcs, act_t, c_t, c_prev, frozen_t=None):
    """dh = dhs[t] + sum_k W_hh^T[j][k] dG_src[b][k] (four per-gate MFMA sums of H products, three additions, one onto dhs:
    (H + 4) E of the magnitudes, lstm_seq.hip:215-232), or + dh_last at the first step walked (:234-237); then the cell backward
    with the carried dc (:248-254)."""
    w = f64(w_hhT)
    H = w.shape[0]
    d = None if dhs_t is None else f64(dhs_t)
    if dG_src16 is not None:
        g = f64(dG_src16)
        rec, mag = g @ w.T, g.abs() @ w.abs().T
        tol = (H + 4) * E * (mag + (0 if d is None else d.abs()))
    else:
        rec, tol = (None if dh_last is None else f64(dh_last)), None
    return lstm_cell_bwd(d, rec, dcs, act_t, c_prev, c_t, frozen=frozen_t, tol_dh=tol, tol_dc_in=tol_dcs)


def lstm_seq_dh0(dG_first16, w_hhT):
    """the extra pass: dh0 = dG[first step] W_hh, (H + 3) E of the magnitudes"""
    w, g = f64(w_hhT), f64(dG_first16)
    return g @ w.T, (w.shape[0] + 3) * E * (g.abs() @ w.abs().T)


def lstm_seq_bwd(dhs, dh_last, dc_last, act, cs, c0, frozen, w_hhT, B, U, reverse=False, dG_stored=None, round_dG=True):
    """the whole backward walk.  dG_stored: the kernel's own stored dG [U][B][4H] — the recurrent term of every step is then taken
    from it (per-step comparison); without it the reference's own (bf16-rounded if round_dG) dG feeds the next step.  The carried
    dc stays in fp64 and its bound grows step by step.  Returns dG, tol_dG [U][B][4H], dh0, tol_dh0, dc0, tol_dc0."""
    act, cs = f64(act).view(U, B, -1), f64(cs).view(U, B, -1)
    H = cs.shape[2]
    dG, tol = torch.zeros(U, B, 4 * H, dtype=F64), torch.zeros(U, B, 4 * H, dtype=F64)
    dcs, tdcs = (None if dc_last is None else f64(dc_last)), None
    src = None
    for n in range(U - 1, -1, -1):
        t = U - 1 - n if reverse else n
        tp = t + 1 if reverse else t - 1
        cp = cs[tp] if n > 0 else c0
        r = lstm_seq_step_bwd(None if dhs is None else f64(dhs).view(U, B, H)[t], src, w_hhT, dh_last if n == U - 1 else None, dcs, tdcs,
                              act[t], cs[t], cp, None if frozen is None else frozen[t])
        dG[t], tol[t] = r["dG"], r["tol_dG"]
        dcs, tdcs = r["dc_prev"], r["tol_dc_prev"]
        src = f64(dG_stored).view(U, B, 4 * H)[t] if dG_stored is not None else (bf(dG[t]) if round_dG else dG[t])
    dh0, tdh0 = lstm_seq_dh0(src, w_hhT)
    return dict(dG=dG, tol_dG=tol, dh0=dh0, tol_dh0=tdh0, dc0=dcs, tol_dc0=tdcs)


# ------------------------------------------------------------------ Bahdanau attention of one decoder step (lstm.hip:97-208)
def _lens(lens, n, T):
    return torch.full((n,), T, dtype=torch.int64) if lens is None else lens.to("cpu").long().clamp(max=T)


def bahdanau_fwd(qp, key, value, nv, bias, lens, kv_col=None):
    """qp [B][A]; key [T][Bkv][A]; value [T][Bkv][Cv]; nv, bias [A]; lens [Bkv] (clamped to T).  Hypothesis b reads sentence
    kv_col[b] (b without kv_col).  Returns p [T][B], ctx [B][Cv] (the value whose bf16 rounding is stored) and their bounds."""
    qp, key, value, nv = f64(qp), f64(key), f64(value), f64(nv)
    T, Bkv, A = key.shape
    B = qp.shape[0]
    col = torch.arange(B) if kv_col is None else kv_col.to("cpu").long()
    k, v = key[:, col], value[:, col]
    L = _lens(lens, Bkv, T)[col]
    bs = torch.zeros(A, dtype=F64) if bias is None else f64(bias)
    x = qp[None] + k + bs
    th = torch.tanh(x)
    tth = tanh_tol(x, 2 * E * (qp[None].abs() + k.abs() + bs.abs()))
    s, smag = (nv * th).sum(-1), (nv.abs() * th.abs()).sum(-1)
    tol_s = (nv.abs() * tth).sum(-1) + (math.ceil(A / 64) + 7) * E * smag
    mask = torch.arange(T).view(T, 1) < L.view(1, B)
    sm = s.masked_fill(~mask, -INF)
    mx = sm.max(0).values
    arg = torch.where(mask, s - mx, torch.zeros_like(s))
    e = torch.where(mask, torch.exp(arg), torch.zeros_like(s))
    den = e.sum(0)
    p = torch.where(den > 0, e / den.clamp_min(TINY), torch.zeros_like(e))
    es = torch.where(mask, tol_s, torch.zeros_like(s)).max(0).values
    rel_e = 2 * es + (2 * arg.abs() + 1) * E
    rel_sum = (p * rel_e).sum(0) + (math.ceil(T / 256) + 10) * E
    tol_p = p * (rel_e + rel_sum + 2 * E) + TINY * mask
    ctx = (p[:, :, None] * v).sum(0)
    cmag = (p[:, :, None] * v.abs()).sum(0)
    tol_ctx = (tol_p[:, :, None] * v.abs()).sum(0) + (L.view(B, 1) + 1) * E * cmag
    return dict(p=p, tol_p=tol_p, ctx=ctx, tol_ctx=tol_ctx, s=s, max_arg=float(arg.abs().max()) if arg.numel() else 0.0, ctx_mag=cmag)


def bahdanau_bwd(dctx, qp, key, value, nv, bias, lens, p, dkey0, dvalue0, dnv0, dbias0):
    """dctx [B][Cv]; key [T][B][A]; value [T][B][Cv]; p [T][B] (fp32, as the forward stored it); d*0: what the accumulators hold
    before the call.  Returns dqp (bf16-stored), dkey, dvalue, dnv, dbias AFTER the call and their bounds."""
    dctx, qp, key, value, nv, p = f64(dctx), f64(qp), f64(key), f64(value), f64(nv), f64(p)
    T, B, A = key.shape
    Cv = value.shape[2]
    L = _lens(lens, B, T)
    mask = torch.arange(T).view(T, 1) < L.view(1, B)
    bs = torch.zeros(A, dtype=F64) if bias is None else f64(bias)
    pm = torch.where(mask, p, torch.zeros_like(p))
    # dp[t] = dctx . value[t]: ceil(Cv / 64) additions per lane, the 6 steps of wave_sum (:161-168)
    dp = torch.where(mask, (dctx[None] * value).sum(-1), torch.zeros_like(p))
    tol_dp = (math.ceil(Cv / 64) + 6) * E * (dctx[None].abs() * value.abs()).sum(-1) * mask
    # dot = sum_t p dp: ceil(L / 256) additions per thread, block_sum (:171-173)
    dot = (pm * dp).sum(0)
    tol_dot = (pm * tol_dp).sum(0) + (math.ceil(T / 256) + 11) * E * (pm * dp.abs()).sum(0)
    ds = pm * (dp - dot)
    tol_ds = pm * (tol_dp + tol_dot) + 2 * E * pm * (dp.abs() + dot.abs())
    # dvalue += p dctx (:177-180): the product, the addition
    dv_add = pm[:, :, None] * dctx[None]
    dvalue = f64(dvalue0) + dv_add
    tol_dvalue = 2 * E * (f64(dvalue0).abs() + dv_add.abs()) * mask[:, :, None]
    # through tanh (:182-199)
    x = qp[None] + bs + key
    th = torch.tanh(x)
    tth = tanh_tol(x, 2 * E * (qp[None].abs() + bs.abs() + key.abs()))
    omq = one_minus_sq_tanh(x)
    dpre = ds[:, :, None] * nv * omq * mask[:, :, None]
    tol_dpre = (tol_ds[:, :, None] * nv.abs() * omq + (ds.abs() + tol_ds)[:, :, None] * nv.abs() * (2 * th.abs() * tth + 2 * E)
                + 3 * E * dpre.abs()) * mask[:, :, None]
    dkey = f64(dkey0) + dpre
    tol_dkey = tol_dpre + E * (f64(dkey0).abs() + dpre.abs()) * mask[:, :, None]
    chain = (torch.ceil(L.double() / 4) + 3).view(B, 1)
    dq = dpre.sum(0)
    tol_dq = tol_dpre.sum(0) + chain * E * dpre.abs().sum(0)
    dnt = ds[:, :, None] * th * mask[:, :, None]
    dn = dnt.sum(0)
    tol_dn = ((tol_ds[:, :, None] * th.abs() + (ds.abs() + tol_ds)[:, :, None] * tth) * mask[:, :, None]).sum(0) + (chain + 1) * E * dnt.abs().sum(0)
    # B atomic additions in any order onto the pre-fill (:201-207)
    dnv_mag = f64(dnv0).abs() + dn.abs().sum(0)
    dnv, tol_dnv = f64(dnv0) + dn.sum(0), tol_dn.sum(0) + B * E * dnv_mag
    db0 = torch.zeros(A, dtype=F64) if dbias0 is None else f64(dbias0)
    dbias_mag = db0.abs() + dq.abs().sum(0)
    dbias, tol_dbias = db0 + dq.sum(0), tol_dq.sum(0) + B * E * dbias_mag
    return dict(dqp=dq, tol_dqp=tol_dq, dkey=dkey, tol_dkey=tol_dkey, dvalue=dvalue, tol_dvalue=tol_dvalue, dnv=dnv, tol_dnv=tol_dnv,
                dnv_mag=dnv_mag, dbias=dbias, tol_dbias=tol_dbias, dbias_mag=dbias_mag, mask=mask, dpre=dpre)


# ------------------------------------------------------------------ decode-step attention (decode.hip:31-176)
def decode_attention(q, K, V, kv_row, lens, max_len):
    """q [N][H][dh]; K, V [rows][>= max_len][H][dh] (the head views of the cache); hypothesis n reads row kv_row[n] (n without it),
    len[row] keys (max_len without lens).  Returns probs [N][H][max_len] (zero from L on) and out [N][H][dh] (bf16-stored)."""
    q, K, V = f64(q), f64(K), f64(V)
    N, H, dh = q.shape
    r = torch.arange(N) if kv_row is None else kv_row.to("cpu").long()
    L = torch.full((N,), max_len, dtype=torch.int64) if lens is None else lens.to("cpu").long()[r]
    k, v = K[r][:, :max_len], V[r][:, :max_len]
    s = torch.einsum("nhd,njhd->nhj", q, k)
    smag = torch.einsum("nhd,njhd->nhj", q.abs(), k.abs())
    # vector kernel: dh / 4 products per lane, two shuffle steps; generic: the 6 steps of wave_sum
    tol_s = (dh / 4 + 6) * E * smag
    mask = torch.arange(max_len).view(1, 1, max_len) < L.view(N, 1, 1)
    mask = mask.expand(N, H, max_len)
    mx = s.masked_fill(~mask, -INF).max(-1, keepdim=True).values
    arg = torch.where(mask, s - mx, torch.zeros_like(s))
    e = torch.where(mask, torch.exp(arg), torch.zeros_like(s))
    den = e.sum(-1, keepdim=True)
    p = torch.where(den > 0, e / den.clamp_min(TINY), torch.zeros_like(e))
    es = torch.where(mask, tol_s, torch.zeros_like(s)).max(-1, keepdim=True).values
    rel_e = 2 * es + (2 * arg.abs() + 1) * E
    rel_sum = (p * rel_e).sum(-1, keepdim=True) + (math.ceil(max_len / 64) + 6) * E
    tol_p = p * (rel_e + rel_sum + 2 * E) + TINY * mask
    out = torch.einsum("nhj,njhd->nhd", p, v)
    omag = torch.einsum("nhj,njhd->nhd", p, v.abs())
    tol_out = torch.einsum("nhj,njhd->nhd", p * (rel_e + rel_sum), v.abs()) + (max_len + 4) * E * omag + TINY
    return dict(probs=p, tol_probs=tol_p, out=out, tol_out=tol_out, max_arg=float(arg.abs().max()), out_mag=omag, L=L)


# ------------------------------------------------------------------ exact data movement and selection (decode.hip:178-266, lstm.hip:83-91)
def gather_rows(x, parent):
    return x[parent.to("cpu").long()]


def kv_append_reorder(old_cache, kv_new, parent, L, new_cache0):
    """new[n][0:L] = old[parent[n]][0:L]; new[n][L] = kv_new[n]; rows L + 1 .. Lmax keep what new_cache0 holds"""
    N = kv_new.shape[0]
    par = torch.arange(N) if parent is None else parent.to("cpu").long()
    new = new_cache0.clone()
    new[:, :L] = old_cache[par][:, :L]
    new[:, L] = kv_new
    return new


def beam_mask_rows(lp, pad, unk, eos, unk_penalty, only_eos, forbid_eos, eos_factor, use_eos_factor):
    """fp32 in, fp32 out, every operation a single IEEE operation: exact to restate.  Rule order as in the kernel: NaN -> -inf,
    pad -> -inf, unk penalty, only_eos; then the eos rules against the row maximum taken after those."""
    v = lp.to("cpu").to(F32).clone()
    V = v.shape[1]
    v[torch.isnan(v)] = -INF
    if 0 <= pad < V:
        v[:, pad] = -INF
    if 0 <= unk < V:
        v[:, unk] = v[:, unk] - torch.tensor(unk_penalty, dtype=F32)
    if only_eos:
        keep = v[:, eos].clone()
        v[:] = -INF
        v[:, eos] = keep
    mx = v.max(1).values
    if not only_eos:
        e = v[:, eos].clone()
        if use_eos_factor:
            e[e < torch.tensor(eos_factor, dtype=F32) * mx] = -INF
        if forbid_eos:
            e[:] = -INF
        v[:, eos] = e
    return v


def beam_topk(lp, prev, bsz, beam, nbeam_used, V, k, lower_index_wins=True):
    """per sentence the k best of lp[s*beam + b][v] + prev[s*beam + b] (one fp32 addition) over b < nbeam_used, descending, ties to
    the lower flat index b * V + v; (-inf, 0, 0) where fewer than k candidates are above -inf"""
    x = lp.to("cpu").to(F32).view(bsz, beam, V)[:, :nbeam_used]
    # (without prev the kernel adds 0.f, decode.hip:237: the one fp32 addition is made either way, and -0 + 0 = +0)
    x = x + (torch.zeros(bsz, beam, 1) if prev is None else prev.to("cpu").to(F32).view(bsz, beam, 1))[:, :nbeam_used]
    flat = x.reshape(bsz, nbeam_used * V)
    score = torch.full((bsz, k), -INF, dtype=F32)
    tok, bm = torch.zeros(bsz, k, dtype=torch.int32), torch.zeros(bsz, k, dtype=torch.int32)
    for s in range(bsz):
        row = flat[s] if lower_index_wins else flat[s].flip(0)
        val, idx = torch.sort(row, descending=True, stable=True)
        if not lower_index_wins:
            idx = row.numel() - 1 - idx
        n = min(k, int((val > -INF).sum()))
        score[s, :n], tok[s, :n], bm[s, :n] = val[:n], (idx[:n] % V).int(), (idx[:n] // V).int()
    return score, tok, bm
