"""Plain-torch restatements for the causal Conformer convolution (`encoder.depthwise_conv_causal`): left padding KW-1, no
look-ahead,  Z[t] = sum_k w[k] * U[t - (KW-1) + k]  with zeros before frame 0 of an utterance.

  conv_module / causal_oracle   oracle.torch_ref.conv_module restated with the causal padding, and a context manager that puts it
                                in torch_ref.conv_module's place, so torch_ref.encoder(...) runs a causal model (the reference
                                has no such option: nothing under oracle/ knows it)
  dwconv / glu_dwconv_bwd / dwconv_wgrad
                                the fp64 kernel references of tests/convmodule_ref.py with the causal left pad, from its _shifted
  ConformerStreamRef / run      fp32 chunk-by-chunk restatement of a chunk-streaming causal Conformer encoder (sinusoidal relative
                                positions): per layer the K / V of the last L chunks and the last KW-1 rows of the convolution's
                                input; sub-sampler windows as tests/streaming_ref.py computes them
No call into espresso_amd."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import torch_ref
from tests import convmodule_ref as R
from tests import streaming_ref


# ---- the oracle's convolution module, causal -------------------------------------------------------------------------------
def conv_module(x_btc, sd, p, training, causal, update=None):
    """oracle.torch_ref.conv_module (fairseq/modules/conformer_layer.py:79-101) with `causal`: the depthwise convolution sees
    F.pad(y, (KW-1, 0)) and pads nothing itself.  x: (B, T, C)."""
    _ln, _r, _bn, _drop = torch_ref._ln, torch_ref._r, torch_ref._bn, torch_ref._drop
    y = _ln(x_btc, sd, p + "layer_norm.").transpose(1, 2)
    y = _r(F.conv1d(y, _r(sd[p + "pointwise_conv1.weight"])))
    y = _r(F.glu(y, dim=1))
    w = sd[p + "depthwise_conv.weight"]  # (fp32 in the HIP kernel)
    if causal:
        y = _r(F.conv1d(F.pad(y, (w.shape[-1] - 1, 0)), w, groups=w.shape[0]))
    else:
        y = _r(F.conv1d(y, w, padding=(w.shape[-1] - 1) // 2, groups=w.shape[0]))
    y = _bn(y, sd, p + "batch_norm.", training, update=update)
    y = _r(F.silu(y))
    y = F.conv1d(y, _r(sd[p + "pointwise_conv2.weight"]))
    return _drop(y, "conv.out", "BCT").transpose(1, 2)  # :100


@contextlib.contextmanager
def causal_oracle():
    """Inside, torch_ref.conformer_layer (hence torch_ref.encoder) uses the causal convolution module."""
    orig = torch_ref.conv_module
    torch_ref.conv_module = lambda x_btc, sd, p, training, update=None: conv_module(x_btc, sd, p, training, True, update)
    try:
        yield
    finally:
        torch_ref.conv_module = orig


# ---- fp64 kernel references (tests/convmodule_ref.py with PAD = KW-1) ---------------------------------------------------------
def dwconv(U, w, B, T, KW):
    """Z[b,t,c] = sum_k w[c,k] * U[b, t-(KW-1)+k, c], zero outside [0,T) per utterance  ->  (Z, sum_k |w*u|)"""
    U, w = R.f64(U), R.f64(w)
    Z, mag = torch.zeros_like(U), torch.zeros_like(U)
    for k in range(KW):
        term = R._shifted(U, B, T, k - (KW - 1)) * w[:, k]
        Z += term
        mag += term.abs()
    return Z, mag


def glu_dwconv_bwd(dZ, Y, w, B, T, KW):
    """dU[t] = sum_k w[k] * dZ[t+(KW-1)-k], then the GLU backward  ->  (dY [M][2C], sum_k |w*dz| times the same factor)"""
    dZ, Y, w = R.f64(dZ), R.f64(Y), R.f64(w)
    C = dZ.shape[-1]
    dU, mag = torch.zeros_like(dZ), torch.zeros_like(dZ)
    for k in range(KW):
        term = R._shifted(dZ, B, T, (KW - 1) - k) * w[:, k]
        dU += term
        mag += term.abs()
    a, sg = Y[:, :C], torch.sigmoid(Y[:, C:])
    fa, fg = sg, a * sg * (1.0 - sg)
    return torch.cat([dU * fa, dU * fg], 1), torch.cat([mag * fa.abs(), mag * fg.abs()], 1)


def dwconv_wgrad(dZ, U, B, T, KW):
    """dw[c,k] = sum_{b,t} dZ[b,t,c] * U[b, t-(KW-1)+k, c]  ->  (dw [C][KW], sum |dz*u|)"""
    dZ, U = R.f64(dZ), R.f64(U)
    dw = torch.zeros(dZ.shape[-1], KW, dtype=torch.float64, device=dZ.device)
    mag = torch.zeros_like(dw)
    for k in range(KW):
        term = dZ * R._shifted(U, B, T, k - (KW - 1))
        dw[:, k] = term.sum(0)
        mag[:, k] = term.abs().sum(0)
    return dw, mag


# ---- streamed restatement ---------------------------------------------------------------------------------------------------
class ConformerStreamRef:
    """One stream.  State: unconsumed feature frames; per layer the (K, V) of at most L+1 chunks and the last KW-1 rows of the
    depthwise convolution's input (zeros at the start: the utterance's left padding)."""

    def __init__(self, sd, H, cs, L):
        self.sd = {k: v.float() for k, v in sd.items() if v.is_floating_point()}
        self.H, self.cs, self.L = H, cs, L
        self.nl = 0
        while f"layers.{self.nl}.final_layer_norm.weight" in sd:
            self.nl += 1
        C = self.sd["fc0.weight"].shape[0]
        self.KW = self.sd["layers.0.conv_module.depthwise_conv.weight"].shape[-1]
        self.pe = torch_ref.sinusoidal_rel_pe((L + 1) * cs, C)  # row (L+1)*cs - 1 + d <-> distance d = key - query
        self.feats, self.total, self.out_frames, self.final = None, 0, 0, False
        self.kc = [[] for _ in range(self.nl)]
        self.carry = [torch.zeros(self.KW - 1, C) for _ in range(self.nl)]

    def accept(self, piece, final=False):
        S = streaming_ref
        self.feats = piece if self.feats is None else torch.cat([self.feats, piece])
        self.total = self.feats.shape[0]
        self.final = final
        outs = []
        while True:
            o0 = self.out_frames
            if self.final:
                n = min(self.cs, -(-self.total // S.STRIDE) - o0)
            else:
                n = self.cs if self.total >= S.STRIDE * (o0 + self.cs - 1) + S.RF + 1 else 0
            if n <= 0:
                break
            outs.append(self._chunk(o0, n))
            self.out_frames += n
        return torch.cat(outs) if outs else torch.zeros(0, self.sd["fc_out.weight"].shape[0])

    def _ln(self, x, p):
        return F.layer_norm(x, (x.shape[-1],), self.sd[p + "weight"], self.sd[p + "bias"], 1e-5)

    def _ffn(self, x, p):
        sd = self.sd
        y = F.linear(self._ln(x, p + "layer_norm."), sd[p + "w_1.weight"], sd[p + "w_1.bias"])
        return F.linear(F.silu(y), sd[p + "w_2.weight"], sd[p + "w_2.bias"])

    def _chunk(self, o0, n):
        S, sd = streaming_ref, self.sd
        s0 = max(0, S.STRIDE * o0 - S.MARGIN)
        last = self.final and o0 + n >= -(-self.total // S.STRIDE)
        e0 = self.total if last else min(self.total, S.STRIDE * (o0 + n - 1) + S.RF + 1)
        d = o0 - s0 // S.STRIDE
        x = S.subsample(self.feats[s0:e0], sd)[d:d + n]
        x = F.linear(x, sd["fc0.weight"], sd["fc0.bias"])
        if "layernorm_embedding.weight" in sd:
            x = self._ln(x, "layernorm_embedding.")
        for l in range(self.nl):
            x = self._layer(l, x, o0)
        return F.linear(x, sd["fc_out.weight"], sd["fc_out.bias"])

    def _attention(self, l, x, o0):
        sd, H = self.sd, self.H
        a = f"layers.{l}.self_attn."
        n, C = x.shape
        dh = C // H
        q = F.linear(x, sd[a + "q_proj.weight"], sd[a + "q_proj.bias"])
        k = F.linear(x, sd[a + "k_proj.weight"], sd[a + "k_proj.bias"])
        v = F.linear(x, sd[a + "v_proj.weight"], sd[a + "v_proj.bias"])
        self.kc[l].append((k, v))
        self.kc[l] = self.kc[l][-(self.L + 1):]
        Kc, Vc = torch.cat([e[0] for e in self.kc[l]]), torch.cat([e[1] for e in self.kc[l]])
        Sn = Kc.shape[0]
        key_pos = torch.arange(o0 + n - Sn, o0 + n)  # the cache holds the Sn frames that end with this chunk
        qu = ((q + sd[a + "pos_bias_u"].reshape(-1)) * dh ** -0.5).view(n, H, dh)
        qv = ((q + sd[a + "pos_bias_v"].reshape(-1)) * dh ** -0.5).view(n, H, dh)
        pp = F.linear(self.pe, sd[a + "pos_proj.weight"]).view(-1, H, dh)
        idx = (self.pe.shape[0] // 2) + key_pos[None, :] - (o0 + torch.arange(n))[:, None]  # [n][Sn]
        s = torch.einsum("nhd,shd->hns", qu, Kc.view(Sn, H, dh)) + torch.einsum("nhd,nshd->hns", qv, pp[idx])
        o = torch.einsum("hns,shd->nhd", torch.softmax(s, -1), Vc.view(Sn, H, dh)).reshape(n, C)
        return F.linear(o, sd[a + "out_proj.weight"], sd[a + "out_proj.bias"])

    def _conv(self, l, x):
        sd, p = self.sd, f"layers.{l}.conv_module."
        y = F.linear(self._ln(x, p + "layer_norm."), sd[p + "pointwise_conv1.weight"][:, :, 0])
        u = F.glu(y, dim=1)
        X = torch.cat([self.carry[l], u])              # [KW-1+n][C]
        self.carry[l] = X[X.shape[0] - (self.KW - 1):]
        w = sd[p + "depthwise_conv.weight"]            # [C][1][KW]
        z = F.conv1d(X.t()[None], w, groups=w.shape[0])[0].t()
        b = p + "batch_norm."
        z = F.batch_norm(z, sd[b + "running_mean"], sd[b + "running_var"], sd[b + "weight"], sd[b + "bias"], False, 0.0, 1e-5)
        return F.linear(F.silu(z), sd[p + "pointwise_conv2.weight"][:, :, 0])

    def _layer(self, l, x, o0):
        p = f"layers.{l}."
        x = 0.5 * self._ffn(x, p + "ffn1.") + x
        x = self._attention(l, self._ln(x, p + "self_attn_layer_norm."), o0) + x
        x = self._conv(l, x) + x
        x = 0.5 * self._ffn(x, p + "ffn2.") + x
        return self._ln(x, p + "final_layer_norm.")


def run(sd, feats, pieces, H, cs, L):
    """Feed `feats` [T][F] in pieces of the given sizes (cycled); the last piece is marked final."""
    r = ConformerStreamRef(sd, H, cs, L)
    outs, pos, k = [], 0, 0
    while pos < feats.shape[0]:
        n = min(pieces[k % len(pieces)], feats.shape[0] - pos)
        k += 1
        outs.append(r.accept(feats[pos:pos + n], final=pos + n >= feats.shape[0]))
        pos += n
    return torch.cat(outs)
