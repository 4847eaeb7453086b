"""fp32 chunk-by-chunk restatement of a chunk-streaming transformer encoder (absolute positions, pre- or post-LN) with explicit
per-layer K / V caches and windowed sub-sampling, written from the streaming description: a chunk of `cs` encoder frames is
computed as soon as the feature frames of its receptive field (+-RF around frame stride*j) are there, from a window that
starts `margin` frames early (rows discarded) — zero padding only at the utterance start and its true end — and attends to the
cached K / V of the previous L chunks plus its own."""
import torch
import torch.nn.functional as F

STRIDES = ((1, 1), (2, 2), (1, 1), (2, 2))
STRIDE, RF, MARGIN = 4, 6, 8


def subsample(window, sd):
    """conv3x3 + BatchNorm (running statistics) + ReLU x 4 on one unpadded window [T][F] -> [ceil(T/4)][F' * C] (c * F' + f)."""
    x = window[None, None]
    i = 0
    while f"pre_encoder.convolutions.{i}.weight" in sd:
        x = F.conv2d(x, sd[f"pre_encoder.convolutions.{i}.weight"], sd[f"pre_encoder.convolutions.{i}.bias"], stride=STRIDES[i], padding=1)
        p = f"pre_encoder.batchnorms.{i}."
        x = F.relu(F.batch_norm(x, sd[p + "running_mean"], sd[p + "running_var"], sd[p + "weight"], sd[p + "bias"], False, 0.0, 1e-5))
        i += 1
    return x[0].permute(1, 0, 2).reshape(x.shape[2], -1)


def cache_keys(c, n, cs, L):
    """Absolute frame indices the cache holds when chunk c (n rows) is processed."""
    return list(range(max(0, c - L) * cs, c * cs + n))


class StreamRef:
    def __init__(self, sd, H, cs, L, normalize_before):
        self.sd, self.H, self.cs, self.L, self.pre_ln = {k: v.float() for k, v in sd.items() if v.is_floating_point()}, H, cs, L, normalize_before
        self.nl = 0
        while f"layers.{self.nl}.fc1.weight" in sd:
            self.nl += 1
        self.feats = None
        self.total = 0
        self.out_frames = 0
        self.kc = [[] for _ in range(self.nl)]  # per layer: list of (K, V) per chunk, at most L + 1 kept
        self.final = False

    def accept(self, piece, final=False):
        self.feats = piece if self.feats is None else torch.cat([self.feats, piece])
        self.total = self.feats.shape[0]
        self.final = final
        outs = []
        while True:
            o0 = self.out_frames
            if self.final:
                n = min(self.cs, -(-self.total // STRIDE) - o0)
            else:
                n = self.cs if self.total >= STRIDE * (o0 + self.cs - 1) + RF + 1 else 0
            if n <= 0:
                break
            outs.append(self._chunk(o0, n))
            self.out_frames += n
        return torch.cat(outs) if outs else torch.zeros(0, self.sd["fc_out.weight"].shape[0])

    def _ln(self, x, p):
        return F.layer_norm(x, (x.shape[-1],), self.sd[p + "weight"], self.sd[p + "bias"], 1e-5)

    def _chunk(self, o0, n):
        sd = self.sd
        s0 = max(0, STRIDE * o0 - MARGIN)
        last = self.final and o0 + n >= -(-self.total // STRIDE)
        e0 = self.total if last else min(self.total, STRIDE * (o0 + n - 1) + RF + 1)
        d = o0 - s0 // STRIDE
        x = subsample(self.feats[s0:e0], sd)[d:d + n]
        x = F.linear(x, sd["fc0.weight"], sd["fc0.bias"])
        if "embed_positions.weight" in sd:
            x = x + sd["embed_positions.weight"][o0 + 1:o0 + n + 1]
        if "layernorm_embedding.weight" in sd:
            x = self._ln(x, "layernorm_embedding.")
        for l in range(self.nl):
            x = self._layer(l, x)
        if "layer_norm.weight" in sd:
            x = self._ln(x, "layer_norm.")
        return F.linear(x, sd["fc_out.weight"], sd["fc_out.bias"])

    def _layer(self, l, x):
        sd, H = self.sd, self.H
        p = f"layers.{l}."
        C = x.shape[1]
        dh = C // H
        xin = self._ln(x, p + "self_attn_layer_norm.") if self.pre_ln else x
        a = p + "self_attn."
        q = F.linear(xin, sd[a + "q_proj.weight"], sd[a + "q_proj.bias"]) * dh ** -0.5
        k = F.linear(xin, sd[a + "k_proj.weight"], sd[a + "k_proj.bias"])
        v = F.linear(xin, sd[a + "v_proj.weight"], sd[a + "v_proj.bias"])
        self.kc[l].append((k, v))
        self.kc[l] = self.kc[l][-(self.L + 1):]
        Kc = torch.cat([e[0] for e in self.kc[l]])
        Vc = torch.cat([e[1] for e in self.kc[l]])
        n, S = x.shape[0], Kc.shape[0]
        s = torch.einsum("nhd,shd->hns", q.view(n, H, dh), Kc.view(S, H, dh))
        o = torch.einsum("hns,shd->nhd", torch.softmax(s, -1), Vc.view(S, H, dh)).reshape(n, C)
        y = F.linear(o, sd[a + "out_proj.weight"], sd[a + "out_proj.bias"]) + x
        if not self.pre_ln:
            y = self._ln(y, p + "self_attn_layer_norm.")
            z = F.linear(F.relu(F.linear(y, sd[p + "fc1.weight"], sd[p + "fc1.bias"])), sd[p + "fc2.weight"], sd[p + "fc2.bias"])
            return self._ln(y + z, p + "final_layer_norm.")
        z = self._ln(y, p + "final_layer_norm.")
        z = F.linear(F.relu(F.linear(z, sd[p + "fc1.weight"], sd[p + "fc1.bias"])), sd[p + "fc2.weight"], sd[p + "fc2.bias"])
        return y + z


def run(sd, feats, pieces, H, cs, L, normalize_before):
    """Feed `feats` [T][F] in pieces of the given sizes (cycled); the last piece is marked final."""
    r = StreamRef(sd, H, cs, L, normalize_before)
    outs, pos, k = [], 0, 0
    while pos < feats.shape[0]:
        n = min(pieces[k % len(pieces)], feats.shape[0] - pos)
        k += 1
        outs.append(r.accept(feats[pos:pos + n], final=pos + n >= feats.shape[0]))
        pos += n
    return torch.cat(outs)
