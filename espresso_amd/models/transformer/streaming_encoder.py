"""StreamingEncoder — exact chunk-by-chunk inference of a chunk-streaming transformer or causal-conformer encoder for many
streams at once.

A model trained with `encoder.chunk_size = cs > 0`, `chunk_left_window = L`, `chunk_right_window = 0` sees, for a frame of
chunk c, the frames of chunks c-L .. c (tools/utils.py chunk_streaming_mask, always_partial_in_last=True at inference).  With
no right window the output of layer l for chunk c depends only on layer l-1 outputs of chunks c-L .. c, so caching every
layer's projected K / V of the last L chunks reproduces the offline masked pass.  The conv sub-sampler has a receptive
field of +-RF feature frames per output frame (6 for the recipes' strides), so a chunk is computed from a window of feature
frames that starts `margin` frames early (a multiple of the total stride, rows discarded) and ends RF frames late;
zero padding then sits only where the offline pass has it (utterance start and true end).

State per stream: unconsumed feature frames (and samples) incl. the look-ahead and the left margin; one bf16 ring of
(L+1)*cs slots x 2C per layer (kernels.stream_kv_append / stream_attention); a device frame counter.  The host mirrors
the counters from the lengths it is given, so no device value is read back to run a chunk.

Conformer layers stream only with `encoder.depthwise_conv_causal`: the depthwise convolution then reads the frame and the
KW-1 before it, so a layer keeps, besides its K / V ring, the last KW-1 rows of the convolution's input per stream (bf16
[KW-1][C], zero at the start of an utterance: its left padding; kernels.stream_glu_dwconv_bn_act).  BatchNorm uses the running
statistics, as every inference pass does.  The reference's symmetric module looks (KW-1)/2 frames ahead in each layer and is
refused.

LayerNorm, the QKV / out-proj / FFN GEMMs and the sub-sampler are the offline path's kernels, run on the [sum n_new][C] rows
of all streams that have a chunk ready."""
from typing import Dict, List, Optional, Sequence

import torch

from ... import functional as F
from ... import kernels as K


def check_streamable(cfg):
    """Raise, naming the option, for encoder configurations whose streaming pass cannot equal the offline one."""
    e = cfg.encoder
    causal = bool(getattr(e, "depthwise_conv_causal", False))
    if e.layer_type != "transformer" and not (e.layer_type == "conformer" and causal):
        ahead = (int(getattr(e, "depthwise_conv_kernel_size", 31)) - 1) // 2
        raise NotImplementedError(
            f"streaming needs encoder.layer_type: transformer, or conformer with encoder.depthwise_conv_causal: true (got "
            f"{e.layer_type} with depthwise_conv_causal: {causal}: the symmetric depthwise convolution looks {ahead} frames ahead in "
            "every layer)")
    if int(e.chunk_size) <= 0:
        raise NotImplementedError("streaming needs a chunk-streaming model: encoder.chunk_size must be > 0")
    if int(e.chunk_right_window) > 0:
        raise NotImplementedError("streaming is exact only without look-ahead: encoder.chunk_right_window must be 0")
    from ...tools import utils as speech_utils

    if speech_utils.eval_str_nested_list_or_tuple(e.conv_channels, type=int) is None:
        raise NotImplementedError("streaming needs the conv sub-sampler: encoder.conv_channels must be set (the offline encoder "
                                  "does not run without it either)")
    tc = speech_utils.eval_str_nested_list_or_tuple(e.transformer_context, type=int)
    if tc is not None and (tc[0] is not None or tc[1] is not None):
        raise NotImplementedError("streaming does not implement encoder.transformer_context (use chunk_size / chunk_left_window)")
    if e.layer_type == "conformer":
        C, KW, cs = int(e.embed_dim), int(e.depthwise_conv_kernel_size), int(e.chunk_size)
        if C % 8 or KW not in (3, 7, 15, 31) or cs > 128:  # what ea_stream_convmodule_supported refuses
            raise NotImplementedError(
                f"streaming a conformer needs encoder.embed_dim % 8 == 0, encoder.depthwise_conv_kernel_size in (3, 7, 15, 31) and "
                f"encoder.chunk_size <= 128 (got embed_dim {C}, depthwise_conv_kernel_size {KW}, chunk_size {cs})")


class _Stream:
    __slots__ = ("slot", "feats", "base", "total", "final", "out_frames", "wav", "wav_done")

    def __init__(self, slot):
        self.slot = slot
        self.feats = None      # device fp32 [n][F]: feature frames base .. base+n
        self.base = 0
        self.total = 0         # feature frames received so far
        self.final = False
        self.out_frames = 0    # encoder frames emitted
        self.wav = None        # unconsumed samples (accept_waveform)
        self.wav_done = False


class StreamingEncoder:
    def __init__(self, model, max_streams: int, frontend=None):
        enc = getattr(model, "encoder", model)
        self.enc = enc
        cfg = enc.cfg
        check_streamable(cfg)
        self.cfg = cfg
        self.cs = int(cfg.encoder.chunk_size)
        self.L = int(cfg.encoder.chunk_left_window)
        self.C = enc.embed_dim
        self.H = cfg.encoder.attention_heads
        self.dh = self.C // self.H
        if not K.stream_attention_supported(self.dh, self.cs, self.L, self.C):
            raise NotImplementedError(
                f"ea_stream_attention does not take head dim {self.dh}, chunk_size {self.cs}, chunk_left_window {self.L}")
        self.max_streams = int(max_streams)
        self.frontend = frontend
        self.device = next(enc.parameters()).device
        pre = enc.pre_encoder
        self.stride = 1
        rf = 0
        for s in pre.strides:  # 3x3 convolutions, padding 1: each adds +-1 frame at its input resolution
            rf += self.stride
            self.stride *= pre._stride2(s)[0]
        self.rf = rf
        self.margin = -(-rf // self.stride) * self.stride  # left discard margin, in feature frames
        self.W = (self.L + 1) * self.cs
        nl = len(enc.layers)
        self.caches = [torch.zeros(self.max_streams, self.W, 2 * self.C, dtype=torch.bfloat16, device=self.device) for _ in range(nl)]
        self.frames = torch.zeros(self.max_streams, dtype=torch.int32, device=self.device)
        # conformer layers: the last KW-1 rows of the depthwise convolution's input per stream, and BatchNorm's mean / rstd from
        # the running statistics (constants of an inference pass)
        self.conformer = cfg.encoder.layer_type == "conformer"
        self.KW = int(cfg.encoder.depthwise_conv_kernel_size) if self.conformer else 0
        self.carries, self._bn_mr, self._dw_w, self._carry_all = [], [], [], None
        if self.conformer:
            if not K.stream_convmodule_supported(self.C, self.KW, self.cs):
                raise NotImplementedError(f"ea_stream_glu_dwconv_bn_act does not take embed_dim {self.C}, depthwise_conv_kernel_size "
                                          f"{self.KW}, chunk_size {self.cs}")
            # one allocation [layers][max_streams][KW-1][C], so that open() clears a slot's rows of every layer in one launch
            self._carry_all = torch.zeros(nl, self.max_streams, self.KW - 1, self.C, dtype=torch.bfloat16, device=self.device)
            self.carries = [self._carry_all[i] for i in range(nl)]
            with torch.no_grad():
                for l in enc.layers:
                    bn = l.conv_module.batch_norm
                    self._bn_mr.append(K.bn_from_running(bn.running_mean, bn.running_var, bn.eps))
                    self._dw_w.append(l.conv_module.depthwise_conv.weight.detach().float().reshape(self.C, self.KW).contiguous())
        self.streams: Dict[object, _Stream] = {}
        self.resampler = None  # a StreamResampler, once a stream is opened at another rate than the front-end's
        self._free = list(range(self.max_streams - 1, -1, -1))
        self._zero_table = None
        with torch.no_grad():
            self._fc0_w = enc._fc0_weight().detach().contiguous() if enc.fc0 is not None else None
            self._pp = [self._projected_table(l) for l in enc.layers]

    # ---- per-model constants -------------------------------------------------------------------------------------------
    def _projected_table(self, layer):
        """bf16 [2W-1][C]: row W-1+d <-> relative position d = key - query, projected by pos_proj once (sinusoidal) or the
        learned table's slice."""
        pe = layer.positional_embedding[0]
        if pe is None:
            return None
        if getattr(pe, "learnable", False):
            return K.cast_f32_to_bf16(pe.table(self.W, self.device, num_heads=self.H, embed_dim=self.C).detach().contiguous())
        t = pe.table(self.W, self.device).contiguous()
        R = t.shape[0]
        pp = torch.empty(R, self.C, dtype=torch.bfloat16, device=self.device)
        K.gemm(t, F.bf16_weight(layer.self_attn.pos_proj.weight), pp, R, self.C, self.C, lda=self.C, ldb=self.C, ldc=self.C)
        return pp

    def cache_bytes_per_stream(self) -> int:
        return len(self.caches) * self.W * 2 * self.C * 2 + len(self.carries) * (self.KW - 1) * self.C * 2

    # ---- stream management ---------------------------------------------------------------------------------------------
    def open(self, stream_ids: Sequence, rates: Optional[Sequence[int]] = None):
        """rates: the sample rate of the audio `accept_waveform` will get for each stream (None: the front-end's).  A stream at
        another rate is converted piece by piece (data/resample.py: StreamResampler), to the bits of an offline conversion."""
        if rates is not None and self.frontend is not None:
            odd = [(sid, int(r)) for sid, r in zip(stream_ids, rates) if int(r) != self.frontend.sample_rate]
            if odd:
                if self.resampler is None:
                    from ...data.resample import StreamResampler

                    self.resampler = StreamResampler(self.device, self.frontend.sample_rate)
                self.resampler.open([sid for sid, _ in odd], [r for _, r in odd])
        for sid in stream_ids:
            if sid in self.streams:
                raise ValueError(f"stream {sid!r} is already open")
            if not self._free:
                raise RuntimeError(f"all {self.max_streams} stream slots are in use")
            st = _Stream(self._free.pop())
            self.streams[sid] = st
            self.frames[st.slot:st.slot + 1].zero_()
            if self._carry_all is not None:  # the utterance's left zero padding
                self._carry_all[:, st.slot].zero_()

    def close(self, stream_ids: Sequence):
        for sid in stream_ids:
            st = self.streams.pop(sid)
            self._free.append(st.slot)
        if self.resampler is not None:
            self.resampler.close(stream_ids)

    # ---- input ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def accept_waveform(self, stream_ids, waves: Sequence[torch.Tensor], final):
        """waves: one 1-D fp32 tensor of new samples per stream (int16 scale, as the front-end expects; at the rate the stream
        was opened with).  Kaldi fbank frames are independent of each other (snip_edges): frame t covers samples
        [t*shift, t*shift + frame_len)."""
        fe = self.frontend
        assert fe is not None, "accept_waveform needs the GpuFbankFrontend given at construction"
        final = [final] * len(stream_ids) if isinstance(final, bool) else list(final)
        if self.resampler is not None:
            odd = [b for b, sid in enumerate(stream_ids) if sid in self.resampler.streams]
            if odd:
                conv = self.resampler.accept([stream_ids[b] for b in odd], [waves[b] for b in odd], [final[b] for b in odd])
                waves = list(waves)
                for b, w in zip(odd, conv):
                    waves[b] = w
        pend, counts = [], []
        for sid, w in zip(stream_ids, waves):
            st = self.streams[sid]
            w = w.to(self.device, torch.float32)
            st.wav = w if st.wav is None else torch.cat([st.wav, w])
            pend.append(st.wav)
            counts.append(int(st.wav.numel()))
        nf = [fe.num_frames(n) for n in counts]
        Tm = max(nf) if nf else 0
        lengths = nf
        if Tm > 0:
            offs = [0]
            for n in counts:
                offs.append(offs[-1] + n)
            feat, _, _ = fe(torch.cat(pend), torch.tensor(offs, dtype=torch.int64).to(self.device), counts, train=False)
        else:
            feat = torch.zeros(len(stream_ids), 0, fe.nmel, device=self.device)
        for sid, n in zip(stream_ids, nf):
            st = self.streams[sid]
            st.wav = st.wav[n * fe.frame_shift:] if n > 0 else st.wav
        return self.accept_features(stream_ids, feat, lengths, final)

    @torch.no_grad()
    def accept_features(self, stream_ids, feats, lengths, final):
        """feats fp32 [B][Tmax][F] (row b: the next lengths[b] feature frames of stream_ids[b]); final: bool or one per stream
        (True: the utterance ends with these frames; its short last chunk is flushed).
        Returns (out bf16/fp32 [sum counts][D] — the encoder's output rows (vocabulary logits when it has fc_out), stream by
        stream in the order of stream_ids, frames in time order — and counts: new encoder frames per stream)."""
        final = [final] * len(stream_ids) if isinstance(final, bool) else list(final)
        lengths = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        sts = [self.streams[s] for s in stream_ids]
        for b, st in enumerate(sts):
            if st.final:
                raise ValueError(f"stream {stream_ids[b]!r} was already given its final piece")
            n = lengths[b]
            if n > 0:
                piece = feats[b, :n].to(self.device, torch.float32)
                st.feats = piece if st.feats is None else torch.cat([st.feats, piece])
                st.total += n
            st.final = bool(final[b])
        outs: List[List[torch.Tensor]] = [[] for _ in sts]
        while True:
            ready = []
            for b, st in enumerate(sts):
                n = self._ready_rows(st)
                if n > 0:
                    ready.append((b, st, n))
            if not ready:
                break
            y, offs = self._step(ready)
            for (b, st, n), r0 in zip(ready, offs):
                outs[b].append(y[r0:r0 + n])
                st.out_frames += n
                self._trim(st)
        counts = [sum(t.shape[0] for t in o) for o in outs]
        flat = [t for o in outs for t in o]
        if not flat:
            return None, counts
        return (flat[0] if len(flat) == 1 else torch.cat(flat)), counts

    # ---- chunk scheduling (host integers only) ----------------------------------------------------------------------------
    def max_rows_per_accept(self, n_samples: int, rate: Optional[int] = None) -> int:
        """An upper bound on the encoder frames one `accept_waveform` of at most n_samples new samples returns for a stream: the
        rows of the new feature frames, plus what the stream held back (less than a chunk and the receptive field of its last
        row), which a final piece flushes.  rate: the rate n_samples are counted at (None: the front-end's); what the resampler
        held back of earlier pieces (its filter's reach, K inputs) comes out with a later one."""
        if rate is not None and int(rate) != self.frontend.sample_rate:
            from ...data.resample import resample_plan

            fo = self.frontend.sample_rate
            n_samples = -(-(n_samples + resample_plan(int(rate), fo).K + 1) * fo // int(rate)) + 1
        n = n_samples // self.frontend.frame_shift + 2  # the samples left over from the last piece complete one more frame
        return -(-n // self.stride) + self.cs + -(-(self.rf + 1) // self.stride) + 1

    def _out_total(self, st):
        return -(-st.total // self.stride)

    def _ready_rows(self, st) -> int:
        """Rows of the next chunk when it can be computed now, else 0."""
        o0 = st.out_frames
        if st.final:
            return min(self.cs, self._out_total(st) - o0)
        need = self.stride * (o0 + self.cs - 1) + self.rf + 1  # last frame in the receptive field of the chunk's last row
        return self.cs if st.total >= need else 0

    def _window(self, st, n):
        o0 = st.out_frames
        s0 = max(0, self.stride * o0 - self.margin)
        e0 = st.total if (st.final and o0 + n >= self._out_total(st)) else self.stride * (o0 + n - 1) + self.rf + 1
        return s0, min(e0, st.total)

    def _trim(self, st):
        keep_from = max(0, self.stride * st.out_frames - self.margin)
        if st.feats is not None and keep_from > st.base:
            st.feats = st.feats[keep_from - st.base:]
            st.base = keep_from

    # ---- one chunk for every ready stream --------------------------------------------------------------------------------
    def _step(self, ready):
        enc, cs, C, H = self.enc, self.cs, self.C, self.H
        B = len(ready)
        offs, r = [], 0
        for _, _, n in ready:
            offs.append(r)
            r += n
        M = r
        # sub-sampler: streams grouped by window length so that no row of a call is padded (the batched pass lets a padded
        # tail leak into the last real frames)
        groups: Dict[tuple, list] = {}
        for k, (_, st, n) in enumerate(ready):
            s0, e0 = self._window(st, n)
            groups.setdefault((e0 - s0, st.out_frames - s0 // self.stride), []).append((k, st, n, s0, e0))
        parts, gidx, row_base = [], [0] * M, 0
        for (wl, discard), members in groups.items():
            src = torch.stack([st.feats[s0 - st.base:e0 - st.base] for _, st, _, s0, e0 in members])
            lens = torch.full((len(members),), wl, dtype=torch.long, device=self.device)
            xg = enc.pre_encoder(src, lens)[0]
            Tw = xg.shape[0] // len(members)
            for gi, (k, _, n, _, _) in enumerate(members):
                for i in range(n):
                    gidx[offs[k] + i] = row_base + gi * Tw + discard + i
            parts.append(xg)
            row_base += xg.shape[0]
        xs = parts[0] if len(parts) == 1 else torch.cat(parts)
        # one upload per chunk: (slot, n_new, row_off) [3][B], sub-sampler row gather [M], absolute positions [M] as int64
        pos = [v for _, st, n in ready for i in range(n) for v in (st.out_frames + i + 1, 0)]
        head = [st.slot for _, st, _ in ready] + [n for _, _, n in ready] + offs + gidx
        if len(head) % 2:
            head.append(0)  # keeps the int64 view of the positions 8-byte aligned
        host = torch.tensor(head + pos, dtype=torch.int32)
        if self.device.type == "cuda":
            host = host.pin_memory()
        dev = host.to(self.device, non_blocking=True)
        pos64 = dev[len(head):].view(torch.int64)
        meta = dev[:3 * B].view(3, B)
        x = K.gather_rows(xs.contiguous(), dev[3 * B:3 * B + M])
        if enc.fc0 is not None:
            x = F.linear(x, self._fc0_w, enc.fc0.bias)
        if enc.abs_positions or enc.embed_scale != 1.0:
            x = self._add_positions(x, pos64)
        if enc.layernorm_embedding is not None:
            x = F.layer_norm(x, enc.layernorm_embedding.weight, enc.layernorm_embedding.bias)
        run_layer = self._conformer_layer if self.conformer else self._layer
        for li, layer in enumerate(enc.layers):
            x = run_layer(layer, li, x, meta, B, M)
        if enc.layer_norm is not None:
            x = F.layer_norm(x, enc.layer_norm.weight, enc.layer_norm.bias)
        K.stream_advance(self.frames, meta, B, cs)
        fc_out = getattr(enc, "fc_out", None)
        if fc_out is not None:
            x = F.linear(x, fc_out.weight, fc_out.bias)
        return x, offs

    def _add_positions(self, x, pos):
        enc = self.enc
        if not enc.abs_positions:  # embed_scale alone: a one-row zero table and zero indices, made once
            if self._zero_table is None:
                self._zero_table = (torch.zeros(1, self.C, device=x.device),
                                    torch.zeros(self.cs * self.max_streams, dtype=torch.int64, device=x.device))
            table, pos = self._zero_table[0], self._zero_table[1][:pos.shape[0]]
        elif enc.embed_positions is not None:
            table = enc.embed_positions.weight
        else:
            need = int(max(st.out_frames for st in self.streams.values())) + self.cs + 2
            if enc._sin_table is None or enc._sin_table.shape[0] < need or enc._sin_table.device != x.device:
                from .speech_transformer_base import sinusoidal_positional_table

                enc._sin_table = sinusoidal_positional_table(max(2 * need, 1024), self.C, 0).to(x.device)
            table = enc._sin_table
        return F.add_positions(x, table, pos, enc.embed_scale)

    def _attention(self, layer, li, x, meta, B, M, pre_ln):
        """x + out_proj(attention over the ring cache) of the new rows; `pre_ln`: LayerNorm before the QKV projection."""
        C, H, dh, cs, L = self.C, self.H, self.dh, self.cs, self.L
        a = layer.self_attn
        pp = self._pp[li]
        ln1 = layer.self_attn_layer_norm
        xn = K.layernorm_fwd(x, ln1.weight, ln1.bias, 1e-5)[0] if pre_ln else x
        _, bqkv, wqkv16 = a.fused_qkv()
        qkv = torch.empty(M, 3 * C, dtype=torch.bfloat16, device=x.device)
        K.gemm(xn, wqkv16, qkv, M, 3 * C, C, lda=C, ldb=C, ldc=3 * C, bias=bqkv)
        relpos = pp is not None
        learned = relpos and a.pos_proj is None
        scaling = dh ** -0.5
        if learned or not relpos:
            qu, _ = K.relpos_q_prep(qkv, 3 * C, None, None, M, C, scaling, want_qv=False)
            qv = qu
        else:
            qu, qv = K.relpos_q_prep(qkv, 3 * C, a.pos_bias_u, a.pos_bias_v, M, C, scaling, want_qv=True)
        K.stream_kv_append(qkv[:, C:], 3 * C, self.caches[li], meta, self.frames, B, C, cs, L, M)
        o = K.stream_attention(qu, qv, self.caches[li], pp, self.W - 1, meta, self.frames, B, H, dh, cs, L)
        y = torch.empty(M, C, dtype=torch.bfloat16, device=x.device)
        K.gemm(o, F.bf16_weight(a.out_proj.weight), y, M, C, C, lda=C, ldb=C, ldc=C, bias=a.out_proj.bias, resid=x, ldr=C)
        return y

    def _layer(self, layer, li, x, meta, B, M):
        pre_ln = layer.normalize_before
        ln1 = layer.self_attn_layer_norm
        y = self._attention(layer, li, x, meta, B, M, pre_ln)
        act = "silu" if layer.activation_fn == "swish" else layer.activation_fn
        fl = layer.final_layer_norm
        if pre_ln:
            return F.ffn_module(y, fl.weight, fl.bias, layer.fc1.weight, layer.fc1.bias, layer.fc2.weight, layer.fc2.bias, act=act,
                                out_scale=1.0)
        y = F.layer_norm(y, ln1.weight, ln1.bias)
        y = F.ffn_module(y, None, None, layer.fc1.weight, layer.fc1.bias, layer.fc2.weight, layer.fc2.bias, act=act, out_scale=1.0)
        return F.layer_norm(y, fl.weight, fl.bias)

    def _conformer_layer(self, layer, li, x, meta, B, M):
        """ConformerWithRelativePositionalEmbeddingEncoderLayer.forward for the new rows: ffn1, attention over the ring cache, the
        convolution module with the carried rows, ffn2, final LayerNorm."""
        C = self.C
        f = layer.ffn1
        x = F.ffn_module(x, f.layer_norm.weight, f.layer_norm.bias, f.w_1.weight, f.w_1.bias, f.w_2.weight, f.w_2.bias, act="silu",
                         out_scale=0.5)
        x = self._attention(layer, li, x, meta, B, M, True)
        c = layer.conv_module
        xn = K.layernorm_fwd(x, c.layer_norm.weight, c.layer_norm.bias, 1e-5)[0]
        Y = torch.empty(M, 2 * C, dtype=torch.bfloat16, device=x.device)
        K.gemm(xn, F.bf16_weight(c.pointwise_conv1.weight).view(2 * C, C), Y, M, 2 * C, C, lda=C, ldb=C, ldc=2 * C)
        Hh = K.stream_glu_dwconv_bn_act(Y, self._dw_w[li], self._bn_mr[li], c.batch_norm.weight, c.batch_norm.bias, self.carries[li],
                                        meta, B, self.cs)
        y = torch.empty(M, C, dtype=torch.bfloat16, device=x.device)
        K.gemm(Hh, F.bf16_weight(c.pointwise_conv2.weight).view(C, C), y, M, C, C, lda=C, ldb=C, ldc=C, resid=x, ldr=C)
        f = layer.ffn2
        y = F.ffn_module(y, f.layer_norm.weight, f.layer_norm.bias, f.w_1.weight, f.w_1.bias, f.w_2.weight, f.w_2.bias, act="silu",
                         out_scale=0.5)
        return F.layer_norm(y, layer.final_layer_norm.weight, layer.final_layer_norm.bias)
