"""StreamingTransducerFrameBeamDecoder — the frame-synchronous transducer beam search of tools/transducer_frame_beam_decoder.py
(TransducerFrameBeamDecoder, which stays as it is) over encoder frames that arrive a chunk at a time, with the interface of the
other streaming decoders (`open`, `accept`, `partial`, `finish`, `close`), optional shallow fusion of one sub-word LSTM LM and
partial results.  The contract is DESIGN.md section 3.5; the streamed form is section 3.4; the slot pool and the rows a stream
carries are those of tools/beam_common.py (StreamSlots, CarriedRows).

Everything a stream carries lives on the device, allocated once: the search state (beam, prefix table, frame counter:
`state_bytes_per_stream()` bytes per slot, csrc/rnnt_beam.hip), the predictor's LSTM state and output row, which start as the
predictor after `bos`, and, with an LM, its LSTM state and log-prob row, which start as the LM after its eos.

`accept` runs `joint_encoder_branch` on the packed rows once, gathers the listed streams' predictor (and LM) rows, and then per
frame index j < max(counts): gathers the frame's encoder rows (ea_gather_rows), `joint_step`, the step
(ea_rnnt_frame_beam_stream_step), `reorder_state` + `advance(token, state, keep_row)` for the predictor (and the LM) — the loop
of the offline decoder; the rows go back to their slots after the last frame.  A stream with fewer frames than j gets the
identity triple from the step (its rows keep their state, as a finished utterance's do offline), so nothing is read back and
nothing synchronises.  The per-frame code is the offline kernels': one body, wrapped once per search (the tests hold the two
wrappers to each other bit for bit), so `close` returns what TransducerFrameBeamDecoder.search returns for the whole utterance,
whatever the pieces.

`partial` reads, per stream, the live hypothesis with the best score and the stable prefix: the tokens shared by every live
hypothesis.  Every later hypothesis is a stay or an extension of a live one (a merge lands on a live sequence), so the stable
tokens never change again.

Hotword biasing: with `context_graph` (tools/context_graph.ContextGraph) the state, the reset, every step, the finish and the
partial are those of the bias family (ea_rnnt_frame_beam_stream_bias_*): a slot also holds the automaton state and the running
bias of every beam slot, `partial` returns the live hypothesis with the best score + running bias, and `close` returns what
TransducerFrameBeamDecoder.search with the same graph returns.  The tables are uploaded once; the loop still reads nothing back.

Time stamps: with `token_times=True` a slot also has a times slot (K.rnnt_frame_beam_stream_times_state), the reset, the steps and
the finish are those of the times family (ea_rnnt_frame_beam_stream_times_*), `finish_tensors` also returns (times, vscores) with
frames counted from the stream's first frame, and `finish` / `close` put "times" and "viterbi_score" into the hypotheses: what the
offline decoder with token_times returns for the whole utterance.  `partial` carries no times.

Endpointing: with `endpoint=EndpointRules(...)` (tools/beam_common.py) the decoder uses the times family and also has
`endpoint_tensors` / `endpoint` (ea_rnnt_frame_beam_stream_endpoint: per stream (rule, F, L, E) of the hypothesis `partial` reports,
read only), `end_segment` (the hypotheses of `finish`, then the slot restarts: search state, times state, predictor and LM rows
start fresh) and `room`.  A segment's hypotheses are, bit for bit, what TransducerFrameBeamDecoder with token_times returns for
that segment's frames alone.  Rules are read after an `accept`, so segments end on piece boundaries; the thresholds count frames
and do not depend on the pieces.  Without `endpoint` nothing changes: a stream that would pass `max_frames` raises."""
from typing import Dict, List

import torch

from .. import kernels as K
from .beam_common import CarriedRows, StreamSlots, hyps_from_tensors, step_triple
from .transducer_frame_beam_decoder import TransducerFrameBeamDecoder


class StreamingTransducerFrameBeamDecoder(StreamSlots):
    def __init__(self, model, dictionary, beam_size, max_streams, max_frames, nbest=1, beam_size_token=None, temperature=1.0,
                 normalize_scores=True, lm_model=None, lm_weight=0.0, model_predicts_eos=False, context_graph=None, token_times=False,
                 endpoint=None):
        # validation and defaults of the offline decoder
        o = TransducerFrameBeamDecoder(model, dictionary, beam_size=beam_size, nbest=nbest, beam_size_token=beam_size_token,
                                       temperature=temperature, normalize_scores=normalize_scores, lm_model=lm_model,
                                       lm_weight=lm_weight, model_predicts_eos=model_predicts_eos, context_graph=context_graph)
        self.offline = o
        self.context_graph = o.context_graph
        self.model, self.lm_model, self.lm_weight = o.model, o.lm_model, o.lm_weight
        self.pad, self.blank, self.bos, self.eos, self.vocab_size = o.pad, o.blank, o.bos, o.eos, o.vocab_size
        self.beam_size, self.beam_size_token, self.nbest = o.beam_size, o.beam_size_token, o.nbest
        self.symbols_to_strip_from_output = o.symbols_to_strip_from_output
        StreamSlots.__init__(self, "streaming transducer frame beam search", max_streams, max_frames)
        self._step = dict(max_frames=self.max_frames, V=o.vocab_size, beam=o.beam_size, K=o.beam_size_token, blank=o.blank,
                          eos=o.eos if o.model_predicts_eos else -1, temperature=o.temperature, lm_weight=o.lm_weight,
                          lm_no_blank=o.no_blank_in_lm)
        self.state = self.graph = None
        self.token_times = bool(token_times) or endpoint is not None  # the endpoint probe reads the times state
        self.endpoint_rules = endpoint
        dev = next(self.model.parameters()).device if self.model is not None else None
        if dev is not None and dev.type == "cuda":
            self._allocate(dev)

    def state_bytes_per_stream(self) -> int:
        from .. import _lib

        if self.context_graph is not None:
            return int(_lib.lib().ea_rnnt_frame_beam_stream_bias_state_bytes(self.max_frames, self.beam_size))
        return int(_lib.lib().ea_rnnt_frame_beam_stream_state_bytes(self.max_frames, self.beam_size))

    # ---- device plumbing -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _allocate(self, device):
        """The search state and the per-slot rows, once; the rows every new stream starts from (the predictor after `bos`, the
        LM after its eos)."""
        R, dec = self.max_streams * self.beam_size, self.model.decoder
        self.graph = self.offline.graph_tables(device)
        make_state = K.rnnt_frame_beam_stream_state if self.graph is None else K.rnnt_frame_beam_stream_bias_state
        self.state, _ = make_state(self.max_streams, self.max_frames, self.beam_size, device)
        if self.token_times:
            self._allocate_times(K.rnnt_frame_beam_stream_times_state, self.beam_size, device)
        out, st = dec.advance(torch.full((1,), self.bos, dtype=torch.int32, device=device), dec.init_state(1, device))
        self.pred = dec.init_state(R, device)
        self.pred_out = out.new_zeros(R, out.shape[1])
        carried = [(self.pred, st), (self.pred_out, out)]
        self.lm = self.lm_rows = None
        if self.lm_model is not None:
            lst, lrows = self.offline.lm_start(1, device)
            self.lm = self.offline.lm_init_state(R, device)
            self.lm_rows = lrows.new_zeros(R, lrows.shape[1])
            carried += [(self.lm, lst), (self.lm_rows, lrows)]
        self._rows = CarriedRows(self.beam_size, self.max_streams, carried)

    def _ensure(self, device):
        """Buffers on `device`; slots opened since the last launch are reset and get their start rows (kernels, no
        synchronisation)."""
        if self.state is None:
            self._allocate(device)
        device = self.state.device
        if self._unreset:
            slots = self._ints(self._unreset, device)
            if self.token_times:
                K.rnnt_frame_beam_stream_times_reset(self.state, self.times_state, slots, self.max_frames, self.beam_size,
                                                     biased=self.graph is not None)
            else:
                reset = K.rnnt_frame_beam_stream_reset if self.graph is None else K.rnnt_frame_beam_stream_bias_reset
                reset(self.state, slots, self.max_frames, self.beam_size)
            self._rows.reset(slots)
            self._unreset = []
        return device

    def _device(self):
        return self.state.device if self.state is not None else next(self.model.parameters()).device

    # ---- the streaming interface -----------------------------------------------------------------------------------------
    @torch.no_grad()
    def accept(self, stream_ids, enc_rows, counts):
        """enc_rows [sum counts][C]: new encoder frames, stream by stream in the order of stream_ids (StreamingEncoder's
        output); advances every stream over its frames.  Nothing is read back."""
        ready, meta = self._pack(stream_ids, counts, enc_rows)
        if not ready:
            return
        model, dec, beam = self.model, self.model.decoder, self.beam_size
        dev = self._ensure(enc_rows.device)
        E = model.joint_encoder_branch(enc_rows.contiguous()).contiguous()
        n, Tm = len(ready), max(c for _, c, _ in ready)
        slot_idx, n_new, row_off = meta[0], meta[1], meta[2]
        rows = self._rows.rows_of(slot_idx)
        # encoder row of every (frame index, listed stream, beam slot); past a stream's count its last row, never used
        frame = torch.minimum(torch.arange(Tm, dtype=torch.int32, device=dev).unsqueeze(1), (n_new - 1).unsqueeze(0))
        frame_rows = (row_off.unsqueeze(0) + frame).repeat_interleave(beam, dim=1).contiguous()  # [Tm][n * beam]
        out = step_triple(n * beam, dev)
        state, dec_out, *lm = self._rows.gather(rows)  # lm: (LSTM state, log-prob rows) with an LM
        for j in range(Tm):
            logits = model.joint_step(K.gather_rows(E, frame_rows[j]), dec_out)
            lm_rows = lm[1] if lm else None
            if self.token_times:
                K.rnnt_frame_beam_stream_times_step(logits, slot_idx, n_new, j, self.state, self.times_state, out, graph=self.graph,
                                                    lm_rows=lm_rows, **self._step)
            elif self.graph is None:
                K.rnnt_frame_beam_stream_step(logits, slot_idx, n_new, j, self.state, out, lm_rows=lm_rows, **self._step)
            else:
                K.rnnt_frame_beam_stream_bias_step(logits, slot_idx, n_new, j, self.state, self.graph, out, lm_rows=lm_rows, **self._step)
            state = dec.reorder_state(state, out[0])
            dec_out, state = dec.advance(out[1], state, keep_row=out[2])
            if lm:
                lm = self.offline.lm_update(lm[0], *out)
        self._rows.scatter(rows, [state, dec_out, *lm])
        self._advance(ready)

    @torch.no_grad()
    def finish_tensors(self, stream_ids, nbest=None, max_u=None):
        """Device tensors (tokens int32 [n][nbest][U], lengths, scores, nhyp; with token_times also times int32 [n][nbest][U]
        and vscores) of the streams as if they ended now; their state is left as it is."""
        slots = self._slots_of(stream_ids, self._ensure(self._device()))
        args = (self.max_frames, self.beam_size, self.nbest if nbest is None else nbest, self.pad,
                self._max_u(stream_ids) if max_u is None else max_u)
        if self.token_times:
            return K.rnnt_frame_beam_stream_times_finish(self.state, self.times_state, slots, *args, graph=self.graph,
                                                         normalize=self.offline.normalize_scores)
        if self.graph is None:
            return K.rnnt_frame_beam_stream_finish(self.state, slots, *args, normalize=self.offline.normalize_scores)
        return K.rnnt_frame_beam_stream_bias_finish(self.state, slots, self.graph, *args, normalize=self.offline.normalize_scores)

    @torch.no_grad()
    def partial_tensors(self, stream_ids, max_u=None):
        """Device tensors (tokens int32 [n][U], lengths, scores, stable_len) of the streams' best live hypotheses."""
        slots = self._slots_of(stream_ids, self._ensure(self._device()))
        partial = K.rnnt_frame_beam_stream_partial if self.graph is None else K.rnnt_frame_beam_stream_bias_partial
        return partial(self.state, slots, self.max_frames, self.beam_size, self.pad, self._max_u(stream_ids) if max_u is None else max_u)

    @torch.no_grad()
    def endpoint_tensors(self, stream_ids):
        """Device tensor int32 [n][4] = (rule, F, L, E) of the streams under the decoder's EndpointRules; the state is read only."""
        self._need_endpoint()
        slots = self._slots_of(stream_ids, self._ensure(self._device()))
        return K.rnnt_frame_beam_stream_endpoint(self.state, self.times_state, slots, self.max_frames, self.beam_size,
                                                 *self.endpoint_rules.frames(), biased=self.graph is not None)

    @torch.no_grad()
    def partial(self, stream_ids):
        """Per stream (tokens of the live hypothesis with the best score, stable_len, score): the first stable_len tokens are
        those every later result starts with.  One readback."""
        if not stream_ids:
            return []
        return self._read_partial(*self.partial_tensors(stream_ids))

    @torch.no_grad()
    def finish(self, sid) -> List[Dict[str, torch.Tensor]]:
        """Up to nbest hypotheses of a stream in the generators' format, as if it ended now; the stream goes on."""
        return hyps_from_tensors(*(t.cpu() for t in self.finish_tensors([sid])))[0]

    @torch.no_grad()
    def close(self, sid) -> List[Dict[str, torch.Tensor]]:
        """`finish`, and the stream's slot is free afterwards."""
        hyps = self.finish(sid)
        self._release(sid)
        return hyps

    _finished = finish
