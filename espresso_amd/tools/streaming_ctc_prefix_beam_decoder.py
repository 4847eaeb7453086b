"""StreamingCTCPrefixBeamDecoder — the CTC prefix beam search of tools/ctc_prefix_beam_search.py (CTCPrefixBeamSearchDecoder,
which stays as it is) over encoder frames that arrive a chunk at a time: alone, with shallow fusion of one sub-word LSTM LM,
with hotword biasing (`context_graph`) or with both, with the interface of StreamingCTCLexiconBeamDecoder (`open`, `accept`,
`accept_lprobs`, `partial`, `finish`, `close`) and partial results.  The streamed form is DESIGN.md section 3.4; the slot pool
and the rows a stream carries are those of tools/beam_common.py (StreamSlots, CarriedRows).

Everything a stream carries lives on the device, allocated once: the search state (frame counter, beam, prefix table with its
hash, the hypotheses' states in the context graph and running biases: `state_bytes_per_stream()` bytes per slot,
csrc/ctc_beam.hip) and, with an LM, its LSTM state and log-prob row, which start as the LM after its eos (with a
models.token_ngram_lm.TokenNGramLM: one int32 context row in place of the LSTM state, starting after <s>).

Without an LM `accept_lprobs` is one launch (ea_ctc_prefix_beam_stream_step) for all the streams that got frames.  With one it
gathers the listed streams' LM rows and then per frame index j < max(counts): the step of frame j, `lm_update(state, parent,
token, keep)` — the loop of the offline decoder; the rows go back to their slots after the last frame.  A stream with fewer
frames than j gets the identity triple from the step (its rows keep their state, as a finished utterance's do offline), so
nothing is read back and nothing synchronises.  The per-frame code is the offline kernel's (one body, two wrappers), so `close`
returns, bit for bit, what CTCPrefixBeamSearchDecoder.search returns for the whole utterance, whatever the pieces and whatever
`max_frames`.

`partial` reads, per stream, the hypothesis the beam currently ranks first (its in-beam score: LM and running bias included,
the LM's end-of-sentence term and the bias still pending not) and the stable prefix: the tokens shared by every live hypothesis
with a finite score.  Every later hypothesis with a finite score is a stay or an extension of one of those (a merge lands on
the extension of one), so the stable tokens never change again.

Time stamps: with `token_times=True` a slot also has a times slot (K.ctc_prefix_beam_stream_times_state), the reset, the steps and
the finish are those of the times family (ea_ctc_prefix_beam_stream_times_*), `finish` also returns (times, vscores) with frames
counted from the stream's first frame, and `close` puts "times" and "viterbi_score" into the hypotheses: what the offline
decoder with token_times returns for the whole utterance.  `partial` carries no times.

Endpointing: with `endpoint=EndpointRules(...)` (tools/beam_common.py) the decoder uses the times family and also has
`endpoint_tensors` / `endpoint` (ea_ctc_prefix_beam_stream_endpoint: per stream (rule, F, L, E) of the hypothesis `partial` reports,
read only), `end_segment` (the hypotheses of `finish`, then the slot restarts: search state, times state and LM rows start fresh)
and `room`.  A segment's hypotheses are, bit for bit, what CTCPrefixBeamSearchDecoder with token_times returns for that segment's
frames alone.  Rules are read after an `accept`, so segments end on piece boundaries; the thresholds count frames and do not
depend on the pieces.  Without `endpoint` nothing changes: a stream that would pass `max_frames` raises."""
from typing import Dict, List

import torch

from .. import kernels as K
from .beam_common import CarriedRows, StreamSlots, hyps_from_tensors, is_token_ngram, step_triple
from .ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder


class StreamingCTCPrefixBeamDecoder(StreamSlots):
    def __init__(self, dictionary, max_streams, max_frames, beam_size=10, nbest=1, beam_size_token=None, lm_model=None, lm_weight=0.0,
                 insertion_bonus=0.0, blank=None, context_graph=None, token_times=False, endpoint=None):
        # validation and defaults of the offline decoder
        o = CTCPrefixBeamSearchDecoder([None], dictionary, beam_size=beam_size, nbest=nbest, beam_size_token=beam_size_token,
                                       lm_model=lm_model, lm_weight=lm_weight, insertion_bonus=insertion_bonus, blank=blank,
                                       context_graph=context_graph)
        self.offline = o
        self.context_graph, self.lm_model = o.context_graph, o.lm_model
        self.pad, self.eos, self.blank, self.vocab_size = o.pad, o.eos, o.blank, o.vocab_size
        self.beam_size, self.beam_size_token, self.nbest = o.beam_size, o.beam_size_token, o.nbest
        self.lm_weight, self.insertion_bonus = o.lm_weight, o.insertion_bonus
        StreamSlots.__init__(self, "streaming CTC prefix beam search", max_streams, max_frames)
        self._search = dict(max_frames=self.max_frames, V=o.vocab_size, beam=o.beam_size, K=o.beam_size_token, blank=o.blank,
                            ins_bonus=o.insertion_bonus)
        self.state = self.graph = self.lm = self.lm_rows = self._rows = None  # allocated on the device of the first frames
        self.token_times = bool(token_times) or endpoint is not None  # the endpoint probe reads the times state
        self.endpoint_rules = endpoint

    def state_bytes_per_stream(self) -> int:
        from .. import _lib

        return int(_lib.lib().ea_ctc_prefix_beam_stream_state_bytes(self.max_frames, self.beam_size))

    # ---- device plumbing -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _allocate(self, device):
        """The search state, the graph tables and, with an LM, the per-slot rows and the row every new stream starts from (the
        LM after its eos), once."""
        self.state, _ = K.ctc_prefix_beam_stream_state(self.max_streams, self.max_frames, self.beam_size, device)
        if self.token_times:
            self._allocate_times(K.ctc_prefix_beam_stream_times_state, self.beam_size, device)
        if self.context_graph is not None:
            self.graph = self.context_graph.cuda(device)
        if self.lm_model is not None:
            R = self.max_streams * self.beam_size
            start_state, start_rows = self.offline.lm_start(1, device)
            self.lm = self.offline.lm_init_state(R, device)
            self.lm_rows = start_rows.new_zeros(R, start_rows.shape[1])
            self._rows = CarriedRows(self.beam_size, self.max_streams, [(self.lm, start_state), (self.lm_rows, start_rows)])

    def _ensure(self, device):
        """Buffers on `device`; slots opened since the last launch are reset and get their LM-start rows (kernels, no
        synchronisation)."""
        if self.state is None:
            self._allocate(device)
        device = self.state.device
        if self._unreset:
            slots = self._ints(self._unreset, device)
            if self.token_times:
                K.ctc_prefix_beam_stream_times_reset(self.state, self.times_state, slots, self.max_frames, self.beam_size)
            else:
                K.ctc_prefix_beam_stream_reset(self.state, slots, self.max_frames, self.beam_size)
            if self.lm is not None:
                self._rows.reset(slots)
            self._unreset = []
        return device

    def _device(self):
        if self.state is not None:
            return self.state.device
        if is_token_ngram(self.lm_model):
            if self.lm_model.device is not None:
                return self.lm_model.device
        elif self.lm_model is not None:
            return next(self.lm_model.parameters()).device
        return torch.device("cuda", torch.cuda.current_device())

    # ---- the streaming interface -----------------------------------------------------------------------------------------
    @torch.no_grad()
    def accept(self, stream_ids, logits, counts):
        """logits [sum counts][>=V] (StreamingEncoder output, stream by stream): log-softmax, then `accept_lprobs`."""
        M = sum(counts)
        if M == 0:
            return
        self._check_room(stream_ids, counts)
        self.accept_lprobs(stream_ids, K.log_softmax(logits, M, self.vocab_size, logits.stride(0)), counts)

    @torch.no_grad()
    def accept_lprobs(self, stream_ids, lprobs, counts):
        """lprobs fp32/bf16 [sum counts][V] log-probs, packed stream by stream in the order of stream_ids.  Nothing is read back."""
        ready, meta = self._pack(stream_ids, counts, lprobs)
        if not ready:
            return
        dev = self._ensure(lprobs.device)
        Tm = max(c for _, c, _ in ready)
        if self.token_times:
            def step(lprobs, meta, state, **kw):
                K.ctc_prefix_beam_stream_times_step(lprobs, meta, state, self.times_state, **kw)
        else:
            step = K.ctc_prefix_beam_stream_step
        if self.lm is None:
            step(lprobs, meta, self.state, graph=self.graph, j0=0, j1=Tm, **self._search)
        else:
            rows = self._rows.rows_of(meta[0])
            lm_state, lm_rows = self._rows.gather(rows)
            lm_out = step_triple(len(ready) * self.beam_size, dev)
            for j in range(Tm):
                step(lprobs, meta, self.state, graph=self.graph, j0=j, j1=j + 1, lm_rows=lm_rows, lm_weight=self.lm_weight,
                     lm_out=lm_out, **self._search)
                lm_state, lm_rows = self.offline.lm_update(lm_state, *lm_out)
            self._rows.scatter(rows, [lm_state, lm_rows])
        self._advance(ready)

    @torch.no_grad()
    def finish(self, stream_ids, nbest=None, max_u=None):
        """Device tensors (tokens int32 [n][nbest][U], lengths, scores, nhyp; with token_times also times int32 [n][nbest][U]
        and vscores) of the streams as if they ended now; their state is left as it is."""
        slots = self._slots_of(stream_ids, self._ensure(self._device()))
        lm = {}
        if self.lm is not None:
            lm = dict(lm_rows=K.gather_rows(self.lm_rows, self._rows.rows_of(slots)), lm_weight=self.lm_weight, eos=self.eos)
        args = (slots, self.max_frames, self.beam_size, self.nbest if nbest is None else nbest, self.pad,
                self._max_u(stream_ids) if max_u is None else max_u)
        if self.token_times:
            return K.ctc_prefix_beam_stream_times_finish(self.state, self.times_state, *args, graph=self.graph,
                                                         ins_bonus=self.insertion_bonus, **lm)
        return K.ctc_prefix_beam_stream_finish(self.state, *args, graph=self.graph, ins_bonus=self.insertion_bonus, **lm)

    @torch.no_grad()
    def partial_tensors(self, stream_ids, max_u=None):
        """Device tensors (tokens int32 [n][U], lengths, scores, stable_len) of the streams' best live hypotheses."""
        slots = self._slots_of(stream_ids, self._ensure(self._device()))
        return K.ctc_prefix_beam_stream_partial(self.state, slots, self.max_frames, self.beam_size, self.pad,
                                                self._max_u(stream_ids) if max_u is None else max_u,
                                                lm_weight=self.lm_weight if self.lm is not None else 0.0, ins_bonus=self.insertion_bonus,
                                                biased=self.graph is not None)

    @torch.no_grad()
    def endpoint_tensors(self, stream_ids):
        """Device tensor int32 [n][4] = (rule, F, L, E) of the streams under the decoder's EndpointRules; the state is read only."""
        self._need_endpoint()
        slots = self._slots_of(stream_ids, self._ensure(self._device()))
        return K.ctc_prefix_beam_stream_endpoint(self.state, self.times_state, slots, self.max_frames, self.beam_size,
                                                 *self.endpoint_rules.frames(), lm_weight=self.lm_weight if self.lm is not None else 0.0,
                                                 ins_bonus=self.insertion_bonus, biased=self.graph is not None)

    @torch.no_grad()
    def partial(self, stream_ids) -> List[Dict[str, object]]:
        """Per stream: `tokens` of the hypothesis the beam ranks first, its in-beam `score` and `stable`, the leading tokens
        that every later result starts with.  One readback."""
        if not stream_ids:
            return []
        return [{"tokens": toks, "stable": toks[:k], "score": score}
                for toks, k, score in self._read_partial(*self.partial_tensors(stream_ids))]

    @torch.no_grad()
    def close(self, sid) -> List[Dict[str, torch.Tensor]]:
        """Up to nbest finished hypotheses of a stream in the generators' format; its slot is free afterwards."""
        hyps = self._finished(sid)
        self._release(sid)
        return hyps

    def _finished(self, sid):
        return hyps_from_tensors(*(t.cpu() for t in self.finish([sid])))[0]
