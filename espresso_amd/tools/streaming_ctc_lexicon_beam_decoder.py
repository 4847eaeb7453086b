"""StreamingCTCLexiconBeamDecoder — the lexicon-constrained CTC prefix beam search with n-gram fusion of
tools/ctc_lexicon_beam_search.py over encoder frames that arrive a chunk at a time, with the interface of
StreamingCTCDecoder (`open`, `accept`, `close`) and partial results.

The search state of a stream (the beam and its prefix table, `state_bytes_per_stream()` bytes) stays on the device in one
of `max_streams` slots; the slot pool, the refusal of a stream that would pass `max_frames` and the (slot, n_new, row_off)
description of an `accept` are those of tools/beam_common.py (StreamSlots).  `accept` is a log-softmax and one launch
(csrc/ctc_lexicon_beam.hip, ea_ctc_lexicon_stream_step) for all the streams that got frames; nothing comes back to the host.
The per-frame code is the offline kernel's, so `close` returns, bit for bit, what CTCLexiconBeamSearchDecoder.search returns
for the whole utterance, whatever the pieces.

`partial` reads, per stream, the hypothesis the beam currently ranks first and the stable prefix: the tokens shared by
every live hypothesis with a finite score.  A hypothesis with a finite score has only prefixes with finite scores, so every
hypothesis that can still be returned descends from one of those: the stable tokens never change again."""
from typing import Dict, List

import torch

from .. import kernels as K
from .beam_common import StreamSlots, hyps_from_tensors
from .ctc_lexicon_beam_search import CTCLexiconBeamSearchDecoder


class StreamingCTCLexiconBeamDecoder(StreamSlots):
    def __init__(self, dictionary, ngram_lm, lexicon, max_streams, max_frames, beam_size=10, nbest=1, beam_size_token=None,
                 lm_weight=2.0, word_score=-1.0, insertion_bonus=0.0, blank=None):
        # validation and defaults of the offline decoder
        o = CTCLexiconBeamSearchDecoder([None], dictionary, ngram_lm, lexicon, beam_size=beam_size, nbest=nbest,
                                        beam_size_token=beam_size_token, lm_weight=lm_weight, word_score=word_score,
                                        insertion_bonus=insertion_bonus, blank=blank)
        self.offline = o
        self.pad, self.blank, self.vocab_size = o.pad, o.blank, o.vocab_size
        self.beam_size, self.beam_size_token, self.nbest = o.beam_size, o.beam_size_token, o.nbest
        self.lm_weight, self.word_score, self.insertion_bonus = o.lm_weight, o.word_score, o.insertion_bonus
        self.ngram_lm, self.lexicon = ngram_lm, lexicon
        StreamSlots.__init__(self, "streaming CTC lexicon beam search", max_streams, max_frames)
        self.state = None  # allocated on the device of the first frames

    def state_bytes_per_stream(self) -> int:
        from .. import _lib

        return int(_lib.lib().ea_ctc_lexicon_stream_state_bytes(self.max_frames, self.beam_size))

    # ---- device plumbing -------------------------------------------------------------------------------------------------
    def _ensure(self, device):
        """State buffer and tables on `device`; slots opened since the last launch are reset (a kernel, no synchronisation)."""
        if self.state is None:
            self.state, _ = K.ctc_lexicon_stream_state(self.max_streams, self.max_frames, self.beam_size, device)
        device = self.state.device
        tables = self.offline._tables(device)
        if self._unreset:
            K.ctc_lexicon_stream_reset(self.state, self._ints(self._unreset, device), self.ngram_lm.handle, self.max_frames,
                                       self.beam_size)
            self._unreset = []
        return tables

    def _device(self):
        if self.state is not None:
            return self.state.device
        return self.ngram_lm.device if self.ngram_lm.device is not None else torch.device("cuda", torch.cuda.current_device())

    # ---- the streaming interface -----------------------------------------------------------------------------------------
    @torch.no_grad()
    def accept(self, stream_ids, logits, counts):
        """logits [sum counts][>=V] (StreamingEncoder output, stream by stream): log-softmax, then one step launch."""
        M = sum(counts)
        if M == 0:
            return
        self._check_room(stream_ids, counts)
        self.accept_lprobs(stream_ids, K.log_softmax(logits, M, self.vocab_size, logits.stride(0)), counts)

    @torch.no_grad()
    def accept_lprobs(self, stream_ids, lprobs, counts):
        """lprobs fp32/bf16 [sum counts][V] log-probs, packed stream by stream in the order of stream_ids."""
        ready, meta = self._pack(stream_ids, counts, lprobs)
        if not ready:
            return
        trie, word_start = self._ensure(lprobs.device)
        K.ctc_lexicon_stream_step(lprobs, meta, self.state, self.ngram_lm.handle, trie, word_start, self.lexicon.space,
                                  self.max_frames, self.vocab_size, self.beam_size, self.beam_size_token, self.blank,
                                  self.lm_weight, self.word_score, self.insertion_bonus)
        self._advance(ready)

    @torch.no_grad()
    def finish(self, stream_ids, nbest=None):
        """Device tensors (tokens int32 [n][nbest][U], lengths, scores, nhyp) of the streams as if they ended now; their
        state is left as it is."""
        dev = self._device()
        trie, _ = self._ensure(dev)
        return K.ctc_lexicon_stream_finish(self.state, self._slots_of(stream_ids, dev), self.ngram_lm.handle, trie, self.max_frames,
                                           self.beam_size, self.nbest if nbest is None else nbest, self.pad,
                                           self._max_u(stream_ids), self.lm_weight, self.word_score, self.insertion_bonus)

    @torch.no_grad()
    def partial(self, stream_ids) -> List[Dict[str, object]]:
        """Per stream: `tokens` of the hypothesis the beam ranks first, its in-beam `score` (smeared LM sum included) and
        `stable`, the leading tokens that every later result starts with.  One readback."""
        if not stream_ids:
            return []
        dev = self._device()
        self._ensure(dev)
        out = K.ctc_lexicon_stream_partial(self.state, self._slots_of(stream_ids, dev), self.max_frames, self.beam_size, self.pad,
                                           self._max_u(stream_ids), self.insertion_bonus)
        return [{"tokens": toks, "stable": toks[:k], "score": score} for toks, k, score in self._read_partial(*out)]

    @torch.no_grad()
    def close(self, sid):
        """Up to nbest finished hypotheses of a stream in the generators' format (an empty one scored -inf when none is
        finite); its slot is free afterwards."""
        hyps = hyps_from_tensors(*(t.cpu() for t in self.finish([sid])))[0]
        self._release(sid)
        return hyps or [self.offline._empty_hypothesis()]
