"""StreamingCTCLexiconBeamDecoder — the lexicon-constrained CTC prefix beam search with n-gram fusion of
tools/ctc_lexicon_beam_search.py over encoder frames that arrive a chunk at a time, with the interface of
StreamingCTCDecoder (`open`, `accept`, `close`) and partial results.

The search state of a stream (the beam and its prefix table, `state_bytes_per_stream()` bytes) stays on the device in one
of `max_streams` slots.  `accept` is a log-softmax and one launch (csrc/ctc_lexicon_beam.hip, ea_ctc_lexicon_stream_step)
for all the streams that got frames; nothing comes back to the host.  The per-frame code is the offline kernel's, so `close`
returns, bit for bit, what CTCLexiconBeamSearchDecoder.search returns for the whole utterance, whatever the pieces.

`partial` reads, per stream, the hypothesis the beam currently ranks first and the stable prefix: the tokens shared by
every live hypothesis with a finite score.  A hypothesis with a finite score has only prefixes with finite scores, so every
hypothesis that can still be returned descends from one of those: the stable tokens never change again.

The prefix table of a slot is sized for `max_frames` encoder frames; a stream that would pass it is refused before anything
is launched."""
from typing import Dict, List

import torch

from .. import kernels as K
from .ctc_lexicon_beam_search import CTCLexiconBeamSearchDecoder


class StreamingCTCLexiconBeamDecoder:
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
        if max_streams < 1 or max_frames < 1:
            raise ValueError(f"streaming CTC lexicon beam search: max_streams {max_streams} and max_frames {max_frames} must be positive")
        self.max_streams, self.max_frames = int(max_streams), int(max_frames)
        self.state = None  # allocated on the device of the first frames
        self._free = list(range(self.max_streams - 1, -1, -1))
        self.streams: Dict[object, list] = {}  # stream id -> [slot, frames consumed]
        self._unreset: List[int] = []

    def state_bytes_per_stream(self) -> int:
        from .. import _lib

        return int(_lib.lib().ea_ctc_lexicon_stream_state_bytes(self.max_frames, self.beam_size))

    # ---- device plumbing -------------------------------------------------------------------------------------------------
    def _ints(self, values, device):
        host = torch.tensor(values, dtype=torch.int32)
        if device.type == "cuda":
            host = host.pin_memory()
        return host.to(device, non_blocking=True)

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
    def open(self, stream_ids):
        for sid in stream_ids:
            if sid in self.streams:
                raise ValueError(f"stream {sid!r} is already open")
            if not self._free:
                raise RuntimeError(f"all {self.max_streams} stream slots are in use")
            slot = self._free.pop()
            self.streams[sid] = [slot, 0]
            self._unreset.append(slot)

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
        counts = [int(c) for c in counts]
        assert len(stream_ids) == len(counts) and len(set(stream_ids)) == len(stream_ids) and lprobs.shape[0] == sum(counts)
        self._check_room(stream_ids, counts)
        ready = [(self.streams[sid], c) for sid, c in zip(stream_ids, counts)]
        if not any(c for _, c in ready):
            return
        trie, word_start = self._ensure(lprobs.device)
        offs, r = [], 0
        for _, c in ready:
            offs.append(r)
            r += c
        meta = self._ints([st[0] for st, _ in ready] + [c for _, c in ready] + offs, lprobs.device).view(3, len(ready))
        K.ctc_lexicon_stream_step(lprobs, meta, self.state, self.ngram_lm.handle, trie, word_start, self.lexicon.space,
                                  self.max_frames, self.vocab_size, self.beam_size, self.beam_size_token, self.blank,
                                  self.lm_weight, self.word_score, self.insertion_bonus)
        for st, c in ready:
            st[1] += c

    def _check_room(self, stream_ids, counts):
        for sid, c in zip(stream_ids, counts):
            if self.streams[sid][1] + int(c) > self.max_frames:
                raise ValueError(f"stream {sid!r}: {self.streams[sid][1]} + {int(c)} encoder frames exceed max_frames {self.max_frames}")

    def _max_u(self, stream_ids):
        return max([1] + [self.streams[sid][1] for sid in stream_ids])

    @torch.no_grad()
    def finish(self, stream_ids, nbest=None):
        """Device tensors (tokens int32 [n][nbest][U], lengths, scores, nhyp) of the streams as if they ended now; their
        state is left as it is."""
        dev = self._device()
        trie, _ = self._ensure(dev)
        slots = self._ints([self.streams[sid][0] for sid in stream_ids], dev)
        return K.ctc_lexicon_stream_finish(self.state, slots, self.ngram_lm.handle, trie, self.max_frames, self.beam_size,
                                           self.nbest if nbest is None else nbest, self.pad, self._max_u(stream_ids),
                                           self.lm_weight, self.word_score, self.insertion_bonus)

    @torch.no_grad()
    def partial(self, stream_ids) -> List[Dict[str, object]]:
        """Per stream: `tokens` of the hypothesis the beam ranks first, its in-beam `score` (smeared LM sum included) and
        `stable`, the leading tokens that every later result starts with.  One readback."""
        if not stream_ids:
            return []
        dev = self._device()
        self._ensure(dev)
        slots = self._ints([self.streams[sid][0] for sid in stream_ids], dev)
        U = self._max_u(stream_ids)
        tokens, lengths, scores, stable = K.ctc_lexicon_stream_partial(self.state, slots, self.max_frames, self.beam_size, self.pad,
                                                                       U, self.insertion_bonus)
        packed = torch.cat([tokens, lengths[:, None], stable[:, None], scores.view(torch.int32)[:, None]], dim=1).cpu()
        out = []
        for row in packed:
            n, k = int(row[U]), int(row[U + 1])
            toks = row[:n].tolist()
            out.append({"tokens": toks, "stable": toks[:k], "score": float(row[U + 2:U + 3].view(torch.float32))})
        return out

    @torch.no_grad()
    def close(self, sid):
        """Up to nbest finished hypotheses of a stream in the generators' format (an empty one scored -inf when none is
        finite); its slot is free afterwards."""
        tokens, lengths, scores, nhyp = (t.cpu() for t in self.finish([sid]))
        slot, _ = self.streams.pop(sid)
        self._free.append(slot)
        hyps = [{"tokens": tokens[0, i, : int(lengths[0, i])].to(torch.long), "score": scores[0, i], "attention": None,
                 "alignment": None} for i in range(int(nhyp[0]))]
        if not hyps:
            hyps = [{"tokens": torch.zeros(0, dtype=torch.long), "score": torch.tensor(float("-inf")), "attention": None,
                     "alignment": None}]
        return hyps
