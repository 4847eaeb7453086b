"""What the beam-search decoders share on the host: the hypothesis lists of `generate`, the triple a
step writes, the LM stepping of the offline decoders (BeamDecoderMixin: the LSTM LM, or the sub-word n-gram LM of
models/token_ngram_lm.py, whose state is one int32 context row per hypothesis), and for the three streamed decoders the pool of state
slots (StreamSlots) and the rows a stream carries between `accept` calls besides its search state (CarriedRows).

A streamed decoder keeps, per open stream, one of `max_streams` slots of its device state and the number of encoder frames
consumed.  `open` only marks a slot: the decoder's `_ensure` resets the slots listed in `_unreset` before the next launch that
needs them.  A released slot is the next one handed out.  An `accept` describes its work to the step kernels as `meta`, int32
[3][n] = (slot, n_new, row_off) of the streams that got frames, uploaded in one pinned copy; a stream that would pass
`max_frames` is refused before that.  With an LSTM (predictor, LM) the rows of slot s are rows s * beam .. s * beam + beam - 1
of [max_streams * beam]-row tensors: gathered before the frame loop of an `accept`, scattered back after it."""
from typing import Dict, List

import torch

from .. import kernels as K


def hyps_from_tensors(tokens, lengths, scores, nhyp, times=None, vscores=None) -> List[List[Dict[str, torch.Tensor]]]:
    """Host tensors (tokens [B][nbest][U], lengths [B][nbest], scores [B][nbest], nhyp [B]) of a search -> per utterance its
    nhyp hypotheses in the generators' format, best first.  With the outputs of a search with time stamps (times int32
    [B][nbest][U], vscores fp32 [B][nbest]) every hypothesis also has "times" (int64 [len]: the encoder frame at which each
    token starts on its best alignment path) and "viterbi_score" (that path's score)."""
    hyps = [[{"tokens": tokens[b, i, : int(lengths[b, i])].to(torch.long), "score": scores[b, i], "attention": None,
              "alignment": None} for i in range(int(nhyp[b]))] for b in range(tokens.shape[0])]
    if times is not None:
        for b, utt in enumerate(hyps):
            for i, h in enumerate(utt):
                h["times"] = times[b, i, : int(lengths[b, i])].to(torch.long)
                h["viterbi_score"] = vscores[b, i]
    return hyps


def step_triple(N, device):
    """(parent int32, token int32, keep uint8), each [N]: what a step writes for the predictor / LM update that follows it."""
    return (torch.empty(N, dtype=torch.int32, device=device), torch.empty(N, dtype=torch.int32, device=device),
            torch.empty(N, dtype=torch.uint8, device=device))


def is_token_ngram(lm_model):
    """Whether a decoder's `lm_model` is the sub-word n-gram LM (models/token_ngram_lm.py) rather than the LSTM LM."""
    from ..models.token_ngram_lm import TokenNGramLM

    return isinstance(lm_model, TokenNGramLM)


def check_token_ngram(lm_model, lm_weight, dictionary, blank, search_name):
    """A decoder's constructor, for a TokenNGramLM: it is built over the decoder's dictionary and for the decoder's blank (the
    column it holds at -inf), and its weight is positive (its rows hold -inf, and 0 * -inf in the fusion is NaN)."""
    if list(lm_model.dictionary.symbols) != list(dictionary.symbols):
        raise ValueError(f"{search_name}: the token n-gram LM was built for another dictionary")
    if lm_model.blank != blank:
        raise ValueError(f"{search_name}: the token n-gram LM was built with blank {lm_model.blank}, the search's blank is {blank}")
    if not lm_weight > 0:
        raise ValueError(f"{search_name}: a token n-gram LM needs lm_weight > 0 (got {lm_weight}): its rows hold -inf")


class BeamDecoderMixin:
    """`decode` and the LM state of the beams for a decoder with `_generate`, `eos` and (for the LM methods) `lm_model`."""

    def _lm_tokens(self, tokens):
        """Search token ids -> the LM dictionary's."""
        return tokens

    def _lm_rows(self, feat):
        logits = self.lm_model.decoder.output_layer(feat)
        return K.log_softmax(logits, logits.shape[0], logits.shape[1], logits.stride(0))

    def lm_start(self, N, device):
        """LM state and log-prob rows fp32 [N][LM vocabulary] of N empty hypotheses: the LSTM state after the LM's eos as BOS,
        or with a TokenNGramLM the n-gram contexts after <s>."""
        if is_token_ngram(self.lm_model):
            return self.lm_model.start(N, device)
        lmd = self.lm_model.decoder
        state = lmd.init_state(N, device)
        feat, state = lmd.advance(self._lm_tokens(torch.full((N,), self.eos, dtype=torch.int32, device=device)), state)
        return state, self._lm_rows(feat)

    def lm_update(self, state, parent, token, keep):
        """After one step: every row continues row `parent` of the previous frame; rows with keep == 0 appended `token`, the
        others keep their parent's LM state (and so recompute its row)."""
        if is_token_ngram(self.lm_model):
            return self.lm_model.update(state, parent, token, keep)
        lmd = self.lm_model.decoder
        state = lmd.reorder_state(state, parent)
        feat, state = lmd.advance(self._lm_tokens(token), state, keep_row=keep)
        return state, self._lm_rows(feat)

    def lm_init_state(self, N, device):
        """The LM state of N rows that a reset fills before anything reads them (the streamed decoders' per-slot rows)."""
        if is_token_ngram(self.lm_model):
            return self.lm_model.init_state(N, device)
        return self.lm_model.decoder.init_state(N, device)

    @torch.no_grad()
    def decode(self, models, sample, **kwargs):
        """(1-best tokens B x U padded with pad, scores B (-inf: no hypothesis), None) — the validation-time API of the
        generators."""
        tokens, lengths, scores, _ = self._generate(sample)
        U = max(1, int(lengths[:, 0].max()))
        return tokens[:, 0, :U].to(torch.long), scores[:, 0], None


class EndpointRules:
    """When a streamed CTC / transducer beam search ends a segment ("Endpointing"): three thresholds in
    encoder frames, each switched off when <= 0.  For a slot with F frames whose best live hypothesis has L tokens, the last of
    them starting at frame E of its best alignment path (-1 when L == 0), the rule is the first that holds of
      1 "silence": L > 0 and F - 1 - E >= silence_frames (that many frames after the last token's),
      2 "empty":   L == 0 and F >= empty_frames,
      3 "length":  F >= segment_frames,
    else 0.  The endpoint kernels (ea_*_stream_endpoint) evaluate exactly this on the device; `decide` restates it on the host.
    4 "room" is the caller's: a segment ended because the next piece would not fit the slot (`StreamSlots.room`)."""

    NAMES = ("", "silence", "empty", "length", "room")
    SILENCE, EMPTY, LENGTH, ROOM = 1, 2, 3, 4

    def __init__(self, silence_frames=0, empty_frames=0, segment_frames=0):
        self.silence_frames, self.empty_frames, self.segment_frames = int(silence_frames), int(empty_frames), int(segment_frames)

    def frames(self):
        return self.silence_frames, self.empty_frames, self.segment_frames

    def decide(self, F, L, E) -> int:
        if self.silence_frames > 0 and L > 0 and F - 1 - E >= self.silence_frames:
            return self.SILENCE
        if self.empty_frames > 0 and L == 0 and F >= self.empty_frames:
            return self.EMPTY
        if self.segment_frames > 0 and F >= self.segment_frames:
            return self.LENGTH
        return 0


class StreamSlots:
    """The slot pool of a streamed beam decoder: `streams` maps a stream id to [slot, frames consumed].

    Endpointing (the CTC prefix and the transducer frame beam decoders, built with `endpoint=EndpointRules(...)`): `endpoint`
    reads the rule of every listed stream, `end_segment` returns what `finish` gives for a stream and restarts its slot, and
    `room` names the streams whose next piece would not fit, whose segment the caller ends first.  Rules are read after an
    `accept`, so a segment ends on a piece boundary; the thresholds themselves count frames and do not depend on the pieces."""

    def __init__(self, search_name, max_streams, max_frames):
        if max_streams < 1 or max_frames < 1:
            raise ValueError(f"{search_name}: max_streams {max_streams} and max_frames {max_frames} must be positive")
        self.max_streams, self.max_frames = int(max_streams), int(max_frames)
        self._free = list(range(self.max_streams - 1, -1, -1))
        self.streams: Dict[object, list] = {}
        self._unreset: List[int] = []  # slots opened since the last reset launch
        self.times_state = None  # the per-slot state of the time stamps, for a decoder asked for them
        self.endpoint_rules = None  # EndpointRules of a decoder built with `endpoint`

    def restart(self, sid):
        """The stream starts a new segment in the slot it has: its frame count goes to 0 and the decoder's `_ensure` resets the
        slot (search state, times state, LM / predictor rows) before the next launch that needs it."""
        st = self.streams[sid]
        st[1] = 0
        if st[0] not in self._unreset:
            self._unreset.append(st[0])

    def room(self, stream_ids, counts):
        """The streams whose next piece (`counts` encoder frames) would pass max_frames: the caller ends their segment before
        that accept (rule 4, "room"), so an endpointed stream never raises for room.  A piece longer than max_frames itself
        never fits."""
        return [sid for sid, c in zip(stream_ids, counts) if self.streams[sid][1] > 0 and self.streams[sid][1] + int(c) > self.max_frames]

    def _need_endpoint(self):
        if self.endpoint_rules is None:
            raise ValueError("this decoder was built without `endpoint` rules")

    @torch.no_grad()
    def endpoint(self, stream_ids):
        """Per stream (rule, F, L, E) of EndpointRules, from one readback of `endpoint_tensors`."""
        if not stream_ids:
            return []
        return [tuple(row) for row in self.endpoint_tensors(stream_ids).cpu().tolist()]

    @torch.no_grad()
    def end_segment(self, sid) -> List[Dict[str, torch.Tensor]]:
        """Up to nbest finished hypotheses (with "times" and "viterbi_score", frames counted from the segment's first frame) of
        the stream's current segment, as `close` returns them; the stream stays open and starts a new segment in its slot."""
        self._need_endpoint()
        hyps = self._finished(sid)  # the decoder's: what its `close` reads before it releases the slot
        self.restart(sid)
        return hyps

    def _allocate_times(self, make_state, beam, device):
        """The times state beside the search state (make_state: the K.*_stream_times_state of the search); the decoder's reset
        launch resets a slot's times slot with the slot."""
        self.times_state, _ = make_state(self.max_streams, self.max_frames, beam, device)

    def open(self, stream_ids):
        for sid in stream_ids:
            if sid in self.streams:
                raise ValueError(f"stream {sid!r} is already open")
            if not self._free:
                raise RuntimeError(f"all {self.max_streams} stream slots are in use")
            slot = self._free.pop()
            self.streams[sid] = [slot, 0]
            self._unreset.append(slot)

    def _release(self, sid):
        slot, _ = self.streams.pop(sid)
        self._free.append(slot)

    def _check_room(self, stream_ids, counts):
        for sid, c in zip(stream_ids, counts):
            if self.streams[sid][1] + int(c) > self.max_frames:
                raise ValueError(f"stream {sid!r}: {self.streams[sid][1]} + {int(c)} encoder frames exceed max_frames {self.max_frames}")

    def _max_u(self, stream_ids):
        return max([1] + [self.streams[sid][1] for sid in stream_ids])

    @staticmethod
    def _ints(values, device):
        host = torch.tensor(values, dtype=torch.int32)
        if device.type == "cuda":
            host = host.pin_memory()
        return host.to(device, non_blocking=True)

    def _slots_of(self, stream_ids, device):
        return self._ints([self.streams[sid][0] for sid in stream_ids], device)

    def _pack(self, stream_ids, counts, rows):
        """The pieces of an `accept`: rows [sum counts][...] packed stream by stream in the order of stream_ids.  Returns
        (ready, meta): ready lists (stream entry, count, row offset) of the streams that got frames, meta is int32 [3][n] =
        (slot, n_new, row_off) of those on the device of `rows`; ([], None) when there is nothing to do.  A stream that would
        pass max_frames raises before anything is uploaded."""
        counts = [int(c) for c in counts]
        assert len(stream_ids) == len(counts) and len(set(stream_ids)) == len(stream_ids) and rows.shape[0] == sum(counts)
        self._check_room(stream_ids, counts)
        ready, r = [], 0
        for sid, c in zip(stream_ids, counts):
            if c > 0:
                ready.append((self.streams[sid], c, r))
            r += c
        if not ready:
            return ready, None
        meta = self._ints([st[0] for st, _, _ in ready] + [c for _, c, _ in ready] + [o for _, _, o in ready], rows.device)
        return ready, meta.view(3, len(ready))

    @staticmethod
    def _advance(ready):
        """After the launches of an `accept`: the streams have consumed their pieces."""
        for st, c, _ in ready:
            st[1] += c

    @staticmethod
    def _read_partial(tokens, lengths, scores, stable):
        """The device tensors of a `partial` call (tokens int32 [n][U], lengths, scores fp32, stable_len) in one readback, the
        score bits carried through an int32 column: per stream (tokens, stable_len, score)."""
        U = tokens.shape[1]
        packed = torch.cat([tokens, lengths[:, None], stable[:, None], scores.view(torch.int32)[:, None]], dim=1).cpu()
        return [(row[: int(row[U])].tolist(), int(row[U + 1]), float(row[U + 2:U + 3].view(torch.float32))) for row in packed]


class CarriedRows:
    """The rows the slots carry besides the search state.  `carried` lists (rows, start) pairs: `rows` an LSTM state dict
    (name -> per-layer [max_streams * beam][H] tensors) or one [max_streams * beam][W] tensor (fp32 rows, or the int32 contexts of
    a token n-gram LM), `start` the same with one row:
    what a new stream starts from."""

    def __init__(self, beam, max_streams, carried):
        self.beam, self.carried = beam, carried
        self._pairs = []  # (tensor, its start row), flat
        for rows, start in carried:
            if isinstance(rows, dict):
                self._pairs += [(t, s) for k in rows for t, s in zip(rows[k], start[k])]
            else:
                self._pairs.append((rows, start))
        assert all(t.shape[0] == max_streams * beam and s.shape[0] == 1 for t, s in self._pairs)
        self._beam_ar = torch.arange(beam, dtype=torch.int32, device=self._pairs[0][0].device)

    def rows_of(self, slots):
        """slots int32 [n] on the device -> their rows int32 [n * beam]."""
        return (slots.unsqueeze(1) * self.beam + self._beam_ar.unsqueeze(0)).reshape(-1)

    def reset(self, slots):
        rows = self.rows_of(slots).long()
        for t, s in self._pairs:
            t.index_copy_(0, rows, s.expand(rows.numel(), -1))

    def gather(self, rows):
        """One value per carried item, in their order: the listed rows of a state dict as a state dict, of a tensor as a tensor."""
        return [{k: [K.gather_rows(t, rows) for t in v] for k, v in item.items()} if isinstance(item, dict)
                else K.gather_rows(item, rows) for item, _ in self.carried]

    def scatter(self, rows, values):
        """`values` as `gather` returns them go back to the listed rows."""
        rows = rows.long()
        for (item, _), new in zip(self.carried, values):
            if isinstance(item, dict):
                for k, v in item.items():
                    for t, n in zip(v, new[k]):
                        t.index_copy_(0, rows, n)
            else:
                item.index_copy_(0, rows, new)
