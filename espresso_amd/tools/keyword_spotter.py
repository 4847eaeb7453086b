"""Keyword spotting with a CTC model: where a list of phrases is spoken, and how sure the model is, from the per-frame CTC
log-probs alone (csrc/kws.hip; the rule is in include/espresso_amd.h and DESIGN.md section 3.7).  No beam search runs and no
transcript is needed: every (stream, keyword) pair is a small max-plus scan with a free start frame, so an occurrence a beam
would have pruned is still found, and every hit carries a score.

`read_keywords` reads a phrase file in the format of `--hotwords` (tools/context_graph.read_hotwords), the number after the TAB
being the keyword's threshold theta.  `CTCKeywordSpotter` has the conventions of StreamingCTCDecoder and the streamed beam
decoders -- `open`, `accept` (logits, log-softmax, one step), `poll` (the hits emitted since the last poll, one read-back),
`close` (flush, the rest) -- and `spot`, the offline path: the encoder forward as CTCForcedAligner.align runs it, then the batch
through temporary slots.  The per-frame code is the same for both, so the polls of a stream fed in any pieces plus its `close`
are, bit for bit, the hits of `spot` over the whole utterance.

A hit is a dict: `keyword` (index), `text`, `start`, `end` (inclusive encoder frames, counted from the stream's first frame),
`score` (e, the keyword path's log-prob relative to the greedy path's, <= 0) and `confidence` = exp(e / L) in (0, 1].  A hit is
reported `hold_frames` after its end (a better overlapping candidate may still replace it until then), or at the audio's end."""
import math
from typing import Dict, List, Sequence

import numpy as np
import torch

from .. import kernels as K
from .beam_common import StreamSlots

MAX_KEYWORD_TOKENS = 64


def read_keywords(path: str, dictionary, blank: int, default_threshold: float) -> List[Dict]:
    """A keyword file: one phrase per line, optionally `<TAB>threshold` (theta in (0, 1]); `#` comments and blank lines are
    skipped, the text is tokenised as `--hotwords` phrases are.  Returns [{"tokens", "threshold", "text"}].  Refused, with the
    line number: what read_hotwords refuses, a threshold above 1, a phrase of more than 64 tokens and a duplicate phrase."""
    from .context_graph import read_hotwords

    if not 0.0 < default_threshold <= 1.0:
        raise ValueError(f"the default threshold {default_threshold} is outside (0, 1]")
    entries = read_hotwords(path, dictionary, blank, default_threshold)
    with open(path, encoding="utf-8") as f:  # the lines read_hotwords kept, for the messages and the hits' text
        kept = [(no, line.rstrip("\r\n")) for no, line in enumerate(f, 1) if line.strip() and not line.lstrip().startswith("#")]
    assert len(kept) == len(entries)
    out, seen = [], {}
    for (lineno, line), (ids, theta) in zip(kept, entries):
        text = line.split("\t", 1)[0].strip()
        if theta > 1.0:
            raise ValueError(f"{path}:{lineno}: threshold {theta} is above 1")
        if len(ids) > MAX_KEYWORD_TOKENS:
            raise ValueError(f"{path}:{lineno}: phrase {text!r} has {len(ids)} tokens, more than {MAX_KEYWORD_TOKENS}")
        if tuple(ids) in seen:
            raise ValueError(f"{path}:{lineno}: phrase {text!r} repeats line {seen[tuple(ids)]}")
        seen[tuple(ids)] = lineno
        out.append({"tokens": list(ids), "threshold": float(theta), "text": text})
    return out


def keyword_tau(length: int, theta: float) -> np.float32:
    """tau = L * ln(theta), in fp32: what the detection compares e(tok_L) with."""
    return np.float32(length) * np.float32(math.log(theta))


def sort_hits(hits: List[Dict]) -> List[Dict]:
    """By (end, keyword index): the order in which a stream reports them."""
    return sorted(hits, key=lambda h: (h["end"], h["keyword"]))


def hit_seconds(hit: Dict, seconds_per_frame: float):
    """(start_s, end_s) of a hit: `end` is inclusive, so end_s = (end + 1) * seconds per encoder frame."""
    return hit["start"] * seconds_per_frame, (hit["end"] + 1) * seconds_per_frame


def output_line(utt: str, hit: Dict, seconds_per_frame: float) -> str:
    """utt<TAB>start_s<TAB>end_s<TAB>confidence<TAB>keyword"""
    s, e = hit_seconds(hit, seconds_per_frame)
    return "{}\t{:.3f}\t{:.3f}\t{:.4f}\t{}".format(utt, s, e, hit["confidence"], hit["text"])


class CTCKeywordSpotter(StreamSlots):
    def __init__(self, dictionary, keywords, max_streams, hold_frames, max_hits=64, blank=None):
        """keywords: [{"tokens", "threshold"[, "text"]}] (read_keywords) or (tokens, threshold) pairs."""
        self.dictionary = dictionary
        self.blank = dictionary.bos() if blank is None else blank
        self.vocab_size = len(dictionary)
        self.hold_frames, self.max_hits = int(hold_frames), int(max_hits)
        if self.hold_frames < 0 or self.max_hits < 1:
            raise ValueError(f"keyword spotter: hold_frames {hold_frames} must not be negative and max_hits {max_hits} must be positive")
        self.keywords = []
        for i, kw in enumerate(keywords):
            kw = dict(kw) if isinstance(kw, dict) else {"tokens": list(kw[0]), "threshold": float(kw[1])}
            ids, theta = [int(t) for t in kw["tokens"]], float(kw["threshold"])
            if not 1 <= len(ids) <= MAX_KEYWORD_TOKENS:
                raise ValueError(f"keyword {i}: {len(ids)} tokens, outside [1, {MAX_KEYWORD_TOKENS}]")
            if any(t < 0 or t >= self.vocab_size or t == self.blank for t in ids):
                raise ValueError(f"keyword {i}: a token outside the dictionary, or the blank")
            if not 0.0 < theta <= 1.0:
                raise ValueError(f"keyword {i}: threshold {theta} is outside (0, 1]")
            if kw.get("text") is None:
                kw["text"] = dictionary.string(torch.tensor(ids, dtype=torch.long), bpe_symbol=None)
            kw["tokens"], kw["threshold"] = ids, theta
            self.keywords.append(kw)
        if not self.keywords:
            raise ValueError("keyword spotter: no keywords")
        StreamSlots.__init__(self, "CTC keyword spotter", max_streams, 2 ** 31 - 1)  # (no bound on a stream's frames)
        self.Lmax = max(len(kw["tokens"]) for kw in self.keywords)
        self.overflowed = 0  # hits that did not fit into max_hits between two polls
        self.state = self.tables = None  # allocated on the device of the first frames

    def state_bytes_per_stream(self) -> int:
        return K.ctc_kws_state_bytes(len(self.keywords), self.Lmax, self.max_hits)

    # ---- device plumbing -------------------------------------------------------------------------------------------------
    def _tables(self, device):
        """(tokens int32 [K][Lmax], lengths int32 [K], tau fp32 [K]) on the device, once."""
        if self.tables is None or self.tables[0].device != device:
            self.tables = tuple(torch.from_numpy(a).to(device) for a in keyword_lists(self.keywords))
        return self.tables

    def _ensure(self, device):
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.state is None:
            self.state, _ = K.ctc_kws_state(self.max_streams, len(self.keywords), self.Lmax, self.max_hits, device)
        device = self.state.device
        tables = self._tables(device)
        if self._unreset:
            K.ctc_kws_reset(self.state, self._ints(self._unreset, device), tables, self.max_hits)
            self._unreset = []
        return device

    def _device(self):
        return self.state.device if self.state is not None else torch.device("cuda", torch.cuda.current_device())

    def _read(self, outputs, n) -> List[List[Dict]]:
        """The device outputs of ea_ctc_kws_hits in one read-back -> per slot its hits, sorted."""
        starts, ends, scores, counts = outputs
        Kk, H = len(self.keywords), self.max_hits
        host = torch.cat([starts.view(n, -1), ends.view(n, -1), scores.view(torch.int32).view(n, -1), counts], dim=1).cpu().numpy()
        out = []
        for row in host:
            st, en = row[: Kk * H].reshape(Kk, H), row[Kk * H: 2 * Kk * H].reshape(Kk, H)
            sc, cnt = row[2 * Kk * H: 3 * Kk * H].view(np.float32).reshape(Kk, H), row[3 * Kk * H:]
            hits = []
            for k, kw in enumerate(self.keywords):
                self.overflowed += max(0, int(cnt[k]) - H)
                for h in range(min(int(cnt[k]), H)):
                    e = float(sc[k, h])
                    hits.append({"keyword": k, "text": kw["text"], "start": int(st[k, h]), "end": int(en[k, h]), "score": e,
                                 "confidence": math.exp(e / len(kw["tokens"]))})
            out.append(sort_hits(hits))
        return out

    # ---- the streaming interface -----------------------------------------------------------------------------------------
    @torch.no_grad()
    def accept(self, stream_ids, logits, counts):
        """logits [sum counts][>=V] (StreamingEncoder output, stream by stream): log-softmax, then `accept_lprobs`."""
        M = sum(counts)
        if M == 0:
            return
        self.accept_lprobs(stream_ids, K.log_softmax(logits, M, self.vocab_size, logits.stride(0)), counts)

    @torch.no_grad()
    def accept_lprobs(self, stream_ids, lprobs, counts):
        """lprobs fp32 [sum counts][>=V] log-probs, packed stream by stream in the order of stream_ids: one step, nothing read
        back."""
        ready, meta = self._pack(stream_ids, counts, lprobs)
        if not ready:
            return
        self._ensure(lprobs.device)
        K.ctc_kws_step(lprobs, meta, self.state, self.tables, self.max_hits, self.vocab_size, self.blank, self.hold_frames)
        self._advance(ready)

    @torch.no_grad()
    def poll(self, stream_ids) -> List[List[Dict]]:
        """Per stream the hits emitted since the last poll, sorted by (end, keyword index); one read-back."""
        if not stream_ids:
            return []
        slots = self._slots_of(stream_ids, self._ensure(self._device()))
        return self._read(K.ctc_kws_hits(self.state, slots, self.tables, self.max_hits, flush=False, clear=True), len(stream_ids))

    @torch.no_grad()
    def close(self, sid) -> List[Dict]:
        """The audio of the stream has ended: its open hits are emitted and the hits not polled yet returned; the slot is free."""
        slots = self._slots_of([sid], self._ensure(self._device()))
        hits = self._read(K.ctc_kws_hits(self.state, slots, self.tables, self.max_hits, flush=True, clear=True), 1)[0]
        self._release(sid)
        return hits

    # ---- offline ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def spot_lprobs(self, lprobs, lengths) -> List[List[Dict]]:
        """lprobs fp32 [B][T][>=V] log-probs (a contiguous batch), lengths int32 [B] on its device: reset, one step over the
        whole utterances, the hits with a flush -- in B temporary slots.  One read-back."""
        B, T = lprobs.shape[:2]
        dev = lprobs.device
        tables = self._tables(dev)
        if B == 0:
            return []
        state, _ = K.ctc_kws_state(B, len(self.keywords), self.Lmax, self.max_hits, dev)
        slots = torch.arange(B, dtype=torch.int32, device=dev)
        meta = torch.stack([slots, lengths.to(torch.int32).clamp(max=T), slots * T]).contiguous()
        K.ctc_kws_reset(state, slots, tables, self.max_hits)
        K.ctc_kws_step(lprobs.reshape(B * T, lprobs.shape[2]), meta, state, tables, self.max_hits, self.vocab_size, self.blank,
                       self.hold_frames)
        return self._read(K.ctc_kws_hits(state, slots, tables, self.max_hits, flush=True, clear=False), B)

    @torch.no_grad()
    def spot(self, model, sample) -> List[List[Dict]]:
        """The hits of every utterance of a batch: the encoder forward as CTCForcedAligner.align runs it, then `spot_lprobs`."""
        net_output = model(**sample["net_input"])
        lprobs = model.get_normalized_probs(net_output, log_probs=True)  # T x B x V view of [B][T][V]
        enc_len = net_output["src_lengths"][0].to(torch.int32).contiguous()
        return self.spot_lprobs(lprobs.transpose(0, 1).contiguous(), enc_len)


def keyword_lists(keywords: Sequence[Dict]):
    """(tokens int32 [K][Lmax], lengths int32 [K], tau fp32 [K]) numpy tables of a keyword list, as the library takes them."""
    Lmax = max(len(kw["tokens"]) for kw in keywords)
    tok = np.zeros((len(keywords), Lmax), dtype=np.int32)
    for k, kw in enumerate(keywords):
        tok[k, : len(kw["tokens"])] = kw["tokens"]
    ln = np.array([len(kw["tokens"]) for kw in keywords], dtype=np.int32)
    tau = np.array([keyword_tau(len(kw["tokens"]), kw["threshold"]) for kw in keywords], dtype=np.float32)
    return tok, ln, tau
