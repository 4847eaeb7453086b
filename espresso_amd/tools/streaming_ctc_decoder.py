"""Streaming greedy CTC decoding: the collapse of espresso/tools/ctc_decoder.py:172-188 (max over V, unique_consecutive,
drop blank) applied to encoder frames that arrive a chunk at a time, with the previous frame's argmax carried across chunk
boundaries so that a repeat straddling a boundary is emitted once.  Per-frame maxima come from ea_ctc_greedy_decode (every
frame as a one-frame utterance, one launch pair for all streams); the collapse itself is a few integers per chunk on the
host, where the tokens are wanted anyway."""
from typing import Dict, List, Sequence, Tuple

import torch

from .. import kernels as K


def collapse_step(prev: int, ids: Sequence[int], blank: int) -> Tuple[List[int], int]:
    """(tokens emitted by the frames `ids` given the previous frame's argmax `prev` (-1 at the start), new `prev`)."""
    out = []
    for t in ids:
        if t != prev and t != blank:
            out.append(int(t))
        prev = int(t)
    return out, prev


class StreamingCTCDecoder:
    def __init__(self, dictionary, blank=None):
        self.pad = dictionary.pad()
        self.blank = dictionary.bos() if blank is None else blank
        self.vocab_size = len(dictionary)
        self.state: Dict[object, list] = {}

    def open(self, stream_ids):
        for sid in stream_ids:
            self.state[sid] = [-1, [], 0.0]  # previous argmax, tokens, score

    @torch.no_grad()
    def accept(self, stream_ids, logits, counts) -> List[List[int]]:
        """logits [sum counts][>=V] (StreamingEncoder output, stream by stream); returns the tokens each stream emitted."""
        new = [[] for _ in stream_ids]
        M = sum(counts)
        if M == 0:
            return new
        V = self.vocab_size
        lp = K.log_softmax(logits, M, V, logits.stride(0))
        ones = torch.ones(M, dtype=torch.int32, device=lp.device)
        tokens, out_len, score, _ = K.ctc_greedy_decode(lp, ones, M, 1, V, self.blank, self.pad, want_align=False)
        tok, n, sc = tokens.view(-1).tolist(), out_len.tolist(), score.tolist()
        r = 0
        for b, (sid, c) in enumerate(zip(stream_ids, counts)):
            st = self.state[sid]
            ids = [tok[i] if n[i] else self.blank for i in range(r, r + c)]
            new[b], st[0] = collapse_step(st[0], ids, self.blank)
            st[1] += new[b]
            st[2] += sum(sc[r:r + c])
            r += c
        return new

    def close(self, sid):
        """The finished hypothesis of a stream in the generators' format."""
        _, toks, score = self.state.pop(sid)
        return {"tokens": torch.tensor(toks, dtype=torch.long), "score": torch.tensor(score), "attention": None, "alignment": None}
