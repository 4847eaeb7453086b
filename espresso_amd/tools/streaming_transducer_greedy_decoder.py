"""Streaming greedy transducer search: the search of tools/transducer_greedy_decoder.py (TransducerGreedyDecoder, which stays as
it is) on encoder frames that arrive a chunk at a time.  Per stream the predictor's (h, c) state, the last emitted token, the
token grid and the score are carried across chunks; for every frame up to `max_num_expansions_per_step` non-blank symbols are
emitted and a row that emits blank keeps its predictor state, exactly as offline — so the hypothesis of an utterance fed in
chunks is the one the offline search returns for the same encoder output.  No LM fusion under streaming."""
from typing import Dict, List

import torch

from .. import kernels as K


class StreamingTransducerGreedyDecoder:
    def __init__(self, model, dictionary, max_num_expansions_per_step=2, eos=None, bos=None, blank=None):
        self.model = model
        self.eos = dictionary.eos() if eos is None else eos
        self.bos = dictionary.eos() if bos is None else bos
        self.blank = dictionary.bos() if blank is None else blank
        self.symbols_to_strip_from_output = {self.eos, self.bos, self.blank}
        self.vocab_size = len(dictionary)
        assert max_num_expansions_per_step > 0, "--max-num-expansions-per-step must be at least 1"
        self.max_num_expansions_per_step = max_num_expansions_per_step
        self.model.eval()
        self.state: Dict[object, dict] = {}

    def open(self, stream_ids):
        dev = next(self.model.parameters()).device
        for sid in stream_ids:
            self.state[sid] = {"pred": self.model.decoder.init_state(1, dev), "tokens": [], "scores": [],
                               "prev": torch.full((1,), self.bos, dtype=torch.long, device=dev)}

    @torch.no_grad()
    def accept(self, stream_ids, enc_rows, counts):
        """enc_rows bf16 [sum counts][C]: new encoder frames, stream by stream (StreamingEncoder's output); advances every
        stream over its frames."""
        live = [(sid, c) for sid, c in zip(stream_ids, counts) if c > 0]
        if not live:
            return
        model, V, Ex = self.model, self.vocab_size, self.max_num_expansions_per_step
        dev = enc_rows.device
        bsz, Tm = len(live), max(c for _, c in live)
        E = model.joint_encoder_branch(enc_rows.contiguous())
        # packed rows -> [bsz][Tm] (rows past a stream's count repeat row 0 and are never used: blank_mask covers them)
        idx, r = [], 0
        for sid, c in zip(stream_ids, counts):
            if c > 0:
                idx += list(range(r, r + c)) + [0] * (Tm - c)
            r += c
        E = K.gather_rows(E.contiguous(), torch.tensor(idx, dtype=torch.int32).to(dev)).view(bsz, Tm, -1)
        enc_len = torch.tensor([c for _, c in live], device=dev)
        sts = [self.state[sid] for sid, _ in live]
        state = {n: [torch.cat([s["pred"][n][l] for s in sts]) for l in range(len(sts[0]["pred"][n]))] for n in sts[0]["pred"]}
        prev = torch.cat([s["prev"] for s in sts])
        tokens = torch.full((bsz, Tm, Ex + 1), self.blank, dtype=torch.long, device=dev)
        scores = torch.zeros((bsz, Tm, Ex + 1), dtype=torch.float32, device=dev)
        for step in range(Tm):
            blank_mask = step >= enc_len
            k = 0
            while not bool(blank_mask.all()) and k < Ex + 1:
                dec_out, new_state = model.decoder.advance(prev, state)
                logits = model.joint_step(E[:, step].contiguous(), dec_out)[:, :V]
                lprobs = K.log_softmax(logits, bsz, V, logits.stride(0))
                if k < Ex:
                    sc, tk = lprobs.max(-1)
                    sc = sc.masked_fill(blank_mask, 0.0)
                    blank_mask = blank_mask | (tk == self.blank)
                    tk = tk.masked_fill(blank_mask, self.blank)
                    scores[:, step, k] = sc
                    tokens[:, step, k] = tk
                    prev = torch.where(blank_mask, prev, tk)
                else:  # the score of the closing blank if the frame has not emitted one yet
                    scores[:, step, k] = torch.where(blank_mask, scores[:, step, k], lprobs[:, self.blank])
                    blank_mask = torch.ones_like(blank_mask)
                keep = blank_mask.unsqueeze(1)
                state = {n: [torch.where(keep, o, nw) for o, nw in zip(state[n], new_state[n])] for n in state}
                k += 1
        for b, (s, (_, c)) in enumerate(zip(sts, live)):
            s["pred"] = {n: [t[b:b + 1] for t in state[n]] for n in state}
            s["prev"] = prev[b:b + 1]
            s["tokens"].append(tokens[b, :c].reshape(-1))
            s["scores"].append(scores[b, :c].sum())

    def close(self, sid):
        """The finished hypothesis in the generators' format: tokens [T * (E + 1)] (blanks included, as offline), summed score."""
        s = self.state.pop(sid)
        dev = s["prev"].device
        toks = torch.cat(s["tokens"]) if s["tokens"] else torch.zeros(0, dtype=torch.long, device=dev)
        score = torch.stack(s["scores"]).sum() if s["scores"] else torch.zeros((), device=dev)
        return {"tokens": toks, "score": score, "attention": None, "alignment": None}
