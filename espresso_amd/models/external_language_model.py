"""Multi-level (sub-word + word) language model for sub-word beam search — espresso/models/external_language_model.py:306-567
(Hori et al. 2017, "Multi-level language modeling and decoding for open vocabulary end-to-end speech recognition", adapted
to sentences that end with <space> before <eos>).  The look-ahead word LM lives in tensorized_lookahead_language_model.py.

Host side: state bookkeeping only.  Per step both LSTM LMs run their bf16 `advance` + `output_layer` (the word LM with frozen
rows except where the last sub-word is <space> = the reference's masked_copy_cached_state), and `ea_multilevel_lm_step`
does everything else in one launch: the word-level log-softmax of the refreshed rows, the prefix-tree transition, the
running sub-word score of the current word and the edited sub-word output row.  No step reads anything back to the host."""
import math

import torch

from .. import kernels as K
from ..tools.tensorized_prefix_tree import TensorizedPrefixTree, tokenize


class MultiLevelLanguageModel:
    def __init__(self, wordlm, subwordlm, subwordlm_weight: float = 0.8, oov_penalty: float = 1.0, open_vocab: bool = True):
        self.wordlm, self.subwordlm = wordlm, subwordlm
        self.wordlm_decoder, self.subwordlm_decoder = wordlm.decoder, subwordlm.decoder
        self.decoder = self  # fairseq-style access: model.decoder.dictionary
        self.dictionary = self.wordlm_decoder.dictionary
        self.subwordlm_weight = float(subwordlm_weight)
        self.log_oov_penalty = math.log(oov_penalty)
        self.open_vocab = bool(open_vocab)
        wd, sd = self.dictionary, self.subwordlm_decoder.dictionary
        self.word_eos_idx, self.word_unk_idx = wd.eos(), wd.unk()
        self.subword_space_idx, self.subword_eos_idx = sd.space(), sd.eos()
        self.subword_vocab_size = len(sd)
        nls = getattr(sd, "non_lang_syms", None)
        self.tree = TensorizedPrefixTree.build(wd, sd, lambda x: tokenize(x, non_lang_syms=nls).split(" "))

    def eval(self):
        self.wordlm.eval()
        self.subwordlm.eval()
        return self

    def max_positions(self):
        return int(1e5)

    def init_incremental(self, bsz, beam):
        dev = self.wordlm_decoder.embed_tokens.weight.device
        n = bsz * beam
        return {"word": self.wordlm_decoder.init_state(n, dev), "sub": self.subwordlm_decoder.init_state(n, dev), "word_lp": None,
                "prev_out": None, "cum": None, "nodes": None}

    @torch.no_grad()
    def step(self, state, tokens, step, parent=None):
        """tokens [N][step+1] sub-word history; returns fp32 sub-word log-probs [N][Vs] (already log-probs: :546-552)."""
        dev = tokens.device
        N = tokens.shape[0]
        prev = tokens[:, -1].to(torch.int32).contiguous()
        children, prev_sub, word_idx, _ = self.tree.device_tensors(dev)
        if state["word_lp"] is None:  # first step: every hypothesis starts a word after the sentence start <eos>
            w = torch.full((N,), self.word_eos_idx, dtype=torch.long, device=dev)
            wfeat, state["word"] = self.wordlm_decoder.advance(w, state["word"])
            state["word_lp"] = torch.empty(N, len(self.dictionary), dtype=torch.float32, device=dev)
            state["cum"] = torch.empty(N, dtype=torch.float32, device=dev)
            state["nodes"] = torch.empty(N, dtype=torch.int32, device=dev)
        else:
            if parent is not None:
                self._reorder(state, parent)
            w = word_idx[state["nodes"].long()].long()
            w = torch.where(w < 0, torch.full_like(w, self.word_unk_idx), w)
            frozen = (prev != self.subword_space_idx).to(torch.uint8).contiguous()  # the word LM only advances after <space>
            wfeat, state["word"] = self.wordlm_decoder.advance(w, state["word"], keep_row=frozen)
        word_logits = self.wordlm_decoder.output_layer(wfeat)
        sfeat, state["sub"] = self.subwordlm_decoder.advance(prev, state["sub"])
        sub_logits = self.subwordlm_decoder.output_layer(sfeat)
        out = K.multilevel_lm_step(word_logits, sub_logits, prev, state["prev_out"], state["word_lp"], state["cum"], state["nodes"],
                                   children, prev_sub, word_idx, self.subwordlm_weight, self.log_oov_penalty, self.open_vocab,
                                   self.word_eos_idx, self.word_unk_idx, self.subword_space_idx, self.subword_eos_idx,
                                   TensorizedPrefixTree.root_id)
        state["prev_out"] = out
        return out

    def _reorder(self, state, order):
        """reorder_incremental_state (:554-567) of the wrapper and both LMs: every cached row follows its surviving beam."""
        idx = order.to(torch.int32).contiguous()
        state["word"] = self.wordlm_decoder.reorder_state(state["word"], idx)
        state["sub"] = self.subwordlm_decoder.reorder_state(state["sub"], idx)
        state["word_lp"] = K.gather_rows(state["word_lp"], idx)
        state["prev_out"] = K.gather_rows(state["prev_out"], idx)
        state["cum"] = K.gather_rows(state["cum"].view(-1, 1), idx).view(-1)
        state["nodes"] = K.gather_rows(state["nodes"].view(-1, 1).view(torch.float32), idx).view(torch.int32).view(-1)

    def shrink(self, state, keep_rows):
        if state["word_lp"] is None:
            idx = keep_rows.to(torch.int32).contiguous()
            state["word"] = self.wordlm_decoder.reorder_state(state["word"], idx)
            state["sub"] = self.subwordlm_decoder.reorder_state(state["sub"], idx)
        else:
            self._reorder(state, keep_rows)
