"""CTCLexiconBeamSearchDecoder — lexicon-constrained CTC prefix beam search with shallow fusion of a word n-gram LM (ARPA),
with the generator API of CTCPrefixBeamSearchDecoder (`generate`, `decode`).  It stands where the reference puts
Flashlight's KenLM lexicon decoder (espresso/tools/ctc_decoder.py:24-71: `lm_model`, `lexicon`, `lm_weight` 2.0,
`word_score` -1.0, `unk_weight` -inf: a closed vocabulary, `sil_weight` 0).

The search is that of tools/ctc_prefix_beam_search.py (K best non-blank tokens per frame, stay and extend, merging of equal
token sequences, the same tie rules).  A hypothesis y is completed words w_1..w_m and a partial word p (a lexicon trie
node); its score is
    log(p_b + p_nb) + lm_weight * (L(y) + S(p)) + word_score * m + insertion_bonus * |y|
with L(y) = sum_i ln P(w_i | w_{i-n+1..i-1}) (<s> as the start) and S(p) = max ln P_1(w) over the lexicon words below p
(S(root) = 0).  It is applied as increments that telescope:
    a token moves p down the trie:  lm_weight * (S(child) - S(node))
    a word is completed:            lm_weight * (ln P(w | ctx) - S(node)) + word_score
    at the end:                     the pending word is completed, then lm_weight * ln P(</s> | ctx)
so the final score of a finished hypothesis is exact and only pruning sees the smeared values.  A word ends when <space> is
appended (space mode: the dictionary has <space>) or when a token starting with U+2581 is appended (word-start mode; that
token then starts the next word from the root).  Leaving the trie, ending a word on a node that is no word, an empty word
and a pending non-word at the end score -inf; an utterance whose every hypothesis is -inf (or that has no frames) returns
none, and `generate` gives it one empty hypothesis scored -inf.

The whole batch is one library call (csrc/ctc_lexicon_beam.hip, ea_ctc_lexicon_beam_search): one workgroup per utterance
walks all frames with the n-gram lookups inline.  `search` returns device tensors without a host synchronisation."""
from typing import Dict, List

import torch

from .. import kernels as K
from .beam_common import BeamDecoderMixin, hyps_from_tensors


class CTCLexiconBeamSearchDecoder(BeamDecoderMixin):
    MAX_BEAM = 64

    def __init__(self, models, dictionary, ngram_lm, lexicon, beam_size=10, nbest=1, beam_size_token=None, lm_weight=2.0,
                 word_score=-1.0, insertion_bonus=0.0, blank=None, **kwargs):
        """ngram_lm: models.ngram_lm.NGramLanguageModel; lexicon: tools.lexicon.LexiconTrie built for `dictionary` and it."""
        self.model = models[0] if isinstance(models, (list, tuple)) else models
        self.pad = dictionary.pad()
        self.blank = dictionary.bos() if blank is None else blank
        self.vocab_size = V = len(dictionary)
        if not 1 <= beam_size <= self.MAX_BEAM:
            raise ValueError(f"CTC lexicon beam search: beam {beam_size} outside [1, {self.MAX_BEAM}]")
        self.beam_size = beam_size
        self.beam_size_token = min(beam_size, V - 1) if beam_size_token is None else beam_size_token
        if not 1 <= self.beam_size_token <= min(self.MAX_BEAM, V - 1):
            raise ValueError(f"CTC lexicon beam search: --ctc-beam-size-token {self.beam_size_token} outside [1, {min(self.MAX_BEAM, V - 1)}]")
        if not 1 <= nbest <= beam_size:
            raise ValueError(f"CTC lexicon beam search: nbest {nbest} outside [1, beam {beam_size}]")
        if lexicon.space != dictionary.space():
            raise ValueError("CTC lexicon beam search: the lexicon was built for another dictionary")
        self.nbest = nbest
        self.ngram_lm, self.lexicon = ngram_lm, lexicon
        self.lm_weight, self.word_score, self.insertion_bonus = float(lm_weight), float(word_score), float(insertion_bonus)
        self._dev_tables = None

    def cuda(self):
        self.model.cuda()
        return self

    def _tables(self, device):
        if self._dev_tables is None or self._dev_tables[0][0].device != device:
            if self.ngram_lm.device is None:
                self.ngram_lm.to(device)
            self._dev_tables = self.lexicon.to(device)
        return self._dev_tables

    @torch.no_grad()
    def search(self, lprobs, in_len):
        """lprobs fp32/bf16 [B][T][V] log-probs (row-contiguous), in_len int [B] -> device tensors (tokens int32
        [B][nbest][T] pad-filled, lengths int32 [B][nbest], scores fp32 [B][nbest] natural log, nhyp int32 [B]), best
        first.  One library call, no host synchronisation."""
        B, T, V = lprobs.shape
        assert V == self.vocab_size and lprobs.stride(2) == 1 and lprobs.stride(0) == T * lprobs.stride(1)
        x = lprobs.view(B * T, V) if lprobs.is_contiguous() else lprobs.reshape(B * T, V)
        in_len = in_len.to(device=lprobs.device, dtype=torch.int32).contiguous()
        trie, word_start = self._tables(lprobs.device)
        ws = K.ctc_lexicon_beam_workspace(B, T, self.beam_size, lprobs.device)
        return K.ctc_lexicon_beam_search(x, in_len, ws, self.ngram_lm.handle, trie, word_start, self.lexicon.space, B, T, V,
                                         self.beam_size, self.beam_size_token, self.blank, self.nbest, self.pad,
                                         self.lm_weight, self.word_score, self.insertion_bonus)

    @torch.no_grad()
    def _generate(self, sample):
        net_output = self.model(**sample["net_input"])
        lprobs = self.model.get_normalized_probs(net_output, log_probs=True)  # T x B x V view of [B][T][V]
        return self.search(lprobs.transpose(0, 1), net_output["src_lengths"][0])

    @staticmethod
    def _empty_hypothesis():
        """What an utterance with nothing finite gets, so that it is still printed and scored."""
        return {"tokens": torch.zeros(0, dtype=torch.long), "score": torch.tensor(float("-inf")), "attention": None, "alignment": None}

    @torch.no_grad()
    def generate(self, models, sample, **kwargs) -> List[List[Dict[str, torch.Tensor]]]:
        return [hyps or [self._empty_hypothesis()] for hyps in hyps_from_tensors(*(t.cpu() for t in self._generate(sample)))]
