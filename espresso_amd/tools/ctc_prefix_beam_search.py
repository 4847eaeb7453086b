"""CTCPrefixBeamSearchDecoder — CTC prefix beam search (Hannun et al. 2014) with optional shallow fusion of one sub-word LSTM
LM, with the generator API of tools/ctc_decoder.CTCDecoder (`generate`, `decode`).  The reference gets a CTC beam only through
Flashlight's KenLM lexicon decoder (espresso/tools/ctc_decoder.py:55-71, an external C++ library); this search fuses the
neural LM the project trains instead.

Each hypothesis is a distinct token prefix y with the log-probabilities pb / pnb of ending in blank / non-blank and the LM
log-probability lm(y) of its tokens after the LM's eos as BOS; its score is logaddexp(pb, pnb) + lm_weight * lm(y) +
insertion_bonus * |y|, and the final score adds lm_weight * log P_lm(eos | y).  Per frame the K best non-blank tokens are the
candidates, every hypothesis stays (blank, repeat of its last token) and extends by every candidate, equal prefixes merge,
and the `beam` best survive (ties: parent slot, stay before extension, token id).

The search is HIP (csrc/ctc_beam.hip): without an LM the whole utterance is one launch; with one, every frame is one step
launch plus the LM update on the device (reorder the LSTM state by parent, advance the rows that appended a token, output
layer, log-softmax).  `search` returns device tensors without a host synchronisation.

`lm_model` may instead be a models.token_ngram_lm.TokenNGramLM, an ARPA n-gram LM over the same dictionary: the loop is the
same, and the LM update of a frame is one launch (csrc/ngram_rows.hip) that advances the contexts and writes the rows.

Hotword biasing: with `context_graph` (tools/context_graph.ContextGraph) every hypothesis also carries its state in the phrase
automaton and a running bias that joins the score unweighted; the final score is the unbiased score of the same tokens plus
the boosts of the phrases it completed.  The candidate tokens of a frame stay the K best by acoustic score: biasing re-ranks
hypotheses, it does not bring back a token outside the top K.  Without a graph the search calls what it always called.

Time stamps: with `token_times=True` the search runs the times family of the kernels (ea_ctc_prefix_beam_times_*), which follows
the best single alignment path of every hypothesis, and `search` also returns times int32 [B][nbest][T] (the frame at which each
token starts on that path, -1 after the hypothesis) and vscores fp32 [B][nbest] (that path's score); `generate` puts them into
the hypotheses as "times" and "viterbi_score".  Tokens and scores are those of the search without times, bit for bit.

Posteriors: with `token_posteriors=True` every hypothesis also carries the acoustic model's own per-token posteriors
(tools/token_posteriors.py: "token_posteriors", "end_posterior", "posterior_score" — no LM, bonus or bias in them), computed from
the log-probs the search read; the search itself is unchanged."""
from typing import Dict, List

import torch

from .. import kernels as K
from .beam_common import BeamDecoderMixin, check_token_ngram, hyps_from_tensors, is_token_ngram, step_triple
from .token_posteriors import CTCTokenPosteriors, attach_posteriors, nbest_rows, score_rows


class CTCPrefixBeamSearchDecoder(BeamDecoderMixin):
    MAX_BEAM = 64

    def __init__(self, models, dictionary, beam_size=10, nbest=1, beam_size_token=None, lm_model=None, lm_weight=0.0,
                 insertion_bonus=0.0, blank=None, context_graph=None, token_times=False, token_posteriors=False, **kwargs):
        self.model = models[0] if isinstance(models, (list, tuple)) else models
        self.pad = dictionary.pad()
        self.eos = dictionary.eos()
        self.blank = dictionary.bos() if blank is None else blank
        self.vocab_size = V = len(dictionary)
        if not 1 <= beam_size <= self.MAX_BEAM:
            raise ValueError(f"CTC prefix beam search: beam {beam_size} outside [1, {self.MAX_BEAM}]")
        self.beam_size = beam_size
        self.beam_size_token = min(beam_size, V - 1) if beam_size_token is None else beam_size_token
        if not 1 <= self.beam_size_token <= min(self.MAX_BEAM, V - 1):
            raise ValueError(f"CTC prefix beam search: --ctc-beam-size-token {self.beam_size_token} outside [1, {min(self.MAX_BEAM, V - 1)}]")
        if not 1 <= nbest <= beam_size:
            raise ValueError(f"CTC prefix beam search: nbest {nbest} outside [1, beam {beam_size}]")
        self.nbest = nbest
        self.lm_model, self.lm_weight, self.insertion_bonus = lm_model, float(lm_weight), float(insertion_bonus)
        if is_token_ngram(lm_model):
            check_token_ngram(lm_model, self.lm_weight, dictionary, self.blank, "CTC prefix beam search")
        elif lm_model is not None:
            lm_dict = lm_model.decoder.dictionary
            assert list(lm_dict.symbols) == list(dictionary.symbols), \
                "CTC prefix beam search fuses an LM over the CTC model's own dictionary (blank <s> included)"
            lm_model.eval()
        if context_graph is not None and context_graph.vocab_size != V:
            raise ValueError(f"CTC prefix beam search: context graph built for {context_graph.vocab_size} tokens, dictionary has {V}")
        self.context_graph = context_graph
        self.token_times = bool(token_times)
        self.posteriors = CTCTokenPosteriors(dictionary, blank=self.blank) if token_posteriors else None

    def cuda(self):
        self.model.cuda()
        if self.lm_model is not None:
            self.lm_model.cuda()
        if self.context_graph is not None:
            self.context_graph.cuda()  # uploaded once per device; `search` uploads when this was not called
        return self

    # ---------------------------------------------------------------- the search
    @torch.no_grad()
    def search(self, lprobs, in_len):
        """lprobs fp32/bf16 [B][T][V] log-probs (row-contiguous), in_len int [B] -> device tensors (tokens int32
        [B][nbest][T] pad-filled, lengths int32 [B][nbest], scores fp32 [B][nbest] natural log, nhyp int32 [B]), best
        first; with token_times also (times int32 [B][nbest][T], vscores fp32 [B][nbest]).  No host synchronisation."""
        B, T, V = lprobs.shape
        assert V == self.vocab_size and lprobs.stride(2) == 1 and lprobs.stride(0) == T * lprobs.stride(1)
        x = lprobs.view(B * T, V) if lprobs.is_contiguous() else lprobs.reshape(B * T, V)
        in_len = in_len.to(device=lprobs.device, dtype=torch.int32).contiguous()
        dev, beam, Kt = lprobs.device, self.beam_size, self.beam_size_token
        step = dict(B=B, T=T, V=V, beam=beam, K=Kt, blank=self.blank, ins_bonus=self.insertion_bonus)
        if self.token_times:
            graph = self.context_graph.cuda(dev) if self.context_graph is not None else None
            ws = (K.ctc_prefix_beam_workspace if graph is None else K.ctc_prefix_beam_bias_workspace)(B, T, beam, dev)
            tws = K.ctc_prefix_beam_times_workspace(B, T, beam, dev)

            def beam_step(x, in_len, ws, **kw):
                K.ctc_prefix_beam_times_step(x, in_len, ws, tws, graph=graph, **kw)

            def beam_finish(ws, *a, **kw):
                return K.ctc_prefix_beam_times_finish(ws, tws, *a, graph=graph, **kw)
        elif self.context_graph is None:
            ws = K.ctc_prefix_beam_workspace(B, T, beam, dev)
            beam_step, beam_finish = K.ctc_prefix_beam_step, K.ctc_prefix_beam_finish
        else:
            graph = self.context_graph.cuda(dev)
            ws = K.ctc_prefix_beam_bias_workspace(B, T, beam, dev)

            def beam_step(x, in_len, ws, **kw):
                K.ctc_prefix_beam_bias_step(x, in_len, ws, graph, **kw)

            def beam_finish(ws, *a, **kw):
                return K.ctc_prefix_beam_bias_finish(ws, graph, *a, **kw)
        if self.lm_model is None:
            beam_step(x, in_len, ws, t0=0, t1=T, **step)
            return beam_finish(ws, B, T, beam, self.nbest, self.pad, ins_bonus=self.insertion_bonus)
        N = B * beam
        state, rows = self.lm_start(N, dev)
        lm_out = step_triple(N, dev)
        if T == 0:
            beam_step(x, in_len, ws, t0=0, t1=0, **step)
        for t in range(T):
            beam_step(x, in_len, ws, t0=t, t1=t + 1, lm_rows=rows, lm_weight=self.lm_weight, lm_out=lm_out, **step)
            state, rows = self.lm_update(state, *lm_out)
        return beam_finish(ws, B, T, beam, self.nbest, self.pad, lm_rows=rows, lm_weight=self.lm_weight,
                           ins_bonus=self.insertion_bonus, eos=self.eos)

    @torch.no_grad()
    def _generate(self, sample, posteriors=None):
        """posteriors: a list that gets the device rows of `score_rows` for the hypotheses, row = utterance * nbest + rank."""
        net_output = self.model(**sample["net_input"])
        lprobs = self.model.get_normalized_probs(net_output, log_probs=True)  # T x B x V view of [B][T][V]
        out = self.search(lprobs.transpose(0, 1), net_output["src_lengths"][0])
        if posteriors is not None:
            posteriors.extend(self.score_hypotheses(lprobs.transpose(0, 1), net_output["src_lengths"][0], out))
        return out

    @torch.no_grad()
    def score_hypotheses(self, lprobs, in_len, out):
        """The device rows (token factors [B * nbest][T], end factors, posterior scores) of what `search` returned for lprobs."""
        tokens, lengths, _, nhyp = out[:4]
        ln, utt = nbest_rows(lengths, nhyp)
        return score_rows(self.posteriors, lprobs, in_len, tokens.reshape(-1, tokens.shape[2]), ln, utt, (self.blank, self.pad))

    @torch.no_grad()
    def generate(self, models, sample, **kwargs) -> List[List[Dict[str, torch.Tensor]]]:
        rows = [] if self.posteriors is not None else None
        out = self._generate(sample, posteriors=rows)
        hyps = hyps_from_tensors(*(t.cpu() for t in out))
        if rows is not None:
            nbest = out[0].shape[1]
            attach_posteriors([u[i] if i < len(u) else None for u in hyps for i in range(nbest)], *(t.cpu() for t in rows))
        return hyps
