"""TransducerFrameBeamDecoder — frame-synchronous transducer beam search (at most one symbol per encoder frame and hypothesis,
equal token sequences merged: the "modified beam search" of other toolkits) with optional shallow fusion of one sub-word LSTM
LM, with the `generate` / `decode` API of the other transducer decoders.  The reference has no such search: its beam search
is the modified Adaptive Expansion Search (tools/transducer_beam_search_decoder.py, kept as it is), whose bookkeeping lives on
the host.  The contract is DESIGN.md section 3.5 and the header of csrc/rnnt_beam.hip.

One encoder pass and one `joint_encoder_branch`; then per frame: gather this frame's rows of the encoder branch for the
B * beam slots, `joint_step`, the step kernels (log-softmax, fusion, per-row top K, merge, selection: csrc/rnnt_beam.hip), and
`reorder_state` + `advance(token, state, keep_row)` for the predictor (and the LM, its output layer and log-softmax).  Beam,
prefix table and selection live in a device workspace; the loop runs over the padded frame count (frames past an
utterance's length are no-ops in the kernel) and never synchronises with the host.

The LM fusion is the mass-preserving one of the two other transducer decoders (transducer_greedy_decoder.py): non-blank
log-probs get lm_weight * log P_lm and are renormalised to the non-blank mass they had; blank is untouched.  `lm_model` may
instead be a models.token_ngram_lm.TokenNGramLM over the model's dictionary (one launch per frame, csrc/ngram_rows.hip): a
token whose LM log-prob is -inf leaves the candidates, as any token with a non-finite fused score does.

Hotword biasing: with `context_graph` (tools/context_graph.ContextGraph) every hypothesis also carries its state in the phrase
automaton and a running bias; the decoder then calls the bias family of the kernels (ea_rnnt_frame_beam_bias_*) for the
workspace, every step and the finish, with the tables uploaded once.  Without a graph the calls are the unbiased ones.

Time stamps: with `token_times=True` the steps and the finish are those of the times family (ea_rnnt_frame_beam_times_*), which
follows the best single alignment path of every hypothesis, and `search` also returns times int32 [B][nbest][T'] (the frame at
which each token is emitted on that path, -1 after the hypothesis) and vscores fp32 [B][nbest] (that path's score, never
normalised); `generate` puts them into the hypotheses as "times" and "viterbi_score"."""
from typing import Dict, List

import torch

from .. import kernels as K
from .beam_common import BeamDecoderMixin, check_token_ngram, hyps_from_tensors, is_token_ngram, step_triple
from .token_posteriors import TransducerTokenPosteriors, attach_posteriors, nbest_rows, score_rows


class TransducerFrameBeamDecoder(BeamDecoderMixin):
    MAX_BEAM = 64

    def __init__(self, models, dictionary, beam_size=5, nbest=1, beam_size_token=None, temperature=1.0, normalize_scores=True,
                 lm_model=None, lm_weight=0.0, model_predicts_eos=False, bos=None, blank=None, eos=None, pad=None,
                 symbols_to_strip_from_output=None, print_alignment=False, context_graph=None, token_times=False,
                 token_posteriors=False, **kwargs):
        if isinstance(models, (list, tuple)):
            if len(models) != 1:
                raise NotImplementedError("the frame-synchronous transducer beam search takes one model: ensembles are not implemented")
            models = models[0]
        if print_alignment:
            raise NotImplementedError("the frame-synchronous transducer beam search produces no alignments (print_alignment)")
        self.model = models
        self.eos = dictionary.eos() if eos is None else eos
        self.bos = dictionary.eos() if bos is None else bos
        self.blank = dictionary.bos() if blank is None else blank
        self.pad = dictionary.pad() if pad is None else pad
        self.model_predicts_eos = model_predicts_eos
        strip = {self.eos, self.bos, self.blank}
        self.symbols_to_strip_from_output = strip.union(symbols_to_strip_from_output) if symbols_to_strip_from_output else strip
        self.vocab_size = V = len(dictionary)
        if not 1 <= beam_size <= self.MAX_BEAM:
            raise ValueError(f"transducer frame beam search: beam {beam_size} outside [1, {self.MAX_BEAM}]")
        self.beam_size = beam_size
        self.beam_size_token = min(beam_size, V - 1) if beam_size_token is None else beam_size_token
        if not 1 <= self.beam_size_token <= min(self.MAX_BEAM, V - 1):
            raise ValueError(f"transducer frame beam search: --transducer-beam-size-token {self.beam_size_token} outside "
                             f"[1, {min(self.MAX_BEAM, V - 1)}]")
        if not 1 <= nbest <= beam_size:
            raise ValueError(f"transducer frame beam search: nbest {nbest} outside [1, beam {beam_size}]")
        self.nbest = nbest
        if not temperature > 0:
            raise ValueError("--temperature must be greater than 0")
        self.temperature = float(temperature)
        self.normalize_scores = bool(normalize_scores)
        if self.model is not None:
            self.model.eval()
        self.lm_model, self.lm_weight = lm_model, float(lm_weight)
        self.no_blank_in_lm = False
        if is_token_ngram(lm_model):  # its rows have V columns: lm_no_blank stays False
            check_token_ngram(lm_model, self.lm_weight, dictionary, self.blank, "transducer frame beam search")
        elif lm_model is not None:
            nlm = len(lm_model.decoder.dictionary)
            if nlm not in (V, V - 1):
                raise ValueError(f"transducer frame beam search: the LM's dictionary has {nlm} entries, the model's {V}: it must "
                                 "be the same dictionary, or that dictionary without the blank")
            self.no_blank_in_lm = nlm == V - 1
            lm_model.eval()
        if context_graph is not None and context_graph.vocab_size != V:
            raise ValueError(f"transducer frame beam search: context graph built for {context_graph.vocab_size} tokens, dictionary has {V}")
        self.context_graph = context_graph
        self.token_times = bool(token_times)
        # the acoustic model's own per-token posteriors of every hypothesis (tools/token_posteriors.py): no LM, no bias,
        # temperature 1, the standard lattice (any number of symbols per frame) although this search allows one
        if token_posteriors and model_predicts_eos:
            raise NotImplementedError("transducer frame beam search: token_posteriors with model_predicts_eos is not implemented (the search folds "
                                      "<eos> into blank, the posterior's lattice does not)")
        self.posteriors = TransducerTokenPosteriors(self.model, dictionary, blank=self.blank, bos=self.bos) if token_posteriors else None

    def cuda(self):
        self.model.cuda()
        if self.lm_model is not None:
            self.lm_model.cuda()
        return self

    def graph_tables(self, device):
        """The context graph's device tables (uploaded once per device), or None without a graph."""
        return self.context_graph.cuda(device) if self.context_graph is not None else None

    def _lm_tokens(self, tokens):
        """The LM's ids: its dictionary may be the model's without the blank."""
        return torch.where(tokens > self.blank, tokens - 1, tokens) if self.no_blank_in_lm else tokens

    # ---------------------------------------------------------------- the search
    @torch.no_grad()
    def search(self, E, enc_len, bos_token=None):
        """E fp32 [B][T'][J] (the joint's encoder branch, `joint_encoder_branch`), enc_len int [B] on the device -> device
        tensors (tokens int32 [B][nbest][T'] pad-filled, lengths int32 [B][nbest], scores fp32 [B][nbest] natural log, nhyp
        int32 [B]), best first; with token_times also (times int32 [B][nbest][T'], vscores fp32 [B][nbest]).  No host
        synchronisation."""
        model, dec = self.model, self.model.decoder
        B, Tp, J = E.shape
        dev, beam, V = E.device, self.beam_size, self.vocab_size
        N = B * beam
        E = E.contiguous().view(B * Tp, J)
        in_len = enc_len.to(device=dev, dtype=torch.int32).contiguous()
        # everything the loop needs, allocated before it: the encoder rows of every (frame, slot), the triples, the workspace
        rows = (torch.arange(B, device=dev, dtype=torch.int32) * Tp).repeat_interleave(beam)
        frame_rows = (rows.unsqueeze(0) + torch.arange(Tp, device=dev, dtype=torch.int32).unsqueeze(1)).contiguous()  # [T'][N]
        out = step_triple(N, dev)
        graph = self.graph_tables(dev)
        ws = K.rnnt_frame_beam_workspace(B, Tp, beam, dev) if graph is None else K.rnnt_frame_beam_bias_workspace(B, Tp, beam, dev)
        tws = K.rnnt_frame_beam_times_workspace(B, Tp, beam, dev) if self.token_times else None
        state = dec.init_state(N, dev)
        dec_out, state = dec.advance(torch.full((N,), self.bos if bos_token is None else bos_token, dtype=torch.int32, device=dev), state)
        lm_state = lm_rows = None
        if self.lm_model is not None:
            lm_state, lm_rows = self.lm_start(N, dev)
        step = dict(B=B, T=Tp, V=V, beam=beam, K=self.beam_size_token, blank=self.blank, eos=self.eos if self.model_predicts_eos else -1,
                    temperature=self.temperature, lm_weight=self.lm_weight, lm_no_blank=self.no_blank_in_lm)
        for t in range(Tp):
            logits = model.joint_step(K.gather_rows(E, frame_rows[t]), dec_out)
            if tws is not None:
                K.rnnt_frame_beam_times_step(logits, in_len, ws, tws, out, t=t, graph=graph, lm_rows=lm_rows, **step)
            elif graph is None:
                K.rnnt_frame_beam_step(logits, in_len, ws, out, t=t, lm_rows=lm_rows, **step)
            else:
                K.rnnt_frame_beam_bias_step(logits, in_len, ws, graph, out, t=t, lm_rows=lm_rows, **step)
            state = dec.reorder_state(state, out[0])
            dec_out, state = dec.advance(out[1], state, keep_row=out[2])
            if self.lm_model is not None:
                lm_state, lm_rows = self.lm_update(lm_state, *out)
        if tws is not None:
            return K.rnnt_frame_beam_times_finish(ws, tws, B, Tp, beam, self.nbest, self.pad, graph=graph, normalize=self.normalize_scores)
        if graph is None:
            return K.rnnt_frame_beam_finish(ws, B, Tp, beam, self.nbest, self.pad, normalize=self.normalize_scores)
        return K.rnnt_frame_beam_bias_finish(ws, graph, B, Tp, beam, self.nbest, self.pad, normalize=self.normalize_scores)

    @torch.no_grad()
    def encode(self, sample):
        """(E fp32 [B][T'][J], encoder output lengths [B]) of a sample: the encoder and the joint's encoder branch, once."""
        net_input = sample["net_input"]
        enc = self.model.encoder(net_input["src_tokens"], net_input["src_lengths"])
        x = enc["_x_bt"][0]
        enc_len = enc["src_lengths"][0]
        B = enc_len.shape[0]
        return self.model.joint_encoder_branch(x).view(B, x.shape[0] // B, -1), enc_len

    @torch.no_grad()
    def _generate(self, sample, bos_token=None, posteriors=None):
        """posteriors: a list that gets the device rows of `score_rows` for the hypotheses, row = utterance * nbest + rank."""
        E, enc_len = self.encode(sample)
        out = self.search(E, enc_len, bos_token=bos_token)
        if posteriors is not None:
            posteriors.extend(self.score_hypotheses(E, enc_len, out, bos_token=bos_token))
        return out

    @torch.no_grad()
    def score_hypotheses(self, E, enc_len, out, bos_token=None):
        """The device rows (token factors [B * nbest][T'], end factors, posterior scores) of what `search` returned for E."""
        tokens, lengths, _, nhyp = out[:4]
        ln, utt = nbest_rows(lengths, nhyp)
        return score_rows(self.posteriors, E, enc_len, tokens.reshape(-1, tokens.shape[2]), ln, utt, (self.blank, self.pad),
                          bos_token=bos_token)

    @torch.no_grad()
    def generate(self, models, sample, **kwargs) -> List[List[Dict[str, torch.Tensor]]]:
        rows = [] if self.posteriors is not None else None
        out = self._generate(sample, bos_token=kwargs.get("bos_token", None), posteriors=rows)
        hyps = hyps_from_tensors(*(t.cpu() for t in out))
        if rows is not None:
            nbest = out[0].shape[1]
            attach_posteriors([u[i] if i < len(u) else None for u in hyps for i in range(nbest)], *(t.cpu() for t in rows))
        return hyps
