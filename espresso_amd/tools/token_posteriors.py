"""Per-token posteriors of CTC and transducer hypotheses: what an attention decoder's positional_scores are for the two other
model families (the reference has them for its attention decoder only).

For a label sequence y1 .. yU let Psi_i = log P(the model's output starts with y1 .. yi | x), summed over all continuations and
all alignments.  Then log c_i = Psi_i - Psi_{i-1} is the posterior of token i given the audio and the tokens before it, log c_end
= log P(y | x) - Psi_U that of stopping after yU, and the factors add up to log P(y | x) = -(CTC / RNN-T loss).  Both recurrences
are one more scan of a lattice the project already builds (csrc/prefix_posterior.hip).

The posterior is the acoustic model's own: no LM, no insertion bonus, no hotword bias, temperature 1, and for a transducer the
standard lattice (any number of symbols per frame) even where the search that found the hypothesis allowed fewer.  It covers the
label sequence the model emitted: symbols the host adds or strips (blank, pad, <eos>) get no factor (0 in "token_posteriors").
How well exp(log c_i) is calibrated against word correctness has not been measured.

The offline decoders take `token_posteriors=True` and then add to every hypothesis "token_posteriors" (fp32 [len(tokens)], the
log c_i), "end_posterior" (log c_end) and "posterior_score" (log P(y | x)), computed from the log-probs / encoder output the
search itself used."""
from typing import Dict, List, Sequence

import torch

from .. import kernels as K

MAX_LABELS = 1023  # labels per hypothesis the kernels take (ea_ctc_prefix_posteriors: Lmax <= 1023, ea_rnnt_...: U1 <= 1024)
JOINT_GROUP_BYTES = 256 << 20  # the joint activations (and, where they are materialised, the logits) of one group of hypotheses


def compact_labels(tokens, lengths, drop: Sequence[int]):
    """Device rows tokens int [N][L] (valid: the first lengths[n]) -> the label sequences without the symbols in `drop`, in
    order: (labels int32 [N][L], n_labels int32 [N], pos int64 [N][L]: the column each label came from).  No synchronisation."""
    N, L = tokens.shape
    cols = torch.arange(L, device=tokens.device).unsqueeze(0)
    keep = cols < lengths.unsqueeze(1)
    for s in drop:
        keep = keep & (tokens != s)
    pos = torch.sort((~keep).to(torch.int8), dim=1, stable=True)[1]
    n_labels = keep.sum(1).to(torch.int32)
    labels = torch.where(cols < n_labels.unsqueeze(1), tokens.gather(1, pos), torch.zeros_like(tokens)).to(torch.int32)
    return labels.contiguous(), n_labels.contiguous(), pos


def spread_factors(logc, total, n_labels, pos, L):
    """Kernel rows logc fp32 [N][>= n + 1] -> (token factors fp32 [N][L] at the columns the labels came from, 0 elsewhere; end
    factor fp32 [N]).  A hypothesis with more than MAX_LABELS labels was not scored: its values are NaN."""
    N, W = logc.shape
    cols = torch.arange(L, device=logc.device).unsqueeze(0)
    src = torch.zeros(N, L, dtype=torch.float32, device=logc.device)
    w = min(W - 1, L)
    src[:, :w] = logc[:, :w]
    src = torch.where(cols < n_labels.unsqueeze(1), src, torch.zeros_like(src))
    tok = torch.zeros(N, L, dtype=torch.float32, device=logc.device).scatter_(1, pos, src)
    end = logc.gather(1, n_labels.clamp(max=W - 1).long().unsqueeze(1)).squeeze(1)
    too_long = n_labels > MAX_LABELS
    nan = torch.full_like(end, float("nan"))
    return (torch.where(too_long.unsqueeze(1), nan.unsqueeze(1).expand(N, L), tok), torch.where(too_long, nan, end),
            torch.where(too_long, nan, total))


def attach_posteriors(hyps: List[Dict], tok, end, total):
    """Host rows (tok [N][L], end [N], total [N]) -> the three keys of hypotheses 0 .. N-1 (hyps[n] is row n)."""
    for n, h in enumerate(hyps):
        if h is not None:
            h["token_posteriors"] = tok[n, : len(h["tokens"])].clone()
            h["end_posterior"] = end[n]
            h["posterior_score"] = total[n]


class CTCTokenPosteriors:
    """Per-token posteriors under an encoder-only CTC model's log-probs (blank = "<s>", as in the `ctc_loss` criterion)."""

    def __init__(self, dictionary, blank=None):
        self.blank = dictionary.bos() if blank is None else blank
        self.vocab_size = len(dictionary)

    @torch.no_grad()
    def score(self, lprobs, enc_len, tokens, lengths, utt):
        """lprobs fp32/bf16 [B][T][V] log-probs (row-contiguous), enc_len int [B]; hypotheses tokens int32 [N][L] (labels only;
        columns past lengths[n] are ignored), lengths int32 [N], utt int32 [N]: the utterance hypothesis n belongs to.  Returns
        device tensors (logc fp32 [N][min(L, 1023) + 1]: log c_1 .. log c_U, log c_end, then 0; total fp32 [N] = log P(y | x)).
        No host synchronisation."""
        B, T, V = lprobs.shape
        assert V == self.vocab_size and lprobs.stride(2) == 1 and lprobs.stride(0) == T * lprobs.stride(1)
        x = lprobs.view(B * T, V) if lprobs.is_contiguous() else lprobs.reshape(B * T, V)
        dev = x.device
        tokens = tokens.to(device=dev, dtype=torch.int32)
        if tokens.shape[1] == 0:
            tokens = torch.zeros(tokens.shape[0], 1, dtype=torch.int32, device=dev)
        tokens = tokens[:, :MAX_LABELS].contiguous()
        as_i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()  # noqa: E731
        return K.ctc_prefix_posteriors(x, tokens, as_i32(utt), as_i32(enc_len), as_i32(lengths), B, T, V, self.blank)


class TransducerTokenPosteriors:
    """Per-token posteriors under a transducer model (blank = "<s>", predictor start symbol = </s>, as in training with the
    `transducer_loss` criterion): the predictor is teacher-forced on every hypothesis and the lattice is the forced aligner's
    (`forced_aligner.joint_lattice`: the fused joint + log-sum-exp pass, the materialised logits for shapes it refuses)."""

    def __init__(self, model, dictionary, blank=None, bos=None, fused=True):
        self.model = model
        self.blank = dictionary.bos() if blank is None else blank
        self.bos = dictionary.eos() if bos is None else bos
        self.pad = dictionary.pad()
        self.fused = fused

    def _node_bytes(self, J, U1):
        """Bytes per lattice node a group holds at once: the bf16 joint activations, plus the fp32 logits where the fused
        kernels do not take the shape."""
        V = self.model.fc_out_params()[0].shape[0]
        fused = self.fused and U1 <= 512 and J % 64 == 0
        return 2 * J + (0 if fused else 4 * ((V + 63) // 64 * 64))

    @torch.no_grad()
    def score(self, encoder_out, enc_len, tokens, lengths, utt, bos_token=None):
        """encoder_out fp32 [B][T][J]: the joint network's encoder branch (`joint_encoder_branch`) of the batch, enc_len int
        [B]; tokens / lengths / utt as CTCTokenPosteriors.score.  Returns device tensors (logc fp32 [N][U + 1], total fp32 [N])
        with U = the longest hypothesis (at most 1023 labels; one host read, of that length).  Hypotheses are scored in groups
        whose joint activations stay under JOINT_GROUP_BYTES."""
        from .forced_aligner import joint_lattice

        B, T, J = encoder_out.shape
        dev = encoder_out.device
        N = tokens.shape[0]
        lengths = lengths.to(device=dev, dtype=torch.int32)
        U = min(MAX_LABELS, max(1, int(lengths.max()) if N else 1))
        tg = torch.zeros(N, U, dtype=torch.int32, device=dev)
        w = min(U, tokens.shape[1])
        tg[:, :w] = tokens[:, :w].to(device=dev, dtype=torch.int32)
        tl = lengths.clamp(0, U).contiguous()
        utt = utt.to(device=dev).long()
        enc_len = enc_len.to(device=dev, dtype=torch.int32)
        logc = torch.empty(N, U + 1, dtype=torch.float32, device=dev)
        total = torch.empty(N, dtype=torch.float32, device=dev)
        group = max(1, JOINT_GROUP_BYTES // max(1, T * (U + 1) * self._node_bytes(J, U + 1)))
        for n0 in range(0, N, group):
            sel = utt[n0: n0 + group]
            E = encoder_out.index_select(0, sel).reshape(-1, J)
            el = enc_len.index_select(0, sel).contiguous()
            lpb, lpy, _ = joint_lattice(self.model, E, el, tg[n0: n0 + group].contiguous(), tl[n0: n0 + group].contiguous(),
                                        self.bos if bos_token is None else bos_token, self.pad, self.blank, self.fused)
            c, t = K.rnnt_prefix_posteriors(lpb.contiguous(), lpy.contiguous(), el, tl[n0: n0 + group].contiguous())
            logc[n0: n0 + group] = c
            total[n0: n0 + group] = t
        return logc, total


def score_rows(scorer, source, enc_len, tokens, lengths, utt, drop, **kw):
    """What a decoder does with its scorer: device rows tokens int [N][L] (valid: the first lengths[n]; symbols in `drop` are
    not labels) -> device (token factors fp32 [N][L], end factors fp32 [N], posterior scores fp32 [N])."""
    lengths = lengths.to(tokens.device).clamp(0, tokens.shape[1])
    labels, n_labels, pos = compact_labels(tokens, lengths, drop)
    logc, total = scorer.score(source, enc_len, labels, n_labels, utt, **kw)
    return spread_factors(logc, total, n_labels, pos, tokens.shape[1])


def nbest_rows(lengths, nhyp):
    """A beam search's lengths int32 [B][nbest] and nhyp int32 [B] -> (lengths int32 [B * nbest] with 0 for the rows past nhyp,
    whose contents are not defined; utt int32 [B * nbest])."""
    B, nbest = lengths.shape
    i = torch.arange(nbest, device=lengths.device).unsqueeze(0)
    ln = torch.where(i < nhyp.unsqueeze(1), lengths, torch.zeros_like(lengths)).reshape(-1)
    return ln, torch.arange(B, device=lengths.device, dtype=torch.int32).repeat_interleave(nbest)


# ------------------------------------------------------------------------------------------------ confidences for the CTM / C- line
def unit_confidences(symbols: Sequence[str], log_factors: Sequence[float], unit: str = "token", space: str = "<space>") -> List[float]:
    """Probabilities in the order `forced_aligner.utterance_units` lists the units of the same symbols: for a token exp(log c_i);
    for a word the product over its own tokens (`space` tokens belong to no word, a sentencepiece mark belongs to its piece)."""
    import math

    from .forced_aligner import SP_SPACE

    if unit != "word":
        return [math.exp(f) for f in log_factors]
    words, cur = [], None
    for sym, f in zip(symbols, log_factors):
        if sym == space:
            cur = None
            continue
        if sym.startswith(SP_SPACE) or cur is None:
            cur = [sym.lstrip(SP_SPACE), float(f)]
            words.append(cur)
        else:
            cur[0] += sym
            cur[1] += float(f)
    return [math.exp(f) for w, f in words if w]


def word_log_factors(symbols: Sequence[str], log_factors: Sequence[float], space: str = "<space>") -> List[List[float]]:
    """The log factors of every word's own tokens, words grouped and ordered as `unit_confidences(..., "word")` groups them (the
    exp of a row's sum is that word's probability there)."""
    from .forced_aligner import SP_SPACE

    words, cur = [], None
    for sym, f in zip(symbols, log_factors):
        if sym == space:
            cur = None
            continue
        if sym.startswith(SP_SPACE) or cur is None:
            cur = [sym.lstrip(SP_SPACE), [float(f)]]
            words.append(cur)
        else:
            cur[0] += sym
            cur[1].append(float(f))
    return [fs for w, fs in words if w]


def segment_confidence(word_factors: Sequence[Sequence[float]]):
    """(mean token log-posterior, lowest word probability, words) of a stretch of words given as rows of `word_log_factors`:
    the mean runs over the words' own tokens, a word's probability is the product over its tokens.  No word: (0.0, 1.0, 0)."""
    import math

    flat = [f for fs in word_factors for f in fs]
    if not flat:
        return 0.0, 1.0, 0
    return sum(flat) / len(flat), min(math.exp(sum(fs)) for fs in word_factors), len(word_factors)


def confidence_line(utt: str, token_log_factors: Sequence[float], end_log_factor: float) -> str:
    """`C-<utt>\\t` + the token probabilities and the end probability, space-separated, 4 decimals."""
    import math

    return "C-{}\t{}".format(utt, " ".join("{:.4f}".format(math.exp(f)) for f in list(token_log_factors) + [end_log_factor]))
