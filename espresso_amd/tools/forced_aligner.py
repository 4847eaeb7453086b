"""Forced alignment of known transcripts with a trained CTC or transducer model: when was each token (and word) spoken.

The reference aligns only through Kaldi (espresso/tools/estimate_initial_state_prior_from_alignments.py); its greedy CTC
timesteps (espresso/tools/ctc_decoder.py:171-186) belong to the hypothesis, not to the transcript.  Here the model runs its
ordinary HIP forward pass and the Viterbi search over the transcript's lattice is HIP too (csrc/align.hip):
  - CTC: encoder + log-softmax, then `ea_ctc_viterbi_align` over the extended label sequence blank y1 blank ... yU blank;
  - transducer: encoder, predictor teacher-forced on <eos> y1 ... yU, the joint network's lattice log p(blank | t,u) and
    log p(y_{u+1} | t,u) from the fused output layer + log-sum-exp pass of the RNN-T loss (the logits are not written; shapes
    the fused kernels do not take go through the materialised logits), then `ea_rnnt_viterbi_align`.
Everything stays on the device until one copy per batch brings the spans, scores and lengths to the host.

A token's span is [start, end) in encoder frames: for CTC the frames of its non-blank run, for a transducer the frame that
emits it (one frame).  `frame_seconds` converts frames to seconds; `word_spans` and `ctm_lines` build the CTM."""
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import kernels as K

SP_SPACE = "▁"  # sentencepiece's word-boundary mark


def _pad_targets(targets, target_lengths, pad_value: int, device):
    """int32 [B][max(1, Lmax)] targets (columns past a target's length = pad_value) and int32 lengths on `device`."""
    if isinstance(targets, (list, tuple)):
        target_lengths = [len(t) for t in targets]
        L = max([1] + target_lengths)
        tg = torch.full((len(targets), L), pad_value, dtype=torch.int32)
        for b, t in enumerate(targets):
            if len(t):
                tg[b, : len(t)] = torch.as_tensor(list(t), dtype=torch.int32)
    else:
        tg = targets.to(torch.int32)
        if tg.shape[1] == 0:
            tg = torch.full((tg.shape[0], 1), pad_value, dtype=torch.int32, device=tg.device)
    tl = torch.as_tensor(target_lengths, dtype=torch.int32)
    tg = tg.to(device)
    tl = tl.to(device)
    cols = torch.arange(tg.shape[1], device=device).unsqueeze(0)
    tg = torch.where(cols < tl.unsqueeze(1), tg, torch.full_like(tg, pad_value)).contiguous()
    return tg, tl.contiguous()


def _results(host: np.ndarray, B: int, L: int, end_offset: Optional[int] = None) -> List[Dict]:
    """Unpack the one int32 host copy [tokens | start | end | lengths | frames | score bits] of a batch."""
    tok = host[: B * L].reshape(B, L)
    st = host[B * L: 2 * B * L].reshape(B, L)
    en = host[2 * B * L: 3 * B * L].reshape(B, L)
    tl = host[3 * B * L: 3 * B * L + B]
    fr = host[3 * B * L + B: 3 * B * L + 2 * B]
    sc = host[3 * B * L + 2 * B:].view(np.float32)
    out = []
    for b in range(B):
        n = int(tl[b])
        feasible = bool(np.isfinite(sc[b]))
        s = st[b, :n].astype(np.int64)
        e = (s + end_offset) if end_offset is not None else en[b, :n].astype(np.int64)
        out.append({"tokens": tok[b, :n].astype(np.int64), "start": s if feasible else np.full(n, -1),
                    "end": e if feasible else np.full(n, -1), "score": float(sc[b]), "frames": int(fr[b]), "feasible": feasible})
    return out


def _attach_posteriors(results: List[Dict], logc, total):
    """The keys of tools/token_posteriors.py for the transcripts of a batch, from the kernels' device rows (one more host copy)."""
    logc, total = logc.cpu().numpy(), total.cpu().numpy()
    for b, r in enumerate(results):
        n = len(r["tokens"])
        r["token_posteriors"] = logc[b, :n].copy()
        r["end_posterior"] = float(logc[b, n])
        r["posterior_score"] = float(total[b])


class CTCForcedAligner:
    """Viterbi alignment of transcripts with an encoder-only CTC model (blank = "<s>", as in the `ctc_loss` criterion)."""

    def __init__(self, models, dictionary, blank=None, token_posteriors=False):
        self.model = models[0] if isinstance(models, (list, tuple)) else models
        self.dictionary = dictionary
        self.blank = dictionary.bos() if blank is None else blank
        self.token_posteriors = bool(token_posteriors)

    @torch.no_grad()
    def align(self, sample, targets, target_lengths=None) -> List[Dict]:
        """targets: [B][Lmax] token ids (tensor, host or device) with target_lengths, or a list of B id lists.  Returns per
        utterance: tokens, start / end (encoder frames, [start, end)), score (Viterbi log-prob), frames (valid encoder frames),
        feasible; with token_posteriors also the three keys of tools/token_posteriors.py for the transcript."""
        net_output = self.model(**sample["net_input"])
        lprobs = self.model.get_normalized_probs(net_output, log_probs=True)  # T x B x V view of [B][T][V]
        Tp, B, V = lprobs.shape
        enc_len = net_output["src_lengths"][0].to(torch.int32).contiguous()
        flat = lprobs.transpose(0, 1).reshape(B * Tp, V)
        tg, tl = _pad_targets(targets, target_lengths, 0, flat.device)
        ts, te, _, score = K.ctc_viterbi_align(flat, tg, enc_len, tl, B, Tp, V, self.blank)
        host = torch.cat([tg.flatten(), ts.flatten(), te.flatten(), tl, enc_len, score.view(torch.int32)]).cpu().numpy()
        out = _results(host, B, tg.shape[1])
        if self.token_posteriors:
            utt = torch.arange(B, dtype=torch.int32, device=flat.device)
            _attach_posteriors(out, *K.ctc_prefix_posteriors(flat, tg, utt, enc_len, tl, B, Tp, V, self.blank))
        return out


class LongFormCTCAligner:
    """Viterbi alignment of ONE recording of any length to its whole transcript with an offline encoder-only CTC model: the
    recording goes through `LongFormCTC.encode` (overlapping windows, joined on the device into one fp32 log-prob matrix on the
    recording's own frame axis, tools/long_form.py), the transcript's lattice through the tiled kernel of csrc/align_long.hip
    (`kernels.ctc_viterbi_align_long`), whatever its length: the one-workgroup kernel of
    `CTCForcedAligner` and its 1023-token cap are not involved.  With `token_posteriors` the tiled sum-product kernel of
    csrc/prefix_posterior_long.hip (`kernels.ctc_prefix_posteriors_long`) scores the same transcript on
    the same matrix."""

    def __init__(self, task, model, plan, dictionary, blank=None, max_tokens=15000, batch_size=24, token_posteriors=False):
        from .long_form import LongFormCTC

        self.model = model
        self.dictionary = dictionary
        self.blank = dictionary.bos() if blank is None else blank
        self.long_form = LongFormCTC(task, plan, self.blank, max_tokens, batch_size)
        self.token_posteriors = bool(token_posteriors)

    @torch.no_grad()
    def align(self, wave, tokens, rate=None) -> Dict:
        """wave: the recording's samples (host), at `rate` (None: the front-end's); tokens: its transcript's ids.  Returns the keys of an entry of
        `CTCForcedAligner.align` (tokens, start / end in the recording's encoder frames, score, frames, feasible) and frame_lp
        (host fp32 [T]: the log-prob of the chosen label in every frame, 0 when nothing was aligned), cuts and cut_scores (the
        junctions of `LongFormCTC.encode`); with token_posteriors also the three keys of tools/token_posteriors.py for the
        transcript.  One host copy."""
        from .long_form import at_frontend_rate

        wave = at_frontend_rate(self.long_form.task.frontend, wave, rate)  # (once, on the device; the grid below is the front-end's)
        lprobs, _, cuts, cut_scores = self.long_form.encode(self.model, wave)
        T, V = lprobs.shape[1], lprobs.shape[2]
        tg = torch.as_tensor(list(tokens), dtype=torch.int32).to(lprobs.device)
        U, J = tg.numel(), cuts.numel()
        ts, te, _, flp, score = K.ctc_viterbi_align_long(lprobs[0], tg, T, V, self.blank)
        parts = [ts, te, cuts.to(torch.int32), score.view(torch.int32), flp.view(torch.int32), cut_scores.view(torch.int32)]
        if self.token_posteriors:  # (appended: the other keys read the same words of the copy as without it)
            logc, total = K.ctc_prefix_posteriors_long(lprobs[0], tg, T, V, self.blank)
            parts += [logc.view(torch.int32), total.view(torch.int32)]
        host = torch.cat(parts).cpu().numpy()
        sc = float(host[2 * U + J: 2 * U + J + 1].view(np.float32)[0])
        feasible = bool(np.isfinite(sc))
        n = 2 * U + 2 * J + 1 + T  # the words of the copy without the posteriors
        out = {"tokens": np.asarray(list(tokens), dtype=np.int64),
               "start": host[:U].astype(np.int64) if feasible else np.full(U, -1),
               "end": host[U: 2 * U].astype(np.int64) if feasible else np.full(U, -1), "score": sc, "frames": T,
               "feasible": feasible, "frame_lp": host[2 * U + J + 1: 2 * U + J + 1 + T].view(np.float32).copy(),
               "cuts": host[2 * U: 2 * U + J].astype(np.int64), "cut_scores": host[2 * U + J + 1 + T: n].view(np.float32).copy()}
        if self.token_posteriors:
            post = host[n:].view(np.float32)
            out["token_posteriors"] = post[:U].copy()
            out["end_posterior"] = float(post[U])
            out["posterior_score"] = float(post[U + 1])
        return out


def cut_segments(words, n_frames: int, max_frames: int, min_gap_frames: int):
    """Cut an aligned recording into utterance-sized segments at its silences.  words: `word_spans` output [(word, start, end)] in
    encoder frames, in order; n_frames: the recording's frames.
    The rule.  Start from one segment holding every word.  While a segment is longer than max_frames, split it at its longest
    inter-word gap (next.start - prev.end) among the gaps of at least min_gap_frames; ties go to the gap nearest the segment's
    middle (|prev.end + next.start - segment start - segment end| smallest), then to the earlier gap; the cut frame is
    prev.end + gap // 2, which ends the left part and starts the right one.  The recording's first segment starts
    min_gap_frames // 2 before its first word and its last one ends as much after its last word, clamped to [0, n_frames].  A
    segment that is too long but has no eligible gap stays whole and is flagged `overlong`.
    Returns [(first_word, end_word, start_frame, end_frame, overlong)] in order: segment k holds words[first_word:end_word]."""
    if not words:
        return []
    pad = min_gap_frames // 2
    todo = [(0, len(words), max(0, min(int(words[0][1]) - pad, n_frames)), max(0, min(int(words[-1][2]) + pad, n_frames)))]
    done = []
    while todo:
        a, b, s, e = todo.pop()
        best = None
        if e - s > max_frames:
            for k in range(a, b - 1):
                left, right = int(words[k][2]), int(words[k + 1][1])
                gap = right - left
                if gap < min_gap_frames:
                    continue
                key = (-gap, abs(left + right - s - e), k)
                if best is None or key < best[0]:
                    best = (key, k, left + gap // 2)
        if best is None:
            done.append((a, b, s, e, e - s > max_frames))
        else:
            _, k, c = best
            todo.append((k + 1, b, c, e))  # (popped last: the left part first)
            todo.append((a, k + 1, s, c))
    return sorted(done)


@torch.no_grad()
def joint_lattice(m, E, enc_len, tg, tl, bos, pad, blank, fused=True):
    """The transducer lattice of targets tg int32 [B][U] (lengths tl int32 [B]) from the joint network's encoder branch E
    [B * T'][J] (row = utterance * T' + frame) and encoder lengths int32 [B]: the predictor teacher-forced on bos y1 ... yU, then
    the fused output layer + log-sum-exp pass of the RNN-T loss (`fused=False`, or a shape the fused kernels do not take: the
    materialised logits).  Returns (lpb, lpy fp32 [B][T'][U+1], loss fp32 [B]).  The forced aligner and the per-token posteriors
    (tools/token_posteriors.py) both read the lattice here."""
    B = enc_len.numel()
    T = E.shape[0] // B
    U1 = tg.shape[1] + 1
    prev = torch.full((B, U1), pad, dtype=torch.long, device=tg.device)
    prev[:, 0] = bos
    cols = torch.arange(U1 - 1, device=tg.device).unsqueeze(0)
    prev[:, 1:] = torch.where(cols < tl.unsqueeze(1), tg.long(), torch.full_like(prev[:, 1:], pad))
    dec, _ = m.decoder.extract_features(prev)
    D = m._joint_decoder_branch(dec.reshape(B * U1, -1)).contiguous()
    w, b = m.fc_out_params()
    V = w.shape[0]
    w16 = K.cast_f32_to_bf16(w.detach().contiguous())
    Z = K.joint_add_relu(E, D, B, T, U1) if fused else None
    if fused and U1 <= 512 and E.dtype == D.dtype == torch.float32 and K.joint_rnnt_supported(Z, w16):
        loss, ws = K.joint_rnnt_loss_fwd(Z, w16, b, tg, enc_len, tl, B, T, U1, blank)
        lpb, lpy = K.joint_rnnt_lattice(ws, B, T, U1, V)
    else:
        from .. import functional as F

        logits = F.transducer_joint(E, D, w, b, B, T, U1)
        loss, ws = K.rnnt_loss_fwd(logits, tg, enc_len, tl, blank)
        lpb, lpy = K.rnnt_lattice(ws, B, T, U1)
    return lpb, lpy, loss


class TransducerForcedAligner:
    """Viterbi alignment of transcripts with a transducer model (blank = "<s>", predictor start symbol = </s>, as in training
    with the `transducer_loss` criterion).  `fused=False` forces the materialised-logits lattice (what shapes the fused joint
    does not take use anyway)."""

    def __init__(self, models, dictionary, blank=None, bos=None, fused=True, token_posteriors=False):
        self.model = models[0] if isinstance(models, (list, tuple)) else models
        self.dictionary = dictionary
        self.blank = dictionary.bos() if blank is None else blank
        self.bos = dictionary.eos() if bos is None else bos
        self.pad = dictionary.pad()
        self.fused = fused
        self.token_posteriors = bool(token_posteriors)

    @torch.no_grad()
    def lattice(self, sample, tg, tl):
        """(lpb, lpy fp32 [B][T'][U+1], encoder lengths int32 [B], loss fp32 [B]) of targets tg int32 [B][U]."""
        m = self.model
        ni = sample["net_input"]
        enc = m.encoder(ni["src_tokens"], ni["src_lengths"])
        x = enc["_x_bt"][0]
        enc_len = enc["src_lengths"][0].to(torch.int32).contiguous()
        lpb, lpy, loss = joint_lattice(m, m.joint_encoder_branch(x).contiguous(), enc_len, tg, tl, self.bos, self.pad, self.blank,
                                       self.fused)
        return lpb, lpy, enc_len, loss

    @torch.no_grad()
    def align(self, sample, targets, target_lengths=None) -> List[Dict]:
        """As CTCForcedAligner.align; a token's span is the one frame that emits it."""
        dev = sample["net_input"]["src_tokens"].device
        tg, tl = _pad_targets(targets, target_lengths, 0, dev)
        lpb, lpy, enc_len, _ = self.lattice(sample, tg, tl)
        emit, score = K.rnnt_viterbi_align(lpb, lpy, enc_len, tl)
        host = torch.cat([tg.flatten(), emit.flatten(), emit.flatten(), tl, enc_len, score.view(torch.int32)]).cpu().numpy()
        out = _results(host, tg.shape[0], tg.shape[1], end_offset=1)
        if self.token_posteriors:
            _attach_posteriors(out, *K.rnnt_prefix_posteriors(lpb.contiguous(), lpy.contiguous(), enc_len, tl))
        return out


# ------------------------------------------------------------------------------------------------ frames, words, CTM
def subsampling_factor(encoder) -> int:
    """Input frames per encoder frame, from the encoder's own length arithmetic (the sub-sampler's time strides)."""
    probe = 720720 ** 2  # divisible by every product of two strides up to 16
    return int(round(probe / int(encoder.output_lengths(probe))))


def frame_seconds(model, frame_shift_seconds: float) -> float:
    """Seconds per encoder frame = the front-end's frame shift x the model's sub-sampling factor."""
    return frame_shift_seconds * subsampling_factor(model.encoder)


def word_spans(symbols: Sequence[str], starts: Sequence[int], ends: Sequence[int], space: str = "<space>"):
    """Group token spans into words: `space` tokens separate words (character dictionaries) and a piece that begins with
    "▁" begins one (sentencepiece).  A word spans from its first token's start to its last token's end.
    Returns [(word, start, end)]."""
    words, cur = [], None
    for sym, s, e in zip(symbols, starts, ends):
        if sym == space:
            cur = None
            continue
        if sym.startswith(SP_SPACE) or cur is None:
            cur = [sym.lstrip(SP_SPACE), int(s), int(e)]
            words.append(cur)
        else:
            cur[0] += sym
            cur[2] = int(e)
    return [(w, s, e) for w, s, e in words if w]


def ctm_lines(utt: str, units, seconds_per_frame: float, confidences: Optional[Sequence[float]] = None) -> List[str]:
    """`utt 1 start dur unit conf` lines (seconds, 3 decimals); units = [(text, start_frame, end_frame)].  The confidence column
    is 1.00 unless `confidences` gives one probability per unit (token_posteriors.unit_confidences), written to 2 decimals."""
    if confidences is None:
        return ["{} 1 {:.3f} {:.3f} {} 1.00".format(utt, s * seconds_per_frame, (e - s) * seconds_per_frame, text)
                for text, s, e in units]
    assert len(confidences) == len(units), (len(confidences), len(units))
    return ["{} 1 {:.3f} {:.3f} {} {:.2f}".format(utt, s * seconds_per_frame, (e - s) * seconds_per_frame, text, c)
            for (text, s, e), c in zip(units, confidences)]


def utterance_units(result: Dict, dictionary, unit: str = "token"):
    """[(text, start_frame, end_frame)] of one feasible alignment result: its tokens, or its words (`word_spans`)."""
    syms = [dictionary[int(t)] for t in result["tokens"]]
    if unit == "word":
        return word_spans(syms, result["start"], result["end"], space=getattr(dictionary, "space_word", "<space>"))
    return [(s, int(a), int(b)) for s, a, b in zip(syms, result["start"], result["end"])]
