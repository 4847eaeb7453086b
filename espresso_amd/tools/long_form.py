"""Long-form recognition for offline CTC models: a recording longer than the model was trained on is cut
into overlapping windows on the encoder's frame grid, the existing offline encoder runs on batches of windows, and two kernels
(csrc/long_form.hip) join the per-window logits on the device into one fp32 log-prob matrix on the recording's own frame axis.
Everything downstream takes log-probs -- the greedy decoder, the prefix and lexicon beam searches, the keyword spotter -- and so
works unchanged and in global time.  The reference has no long-form path.

The plan (host, pure Python).  g = samples per encoder frame (frame shift x the sub-sampler's time stride; 640 for the recipes).
Window W and overlap O are multiples of g, hop H = W - O; a recording of N samples gets Nw = max(1, ceil((N - O) / H)) windows,
window n = samples [n * H, n * H + W), the last one running to the recording's end (its length lies in (O, W]).  With H a multiple
of g, encoder frame j of window n is global frame n * Hf + j (Hf = H / g), a full window has W / g frames and
(Nw - 1) * Hf + T_last is the recording's own frame count: `check_grid` verifies this arithmetic against the front-end and the
model at hand and refuses what breaks it.

The join.  At junction n the cut c in the overlap gives the frames < c to window n and the rest to window n + 1; it is put where
both windows agree on blank for 2 * guard frames, `edge` frames off either end of the overlap (include/espresso_amd.h, "Long-form
recognition").  The defaults of window, overlap, edge and guard are uncalibrated: no trained CTC model and no long corpus was at
hand to measure WER with them.

Offline transducer models: the frame-synchronous searches see the encoder only through one row per
frame, so for them the same windows' ENCODER OUTPUTS are joined instead, into one [T][D] matrix that the search decodes as one
utterance (`LongFormTransducer`, `LongFormTransducerModel`).  Without a blank column the cut goes where the two windows' rows
agree (relative squared distance, include/espresso_amd.h); that rule is as uncalibrated as the defaults."""
import math
import os
from typing import List, Optional

import numpy as np
import torch

from .. import kernels as K

DEFAULT_WINDOW_S, DEFAULT_OVERLAP_S, DEFAULT_GUARD_FRAMES = 30.0, 6.0, 2
UNCALIBRATED = "an option default, uncalibrated: no WER on real long recordings has been measured"


class LongFormPlan:
    """The windows of recordings: W, O, H in samples (multiples of g), Tw = W / g, Of = O / g, Hf = H / g in encoder frames."""

    def __init__(self, g: int, window: int, overlap: int, edge_frames: Optional[int] = None, guard_frames: int = DEFAULT_GUARD_FRAMES):
        if g < 1:
            raise ValueError(f"long-form: {g} samples per encoder frame")
        if window % g or overlap % g:
            raise ValueError(f"long-form: window {window} and overlap {overlap} must be multiples of the {g} samples of an encoder frame")
        if overlap < 2 * g:
            raise ValueError(f"long-form: the overlap ({overlap} samples) must cover at least two encoder frames ({2 * g} samples)")
        if 2 * overlap >= window:
            raise ValueError(f"long-form: the overlap ({overlap} samples) must be less than half the window ({window} samples): a "
                             "frame may lie in two windows, not in three")
        self.g, self.W, self.O, self.H = g, window, overlap, window - overlap
        self.Tw, self.Of, self.Hf = window // g, overlap // g, (window - overlap) // g
        if self.Of > K.LONGFORM_MAX_OVERLAP:
            raise ValueError(f"long-form: an overlap of {self.Of} encoder frames exceeds the {K.LONGFORM_MAX_OVERLAP} the cut kernel holds")
        self.edge = self.Of // 4 if edge_frames is None else int(edge_frames)
        self.guard = int(guard_frames)
        if self.edge < 0 or self.guard < 0:
            raise ValueError("long-form: edge and guard frames must not be negative")
        if 2 * self.edge > self.Of:
            raise ValueError(f"long-form: {self.edge} edge frames on either side leave no cut in an overlap of {self.Of} frames")

    @classmethod
    def from_seconds(cls, g, sample_rate, window_s=DEFAULT_WINDOW_S, overlap_s=DEFAULT_OVERLAP_S, edge_frames=None,
                     guard_frames=DEFAULT_GUARD_FRAMES):
        """Window and overlap in seconds, each rounded to a multiple of g."""
        return cls(g, int(round(window_s * sample_rate / g)) * g, int(round(overlap_s * sample_rate / g)) * g, edge_frames, guard_frames)

    def num_windows(self, n_samples: int) -> int:
        return max(1, -(-(n_samples - self.O) // self.H))

    def windows(self, n_samples: int) -> List[tuple]:
        """(start, length) in samples of every window of a recording of n_samples."""
        nw = self.num_windows(n_samples)
        return [(n * self.H, self.W if n < nw - 1 else n_samples - n * self.H) for n in range(nw)]


def samples_per_frame(frontend, model) -> int:
    """g: the front-end's frame shift x the sub-sampler's total time stride."""
    return int(frontend.frame_shift) * time_stride(model)


def time_stride(model) -> int:
    """The encoder's total time stride, read off `output_lengths`."""
    probe = 1 << 12
    out = int(model.output_lengths(probe))
    if out < 1 or probe % out:
        raise NotImplementedError(f"long-form: the encoder maps {probe} frames to {out}: no integer time stride")
    return probe // out


def check_grid(frontend, model, plan: LongFormPlan):
    """Refuse, naming what breaks it, a front-end or model whose windows do not sit on the recording's frame grid."""
    if getattr(frontend, "specaug", None) is not None and getattr(model, "training", False):
        raise NotImplementedError("long-form: SpecAugment in training mode changes the features per utterance")
    for name in ("dither", "utterance_cmvn", "per_utterance_norm"):
        if getattr(frontend, name, 0):
            raise NotImplementedError(f"long-form: the front-end's {name} makes a window's features differ from the recording's")
    shift, flen = int(frontend.frame_shift), int(frontend.frame_len)
    stride = time_stride(model)
    if plan.g != shift * stride:
        raise NotImplementedError(f"long-form: the plan's {plan.g} samples per encoder frame are not frame shift {shift} x stride {stride}")
    enc = getattr(model, "encoder", model)
    if getattr(getattr(enc, "cfg", None), "encoder", None) is not None and getattr(enc.cfg.encoder, "chunk_size", 0) > 0:
        raise NotImplementedError("long-form runs offline encoders; a chunk-streaming encoder is decoded with --streaming --stream-endpoint")
    pre = getattr(enc, "pre_encoder", None)
    if pre is not None:
        for ks in getattr(pre, "kernel_sizes", []):
            ks = tuple(ks) if isinstance(ks, (list, tuple)) else (ks, ks)
            if ks != (3, 3):
                raise NotImplementedError(f"long-form: sub-sampler kernel size {ks} is not the recipes' 3x3; the frame grid is unverified for it")
    # the arithmetic itself, on the functions as they stand
    if plan.H % shift or frontend.num_frames(plan.H + flen) != plan.H // shift + 1:
        raise NotImplementedError(f"long-form: a hop of {plan.H} samples is not a whole number of front-end frames (frame shift {shift})")
    if int(model.output_lengths(frontend.num_frames(plan.W))) != plan.Tw:
        raise NotImplementedError(f"long-form: a window of {plan.W} samples gives {int(model.output_lengths(frontend.num_frames(plan.W)))} "
                                  f"encoder frames, not {plan.Tw} (frame length {flen}, frame shift {shift}, stride {stride})")
    if (plan.H // shift) % stride:
        raise NotImplementedError(f"long-form: a hop of {plan.H // shift} front-end frames is no multiple of the encoder's stride {stride}")
    if flen > plan.O:
        raise NotImplementedError(f"long-form: the overlap ({plan.O} samples) is shorter than one front-end frame ({flen})")


def window_frames(frontend, model, plan: LongFormPlan, n_samples: int) -> List[int]:
    """Encoder frames of every window of a recording (host arithmetic: `num_frames`, then `output_lengths`)."""
    return [int(model.output_lengths(frontend.num_frames(ln))) for _, ln in plan.windows(n_samples)]


def at_frontend_rate(frontend, wave, rate=None):
    """The recording at the front-end's rate (host fp32): one pass of the device resampler over the whole recording when `rate`
    is another one, the samples themselves otherwise.  Window plans, cuts and times then live on the front-end's grid, whose
    seconds are the recording's (data/resample.py preserves durations)."""
    if rate is None or int(rate) == frontend.sample_rate:
        return wave
    dev = frontend.device
    x = torch.from_numpy(np.ascontiguousarray(wave, dtype=np.float32)).to(dev)
    off = torch.tensor([0, len(wave)], dtype=torch.int64).to(dev)
    y, _, _ = frontend.resampler(x, off, [len(wave)], [int(rate)])
    return y.cpu().numpy()


@torch.no_grad()
def window_rows(task, plan: LongFormPlan, frames_model, wave, max_tokens, batch_size, rows_of):
    """(rows [Nw][Tw][C] of every window of a recording as the model wrote them, counts: host list of frames per window).  The
    windows go through the offline forward in length-sorted batches under the max_tokens / batch_size budget; rows_of(net_input)
    runs it on one batch and answers (rows [B * Tp][C], row pitch >= C; B; Tp).  frames_model: whose `output_lengths` count the
    frames.  One recording's rows stay on the device.  A recording of one window: Tw is that window's own frame count."""
    from ..speech_recognize import collate, make_batches

    dev = task.frontend.device
    wins = plan.windows(len(wave))
    counts = window_frames(task.frontend, frames_model, plan, len(wave))
    Nw = len(wins)
    Tw = plan.Tw if Nw > 1 else counts[0]
    pieces = [wave[a: a + ln] for a, ln in wins]
    names = [str(n) for n in range(Nw)]
    buf = None
    for ids in make_batches(names, [ln for _, ln in wins], max_tokens, batch_size):
        s = task.prepare_sample(collate(ids, names, pieces, dev), train=False)
        rows, B, Tp = rows_of(s["net_input"])
        C = rows.shape[1]
        if Tp > Tw or Tp != max(counts[i] for i in ids):
            raise RuntimeError(f"long-form: a batch of windows has {Tp} encoder frames, the plan {max(counts[i] for i in ids)} (at most {Tw})")
        if buf is None:
            buf = torch.empty(Nw, max(Tw, 1), C, dtype=rows.dtype, device=rows.device)
        src = rows.view(B, Tp, C) if rows.is_contiguous() else torch.as_strided(rows, (B, Tp, C), (Tp * rows.stride(0), rows.stride(0), 1))
        buf[:, :Tp].index_copy_(0, torch.tensor(ids, dtype=torch.long, device=rows.device), src)
    return buf, counts


class LongFormCTC:
    """The front part of long-form recognition: `encode` turns one recording into stitched log-probs."""

    def __init__(self, task, plan: LongFormPlan, blank: int, max_tokens: int = 15000, batch_size: int = 24):
        self.task, self.plan, self.blank = task, plan, int(blank)
        self.max_tokens, self.batch_size = max_tokens, batch_size
        self._checked = None

    @torch.no_grad()
    def window_logits(self, model, wave):
        """(logits [Nw][Tw][V] as the encoder wrote them (bf16, or fp32), counts: host list of frames per window).  The windows
        go through the existing offline forward in length-sorted batches under the max_tokens / batch_size budget; one
        recording's window logits stay on the device.  A recording of one window: Tw is that window's own frame count."""
        if self._checked is not model:
            check_grid(self.task.frontend, model, self.plan)
            self._checked = model

        def rows_of(net_input):
            out = model(**net_input)
            lg = out.get("_logits_bt")
            if not lg:
                raise NotImplementedError("long-form needs an encoder-only CTC model that returns its vocabulary logits")
            B, Tp = out["encoder_padding_mask"][0].shape
            return lg[0], B, Tp

        return window_rows(self.task, self.plan, model, wave, self.max_tokens, self.batch_size, rows_of)

    @torch.no_grad()
    def stitch(self, logits, counts: List[int]):
        """logits [Nw][Tw][V], counts (host) -> (lprobs fp32 [1][T][V], in_len int32 [1], cuts int32 [Nw - 1], scores fp32
        [Nw - 1]): the two kernels, once per recording."""
        Nw, Tw, V = logits.shape
        T = (Nw - 1) * self.plan.Hf + counts[-1]
        cdev = torch.tensor(counts, dtype=torch.int32).to(logits.device)
        cuts, scores = K.longform_cuts(logits, cdev, V, self.plan.Hf if Nw > 1 else max(Tw, 1), self.blank, self.plan.edge, self.plan.guard)
        out = K.longform_stitch(logits, cdev, cuts, V, self.plan.Hf if Nw > 1 else max(Tw, 1), T)
        return out.view(1, T, V), torch.tensor([T], dtype=torch.int32).to(logits.device), cuts, scores

    @torch.no_grad()
    def encode(self, model, wave, rate=None):
        """One recording (host samples, at `rate`; None: the front-end's) -> (lprobs fp32 [1][T][V], in_len, cuts, scores)."""
        logits, counts = self.window_logits(model, at_frontend_rate(self.task.frontend, wave, rate))
        return self.stitch(logits, counts)


class LongFormModel:
    """What the CTC decoders ask of a model -- a forward and `get_normalized_probs` -- answered from stitched log-probs, so that
    `CTCDecoder`, `CTCPrefixBeamSearchDecoder` and `CTCLexiconBeamSearchDecoder` decode a recording as they decode an utterance.
    A sample's net_input is {"wave": the recording's samples (host)}, with "rate" when they are not at the front-end's rate.
    `junctions` collects (cuts, scores) per recording."""

    def __init__(self, model, long_form: LongFormCTC):
        self.model, self.long_form = model, long_form
        self.junctions = []
        self.lprobs = None  # the last recording's matrix [1][T][V] (what `LongFormPosteriors` scores the hypotheses on)

    def __call__(self, wave, rate=None):
        lprobs, in_len, cuts, scores = self.long_form.encode(self.model, wave, **({} if rate is None else {"rate": rate}))
        self.junctions.append((cuts, scores))
        self.lprobs = lprobs
        return {"_lprobs": lprobs, "src_lengths": [in_len], "encoder_padding_mask": [torch.zeros(1, lprobs.shape[1], dtype=torch.bool,
                                                                                                  device=lprobs.device)]}

    def get_normalized_probs(self, net_output, log_probs, sample=None):
        lp = net_output["_lprobs"]
        return (lp if log_probs else lp.exp()).transpose(0, 1)  # T x 1 x V view of [1][T][V]

    def output_lengths(self, in_lengths):
        return self.model.output_lengths(in_lengths)

    def cuda(self):
        return self

    def worst_score(self):
        """The lowest junction score so far (None without junctions): a cut made through speech shows here."""
        s = [sc for _, sc in self.junctions if sc.numel()]
        return float(torch.cat(s).min()) if s else None


class LongFormPosteriors:
    """A generator around a CTC generator that decodes a `LongFormModel`: after the search, every hypothesis of the n-best gets
    the three keys of tools/token_posteriors.py, computed by the tiled kernel (`kernels.ctc_prefix_posteriors_long`, DESIGN.md
    section 3.10) on the matrix the search read, whatever the hypothesis' length.  Blank and pad are no labels (factor 0), as in
    `token_posteriors.score_rows`.  Tokens, scores, order and times are the inner generator's.  One host copy per hypothesis."""

    def __init__(self, generator, model: LongFormModel, dictionary, blank=None):
        self.generator, self.model = generator, model
        self.blank = dictionary.bos() if blank is None else blank
        self.pad = dictionary.pad()

    def __getattr__(self, name):  # (symbols_to_strip_from_output and the like: the inner generator's)
        return getattr(self.generator, name)

    @torch.no_grad()
    def generate(self, models, sample, **kwargs):
        hyps = self.generator.generate(models, sample, **kwargs)
        lprobs = self.model.lprobs
        assert len(hyps) == 1 and lprobs is not None and lprobs.shape[0] == 1, "one recording per sample"
        T, V = lprobs.shape[1], lprobs.shape[2]
        for h in hyps[0]:
            toks = h["tokens"].tolist()
            keep = [k for k, t in enumerate(toks) if t != self.blank and t != self.pad]
            labels = torch.tensor([toks[k] for k in keep], dtype=torch.int32).to(lprobs.device)
            logc, total = K.ctc_prefix_posteriors_long(lprobs[0], labels, T, V, self.blank)
            host = torch.cat([logc, total]).cpu()
            tok = torch.zeros(len(toks), dtype=torch.float32)
            tok[keep] = host[: len(keep)]
            h["token_posteriors"], h["end_posterior"], h["posterior_score"] = tok, host[len(keep)], host[len(keep) + 1]
        self.model.lprobs = None
        return hyps


class LongFormTransducer:
    """The front part of long-form recognition for an offline transducer model: `encode` turns one
    recording into the encoder outputs [T][D] of its frames, each row the bit copy of the owning window's, joined where the two
    windows' encoders agree (kernels.longform_feature_cuts, kernels.longform_stitch_rows).  The frame-synchronous searches see
    the encoder only through one row per frame, so they decode that matrix as one utterance's."""

    def __init__(self, task, plan: LongFormPlan, max_tokens: int = 15000, batch_size: int = 24):
        self.task, self.plan = task, plan
        self.max_tokens, self.batch_size = max_tokens, batch_size
        self._checked = None

    @torch.no_grad()
    def window_features(self, model, wave):
        """(x [Nw][Tw][D] = `_x_bt` of every window as the encoder wrote it, counts: host list of frames per window), batched as
        `LongFormCTC.window_logits` batches them."""
        enc = model.encoder
        if self._checked is not model:
            check_grid(self.task.frontend, enc, self.plan)
            self._checked = model

        def rows_of(net_input):
            out = enc(net_input["src_tokens"], net_input["src_lengths"])
            x = out["_x_bt"][0]
            B = out["src_lengths"][0].shape[0]
            return x, B, x.shape[0] // B

        return window_rows(self.task, self.plan, enc, wave, self.max_tokens, self.batch_size, rows_of)

    @torch.no_grad()
    def stitch(self, features, counts: List[int]):
        """features [Nw][Tw][D], counts (host) -> (X [T][D] in the features' dtype, enc_len int32 [1], cuts int32 [Nw - 1], scores
        fp32 [Nw - 1]): the two kernels, once per recording."""
        Nw, Tw, D = features.shape
        T = (Nw - 1) * self.plan.Hf + counts[-1]
        Hf = self.plan.Hf if Nw > 1 else max(Tw, 1)
        cdev = torch.tensor(counts, dtype=torch.int32).to(features.device)
        cuts, scores = K.longform_feature_cuts(features, cdev, D, Hf, self.plan.edge, self.plan.guard)
        out = K.longform_stitch_rows(features, cdev, cuts, D, Hf, T)
        return out, torch.tensor([T], dtype=torch.int32).to(features.device), cuts, scores

    @torch.no_grad()
    def encode(self, model, wave, rate=None):
        """One recording (host samples, at `rate`; None: the front-end's) -> (X [T][D], enc_len int32 [1], cuts, scores)."""
        features, counts = self.window_features(model, at_frontend_rate(self.task.frontend, wave, rate))
        return self.stitch(features, counts)


def frame_beam_search_bytes(T: int, beam: int, joint_dim: int, nbest: int = 1, biased: bool = False, times: bool = False) -> int:
    """Device bytes `TransducerFrameBeamDecoder.search` allocates for one utterance of T frames, every one of them before its
    loop: the joint's encoder branch fp32 [T][J], the row table int32 [T][beam], the workspace of csrc/rnnt_beam.hip (per
    utterance 3 * tsize + 2 * cap words and change, cap = 1 + T * beam, tsize the power of two >= 2 * cap; 2 * cap more for the
    times) and the readout int32 [nbest][T] (twice with times)."""
    L = K._lib.lib()
    ws = L.ea_rnnt_frame_beam_bias_workspace_bytes(1, T, beam) if biased else L.ea_rnnt_frame_beam_workspace_bytes(1, T, beam)
    tws = L.ea_rnnt_frame_beam_times_workspace_bytes(1, T, beam) if times else 0
    return int(4 * T * joint_dim + 4 * T * beam + ws + tws + 4 * nbest * T * (2 if times else 1))


class _StitchedEncoder:
    """The `encoder` of a `LongFormTransducerModel`."""

    def __init__(self, owner):
        self.owner = owner

    def __call__(self, src_tokens, src_lengths=None, **kwargs):
        """src_tokens: the recording's samples (host array); src_lengths: its sample rate, None for the front-end's."""
        o = self.owner
        x, enc_len, cuts, scores = o.long_form.encode(o.model, src_tokens, **({} if src_lengths is None else {"rate": int(src_lengths)}))
        o.junctions.append((cuts, scores))
        o.check_memory(x.shape[0])
        return {"_x_bt": [x], "src_lengths": [enc_len],
                "encoder_padding_mask": [torch.zeros(1, x.shape[0], dtype=torch.bool, device=x.device)]}

    def output_lengths(self, in_lengths):
        return self.owner.model.encoder.output_lengths(in_lengths)


class LongFormTransducerModel:
    """What the frame-synchronous transducer decoders ask of a model, with the encoder answered from a recording's stitched
    encoder outputs: `.encoder(src_tokens, src_lengths)` takes the recording's samples (host) as src_tokens and their sample rate
    (None: the front-end's) as src_lengths -- `net_input` builds that dict -- and returns `_x_bt` [T][D] and `src_lengths` [1];
    `decoder`, `joint_encoder_branch`, `joint_step` and everything else are the model's.  `TransducerGreedyDecoder` and
    `TransducerFrameBeamDecoder` so decode a recording as they decode an utterance: predictor, LM, context-graph state and time
    nodes run from the first frame to the last.  One recording per sample.  `junctions` collects (cuts, scores) per recording.
    search: (beam, nbest, biased, times) of a frame beam search that will read the output: its allocations are then checked
    against the device's free memory before the search starts."""

    def __init__(self, model, long_form: LongFormTransducer, search=None):
        self.model, self.long_form, self.search = model, long_form, search
        self.junctions = []
        self.encoder = _StitchedEncoder(self)

    def __getattr__(self, name):  # (decoder, joint_encoder_branch, joint_step, ...: the model's)
        return getattr(self.__dict__["model"], name)

    @staticmethod
    def net_input(wave, rate=None):
        return {"src_tokens": wave, "src_lengths": rate}

    def eval(self):
        self.model.eval()
        return self

    def cuda(self):
        return self

    def check_memory(self, T: int):
        if self.search is None or not torch.cuda.is_available():
            return
        beam, nbest, biased, times = self.search
        need = frame_beam_search_bytes(T, beam, self.model.proj_encoder.weight.shape[0], nbest, biased, times)
        free = int(torch.cuda.mem_get_info(self.long_form.task.frontend.device)[0])
        if need > free:
            raise ValueError(f"--long-form-transducer: the frame beam search of {T} frames at beam {beam} needs {need} bytes of device "
                             f"memory, {free} are free: decode the recording in parts, or lower --beam")

    def worst_score(self):
        """The lowest junction score so far (None without junctions): 0 = both windows gave the same features around every cut."""
        s = [sc for _, sc in self.junctions if sc.numel()]
        return float(torch.cat(s).min()) if s else None


def add_long_form_args(p):
    p.add_argument("--long-form", action="store_true",
                   help="decode every recording as overlapping windows of an offline encoder-only CTC model, joined on the device "
                        "into one log-prob matrix on the recording's own frame axis (any length; times are global)")
    p.add_argument("--long-form-window-s", type=float, default=None, help=f"--long-form: window in seconds (default {DEFAULT_WINDOW_S:g}; {UNCALIBRATED})")
    p.add_argument("--long-form-overlap-s", type=float, default=None,
                   help=f"--long-form: overlap of consecutive windows in seconds, less than half the window (default {DEFAULT_OVERLAP_S:g}; {UNCALIBRATED})")
    p.add_argument("--long-form-edge-frames", type=int, default=None,
                   help=f"--long-form: encoder frames at either end of an overlap where no cut is made (default: a quarter of the overlap; {UNCALIBRATED})")
    p.add_argument("--long-form-guard-frames", type=int, default=None,
                   help="--long-form: a cut is scored by the lowest blank log-prob either window gives within this many frames of it "
                        f"(default {DEFAULT_GUARD_FRAMES}; {UNCALIBRATED})")


def check_long_form_args(args, tool="speech_recognize"):
    """Refused before anything is loaded: the options of --long-form without it, and --long-form with --streaming, with a search
    that does not read CTC log-probs, with ensembles, alignments and --confidence."""
    opts = (("--long-form-window-s", args.long_form_window_s), ("--long-form-overlap-s", args.long_form_overlap_s),
            ("--long-form-edge-frames", args.long_form_edge_frames), ("--long-form-guard-frames", args.long_form_guard_frames))
    if not args.long_form:
        if getattr(args, "long_form_transducer", False):  # (speech_recognize alone has it: check_long_form_transducer_args)
            return
        for opt, v in opts:
            if v is not None:
                raise ValueError(f"{opt} configures --long-form: give --long-form too")
        return
    if getattr(args, "streaming", False):  # (speech_align has no --streaming)
        raise NotImplementedError("--long-form windows an offline encoder: no --streaming with it (a chunk-streaming model decodes audio "
                                  "of any length with --streaming --stream-endpoint)")
    if tool == "speech_recognize":
        if args.search not in ("ctc", "ctc_beam"):
            raise NotImplementedError("--long-form joins CTC log-probs: it is implemented for --search ctc and --search ctc_beam, not "
                                      f"--search {args.search} (transducer and encoder-decoder models merge token sequences, a different mechanism)" +
                                      _TRANSDUCER_HINT * (args.search in LONG_FORM_TRANSDUCER_SEARCHES))
        if getattr(args, "confidence", False):
            raise NotImplementedError("--long-form is not implemented with --confidence: the posterior kernel holds at most 1023 tokens "
                                      "per hypothesis, fewer than a long recording's transcript")
        if args.print_alignment is not None:
            raise NotImplementedError("--long-form is not implemented with --print-alignment")
        if len(args.path.split(os.pathsep)) > 1:
            raise NotImplementedError("--long-form takes one model")
    for opt, v in opts[:2]:
        if v is not None and not v > 0:
            raise ValueError(f"{opt} must be positive")


def plan_from_args(args, frontend, model) -> LongFormPlan:
    return LongFormPlan.from_seconds(
        samples_per_frame(frontend, model), frontend.sample_rate,
        DEFAULT_WINDOW_S if args.long_form_window_s is None else args.long_form_window_s,
        DEFAULT_OVERLAP_S if args.long_form_overlap_s is None else args.long_form_overlap_s,
        args.long_form_edge_frames, DEFAULT_GUARD_FRAMES if args.long_form_guard_frames is None else args.long_form_guard_frames)


def require_ctc_model(model_name: str):
    """--long-form reads CTC logits: transducer and encoder-decoder models are refused before anything is loaded."""
    from ..speech_align import model_kind

    try:
        kind = model_kind(model_name)
    except NotImplementedError:
        kind = "attention"
    if kind != "ctc":
        raise NotImplementedError(f"--long-form is implemented for encoder-only CTC models, not for the {kind} model '{model_name}': "
                                  "joining windows of a transducer or encoder-decoder model means merging token sequences by time" +
                                  _TRANSDUCER_HINT * (kind == "transducer"))


LONG_FORM_TRANSDUCER_SEARCHES = ("transducer_greedy", "transducer_frame_beam")
_TRANSDUCER_HINT = ("; an offline transducer model is decoded over a whole recording with --long-form-transducer, which joins the "
                    "windows' encoder outputs instead")


def check_long_form_transducer_args(args):
    """--long-form-transducer (speech_recognize): refused before anything is loaded, each with the option's name, together with
    --long-form, --streaming, the searches of CTC and attention models, the host-side Adaptive Expansion Search, --confidence,
    --print-alignment and ensembles.  The four --long-form-* options configure it as they configure --long-form."""
    if not getattr(args, "long_form_transducer", False):
        return
    if args.long_form:
        raise NotImplementedError("--long-form-transducer and --long-form are two paths: --long-form joins the log-probs of an "
                                  "encoder-only CTC model, --long-form-transducer the encoder outputs of a transducer; give one of them")
    if getattr(args, "streaming", False):
        raise NotImplementedError("--long-form-transducer windows an offline encoder: no --streaming with it (a chunk-streaming model "
                                  "decodes audio of any length with --streaming --stream-endpoint)")
    if args.search == "transducer_beam":
        raise NotImplementedError("--long-form-transducer is not implemented for --search transducer_beam: the Adaptive Expansion Search "
                                  "keeps its hypotheses on the host, one by one; use --search transducer_frame_beam or transducer_greedy")
    if args.search not in LONG_FORM_TRANSDUCER_SEARCHES:
        raise NotImplementedError("--long-form-transducer joins the encoder outputs of a transducer model: it is implemented for --search " +
                                  " and --search ".join(LONG_FORM_TRANSDUCER_SEARCHES) + f", not --search {args.search}" +
                                  " (an encoder-only CTC model is decoded with --long-form)" * (args.search in ("ctc", "ctc_beam")))
    if getattr(args, "confidence", False):
        raise NotImplementedError("--long-form-transducer is not implemented with --confidence: the transducer posterior's lattice is "
                                  "frames x tokens, too large for a long recording")
    if args.print_alignment is not None:
        raise NotImplementedError("--long-form-transducer is not implemented with --print-alignment")
    if len(args.path.split(os.pathsep)) > 1:
        raise NotImplementedError("--long-form-transducer takes one model: ensembles (--path a.pt:b.pt) are not implemented")
    for opt, v in (("--long-form-window-s", args.long_form_window_s), ("--long-form-overlap-s", args.long_form_overlap_s)):
        if v is not None and not v > 0:
            raise ValueError(f"{opt} must be positive")


def require_transducer_model(model_name: str):
    """--long-form-transducer reads a transducer's encoder outputs: CTC and encoder-decoder models are refused before anything is
    loaded."""
    from ..speech_align import model_kind

    try:
        kind = model_kind(model_name)
    except NotImplementedError:
        kind = "attention"
    if kind != "transducer":
        raise NotImplementedError(f"--long-form-transducer is implemented for transducer models, not for the {kind} model '{model_name}'" +
                                  " (an encoder-only CTC model is decoded with --long-form)" * (kind == "ctc"))


def log_worst_features(model: LongFormTransducerModel, file):
    cuts = [c for c, _ in model.junctions if c.numel()]
    if not cuts:
        return
    worst = model.worst_score()
    print("| long-form-transducer: {} junctions, lowest cut score {:.4f} (minus the relative squared distance of the two windows' "
          "encoder outputs around the cut, in [-2, 0]; 0 = the windows agree; the scale is uncalibrated)".format(
              sum(c.numel() for c in cuts), worst), file=file)


def log_worst(model: LongFormModel, file):
    cuts = [c for c, _ in model.junctions if c.numel()]
    if not cuts:
        return
    worst = model.worst_score()
    print("| long-form: {} junctions, lowest cut score {:.3f} (log-prob of blank around the cut; near 0 = silence in both windows{})".format(
        sum(c.numel() for c in cuts), worst, ", this low: a cut through speech" if worst < math.log(0.5) else ""), file=file)
