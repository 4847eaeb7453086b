"""Forced-alignment CLI: time every token (or word) of known transcripts with a trained CTC or transducer model and write a
CTM (`utt 1 start dur unit conf`).

Model, dictionary, audio and batching options mean what they mean in `speech_recognize`.  Transcripts (`--text`, `utt_id
text...`) are tokenised as the task tokenises training targets (the dictionary's `--bpe` encoder, else the text is taken as
space-separated tokens).  The model kind decides the aligner: an encoder-only CTC model -> `CTCForcedAligner`, a transducer
-> `TransducerForcedAligner` (tools/forced_aligner.py); attention encoder-decoder models are refused.  Seconds per encoder
frame = the front-end's frame shift x the model's sub-sampling factor.  `--scores` gets one line per utterance (id, encoder
frames, tokens, Viterbi log-prob, log-prob per frame); utterances whose transcript cannot be aligned (too few frames) are
marked `infeasible` there and left out of the CTM.  With `--confidence` the last CTM column is the acoustic model's posterior of
the unit (tools/token_posteriors.py) instead of 1.00.

With `--long-form` every `wav.scp` entry is one recording of any length and its `--text` line the whole transcript: the recording
goes through an offline CTC model as overlapping windows joined on the device (tools/long_form.py) and the
transcript is aligned to all of it by the tiled Viterbi kernel (csrc/align_long.hip); the CTM carries times on
the recording's own axis.  `--segments-dir` then cuts every recording at its silences into utterance-sized segments (`segments`,
`text`, `scores`: Kaldi-style data for training; a segment whose text does not match its audio shows a low mean log-prob per
frame in `scores`).  The segment defaults are uncalibrated.  `--long-form-posteriors` adds the acoustic model's posterior of every
token of the transcript, whatever its length (csrc/prefix_posterior_long.hip): the CTM's last column
carries the unit's probability and `--segments-dir` gets a fourth file, `confidence`, which says which segment holds a word
the model does not hear; `--confidence` itself keeps its 1023-token cap and stays refused with `--long-form`."""
import argparse
import math
import os
import sys
import time
from typing import Dict, List

import torch

from .speech_recognize import (_load_file, audio_seconds, collate, lengths_at, load_member, make_batches, read_scp, read_wav,  # noqa: F401
                               read_waves, resolve_model_config, shard_batches)

DEFAULT_SEGMENT_MAX_S, DEFAULT_SEGMENT_MIN_SILENCE_S = 20.0, 0.3  # option defaults, uncalibrated


def get_parser():
    p = argparse.ArgumentParser("espresso_amd.speech_align", description=__doc__.split("\n")[0])
    p.add_argument("--path", required=True, help="state_dict (or fairseq checkpoint dict with a 'model' entry)")
    p.add_argument("--model", default=None, help="registered model name (default: the checkpoint's cfg.model._name)")
    p.add_argument("--model-config", default=None, help="JSON/YAML file with the recipe's `model:` block (default: the checkpoint's)")
    p.add_argument("--dict", required=True)
    p.add_argument("--wav-scp", required=True)
    p.add_argument("--text", required=True, help="transcripts to align (utt_id text...)")
    p.add_argument("--global-cmvn-stats-path", default=None)
    p.add_argument("--bpe", default=None, choices=["characters_asr", "sentencepiece"],
                   help="tokenise the transcripts with this encoder (as the task does for training targets)")
    p.add_argument("--sentencepiece-model", default=None)
    p.add_argument("--non-lang-syms", default=None, help="non-language symbols (one per line), kept whole by characters_asr")
    p.add_argument("--max-tokens", type=int, default=15000)
    p.add_argument("--batch-size", type=int, default=24)
    p.add_argument("--num-shards", type=int, default=int(os.environ.get("WORLD_SIZE", "1")))
    p.add_argument("--shard-id", type=int, default=int(os.environ.get("RANK", "0")))
    p.add_argument("--device", default=None, help="default: cuda:LOCAL_RANK (cuda:0 outside a launcher)")
    p.add_argument("--output", default="-", help="CTM file (default: stdout)")
    p.add_argument("--unit", default="token", choices=["token", "word"],
                   help="CTM units: tokens, or words (<space> tokens / pieces that begin with the sentencepiece mark separate words)")
    p.add_argument("--scores", default=None, help="per-utterance alignment scores file")
    p.add_argument("--confidence", action="store_true",
                   help="the CTM's last column carries the model's posterior of the unit given the audio and the transcript before it "
                        "(tools/token_posteriors.py; a word: the product over its tokens) instead of 1.00: transcript verification")
    from .tools.long_form import UNCALIBRATED, add_long_form_args

    add_long_form_args(p)  # --long-form: one recording of any length per wav.scp entry, aligned to its whole transcript
    p.add_argument("--long-form-posteriors", action="store_true",
                   help="--long-form: the CTM's last column carries the model's posterior of the unit given the audio and the "
                        "transcript before it, computed for a transcript of any length by the tiled kernel of "
                        "csrc/prefix_posterior_long.hip (a word: the product over its tokens); --segments-dir also gets `confidence` "
                        "(<rec>_<k> mean-token-log-posterior lowest-word-probability words).  How the probabilities relate to word "
                        "correctness has not been measured")
    p.add_argument("--segments-dir", default=None,
                   help="--long-form: cut every aligned recording at its silences into segments and write `segments` (<rec>_<k> <rec> "
                        "start_s end_s), `text` and `scores` (<rec>_<k> frames words mean-log-prob-per-frame [overlong]) there")
    p.add_argument("--segment-max-s", type=float, default=None,
                   help=f"--segments-dir: split segments longer than this many seconds (default {DEFAULT_SEGMENT_MAX_S:g}; {UNCALIBRATED})")
    p.add_argument("--segment-min-silence-s", type=float, default=None,
                   help="--segments-dir: split only at gaps between words of at least this many seconds "
                        f"(default {DEFAULT_SEGMENT_MIN_SILENCE_S:g}; {UNCALIBRATED})")
    return p


def check_args(args):
    """Refused before anything is loaded: the long-form and segment options without --long-form, --long-form --confidence."""
    from .tools.long_form import check_long_form_args

    check_long_form_args(args, tool="speech_align")
    opts = (("--segments-dir", args.segments_dir), ("--segment-max-s", args.segment_max_s),
            ("--segment-min-silence-s", args.segment_min_silence_s))
    if not args.long_form:
        if args.long_form_posteriors:
            raise ValueError("--long-form-posteriors configures --long-form: give --long-form too")
        for opt, v in opts:
            if v is not None:
                raise ValueError(f"{opt} cuts a --long-form alignment into segments: give --long-form too")
        return
    if args.segments_dir is None:
        for opt, v in opts[1:]:
            if v is not None:
                raise ValueError(f"{opt} configures --segments-dir: give --segments-dir too")
    if args.confidence:
        raise NotImplementedError("--long-form is not implemented with --confidence: the posterior kernel holds at most 1023 tokens "
                                  "per transcript, fewer than a long recording's")
    if args.segment_max_s is not None and not args.segment_max_s > 0:
        raise ValueError("--segment-max-s must be positive")
    if args.segment_min_silence_s is not None and args.segment_min_silence_s < 0:
        raise ValueError("--segment-min-silence-s must not be negative")


def model_kind(name: str) -> str:
    """"ctc" (encoder-only CTC) or "transducer" for a registered model name; attention encoder-decoders raise."""
    from . import registry
    from .models.transformer.speech_transformer_encoder_model import SpeechTransformerEncoderModel
    from .models.transformer.speech_transformer_transducer_base import SpeechTransformerTransducerModelBase

    cls = registry.MODEL_REGISTRY.get(name)
    if cls is None:
        raise ValueError(f"unknown model '{name}'")
    if issubclass(cls, SpeechTransformerTransducerModelBase):
        return "transducer"
    if issubclass(cls, SpeechTransformerEncoderModel):
        return "ctc"
    raise NotImplementedError(f"forced alignment is implemented for CTC and transducer models, not for the attention model '{name}': "
                              "its attention alignments of the hypothesis come from `python -m espresso_amd.speech_recognize "
                              "--print-alignment`")


def read_text(path: str) -> Dict[str, str]:
    out = {}
    for line in open(path, encoding="utf-8"):
        parts = line.strip().split(None, 1)
        if parts:
            out[parts[0]] = parts[1] if len(parts) > 1 else ""
    return out


def tokenize(dictionary, text: str, blank: int) -> List[int]:
    """Target ids of a transcript, as the task builds training targets (asr_dataset: encode_line(wordpiece_encode(text)))."""
    ids = dictionary.encode_line(dictionary.wordpiece_encode(text), append_eos=False).tolist()
    if blank in ids:
        raise ValueError(f"transcript {text!r} contains the blank symbol {dictionary[blank]!r}")
    return ids


def write_segments(out_dir, aligned, dictionary, spf, max_frames, min_gap_frames):
    """`segments`, `text` and `scores` of the aligned recordings [(id, result of LongFormCTCAligner.align)] under out_dir: every
    recording cut by `cut_segments` on its word spans; a segment's score is the mean of frame_lp over its frames."""
    from .tools.forced_aligner import cut_segments, utterance_units

    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "segments"), "w", encoding="utf-8") as f_seg, \
            open(os.path.join(out_dir, "text"), "w", encoding="utf-8") as f_text, \
            open(os.path.join(out_dir, "scores"), "w", encoding="utf-8") as f_sc:
        for rec, r in aligned:
            words = utterance_units(r, dictionary, "word")
            for k, (a, b, s, e, overlong) in enumerate(cut_segments(words, r["frames"], max_frames, min_gap_frames)):
                name = "{}_{:04d}".format(rec, k)
                mean = float(r["frame_lp"][s:e].mean()) if e > s else 0.0
                print("{} {} {:.3f} {:.3f}".format(name, rec, s * spf, e * spf), file=f_seg)
                print("{} {}".format(name, " ".join(w for w, _, _ in words[a:b])), file=f_text)
                print("{} {} {} {:.4f}{}".format(name, e - s, b - a, mean, " overlong" if overlong else ""), file=f_sc)


def write_confidence(out_dir, aligned, dictionary, max_frames, min_gap_frames):
    """`confidence` next to the files of `write_segments`, for the same recordings (results with "token_posteriors") and the same
    cuts: one line per segment, `<rec>_<k> mean-token-log-posterior lowest-word-probability words` (`segment_confidence` over
    the segment's words)."""
    from .tools.forced_aligner import cut_segments, utterance_units
    from .tools.token_posteriors import segment_confidence, word_log_factors

    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "confidence"), "w", encoding="utf-8") as f:
        for rec, r in aligned:
            words = utterance_units(r, dictionary, "word")
            rows = word_log_factors([dictionary[int(t)] for t in r["tokens"]], r["token_posteriors"],
                                    space=getattr(dictionary, "space_word", "<space>"))
            assert len(rows) == len(words), (len(rows), len(words))
            for k, (a, b, _, _, _) in enumerate(cut_segments(words, r["frames"], max_frames, min_gap_frames)):
                print("{}_{:04d} {:.4f} {:.4f} {}".format(rec, k, *segment_confidence(rows[a:b])), file=f)


def main(argv=None):
    args = get_parser().parse_args(argv)
    check_args(args)
    from .tools import long_form as LF

    if args.model:  # refuse attention models (--long-form: everything but CTC models) before anything is loaded
        if args.long_form:
            LF.require_ctc_model(args.model)
        model_kind(args.model)
    from .tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from .tools.forced_aligner import (CTCForcedAligner, LongFormCTCAligner, TransducerForcedAligner, ctm_lines, frame_seconds,
                                       utterance_units)
    from .tools.token_posteriors import unit_confidences

    state = _load_file(args.path)
    model_name, model_cfg = resolve_model_config(args.model, args.model_config, state)
    if args.long_form:
        LF.require_ctc_model(model_name)
    kind = model_kind(model_name)
    dev = torch.device(args.device or "cuda:{}".format(int(os.environ.get("LOCAL_RANK", "0"))))
    if dev.type == "cuda":
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(dev)
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(
        dict=args.dict, autoregressive=False, global_cmvn_stats_path=args.global_cmvn_stats_path,
        criterion_name="ctc_loss" if kind == "ctc" else "transducer_loss", non_lang_syms=args.non_lang_syms, bpe=args.bpe,
        sentencepiece_model=args.sentencepiece_model))
    d = task.target_dictionary
    model = load_member(state, model_name, model_cfg, task, dev)
    aligner = None
    if not args.long_form:
        aligner = (CTCForcedAligner if kind == "ctc" else TransducerForcedAligner)([model], d, token_posteriors=args.confidence)
    blank = d.bos() if aligner is None else aligner.blank

    scp = read_scp(args.wav_scp)
    texts = read_text(args.text)
    utt_ids = list(scp.keys())
    missing = [u for u in utt_ids if u not in texts]
    if missing:
        raise ValueError(f"--text has no transcript for {len(missing)} utterance(s), e.g. {missing[0]}")
    targets = {u: tokenize(d, texts[u], blank) for u in utt_ids}
    waves, rates = read_waves([scp[u] for u in utt_ids])
    task.build_frontend(dev)
    fo = task.frontend.sample_rate
    spf = frame_seconds(model, task.frontend.frame_shift / task.frontend.sample_rate)
    results, t_align, audio_s = {}, 0.0, 0.0
    if args.long_form:  # one recording at a time: its windows' stitched log-probs, then the tiled Viterbi search
        aligner = LongFormCTCAligner(task, model, LF.plan_from_args(args, task.frontend, model), d, max_tokens=args.max_tokens,
                                     batch_size=args.batch_size, token_posteriors=args.long_form_posteriors)
        junctions = LF.LongFormModel(model, aligner.long_form)  # (for `log_worst`: the cuts of every recording)
        for i in range(args.shard_id, len(utt_ids), args.num_shards):
            t0 = time.perf_counter()
            r = aligner.align(waves[i], targets[utt_ids[i]], rates[i])  # (one host copy per recording)
            t_align += time.perf_counter() - t0
            audio_s += len(waves[i]) / float(rates[i])
            results[utt_ids[i]] = r
            junctions.junctions.append((torch.from_numpy(r["cuts"]), torch.from_numpy(r["cut_scores"])))
        LF.log_worst(junctions, sys.stderr)
        batches = []
    else:
        batches = shard_batches(make_batches(utt_ids, lengths_at(waves, rates, fo), args.max_tokens, args.batch_size), args.num_shards,
                                args.shard_id)
    for ids in batches:
        sample = collate(ids, utt_ids, waves, dev, rates, fo)
        t0 = time.perf_counter()
        s = task.prepare_sample(sample, train=False)
        out = aligner.align(s, [targets[u] for u in sample["utt_ids"]])  # (one host copy per batch)
        t_align += time.perf_counter() - t0
        audio_s += audio_seconds(sample, fo)
        results.update(zip(sample["utt_ids"], out))

    order = [u for u in utt_ids if u in results]  # wav.scp order
    ctm = sys.stdout if args.output == "-" else open(args.output, "w", encoding="utf-8")
    try:
        for u in order:
            r = results[u]
            if r["feasible"]:
                conf = None
                if args.confidence or args.long_form_posteriors:
                    conf = unit_confidences([d[int(t)] for t in r["tokens"]], r["token_posteriors"], args.unit,
                                            space=getattr(d, "space_word", "<space>"))
                for line in ctm_lines(u, utterance_units(r, d, args.unit), spf, confidences=conf):
                    print(line, file=ctm)
    finally:
        if ctm is not sys.stdout:
            ctm.close()
    if args.scores:
        with open(args.scores, "w", encoding="utf-8") as f:
            for u in order:
                r = results[u]
                per = r["score"] / r["frames"] if r["feasible"] and r["frames"] > 0 else (0.0 if r["feasible"] else -math.inf)
                print("{} {} {} {:.4f} {:.4f}{}".format(u, r["frames"], len(r["tokens"]), r["score"], per,
                                                       "" if r["feasible"] else " infeasible"), file=f)
    if args.segments_dir:
        max_s = DEFAULT_SEGMENT_MAX_S if args.segment_max_s is None else args.segment_max_s
        min_sil = DEFAULT_SEGMENT_MIN_SILENCE_S if args.segment_min_silence_s is None else args.segment_min_silence_s
        aligned = [(u, results[u]) for u in order if results[u]["feasible"]]
        max_frames, min_gap_frames = max(1, int(round(max_s / spf))), int(round(min_sil / spf))
        write_segments(args.segments_dir, aligned, d, spf, max_frames, min_gap_frames)
        if args.long_form_posteriors:
            write_confidence(args.segments_dir, aligned, d, max_frames, min_gap_frames)
    n_bad = sum(not results[u]["feasible"] for u in order)
    print("| aligned {} utterances ({} infeasible) in {:.1f}s, RTF {:.4f}".format(len(order), n_bad, t_align,
                                                                               t_align / max(audio_s, 1e-9)), file=sys.stderr)
    return results


if __name__ == "__main__":
    main()
