"""Batched recognition CLI — the decoding loop and output format of espresso/speech_recognize.py:60-360 on the HIP path:
for every batch run the chosen search (beam search with optional LM / look-ahead word-LM / multi-level LM fusion, CTC greedy,
CTC prefix beam search with optional LSTM-LM or lexicon + n-gram LM fusion (both also streamed), transducer greedy / beam /
frame-synchronous beam, the latter also streamed), print `T-<utt>` (reference) and `H-<utt>`
(hypothesis, score in base 2) lines, accumulate WER / CER with `tools.wer.Scorer`, and close with the "Recognized N utterances
..." summary.

Checkpoint management is fairseq's and stays out of this framework (SURVEY §2 out of scope): the model is built from a
config mapping (`--model-config`, the `model:` block of the recipe YAML as JSON/YAML) and a `state_dict` file (`--path`:
either a plain state_dict or a fairseq checkpoint dict whose `"model"` entry is the state_dict — reference checkpoints load
because the parameter names are identical).  Audio comes from a Kaldi-style `wav.scp` (`utt_id path.wav`, 16-bit PCM read
with the stdlib) and optional `text` (`utt_id tokens...`) files; the front-end (fbank + CMVN) runs on the GPU.

`--long-form` (--search ctc / ctc_beam, an offline encoder-only CTC model) decodes every recording, of any length, as one
utterance: overlapping windows are the batch of the offline forward, their logits are joined on the device into one log-prob
matrix on the recording's own frame axis, and the search reads that (tools/long_form.py; the reference
has no such path).  `--long-form-transducer` (--search transducer_greedy / transducer_frame_beam, an offline transducer model)
does the same for the project's other model family: the windows' encoder outputs are joined on the device where the two
windows agree, and the frame-synchronous search runs over the recording's frames as over one utterance's (DESIGN.md section
3.12)."""
import argparse
import os
import json
import math
import sys
import time
from typing import Dict, Iterable, List, Optional

import numpy as np
import torch


from .data.audio_utils import get_waveform, read_wav  # noqa: E402,F401
from .data.resample import resampled_length  # noqa: E402


def read_waves(paths: List[str]):
    """(waveforms, their sample rates): the rate travels with the samples, and the front-end converts what is not its own."""
    pairs = [get_waveform(p) for p in paths]
    return [w for w, _ in pairs], [int(r) for _, r in pairs]


def lengths_at(waves, rates, fo: int) -> List[int]:
    """Sample counts after conversion to `fo`: what batches are budgeted with and frame counts are taken from."""
    if rates is None:
        return [len(w) for w in waves]
    return [resampled_length(len(w), r, fo) for w, r in zip(waves, rates)]


def audio_seconds(sample, fo: int = 16000) -> float:
    """Duration of a collated batch, every utterance at its own rate."""
    rates = sample.get("wav_rates")
    if rates is None:
        return sum(sample["num_samples"]) / float(fo)
    return sum(n / float(r) for n, r in zip(sample["num_samples"], rates))


def read_scp(path: str) -> Dict[str, str]:
    out = {}
    for line in open(path, encoding="utf-8"):
        line = line.strip()
        if line:
            k, v = line.split(None, 1)
            out[k] = v
    return out


def make_batches(utt_ids: List[str], n_samples: List[int], max_tokens: int, max_sentences: int) -> List[List[int]]:
    """Length-sorted batches under the frame budget (frames = samples / 160), longest first inside a batch."""
    order = sorted(range(len(utt_ids)), key=lambda i: -n_samples[i])
    batches, cur, mx = [], [], 0
    for i in order:
        fr = n_samples[i] // 160 + 1
        if cur and (max(mx, fr) * (len(cur) + 1) > max_tokens or len(cur) + 1 > max_sentences):
            batches.append(cur)
            cur, mx = [], 0
        cur.append(i)
        mx = max(mx, fr)
    if cur:
        batches.append(cur)
    return batches


def shard_batches(batches: List[List[int]], num_shards: int, shard_id: int) -> List[List[int]]:
    """The batches of one decoding replica: espresso/speech_recognize.py:188-189 hands `num_shards = distributed_world_size`,
    `shard_id = distributed_rank` to the batch iterator, whose ShardedIterator (fairseq/data/iterators.py:534-571) deals the
    length-sorted batch list round-robin: replica i decodes batches i, i + n, i + 2n, ... (no collective: SURVEY 8(e) "replicas
    only"); every replica scores its own shard."""
    if not (0 <= shard_id < num_shards):
        raise ValueError(f"--shard-id {shard_id} outside [0, --num-shards {num_shards})")
    return batches[shard_id::num_shards]


def recognize(task, model, generator, batches: Iterable[dict], dictionary, refs: Optional[Dict[str, str]] = None, out=sys.stdout,
              nbest: int = 1, quiet: bool = False, bpe_symbol=None, scorer=None, summary_out=None, attn_plot_dir=None,
              ctm_hyps=None):
    """The loop of espresso/speech_recognize.py:226-330.  `batches` yield dicts with `utt_ids`, `wav`, `wav_offsets`,
    `num_samples` (device tensors / lists as produced by `collate`).  `summary_out`: a second stream for the closing summary
    lines (stdout while `out` is decode.log); `attn_plot_dir`: save the best hypothesis' alignment of every utterance there
    (plot_attention) when the generator returns one.  `ctm_hyps`: a dict that gets utterance -> (its best hypothesis, the symbols stripped from the text) (--ctm).
    Returns (scorer, stats)."""
    from .tools.token_posteriors import confidence_line
    from .tools.utils import plot_attention
    from .tools.wer import Scorer

    if scorer is None:
        scorer = Scorer(dictionary, wer_output_filter=None)
    num_sent, num_tok, t_gen, audio_s = 0, 0, 0.0, 0.0
    for sample in batches:
        t0 = time.perf_counter()
        s = task.prepare_sample(sample, train=False)
        hypos = generator.generate([model], s)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        t_gen += time.perf_counter() - t0
        audio_s += audio_seconds(sample)
        enc_lens = None
        if attn_plot_dir is not None:  # valid encoder frames of every utterance (the plot drops the padded rows)
            enc_lens = model.encoder.output_lengths(s["net_input"]["src_lengths"]).tolist()
        for i, utt in enumerate(sample["utt_ids"]):
            if refs is not None and utt in refs and not quiet:
                print("T-{}\t{}".format(utt, refs[utt]), file=out)
            for j, hypo in enumerate(hypos[i][:nbest]):
                toks = hypo["tokens"].int().cpu()
                strip = getattr(generator, "symbols_to_strip_from_output", None) or {dictionary.eos(), dictionary.pad()}
                hypo_str = dictionary.string(torch.tensor([t for t in toks.tolist() if t not in strip]), bpe_symbol=bpe_symbol)
                if not quiet:
                    print("H-{}\t{}\t{}".format(utt, hypo_str, float(hypo["score"]) / math.log(2)), file=out)
                    if hypo.get("token_posteriors") is not None:  # --confidence: the labels the model emitted, then the end
                        print(confidence_line(utt, [f for t, f in zip(toks.tolist(), hypo["token_posteriors"].tolist())
                                                    if t not in strip], float(hypo["end_posterior"])), file=out)
                if j == 0:
                    if enc_lens is not None and hypo.get("attention") is not None:
                        os.makedirs(attn_plot_dir, exist_ok=True)
                        plot_attention(hypo["attention"][: int(enc_lens[i])].float().cpu(), hypo_str, utt, attn_plot_dir)
                    scorer.add_prediction(utt, hypo_str)
                    if refs is not None and utt in refs:
                        scorer.add_evaluation(utt, refs[utt], hypo_str)
                    num_tok += len(toks)
                    if ctm_hyps is not None:
                        ctm_hyps[utt] = (hypo, strip)
        num_sent += len(sample["utt_ids"])
    lines = ["NOTE: hypothesis and token scores are output in base 2",
             "Recognized {:,} utterances ({} tokens) in {:.1f}s ({:.2f} sentences/s, {:.2f} tokens/s), RTF {:.4f}".format(
                 num_sent, num_tok, t_gen, num_sent / max(t_gen, 1e-9), num_tok / max(t_gen, 1e-9), t_gen / max(audio_s, 1e-9))]
    if refs:
        lines += scorer.summary_lines()
    for f in [out] + ([summary_out] if summary_out is not None else []):
        for line in lines:
            print(line, file=f)
    return scorer, {"sentences": num_sent, "tokens": num_tok, "seconds": t_gen, "rtf": t_gen / max(audio_s, 1e-9)}


def write_results(results_path: str, scorer, has_target: bool):
    """The result files of espresso/speech_recognize.py:338-389 next to decode.log: decoded_char_results.txt and
    decoded_results.txt always; with references also `wer`, `cer` (one line each) and aligned_results.txt."""
    os.makedirs(results_path, exist_ok=True)

    def write(name, text):
        with open(os.path.join(results_path, name), "w", encoding="utf-8") as f:
            f.write(text)

    write("decoded_char_results.txt", scorer.print_char_results())
    write("decoded_results.txt", scorer.print_results())
    if has_target:
        wer_line, cer_line = scorer.summary_lines()
        write("wer", wer_line + "\n")
        write("cer", cer_line + "\n")
        write("aligned_results.txt", scorer.print_aligned_results())


def collate(ids: List[int], utt_ids: List[str], waves: List[np.ndarray], device, rates: Optional[List[int]] = None,
            sample_rate: int = 16000):
    """rates: the sample rate of every entry of `waves` (None: all at `sample_rate`).  The batch carries `wav_rates` only when one
    of its utterances is at another rate than `sample_rate`; `num_samples` stay counts at the utterance's own rate."""
    lens = [len(waves[i]) for i in ids]
    offs = np.zeros(len(ids) + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    sample = {"utt_ids": [utt_ids[i] for i in ids], "wav": torch.from_numpy(np.concatenate([waves[i] for i in ids])).to(device),
              "wav_offsets": torch.from_numpy(offs).to(device), "num_samples": lens, "net_input": {}}
    if rates is not None and any(int(rates[i]) != sample_rate for i in ids):
        sample["wav_rates"] = [int(rates[i]) for i in ids]
    return sample


def build_generator(args, model, dictionary, lm=None, ngram=None, context_graph=None):
    """ngram: (NGramLanguageModel, LexiconTrie) for --search ctc_beam --ngram-lm; context_graph: the ContextGraph of --hotwords
    (--search ctc_beam) or --transducer-hotwords (--search transducer_frame_beam).
    (--search transducer_stream_beam and --search ctc_stream_beam have no generator: recognize_streaming builds their decoders
    from stream_beam_options / ctc_stream_beam_options.)"""
    from .sequence_generator import SequenceGenerator
    from .tools.ctc_decoder import CTCDecoder
    from .tools.ctc_lexicon_beam_search import CTCLexiconBeamSearchDecoder
    from .tools.ctc_prefix_beam_search import CTCPrefixBeamSearchDecoder
    from .tools.transducer_beam_search_decoder import TransducerBeamSearchDecoder
    from .tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder
    from .tools.transducer_greedy_decoder import TransducerGreedyDecoder

    post = bool(getattr(args, "confidence", False))
    if args.search == "ctc":
        return CTCDecoder([model], dictionary, token_posteriors=post)
    if args.search == "ctc_beam" and ngram is not None:
        return CTCLexiconBeamSearchDecoder([model], dictionary, *ngram, beam_size=args.beam, nbest=args.nbest,
                                           beam_size_token=args.ctc_beam_size_token, lm_weight=args.lm_weight,
                                           word_score=args.word_score, insertion_bonus=args.ctc_insertion_bonus)
    if args.search == "ctc_beam":
        return CTCPrefixBeamSearchDecoder([model], dictionary, beam_size=args.beam, nbest=args.nbest,
                                          beam_size_token=args.ctc_beam_size_token, lm_model=lm, lm_weight=args.lm_weight,
                                          insertion_bonus=args.ctc_insertion_bonus, context_graph=context_graph,
                                          token_times=bool(getattr(args, "ctm", None)), token_posteriors=post)
    if args.search == "transducer_greedy":
        return TransducerGreedyDecoder([model], dictionary, max_num_expansions_per_step=args.max_num_expansions_per_step,
                                       lm_model=lm, lm_weight=args.lm_weight, token_posteriors=post)
    if args.search == "transducer_beam":
        return TransducerBeamSearchDecoder([model], dictionary, beam_size=args.beam,
                                           max_num_expansions_per_step=args.max_num_expansions_per_step, expansion_beta=args.expansion_beta,
                                           expansion_gamma=args.expansion_gamma, prefix_alpha=args.prefix_alpha, lm_model=lm,
                                           lm_weight=args.lm_weight, token_posteriors=post)
    if args.search == "transducer_frame_beam":
        return TransducerFrameBeamDecoder([model], dictionary, beam_size=args.beam, nbest=args.nbest,
                                          beam_size_token=args.transducer_beam_size_token, temperature=args.temperature,
                                          normalize_scores=not args.unnormalized, lm_model=lm, lm_weight=args.lm_weight,
                                          context_graph=context_graph, token_times=bool(getattr(args, "ctm", None)),
                                          token_posteriors=post)
    return SequenceGenerator(model if isinstance(model, (list, tuple)) else [model], dictionary, beam_size=args.beam, max_len_a=args.max_len_a, max_len_b=args.max_len_b,
                             min_len=args.min_len, normalize_scores=not args.unnormalized, len_penalty=args.lenpen,
                             unk_penalty=args.unkpen, temperature=args.temperature, lm_model=lm, lm_weight=args.lm_weight,
                             eos_factor=args.eos_factor, print_alignment=getattr(args, "print_alignment", None) is not None)


def stream_beam_options(args, lm=None, context_graph=None):
    """The options of StreamingTransducerFrameBeamDecoder (after model, dictionary, max_streams, max_frames) from the command
    line of --search transducer_stream_beam; context_graph: the ContextGraph of --transducer-hotwords."""
    opts = dict(beam_size=args.beam, nbest=args.nbest, beam_size_token=args.transducer_beam_size_token, temperature=args.temperature,
                normalize_scores=not args.unnormalized, lm_model=lm, lm_weight=args.lm_weight)
    if context_graph is not None:
        opts["context_graph"] = context_graph
    if getattr(args, "ctm", None):
        opts["token_times"] = True
    return opts


def ctc_stream_beam_options(args, lm=None, context_graph=None):
    """The options of StreamingCTCPrefixBeamDecoder (after dictionary, max_streams, max_frames) from the command line of
    --search ctc_stream_beam; context_graph: the ContextGraph of --hotwords."""
    opts = dict(beam_size=args.beam, nbest=args.nbest, beam_size_token=args.ctc_beam_size_token, lm_model=lm, lm_weight=args.lm_weight,
                insertion_bonus=args.ctc_insertion_bonus, context_graph=context_graph)
    if getattr(args, "ctm", None):
        opts["token_times"] = True
    return opts


def endpoint_options(args, seconds_per_frame):
    """The `endpoint` / `seconds_per_frame` arguments of recognize_streaming from the command line of --stream-endpoint: the
    three thresholds in encoder frames (a positive number of seconds is at least one frame; <= 0 stays switched off)."""
    from .tools.beam_common import EndpointRules

    def frames(seconds):
        return max(1, int(round(seconds / seconds_per_frame))) if seconds > 0 else 0

    return dict(endpoint=EndpointRules(frames(args.endpoint_silence_s), frames(args.endpoint_empty_s), frames(args.endpoint_max_segment_s)),
                seconds_per_frame=seconds_per_frame)


def get_parser():
    p = argparse.ArgumentParser("espresso_amd.speech_recognize", description=__doc__.split("\n")[0])
    p.add_argument("--path", required=True, help="state_dict (or fairseq checkpoint dict with a 'model' entry)")
    p.add_argument("--model", default=None, help="registered model name (default: the checkpoint's cfg.model._name, else speech_transformer_base)")
    p.add_argument("--model-config", default=None,
                   help="JSON/YAML file with the recipe's `model:` block (default: the `cfg.model` stored in the checkpoint, as the "
                        "reference rebuilds the model in checkpoint_utils.load_model_ensemble)")
    p.add_argument("--dict", required=True)
    p.add_argument("--wav-scp", required=True)
    p.add_argument("--text", default=None, help="reference transcripts (utt_id tokens...)")
    p.add_argument("--global-cmvn-stats-path", default=None)
    p.add_argument("--search", default="beam", choices=["beam", "ctc", "ctc_beam", "transducer_greedy", "transducer_beam", "transducer_frame_beam", "transducer_stream_beam", "ctc_stream_beam"],
                   help="transducer_stream_beam is the frame-synchronous transducer beam search under --streaming (a search name of "
                        "its own: --search transducer_frame_beam is the offline search and refuses --streaming); ctc_stream_beam "
                        "likewise is the CTC prefix beam search of --search ctc_beam (alone, with --lm-path, with --hotwords) under "
                        "--streaming")
    p.add_argument("--beam", type=int, default=10)
    p.add_argument("--nbest", type=int, default=1)
    p.add_argument("--max-len-a", type=float, default=0.08)
    p.add_argument("--max-len-b", type=int, default=0)
    p.add_argument("--min-len", type=int, default=1)
    p.add_argument("--unnormalized", action="store_true")
    p.add_argument("--lenpen", type=float, default=1.0)
    p.add_argument("--unkpen", type=float, default=0.0)
    p.add_argument("--temperature", type=float, default=1.0)
    p.add_argument("--eos-factor", type=float, default=None)
    p.add_argument("--lm-path", default=None,
                   help="LSTM LM state_dict; `sub.pt:word.pt` with --word-dict = multi-level fusion (sub-word LM, then word LM)")
    p.add_argument("--lm-arch", default="lstm_lm_librispeech")
    p.add_argument("--word-lm-arch", default="lstm_lm_wsj", help="architecture of the word LM of a multi-level `--lm-path a:b`")
    p.add_argument("--lm-weight", type=float, default=0.0)
    p.add_argument("--word-dict", default=None, help="enables look-ahead word-LM fusion (the LM at --lm-path is a word LM)")
    p.add_argument("--oov-penalty", type=float, default=1e-4)
    p.add_argument("--subwordlm-weight", type=float, default=0.8, help="sub-word LM weight of multi-level fusion")
    p.add_argument("--disable-open-vocab", action="store_true",
                   help="look-ahead / multi-level fusion: no probability mass for words outside the --word-dict lexicon")
    p.add_argument("--ctc-beam-size-token", type=int, default=None,
                   help="ctc_beam / ctc_stream_beam: candidate tokens per frame (default: min(--beam, vocabulary size - 1), at most 64)")
    p.add_argument("--ctc-insertion-bonus", type=float, default=0.0, help="ctc_beam / ctc_stream_beam: score added per emitted token")
    p.add_argument("--transducer-beam-size-token", type=int, default=None,
                   help="transducer_frame_beam / transducer_stream_beam: extensions per hypothesis and frame (default: min(--beam, vocabulary size - 1), at "
                        "most 64)")
    p.add_argument("--ngram-lm", default=None,
                   help="ctc_beam: word n-gram LM (plain-text ARPA) fused with --lm-weight under a closed-vocabulary lexicon")
    p.add_argument("--lexicon", default=None,
                   help="ctc_beam --ngram-lm: `word tok1 tok2 ...` lines (default with a <space> dictionary: the ARPA words spelled "
                        "by characters)")
    p.add_argument("--token-ngram-lm", default=None,
                   help="ctc_beam (without --ngram-lm) / ctc_stream_beam / transducer_frame_beam / transducer_stream_beam: ARPA n-gram LM "
                        "over the model's own sub-word units (the dictionary's symbols are its words; plain text, order <= 6), fused "
                        "with --lm-weight in place of an LSTM LM: no --lm-path or --word-dict with it")
    p.add_argument("--word-score", type=float, default=-1.0, help="ctc_beam --ngram-lm: score added per completed word")
    p.add_argument("--hotwords", default=None,
                   help="ctc_beam (without --ngram-lm) / ctc_stream_beam: phrases to bias the search towards, one per line, optionally `<TAB>boost`; "
                        "`#` comments.  A hypothesis gains the boost for every token of a phrase it completes (natural log, not "
                        "scaled by --lm-weight; H- scores include it).  The candidate tokens of a frame stay the "
                        "--ctc-beam-size-token best by acoustic score: biasing re-ranks hypotheses, it does not bring back a token "
                        "outside them")
    p.add_argument("--transducer-hotwords", default=None, metavar="FILE",
                   help="transducer_frame_beam / transducer_stream_beam: the phrase file of --hotwords (same format, --hotword-score, "
                        "--bpe and --sentencepiece-model) for the frame-synchronous transducer beam search, offline and streamed, "
                        "with or without --lm-path.  The extensions of a hypothesis stay the --transducer-beam-size-token best by "
                        "acoustic (and LM-fused) score: biasing re-ranks hypotheses, it does not bring back a token outside them, so "
                        "with it the default of that option no longer amounts to a global top --beam.  --stream-partials then shows "
                        "the hypothesis that leads with its pending boosts counted")
    p.add_argument("--hotword-score", type=float, default=None,
                   help="--hotwords / --transducer-hotwords: boost per token of the phrases that give none of their own (default 1.5)")
    p.add_argument("--bpe", default=None, choices=["characters_asr", "sentencepiece"], help="--hotwords / --transducer-hotwords: sub-word tokeniser of the phrases (as speech_align --bpe)")
    p.add_argument("--sentencepiece-model", default=None, help="--bpe sentencepiece: the model file")
    p.add_argument("--max-num-expansions-per-step", type=int, default=2)
    p.add_argument("--expansion-beta", type=int, default=0)
    p.add_argument("--expansion-gamma", type=float, default=None)
    p.add_argument("--prefix-alpha", type=int, default=None)
    p.add_argument("--max-tokens", type=int, default=15000)
    p.add_argument("--batch-size", type=int, default=24)
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--num-shards", type=int, default=int(os.environ.get("WORLD_SIZE", "1")),
                   help="decode replicas (default: WORLD_SIZE); each takes every num-shards-th batch")
    p.add_argument("--shard-id", type=int, default=int(os.environ.get("RANK", "0")), help="this replica (default: RANK)")
    p.add_argument("--device", default=None, help="default: cuda:LOCAL_RANK (cuda:0 outside a launcher)")
    p.add_argument("--results-path", default=None,
                   help="directory for decode.log, decoded_results.txt, decoded_char_results.txt and, with --text, wer, cer and "
                        "aligned_results.txt")
    p.add_argument("--print-alignment", nargs="?", const="hard", default=None, choices=["hard", "soft"],
                   help="collect the attention alignments; --search beam saves RESULTS_PATH/attn_plots/<utt>.pdf of the best "
                        "hypothesis (needs --results-path and matplotlib)")
    p.add_argument("--ctm", default=None, metavar="FILE",
                   help="ctc_beam (without --ngram-lm) / ctc_stream_beam / transducer_frame_beam / transducer_stream_beam: also write the "
                        "best hypothesis of every utterance as CTM lines (`utt 1 start dur unit 1.00`, `-` = stdout): each token at "
                        "the encoder frame where it starts on the hypothesis' best alignment path, one frame long; the search then "
                        "follows that path on the device")
    p.add_argument("--ctm-unit", default="token", choices=["token", "word"],
                   help="--ctm units: tokens, or words (<space> tokens / pieces that begin with the sentencepiece mark separate "
                        "words; a word runs from its first token's start to its last token's start + one frame)")
    p.add_argument("--confidence", action="store_true",
                   help="ctc / ctc_beam (without --ngram-lm) / transducer_greedy / transducer_beam / transducer_frame_beam: after every "
                        "`H-<utt>` line print `C-<utt>`, the acoustic model's posterior of every emitted token given the audio and "
                        "the tokens before it, then that of ending there (no LM, bonus or bias in them); --ctm then carries the unit's "
                        "probability (a word: the product over its tokens) instead of 1.00")
    p.add_argument("--streaming", action="store_true",
                   help="chunk-by-chunk recognition of a chunk-streaming transformer or causal-conformer encoder (--search ctc, transducer_greedy, "
                        "transducer_stream_beam, ctc_stream_beam, or ctc_beam with --ngram-lm): audio is fed in pieces of --stream-chunk-ms with --streams utterances in flight")
    p.add_argument("--stream-chunk-ms", type=int, default=None, help="--streaming: audio per piece (default 400)")
    p.add_argument("--streams", type=int, default=None, help="--streaming: concurrent utterances (default 16)")
    p.add_argument("--stream-partials", action="store_true",
                   help="--streaming --search ctc_beam --ngram-lm, --search ctc_stream_beam or --search transducer_stream_beam: after every piece print `P-<utt>`, the seconds consumed, the stable "
                        "text and the rest of the currently best hypothesis, whenever the text changed")
    p.add_argument("--stream-endpoint", action="store_true",
                   help="--streaming --search ctc_stream_beam or --search transducer_stream_beam (1-best): decode audio of any length as "
                        "consecutive segments.  After every piece the device decides whether the utterance in a stream has ended "
                        "(--endpoint-silence-s, --endpoint-empty-s, --endpoint-max-segment-s); the segment is then finalised and printed "
                        "as `S-<utt>`, its start and end in seconds, the rule and its text, the stream's search state starts afresh, and "
                        "`H-<utt>` is the segments' text joined.  The state of a stream is sized for one segment, not for the utterance")
    p.add_argument("--endpoint-silence-s", type=float, default=0.8,
                   help="--stream-endpoint: end a segment with text once this long has passed since its last token began (<= 0: never)")
    p.add_argument("--endpoint-empty-s", type=float, default=5.0,
                   help="--stream-endpoint: end a segment without text after this long (<= 0: never)")
    p.add_argument("--endpoint-max-segment-s", type=float, default=20.0,
                   help="--stream-endpoint: end every segment after this long; it sizes the per-stream search state (must be positive)")
    p.add_argument("--wer-output-filter", default=None, help="sed-style word filter applied before WER scoring")
    p.add_argument("--non-lang-syms", default=None, help="non-language symbols (one per line), ignored by WER / CER scoring")
    from .tools.long_form import add_long_form_args

    add_long_form_args(p)  # --long-form: recordings of any length through an offline CTC model (--search ctc / ctc_beam)
    p.add_argument("--long-form-transducer", action="store_true",
                   help="transducer_greedy / transducer_frame_beam: decode every recording as overlapping windows of an offline "
                        "transducer model, their encoder outputs joined on the device into one matrix on the recording's own frame "
                        "axis, which the search reads as one utterance's (any length; one recording per sample; --lm-path, "
                        "--token-ngram-lm, --transducer-hotwords, --nbest and --ctm work as they do on an utterance, times are the "
                        "recording's).  A cut between two windows goes where their encoder outputs agree best; --long-form-window-s, "
                        "--long-form-overlap-s, --long-form-edge-frames and --long-form-guard-frames configure it as they configure "
                        "--long-form.  The agreement rule and these defaults are uncalibrated: no WER on real long recordings has been measured")
    p.add_argument("--long-form-posteriors", action="store_true",
                   help="--long-form (ctc / ctc_beam without --ngram-lm): after every `H-<utt>` line print `C-<utt>` as --confidence "
                        "does, computed after the search for hypotheses of any length by the tiled kernel of "
                        "csrc/prefix_posterior_long.hip on the log-probs the search read; --ctm then carries the unit's probability.  "
                        "How the probabilities relate to word correctness has not been measured")
    return p


def check_long_form_posteriors_args(args):
    """--long-form-posteriors belongs to --long-form and, like --confidence, scores the model's sub-word tokens: refused, before
    anything is loaded, without --long-form and with the lexicon + n-gram search."""
    if not getattr(args, "long_form_posteriors", False):
        return
    if not args.long_form:
        raise ValueError("--long-form-posteriors configures --long-form: give --long-form too")
    if args.ngram_lm:
        raise NotImplementedError("--long-form-posteriors scores the model's sub-word tokens: no --ngram-lm with it (the units of the "
                                  "lexicon search are words)")


def check_ngram_args(args):
    """--ngram-lm is the lexicon + n-gram fusion of --search ctc_beam alone: refused, before anything is loaded, with other
    searches, with an LSTM LM (--lm-path / --word-dict) and with ensembles."""
    if not args.ngram_lm:
        if args.lexicon:
            raise ValueError("--lexicon constrains the n-gram fusion of --search ctc_beam: give --ngram-lm too")
        return
    if args.search != "ctc_beam":
        raise NotImplementedError("--ngram-lm (lexicon + n-gram LM fusion) is implemented for --search ctc_beam only")
    if args.lm_path or args.word_dict:
        raise NotImplementedError("--ngram-lm fuses the n-gram LM alone: no --lm-path or --word-dict with it")
    if len(args.path.split(os.pathsep)) > 1:
        raise NotImplementedError("ensembles are implemented for the attention decoder's beam search (--search beam)")


TOKEN_NGRAM_SEARCHES = ("ctc_beam", "ctc_stream_beam", "transducer_frame_beam", "transducer_stream_beam")
CTM_SEARCHES = TOKEN_NGRAM_SEARCHES  # the four device-resident token-level beam searches


def check_ctm_args(args):
    """--ctm writes the time stamps the four token-level beam searches follow on the device: refused, before anything is
    loaded, for every other search (the attention decoder, the greedy decoders, the Adaptive Expansion Search, the lexicon +
    n-gram search)."""
    if not args.ctm:
        return
    if args.search not in CTM_SEARCHES or (args.search == "ctc_beam" and args.ngram_lm):
        raise NotImplementedError("--ctm (time stamps of the recognised tokens / words) is implemented for --search " +
                                  ", ".join(CTM_SEARCHES) + " only (ctc_beam without --ngram-lm), not --search " + args.search +
                                  " --ngram-lm" * bool(args.ngram_lm) + "; speech_align writes a CTM for a known transcript")


CONFIDENCE_SEARCHES = ("ctc", "ctc_beam", "transducer_greedy", "transducer_beam", "transducer_frame_beam")


def check_confidence_args(args):
    """--confidence prints the acoustic model's per-token posteriors (tools/token_posteriors.py) of the offline CTC and
    transducer searches: refused, before anything is loaded, for the attention decoder (its hypotheses carry positional
    scores), the lexicon + n-gram search (its units are words), every --streaming search (the posterior needs the whole
    utterance's lattice), ensembles, and a transducer that predicts <eos>."""
    if not getattr(args, "confidence", False):
        return
    if args.streaming or args.search in ("transducer_stream_beam", "ctc_stream_beam"):
        raise NotImplementedError("--confidence is not streamed: the posterior of a token needs the whole utterance's lattice (no "
                                  "--streaming, --search ctc_stream_beam or --search transducer_stream_beam with it)")
    if args.search not in CONFIDENCE_SEARCHES:
        raise NotImplementedError("--confidence (per-token posteriors) is implemented for --search " + ", ".join(CONFIDENCE_SEARCHES) +
                                  f" only, not --search {args.search}")
    if args.ngram_lm:
        raise NotImplementedError("--confidence scores the model's sub-word tokens: no --ngram-lm with it (the units of the lexicon "
                                  "search are words)")
    if len(args.path.split(os.pathsep)) > 1:
        raise NotImplementedError("--confidence is the posterior of one model: ensembles (--path a.pt:b.pt) are not implemented")
    if getattr(args, "model_predicts_eos", False):
        raise NotImplementedError("--confidence is not implemented for a transducer that predicts <eos> (model_predicts_eos)")


def hypothesis_ctm_lines(utt, hypo, dictionary, strip, unit, seconds_per_frame):
    """The CTM lines of one hypothesis with "times": every kept token spans [start, start + 1) encoder frames; words as
    tools/forced_aligner.word_spans groups them.  A hypothesis with "token_posteriors" (--confidence) carries the unit's
    probability in the last column instead of 1.00."""
    from .tools.forced_aligner import ctm_lines, utterance_units
    from .tools.token_posteriors import unit_confidences

    keep = [k for k, t in enumerate(hypo["tokens"].tolist()) if int(t) not in strip]
    toks, times = hypo["tokens"].tolist(), hypo["times"].tolist()
    pairs = [(int(toks[k]), int(times[k])) for k in keep]
    result = {"tokens": [t for t, _ in pairs], "start": [f for _, f in pairs], "end": [f + 1 for _, f in pairs]}
    conf = None
    if hypo.get("token_posteriors") is not None:
        post = hypo["token_posteriors"].tolist()
        conf = unit_confidences([dictionary[t] for t, _ in pairs], [post[k] for k in keep], unit,
                                space=getattr(dictionary, "space_word", "<space>"))
    return ctm_lines(utt, utterance_units(result, dictionary, unit), seconds_per_frame, confidences=conf)


def write_ctm(path, utt_ids, ctm_hyps, dictionary, unit, seconds_per_frame):
    """--ctm: the lines of every recognised utterance, in the order of utt_ids."""
    out = sys.stdout if path == "-" else open(path, "w", encoding="utf-8")
    try:
        for utt in utt_ids:
            if utt in ctm_hyps:
                hypo, strip = ctm_hyps[utt]
                for line in hypothesis_ctm_lines(utt, hypo, dictionary, strip, unit, seconds_per_frame):
                    print(line, file=out)
    finally:
        if out is not sys.stdout:
            out.close()


def check_token_ngram_args(args):
    """--token-ngram-lm fuses an n-gram LM over the model's sub-word units into the four token-level beam searches, where they
    otherwise fuse an LSTM LM: refused, before anything is loaded, with every other search, with the lexicon + n-gram search
    (--ngram-lm), with an LSTM LM (--lm-path / --word-dict), with ensembles and with a weight that is not positive."""
    if not args.token_ngram_lm:
        return
    if args.search not in TOKEN_NGRAM_SEARCHES:
        raise NotImplementedError("--token-ngram-lm (sub-word n-gram LM fusion) is implemented for --search " +
                                  ", ".join(TOKEN_NGRAM_SEARCHES) + f" only, not --search {args.search}")
    if args.ngram_lm:
        raise NotImplementedError("--token-ngram-lm fuses a sub-word n-gram LM into the prefix beam search without a lexicon: no "
                                  "--ngram-lm (the word n-gram LM of the lexicon search) with it")
    if args.lm_path or args.word_dict:
        raise NotImplementedError("--token-ngram-lm fuses the n-gram LM alone: no --lm-path or --word-dict with it")
    if len(args.path.split(os.pathsep)) > 1:
        raise NotImplementedError(f"--token-ngram-lm: --search {args.search} takes one model, ensembles are not implemented")
    if not args.lm_weight > 0:
        raise ValueError("--token-ngram-lm needs --lm-weight > 0: the n-gram LM scores some tokens -inf")


# --hotwords is the option of the CTC prefix beam search; the transducer beam searches take the same file under a name of their own
_HOTWORDS_HINT = " (that option biases --search ctc_beam): give the phrase file as --transducer-hotwords"


def check_frame_beam_args(args):
    """--search transducer_frame_beam is the device-resident frame-synchronous beam search of one transducer model, alone or with
    one sub-word LM (an LSTM LM, --lm-path, or an n-gram LM over the same units, --token-ngram-lm), with or without phrase
    biasing (--transducer-hotwords): refused, before anything is loaded, with streaming, the CTC search's --hotwords, the
    lexicon search's word n-gram LM (--ngram-lm), word-level LMs, alignments and ensembles."""
    if args.search != "transducer_frame_beam":
        if args.transducer_beam_size_token is not None and args.search != "transducer_stream_beam":
            raise ValueError("--transducer-beam-size-token configures --search transducer_frame_beam / transducer_stream_beam")
        return
    for opt, v in (("--streaming", args.streaming), ("--hotwords", args.hotwords), ("--ngram-lm", args.ngram_lm),
                   ("--word-dict", args.word_dict), ("--print-alignment", args.print_alignment is not None)):
        if v:
            raise NotImplementedError(f"--search transducer_frame_beam is not implemented with {opt}" + _HOTWORDS_HINT * (opt == "--hotwords"))
    if args.lm_path and len(args.lm_path.split(os.pathsep)) != 1:
        raise NotImplementedError("--search transducer_frame_beam fuses one sub-word LSTM LM: no multi-level --lm-path a:b")
    if len(args.path.split(os.pathsep)) > 1:
        raise NotImplementedError("--search transducer_frame_beam takes one model: ensembles (--path a.pt:b.pt) are not implemented")


def check_stream_beam_args(args):
    """--search transducer_stream_beam is the frame-synchronous transducer beam search of one chunk-streaming transducer model
    under --streaming, alone or with one sub-word LM (--lm-path, or --token-ngram-lm; a name of its own: --search
    transducer_frame_beam --streaming stays refused), with or without phrase biasing (--transducer-hotwords).  Refused, before
    anything is loaded: without --streaming, and with the CTC search's --hotwords, the lexicon search's word n-gram LM
    (--ngram-lm), word-level LMs, multi-level LMs, alignments and ensembles."""
    if args.search != "transducer_stream_beam":
        return
    if not args.streaming:
        raise ValueError("--search transducer_stream_beam is the streamed search: give --streaming too (offline: --search "
                         "transducer_frame_beam)")
    for opt, v in (("--hotwords", args.hotwords), ("--ngram-lm", args.ngram_lm), ("--word-dict", args.word_dict),
                   ("--print-alignment", args.print_alignment is not None)):
        if v:
            raise NotImplementedError(f"--search transducer_stream_beam is not implemented with {opt}" + _HOTWORDS_HINT * (opt == "--hotwords"))
    if args.lm_path and len(args.lm_path.split(os.pathsep)) != 1:
        raise NotImplementedError("--search transducer_stream_beam fuses one sub-word LSTM LM: no multi-level --lm-path a:b")
    if len(args.path.split(os.pathsep)) > 1:
        raise NotImplementedError("--search transducer_stream_beam takes one model: ensembles (--path a.pt:b.pt) are not implemented")


def check_ctc_stream_beam_args(args):
    """--search ctc_stream_beam is the CTC prefix beam search of one chunk-streaming CTC model under --streaming: alone, with one
    sub-word LM (an LSTM LM, --lm-path, or an n-gram LM over the same units, --token-ngram-lm), with phrase biasing (--hotwords) or with both (a name of its own: --streaming --search ctc_beam
    without --ngram-lm, and --hotwords with it, stay refused).  Refused, before anything is loaded: without --streaming, and with
    the lexicon + n-gram search's options, word-level and multi-level LMs, alignments, ensembles and the transducer searches'
    --transducer-hotwords."""
    if args.search != "ctc_stream_beam":
        return
    if not args.streaming:
        raise ValueError("--search ctc_stream_beam is the streamed search: give --streaming too (offline: --search ctc_beam)")
    for opt, v in (("--ngram-lm", args.ngram_lm), ("--lexicon", args.lexicon), ("--word-dict", args.word_dict),
                   ("--print-alignment", args.print_alignment is not None), ("--transducer-hotwords", args.transducer_hotwords)):
        if v:
            raise NotImplementedError(f"--search ctc_stream_beam is not implemented with {opt}" +
                                      " (the lexicon + n-gram search is streamed as --search ctc_beam --ngram-lm)" * (opt in ("--ngram-lm", "--lexicon")) +
                                      " (that option biases the transducer searches): give the phrase file as --hotwords" * (opt == "--transducer-hotwords"))
    if args.lm_path and len(args.lm_path.split(os.pathsep)) != 1:
        raise NotImplementedError("--search ctc_stream_beam fuses one sub-word LSTM LM: no multi-level --lm-path a:b")
    if len(args.path.split(os.pathsep)) > 1:
        raise NotImplementedError("--search ctc_stream_beam takes one model: ensembles (--path a.pt:b.pt) are not implemented")


DEFAULT_HOTWORD_SCORE = 1.5


def check_hotword_args(args):
    """--hotwords biases the prefix beam search of --search ctc_beam, and of --search ctc_stream_beam under --streaming (alone or
    with an LSTM LM): refused, before anything is loaded, with every other search, with the lexicon + n-gram search and with
    --streaming --search ctc_beam.  --transducer-hotwords biases the
    frame-synchronous transducer beam search (--search transducer_frame_beam, and transducer_stream_beam under --streaming; with
    or without an LSTM LM, partials and n-best): refused by name with every other search.  One of the two at most."""
    if not args.hotwords and not args.transducer_hotwords:
        for opt, v in (("--hotword-score", args.hotword_score), ("--bpe", args.bpe), ("--sentencepiece-model", args.sentencepiece_model)):
            if v is not None:
                raise ValueError(f"{opt} configures --hotwords: give --hotwords too")
        return
    if args.hotwords and args.transducer_hotwords:
        raise NotImplementedError("--hotwords and --transducer-hotwords name the phrase file of different searches: give one of them")
    if args.transducer_hotwords and args.search not in ("transducer_frame_beam", "transducer_stream_beam"):
        raise NotImplementedError("--transducer-hotwords (phrase biasing) is implemented for --search transducer_frame_beam and "
                                  f"--search transducer_stream_beam only, not --search {args.search}")
    if args.hotwords and args.search not in ("ctc_beam", "ctc_stream_beam"):
        raise NotImplementedError("--hotwords (phrase biasing) is implemented for --search ctc_beam only (streamed: --search "
                                  f"ctc_stream_beam), not --search {args.search}")
    if args.hotwords and args.ngram_lm:
        raise NotImplementedError("--hotwords biases the prefix beam search without a lexicon: no --ngram-lm with it")
    if args.hotwords and args.streaming and args.search != "ctc_stream_beam":
        raise NotImplementedError("--hotwords is not streamed: no --streaming with it (the streamed biased search is --search "
                                  "ctc_stream_beam)")
    if args.hotword_score is not None and not args.hotword_score > 0:
        raise ValueError("--hotword-score must be positive")


def check_streaming_args(args):
    """--streaming is greedy decoding (CTC or transducer), the lexicon + n-gram beam search (--search ctc_beam --ngram-lm), the
    CTC prefix beam search (--search ctc_stream_beam) or the frame-synchronous transducer beam search (--search
    transducer_stream_beam; these two fuse an LSTM LM under streaming) of one chunk-streaming model: refused, before anything
    is loaded, with every other search, with LSTM-LM fusion elsewhere, ensembles and alignment output.  --stream-endpoint
    (endpointing) goes with the last two alone and with their 1-best."""
    if not args.streaming:
        for opt, v in (("--stream-chunk-ms", args.stream_chunk_ms), ("--streams", args.streams),
                       ("--stream-partials", args.stream_partials or None), ("--stream-endpoint", getattr(args, "stream_endpoint", False) or None)):
            if v is not None:
                raise ValueError(f"{opt} configures --streaming: give --streaming too")
        return
    lexicon_beam = args.search == "ctc_beam" and bool(args.ngram_lm)
    if args.search == "ctc_beam" and not lexicon_beam:
        raise NotImplementedError("--streaming --search ctc_beam needs --ngram-lm: the lexicon + n-gram search is the prefix beam "
                                  "search that is streamed, not the one without LM or with an LSTM LM (that one is streamed "
                                  "as --search ctc_stream_beam)")
    stream_beam = args.search in ("transducer_stream_beam", "ctc_stream_beam")
    if args.search not in ("ctc", "transducer_greedy", "ctc_beam", "transducer_stream_beam", "ctc_stream_beam"):
        raise NotImplementedError("--streaming is implemented for greedy decoding (--search ctc, --search transducer_greedy), for "
                                  "--search ctc_beam with --ngram-lm, for --search ctc_stream_beam and for --search "
                                  f"transducer_stream_beam, not --search {args.search}")
    for opt, v in (("--lm-path", args.lm_path and not stream_beam), ("--word-dict", args.word_dict), ("--ngram-lm", args.ngram_lm and not lexicon_beam),
                   ("--print-alignment", args.print_alignment)):
        if v:
            raise NotImplementedError(f"--streaming decodes without LSTM-LM fusion or alignments: no {opt} with it")
    if args.stream_partials and not (lexicon_beam or stream_beam):
        raise NotImplementedError("--stream-partials prints the partial results of --search ctc_beam --ngram-lm, of --search "
                                  "ctc_stream_beam and of --search transducer_stream_beam")
    if getattr(args, "stream_endpoint", False):
        if not stream_beam:
            raise NotImplementedError("--stream-endpoint (endpointing) is implemented for --search ctc_stream_beam and --search "
                                      f"transducer_stream_beam, not --search {args.search}" + " --ngram-lm" * bool(args.ngram_lm))
        if args.nbest > 1:
            raise NotImplementedError("--stream-endpoint joins the 1-best of consecutive segments: no --nbest > 1 with it")
        if not args.endpoint_max_segment_s > 0:
            raise ValueError("--endpoint-max-segment-s must be positive: it sizes the per-stream search state")
    if len(args.path.split(os.pathsep)) > 1:
        raise NotImplementedError("--streaming takes one model: ensembles (--path a.pt:b.pt) are not streamed")
    if (args.stream_chunk_ms is not None and args.stream_chunk_ms <= 0) or (args.streams is not None and args.streams <= 0):
        raise ValueError("--stream-chunk-ms and --streams must be positive")


def recognize_streaming(task, model, dictionary, utt_ids, waves, dev, chunk_ms=400, streams=16, refs=None, out=sys.stdout,
                        quiet=False, scorer=None, summary_out=None, search="ctc", max_num_expansions_per_step=2, lexicon_beam=None,
                        partials=False, stream_beam=None, ctc_stream_beam=None, ctm_hyps=None, endpoint=None, seconds_per_frame=None,
                        rates=None):
    """The output of `recognize` from a streamed pass: every utterance is read in pieces of `chunk_ms`, `streams` of them in
    flight; a finished utterance frees its slot for the next one (wav.scp order).  search "ctc_beam": lexicon_beam holds the
    arguments of StreamingCTCLexiconBeamDecoder after `dictionary` (n-gram LM, lexicon) and its options; its prefix tables are
    sized for the longest utterance given.  search "transducer_stream_beam": stream_beam holds the options of
    StreamingTransducerFrameBeamDecoder (beam, n-best, LM, ...), search "ctc_stream_beam": ctc_stream_beam those of
    StreamingCTCPrefixBeamDecoder; their prefix tables are sized the same way.  partials: a `P-` line
    per stream whenever its partial text changed.  ctm_hyps: a dict that gets utterance -> (its best hypothesis, the symbols stripped from the text) (--ctm).

    endpoint (--stream-endpoint; search "ctc_stream_beam" / "transducer_stream_beam", 1-best): the EndpointRules, in encoder
    frames, under which an utterance is decoded as consecutive segments.  A slot is then sized for segment_frames plus the most
    frames one accept can bring, whatever the utterance lengths.  After every accept one `endpoint` readback names the streams
    whose segment ends (silence / empty / length); a stream whose next piece would not fit ends its segment before that accept
    ("room").  A closed segment prints `S-<utt>`, its start and end in seconds (seconds_per_frame per encoder frame; default:
    the encoder's stride x the front-end's frame shift), the rule and its text; the segment the audio's end closes is "final".
    Segments end on piece boundaries.  The utterance's hypothesis is the segments' joined: tokens concatenated, scores summed,
    times shifted by each segment's first frame.  The stable field of a `P-` line starts with the closed segments' text.

    rates: the sample rate of every entry of `waves` (None: the front-end's).  Pieces of `chunk_ms` are cut at the utterance's own
    rate and converted by the encoder's StreamResampler; every time printed stays in seconds of the recording."""
    from .models.transformer.streaming_encoder import StreamingEncoder
    from .tools.streaming_ctc_decoder import StreamingCTCDecoder
    from .tools.streaming_ctc_lexicon_beam_decoder import StreamingCTCLexiconBeamDecoder
    from .tools.streaming_ctc_prefix_beam_decoder import StreamingCTCPrefixBeamDecoder
    from .tools.streaming_transducer_frame_beam_decoder import StreamingTransducerFrameBeamDecoder
    from .tools.beam_common import EndpointRules
    from .tools.streaming_transducer_greedy_decoder import StreamingTransducerGreedyDecoder
    from .tools.wer import Scorer

    if scorer is None:
        scorer = Scorer(dictionary, wer_output_filter=None)
    se = StreamingEncoder(model, streams, frontend=task.frontend)
    partial_of = None  # a decoder's partial -> (tokens of the best hypothesis, how many of them are stable)
    # the longest utterance's encoder frames: what a slot of the three beam searches is sized for
    fo = task.frontend.sample_rate
    rates = [fo] * len(waves) if rates is None else [int(r) for r in rates]
    max_frames = max([1] + [-(-task.frontend.num_frames(n) // se.stride) for n in lengths_at(waves, rates, fo)])
    piece_of = [max(1, int(r * chunk_ms / 1000)) for r in rates]  # samples per piece, at the utterance's own rate
    if endpoint is not None:
        if search not in ("ctc_stream_beam", "transducer_stream_beam"):
            raise NotImplementedError("endpointing (--stream-endpoint) is implemented for --search ctc_stream_beam and --search "
                                      f"transducer_stream_beam, not --search {search}")
        opts = ctc_stream_beam if search == "ctc_stream_beam" else stream_beam
        if opts.get("nbest", 1) != 1:
            raise NotImplementedError("endpointing (--stream-endpoint) joins the 1-best of consecutive segments: no --nbest > 1 with it")
        if endpoint.segment_frames > 0:  # a constant of the options: memory per stream no longer grows with the audio
            max_frames = endpoint.segment_frames + max([se.max_rows_per_accept(max(1, int(fo * chunk_ms / 1000)))] +
                                                       [se.max_rows_per_accept(p, r) for p, r in zip(piece_of, rates) if r != fo])
        opts = dict(opts, endpoint=endpoint)
        ctc_stream_beam, stream_beam = (opts, stream_beam) if search == "ctc_stream_beam" else (ctc_stream_beam, opts)
        if seconds_per_frame is None:
            seconds_per_frame = se.stride * task.frontend.frame_shift / task.frontend.sample_rate
    if search == "ctc":
        dec = StreamingCTCDecoder(dictionary)
        strip = {dictionary.eos(), dictionary.pad()}
    elif search == "ctc_beam":
        (ngram_lm, lexicon), opts = lexicon_beam
        dec = StreamingCTCLexiconBeamDecoder(dictionary, ngram_lm, lexicon, streams, max_frames, **opts)
        partial_of = lambda part: (part["tokens"], len(part["stable"]))  # noqa: E731
        strip = {dictionary.eos(), dictionary.pad()}
    elif search == "ctc_stream_beam":
        dec = StreamingCTCPrefixBeamDecoder(dictionary, streams, max_frames, **ctc_stream_beam)
        partial_of = lambda part: (part["tokens"], len(part["stable"]))  # noqa: E731
        strip = {dictionary.eos(), dictionary.pad()}
    elif search == "transducer_stream_beam":
        dec = StreamingTransducerFrameBeamDecoder(model, dictionary, max_streams=streams, max_frames=max_frames, **stream_beam)
        strip = dec.symbols_to_strip_from_output
        partial_of = lambda part: part[:2]  # noqa: E731
    else:
        dec = StreamingTransducerGreedyDecoder(model, dictionary, max_num_expansions_per_step=max_num_expansions_per_step)
        strip = dec.symbols_to_strip_from_output
    pending = list(range(len(utt_ids)))
    live = {}  # utterance index -> samples consumed
    hyps = {}
    shown = {}  # utterance index -> the partial text last printed
    num_tok, audio_s = 0, 0.0

    def text_of(toks):
        return dictionary.string(torch.tensor([t for t in toks if t not in strip], dtype=torch.long), bpe_symbol=None)

    segs = {}  # endpointing: utterance index -> its closed segments (first frame, hypothesis, text)
    seg_frames = {}  # utterance index -> [first frame of the open segment, its frames so far]

    def end_segment(i, hypo, rule):
        start, n = seg_frames[i]
        text = text_of(hypo["tokens"].tolist())
        segs.setdefault(i, []).append((start, hypo, text))
        seg_frames[i] = [start + n, 0]
        if not quiet:
            print("S-{}\t{:.2f}\t{:.2f}\t{}\t{}".format(utt_ids[i], start * seconds_per_frame, (start + n) * seconds_per_frame, rule,
                                                      text), file=out)

    def joined(i):
        """The utterance's hypothesis from its segments: tokens concatenated, scores summed, times shifted."""
        parts = segs[i]
        hypo = dict(parts[0][1])
        hypo["tokens"] = torch.cat([h["tokens"] for _, h, _ in parts])
        hypo["score"] = torch.stack([h["score"] for _, h, _ in parts]).sum()
        if "times" in hypo:
            hypo["times"] = torch.cat([h["times"] + s for s, h, _ in parts])
            hypo["viterbi_score"] = torch.stack([h["viterbi_score"] for _, h, _ in parts]).sum()
        return hypo

    t0 = time.perf_counter()
    while pending or live:
        while pending and len(live) < streams:
            i = pending.pop(0)
            live[i] = 0
            se.open([i], **({} if rates[i] == fo else {"rates": [rates[i]]}))
            dec.open([i])
            seg_frames[i] = [0, 0]
        ids = list(live)
        pieces, final = [], []
        for i in ids:
            a = live[i]
            b = min(len(waves[i]), a + piece_of[i])
            pieces.append(torch.from_numpy(np.ascontiguousarray(waves[i][a:b])).float())
            live[i] = b
            final.append(b >= len(waves[i]))
        logits, counts = se.accept_waveform(ids, pieces, final)
        if logits is not None:
            if endpoint is not None:  # rule 4: a piece that would not fit ends the segment first
                for i in dec.room(ids, counts):
                    end_segment(i, dec.end_segment(i)[0], EndpointRules.NAMES[EndpointRules.ROOM])
            dec.accept(ids, logits, counts)
            if endpoint is not None:
                for i, c, f, (rule, _, _, _) in zip(ids, counts, final, dec.endpoint(ids)):
                    seg_frames[i][1] += c
                    if rule and not f:  # (the audio's end closes the last segment below)
                        end_segment(i, dec.end_segment(i)[0], EndpointRules.NAMES[rule])
        if partials:
            for i, part in zip(ids, dec.partial(ids)):
                toks, k = partial_of(part)
                texts = (text_of(toks[:k]), text_of(toks[k:]))
                if i in segs:
                    texts = (" ".join(t for t in [t for _, _, t in segs[i]] + [texts[0]] if t), texts[1])
                if shown.get(i) != texts:
                    shown[i] = texts
                    print("P-{}\t{:.2f}\t{}\t{}".format(utt_ids[i], live[i] / float(rates[i]), *texts), file=out)
        for i, f in zip(ids, final):
            if f:
                se.close([i])
                h = dec.close(i)
                hyps[i] = h if isinstance(h, list) else [h]
                if endpoint is not None:
                    if seg_frames[i][1] > 0 or i not in segs:
                        end_segment(i, hyps[i][0], "final")
                    hyps[i] = [joined(i)]
                del live[i]
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t_gen = time.perf_counter() - t0
    for i, utt in enumerate(utt_ids):
        if refs is not None and utt in refs and not quiet:
            print("T-{}\t{}".format(utt, refs[utt]), file=out)
        for j, hypo in enumerate(hyps[i]):  # best first (one, but for the nbest of --search ctc_beam)
            hypo_str = dictionary.string(torch.tensor([t for t in hypo["tokens"].tolist() if t not in strip]), bpe_symbol=None)
            if not quiet:
                print("H-{}\t{}\t{}".format(utt, hypo_str, float(hypo["score"]) / math.log(2)), file=out)
            if j == 0:
                scorer.add_prediction(utt, hypo_str)
                if refs is not None and utt in refs:
                    scorer.add_evaluation(utt, refs[utt], hypo_str)
                num_tok += len(hypo["tokens"])
                if ctm_hyps is not None:
                    ctm_hyps[utt] = (hypo, strip)
        audio_s += len(waves[i]) / float(rates[i])
    n = len(utt_ids)
    lines = ["NOTE: hypothesis and token scores are output in base 2",
             "Recognized {:,} utterances ({} tokens) in {:.1f}s ({:.2f} sentences/s, {:.2f} tokens/s), RTF {:.4f}".format(
                 n, num_tok, t_gen, n / max(t_gen, 1e-9), num_tok / max(t_gen, 1e-9), t_gen / max(audio_s, 1e-9))]
    if refs:
        lines += scorer.summary_lines()
    for f in [out] + ([summary_out] if summary_out is not None else []):
        for line in lines:
            print(line, file=f)
    return scorer


def lm_fusion_mode(args):
    """Which LM the search fuses, from `--lm-path` / `--word-dict` / `--search` (espresso/speech_recognize.py:130-148):
    None, "subword" (one sub-word LM), "lookahead" (one word LM + --word-dict) or "multilevel" (`sub.pt:word.pt` +
    --word-dict).  Raises before anything is loaded for combinations that have no implementation."""
    if args.search == "ctc_beam" and args.word_dict:
        raise NotImplementedError("--search ctc_beam fuses one sub-word LSTM LM: no look-ahead or multi-level word LM (--word-dict)")
    if not args.lm_path:
        return None
    paths = args.lm_path.split(os.pathsep)
    if args.search == "ctc_beam" and len(paths) != 1:
        raise NotImplementedError("--search ctc_beam fuses one sub-word LSTM LM: give one --lm-path")
    if len(paths) == 1:
        return "lookahead" if args.word_dict else "subword"
    if len(paths) != 2 or not args.word_dict:
        raise ValueError("--lm-path with two LMs (multi-level fusion) is `sub.pt:word.pt` together with --word-dict")
    if args.search != "beam":
        raise NotImplementedError("multi-level (sub-word + word) LM fusion is implemented for the attention decoder's beam search "
                                  "(--search beam): the transducer decoders fuse one LSTM LM and the CTC decoder none")
    return "multilevel"


def _load_file(path):
    try:
        return torch.load(path, map_location="cpu")
    except Exception:  # checkpoints written by the reference carry Namespace / omegaconf objects next to the tensors
        return torch.load(path, map_location="cpu", weights_only=False)


def _load_state(path):
    sd = _load_file(path)
    return sd["model"] if isinstance(sd, dict) and "model" in sd and isinstance(sd["model"], dict) else sd


def resolve_model_config(model_name, model_config_path, checkpoint):
    """(registered model name, `model:` block as a dict): explicit arguments win; otherwise what the checkpoint's `cfg` holds
    (fairseq/checkpoint_utils.py:422-470 rebuilds the model from `state["cfg"].model` the same way)."""
    import yaml

    stored = None
    cfg = checkpoint.get("cfg") if isinstance(checkpoint, dict) else None
    if cfg is not None:
        stored = cfg["model"] if isinstance(cfg, dict) else getattr(cfg, "model", None)
        if stored is not None and not isinstance(stored, dict):
            try:
                from omegaconf import OmegaConf  # a reference checkpoint opened where omegaconf exists

                stored = OmegaConf.to_container(stored, resolve=True)
            except ImportError:
                stored = dict(vars(stored)) if hasattr(stored, "__dict__") else dict(stored)
    if model_config_path:
        block = json.load(open(model_config_path)) if model_config_path.endswith(".json") else yaml.safe_load(open(model_config_path))
        block = block.get("model", block) if isinstance(block.get("model"), dict) else block  # a whole recipe file is fine too
    elif stored is not None:
        block = dict(stored)
    else:
        raise ValueError("--model-config is required: the checkpoint holds no cfg.model block")
    name = model_name or block.get("_name") or (stored or {}).get("_name") or "speech_transformer_base"
    return name, block


def load_member(state, name, block, task, dev):
    """The model `name` built from its `model:` block for `task`, with the checkpoint's weights, on `dev`, in eval mode."""
    from . import registry

    cls = registry.MODEL_REGISTRY[name]
    cfg_cls = getattr(cls, "config_class", None)
    cfg = cfg_cls.from_dict(block) if cfg_cls is not None else block
    m = cls.build_model(cfg, task)
    sd = state["model"] if isinstance(state, dict) and isinstance(state.get("model"), dict) else state
    if hasattr(m, "upgrade_state_dict_named"):
        sd = m.upgrade_state_dict_named(dict(sd), "")
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


def main(argv=None):
    args = get_parser().parse_args(argv)
    from .tools.long_form import check_long_form_transducer_args

    check_long_form_transducer_args(args)  # first: its refusals name --long-form-transducer, not the search
    check_ctm_args(args)
    check_confidence_args(args)
    check_token_ngram_args(args)
    check_frame_beam_args(args)
    check_stream_beam_args(args)
    check_ctc_stream_beam_args(args)
    if args.print_alignment is not None and not args.results_path:
        raise ValueError("--print-alignment saves attention plots under --results-path: give --results-path")
    check_hotword_args(args)
    check_ngram_args(args)
    check_streaming_args(args)
    from .tools import long_form as LF

    LF.check_long_form_args(args)
    check_long_form_posteriors_args(args)
    lm_mode = lm_fusion_mode(args)
    if args.search == "ctc_beam" and len(args.path.split(os.pathsep)) > 1:
        raise NotImplementedError("ensembles are implemented for the attention decoder's beam search (--search beam)")
    import yaml

    from .data.asr_dictionary import AsrDictionary
    from .models.external_language_model import MultiLevelLanguageModel
    from .models.lstm_lm import LSTMLanguageModelEspresso
    from .models.tensorized_lookahead_language_model import TensorizedLookaheadLanguageModel
    from .tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask

    dev = torch.device(args.device or "cuda:{}".format(int(os.environ.get("LOCAL_RANK", "0"))))
    if dev.type == "cuda":
        if dev.index is None:  # `--device cuda`: set_device needs an explicit index
            dev = torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(dev)
    paths = args.path.split(os.pathsep)  # `--path a.pt:b.pt` = an ensemble (fairseq utils.split_paths in speech_recognize.py:107)
    state = _load_file(paths[0])
    model_name, model_cfg = resolve_model_config(args.model, args.model_config, state)
    if args.long_form:  # before the weights are loaded: an encoder-only CTC model
        LF.require_ctc_model(model_name)
    if args.long_form_transducer:  # likewise: a transducer model
        LF.require_transducer_model(model_name)
    autoregressive = args.search == "beam"
    # the criterion the checkpoint was trained with decides whether "<s>" is the blank (speech_recognition.py:324, 345-347)
    crit = {"beam": "label_smoothed_cross_entropy_v2", "ctc": "ctc_loss", "ctc_beam": "ctc_loss", "ctc_stream_beam": "ctc_loss"}.get(args.search, "transducer_loss")
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(
        dict=args.dict, autoregressive=autoregressive, global_cmvn_stats_path=args.global_cmvn_stats_path, criterion_name=crit,
        non_lang_syms=args.non_lang_syms, wer_output_filter=args.wer_output_filter, bpe=args.bpe,
        sentencepiece_model=args.sentencepiece_model))
    context_graph = None
    if args.hotwords or args.transducer_hotwords:  # before the model: a malformed phrase file fails fast
        from .tools.context_graph import load_context_graph

        d = task.target_dictionary
        context_graph = load_context_graph(args.hotwords or args.transducer_hotwords, d, d.bos(),
                                           DEFAULT_HOTWORD_SCORE if args.hotword_score is None else args.hotword_score)
    ngram = None
    if args.ngram_lm:  # before the model: a malformed ARPA or lexicon file fails fast
        from .models.ngram_lm import NGramLanguageModel
        from .tools.lexicon import build_lexicon

        ngram_lm = NGramLanguageModel(args.ngram_lm)
        ngram = (ngram_lm, build_lexicon(task.target_dictionary, ngram_lm, args.lexicon))
        ngram_lm.to(dev)
    token_lm = None
    if args.token_ngram_lm:  # before the model: a malformed ARPA file, or one over other units, fails fast
        from .models.token_ngram_lm import TokenNGramLM

        token_lm = TokenNGramLM(args.token_ngram_lm, task.target_dictionary, device=dev)
    if args.streaming:  # the encoder options streaming cannot reproduce exactly: refused before the model is built or audio is read
        from . import registry
        from .models.transformer.streaming_encoder import check_streamable

        cfg_cls = getattr(registry.MODEL_REGISTRY[model_name], "config_class", None)
        cfg0 = cfg_cls.from_dict(model_cfg) if cfg_cls is not None else None
        if cfg0 is None or not hasattr(cfg0, "encoder") or not hasattr(cfg0.encoder, "chunk_size"):
            raise NotImplementedError(f"--streaming needs a chunk-streaming transformer or causal-conformer encoder model, not {model_name}")
        check_streamable(cfg0)
    if args.search in ("transducer_frame_beam", "transducer_stream_beam"):  # before the weights are loaded: a transducer model
        from . import registry

        if not hasattr(registry.MODEL_REGISTRY[model_name], "joint_step"):
            raise NotImplementedError(f"--search {args.search} needs a transducer model (predictor + joint), not {model_name}")
    model = load_member(state, model_name, model_cfg, task, dev)
    members = [model]
    for extra in paths[1:]:  # every member is rebuilt from ITS OWN checkpoint's configuration (checkpoint_utils.load_model_ensemble)
        st = _load_file(extra)
        members.append(load_member(st, *resolve_model_config(args.model, args.model_config, st), task, dev))
    if len(members) > 1 and args.search != "beam":
        raise NotImplementedError("ensembles are implemented for the attention decoder's beam search (--search beam)")
    lm = token_lm
    if args.lm_path:
        class _LMTask:
            target_dictionary = source_dictionary = task.target_dictionary
        if args.word_dict:
            _LMTask.word_dictionary = AsrDictionary.load(args.word_dict, enable_bos=False)
        if lm_mode == "multilevel":
            sub_path, word_path = args.lm_path.split(os.pathsep)
            sub_lm = LSTMLanguageModelEspresso.build_model(dict(arch=args.lm_arch, is_wordlm=False), _LMTask)
            sub_lm.load_state_dict(_load_state(sub_path), strict=True)
            word_lm = LSTMLanguageModelEspresso.build_model(dict(arch=args.word_lm_arch, is_wordlm=True), _LMTask)
            word_lm.load_state_dict(_load_state(word_path), strict=True)
            lm = MultiLevelLanguageModel(word_lm.to(dev).eval(), sub_lm.to(dev).eval(), subwordlm_weight=args.subwordlm_weight,
                                         oov_penalty=args.oov_penalty, open_vocab=not args.disable_open_vocab)
        else:
            lm = LSTMLanguageModelEspresso.build_model(dict(arch=args.lm_arch, is_wordlm=bool(args.word_dict)), _LMTask)
            lm.load_state_dict(_load_state(args.lm_path), strict=True)
            lm = lm.to(dev).eval()
            if args.word_dict:
                lm = TensorizedLookaheadLanguageModel(lm, task.target_dictionary, oov_penalty=args.oov_penalty,
                                                      open_vocab=not args.disable_open_vocab)
    gen = None  # (the streamed beam searches build their own decoders in recognize_streaming, which validates the same options)
    if args.search not in ("transducer_stream_beam", "ctc_stream_beam") and not args.long_form and not args.long_form_transducer:
        gen = build_generator(args, members if len(members) > 1 else model, task.target_dictionary, lm, ngram, context_graph)
    scp = read_scp(args.wav_scp)
    utt_ids = list(scp.keys())
    waves, rates = read_waves([scp[u] for u in utt_ids])
    refs = read_scp(args.text) if args.text else None
    task.build_frontend(dev)
    fo = getattr(task.frontend, "sample_rate", 16000)
    batches = shard_batches(make_batches(utt_ids, lengths_at(waves, rates, fo), args.max_tokens, args.batch_size), args.num_shards,
                            args.shard_id)
    if args.num_shards > 1:  # (the defaults come from WORLD_SIZE / RANK: say that this process decodes — and scores — a part only)
        print(f"| decoding shard {args.shard_id} of {args.num_shards}: {sum(len(b) for b in batches)} of {len(utt_ids)} utterances; "
              "WER / CER below cover this shard only", file=sys.stderr)
    from .tools.wer import Scorer

    scorer = Scorer(task.target_dictionary, wer_output_filter=args.wer_output_filter)
    stream = (collate(b, utt_ids, waves, dev, rates, fo) for b in batches)
    lf_model = None
    if args.long_form:  # one recording at a time, its windows are the batch; the generator reads the stitched log-probs
        lf_model = LF.LongFormModel(model, LF.LongFormCTC(task, LF.plan_from_args(args, task.frontend, model), task.target_dictionary.bos(),
                                                          args.max_tokens, args.batch_size))
        gen = build_generator(args, lf_model, task.target_dictionary, lm, ngram, context_graph)
        if args.long_form_posteriors:  # after the search, per hypothesis, on the matrix the search read
            gen = LF.LongFormPosteriors(gen, lf_model, task.target_dictionary)
        batches = shard_batches([[i] for i in range(len(utt_ids))], args.num_shards, args.shard_id)
        stream = ({"utt_ids": [utt_ids[i]], "num_samples": [len(waves[i])],
                   **({"wav_rates": [rates[i]], "net_input": {"wave": waves[i], "rate": rates[i]}} if rates[i] != fo else
                      {"net_input": {"wave": waves[i]}})} for (i,) in batches)
    lft_model = None
    if args.long_form_transducer:  # one recording at a time; the generator's encoder pass is the stitched encoder outputs
        frame_beam = args.search == "transducer_frame_beam"
        lft_model = LF.LongFormTransducerModel(
            model, LF.LongFormTransducer(task, LF.plan_from_args(args, task.frontend, model.encoder), args.max_tokens, args.batch_size),
            search=(args.beam, args.nbest, context_graph is not None, bool(args.ctm)) if frame_beam else None)
        gen = build_generator(args, lft_model, task.target_dictionary, lm, ngram, context_graph)
        batches = shard_batches([[i] for i in range(len(utt_ids))], args.num_shards, args.shard_id)
        stream = ({"utt_ids": [utt_ids[i]], "num_samples": [len(waves[i])], **({"wav_rates": [rates[i]]} if rates[i] != fo else {}),
                   "net_input": lft_model.net_input(waves[i], rates[i] if rates[i] != fo else None)} for (i,) in batches)
    ctm_hyps = {} if args.ctm else None

    from .tools.forced_aligner import frame_seconds

    def finish_ctm():
        if lf_model is not None:
            LF.log_worst(lf_model, sys.stderr)
        if lft_model is not None:
            LF.log_worst_features(lft_model, sys.stderr)
        if ctm_hyps is not None:
            write_ctm(args.ctm, utt_ids, ctm_hyps, task.target_dictionary, args.ctm_unit,
                      frame_seconds(model, task.frontend.frame_shift / task.frontend.sample_rate))

    if args.streaming:
        mine = [i for b in batches for i in b]
        mine.sort()
        s_ids, s_waves = [utt_ids[i] for i in mine], [waves[i] for i in mine]
        s_rates = [rates[i] for i in mine]
        kw = dict(chunk_ms=args.stream_chunk_ms or 400, streams=args.streams or 16, refs=refs, quiet=args.quiet, scorer=scorer,
                  search=args.search, max_num_expansions_per_step=args.max_num_expansions_per_step, partials=args.stream_partials,
                  ctm_hyps=ctm_hyps, rates=s_rates)
        if getattr(args, "stream_endpoint", False):
            kw.update(endpoint_options(args, frame_seconds(model, task.frontend.frame_shift / task.frontend.sample_rate)))
        if args.search == "ctc_beam":
            kw["lexicon_beam"] = (ngram, dict(beam_size=args.beam, nbest=args.nbest, beam_size_token=args.ctc_beam_size_token,
                                              lm_weight=args.lm_weight, word_score=args.word_score,
                                              insertion_bonus=args.ctc_insertion_bonus))
        if args.search == "ctc_stream_beam":
            kw["ctc_stream_beam"] = ctc_stream_beam_options(args, lm, context_graph)
        if args.search == "transducer_stream_beam":
            kw["stream_beam"] = stream_beam_options(args, lm, context_graph)
        if not args.results_path:
            recognize_streaming(task, model, task.target_dictionary, s_ids, s_waves, dev, out=sys.stdout, **kw)
            finish_ctm()
            return scorer
        os.makedirs(args.results_path, exist_ok=True)
        with open(os.path.join(args.results_path, "decode.log"), "w", buffering=1, encoding="utf-8") as log:
            recognize_streaming(task, model, task.target_dictionary, s_ids, s_waves, dev, out=log, summary_out=sys.stdout, **kw)
        finish_ctm()
        has_target = refs is not None and all(u in refs for u in s_ids)
        if has_target:
            scorer.add_ordered_utt_list(s_ids)
        write_results(args.results_path, scorer, has_target)
        return scorer
    if not args.results_path:
        recognize(task, model, gen, stream, task.target_dictionary, refs, out=sys.stdout, nbest=args.nbest, quiet=args.quiet,
                  scorer=scorer, ctm_hyps=ctm_hyps)
        finish_ctm()
        return scorer
    os.makedirs(args.results_path, exist_ok=True)
    # attention plots only for the attention decoder (the reference's is_attention_model: not the CTC / transducer criteria)
    plot_dir = os.path.join(args.results_path, "attn_plots") if args.print_alignment is not None and args.search == "beam" else None
    with open(os.path.join(args.results_path, "decode.log"), "w", buffering=1, encoding="utf-8") as log:
        recognize(task, model, gen, stream, task.target_dictionary, refs, out=log, nbest=args.nbest, quiet=args.quiet, scorer=scorer,
                  summary_out=sys.stdout, attn_plot_dir=plot_dir, ctm_hyps=ctm_hyps)
    finish_ctm()
    decoded = [u for b in batches for u in (utt_ids[i] for i in b)]
    has_target = refs is not None and all(u in refs for u in decoded)
    if has_target:  # wav.scp order of the utterances this process decoded (the reference: dataset.tgt.utt_ids)
        keep = set(decoded)
        scorer.add_ordered_utt_list([u for u in utt_ids if u in keep])
    write_results(args.results_path, scorer, has_target)
    return scorer


if __name__ == "__main__":
    main()
