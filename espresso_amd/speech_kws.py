"""Keyword-spotting CLI: where the phrases of a keyword file are spoken in the audio of a wav.scp, and how sure a trained CTC
model is, offline or streamed.

Model, dictionary, audio, batching and sharding options mean what they mean in `speech_align`.  `--keywords` is a phrase file
in the format of `--hotwords` (one phrase per line, tokenised as transcripts are), the number after a TAB being that keyword's
threshold theta in (0, 1] (default `--threshold`): a phrase is reported where exp(e / L) >= theta, e being the log-prob of the
keyword's best path relative to the greedy path's over the same frames and L its token count (tools/keyword_spotter.py, DESIGN.md
section 3.7).  A hit is final `--hold-ms` after its end -- until then a better overlapping candidate may replace it -- or at the
audio's end.  `--output` gets one line per hit, `utt<TAB>start_s<TAB>end_s<TAB>confidence<TAB>keyword`, in wav.scp order, then by
start time; seconds per encoder frame = the front-end's frame shift x the model's sub-sampling factor, end_s = (end + 1) frames.

With `--streaming` the audio is fed in pieces of `--stream-chunk-ms` with `--streams` utterances in flight through the
StreamingEncoder, as `speech_recognize --streaming` does, and a `K-<utt>` line goes to stdout as soon as a hit is reported:
`K-utt<TAB>reported_s<TAB>start_s<TAB>end_s<TAB>confidence<TAB>keyword`, reported_s being the audio consumed when the hit was
read, so the latency (hold after the hit's end, plus the piece) is visible.

With `--long-form` every recording, of any length, goes through an offline model as overlapping windows whose logits are joined
on the device into one log-prob matrix (tools/long_form.py; the window, overlap, edge and guard defaults are
uncalibrated), and the offline scan runs over that: hits carry the recording's own times.

Only encoder-only CTC models are taken: transducer and attention models are refused before anything is loaded.  The defaults
0.5 and 500 ms are option defaults; their calibration on real speech is unmeasured."""
import argparse
import os
import sys
import time
from typing import Dict, List

import numpy as np
import torch

from .speech_recognize import (_load_file, collate, lengths_at, load_member, make_batches, read_scp, read_wav, read_waves,  # noqa: F401
                               resolve_model_config, shard_batches)


def get_parser():
    p = argparse.ArgumentParser("espresso_amd.speech_kws", description=__doc__.split("\n")[0])
    p.add_argument("--path", required=True, help="state_dict (or fairseq checkpoint dict with a 'model' entry)")
    p.add_argument("--model", default=None, help="registered model name (default: the checkpoint's cfg.model._name)")
    p.add_argument("--model-config", default=None, help="JSON/YAML file with the recipe's `model:` block (default: the checkpoint's)")
    p.add_argument("--dict", required=True)
    p.add_argument("--wav-scp", required=True)
    p.add_argument("--global-cmvn-stats-path", default=None)
    p.add_argument("--bpe", default=None, choices=["characters_asr", "sentencepiece"],
                   help="tokenise the keywords with this encoder (as the task does for training targets)")
    p.add_argument("--sentencepiece-model", default=None)
    p.add_argument("--non-lang-syms", default=None, help="non-language symbols (one per line), kept whole by characters_asr")
    p.add_argument("--max-tokens", type=int, default=15000)
    p.add_argument("--batch-size", type=int, default=24)
    p.add_argument("--num-shards", type=int, default=int(os.environ.get("WORLD_SIZE", "1")))
    p.add_argument("--shard-id", type=int, default=int(os.environ.get("RANK", "0")))
    p.add_argument("--device", default=None, help="default: cuda:LOCAL_RANK (cuda:0 outside a launcher)")
    p.add_argument("--keywords", required=True, help="keyword file: one phrase per line, optionally <TAB>threshold")
    p.add_argument("--threshold", type=float, default=0.5,
                   help="theta of the keywords without one of their own: a phrase is reported where the geometric mean per token of "
                        "p(keyword path) / p(greedy path) reaches it (an option default; its calibration on real speech is unmeasured)")
    p.add_argument("--hold-ms", type=float, default=500.0,
                   help="a hit is final this long after its end; until then a better overlapping candidate replaces it (an option "
                        "default; its calibration on real speech is unmeasured)")
    p.add_argument("--max-hits", type=int, default=64, help="hits kept per utterance and keyword (offline) or between two reads (streamed)")
    p.add_argument("--output", default="-", help="hit file (default: stdout)")
    p.add_argument("--streaming", action="store_true",
                   help="feed the audio in pieces of --stream-chunk-ms with --streams utterances in flight (a chunk-streaming "
                        "encoder) and print a K-<utt> line as soon as a hit is reported")
    p.add_argument("--stream-chunk-ms", type=int, default=None, help="--streaming: audio per piece (default 400)")
    p.add_argument("--streams", type=int, default=None, help="--streaming: concurrent utterances (default 16)")
    from .tools.long_form import add_long_form_args

    add_long_form_args(p)  # --long-form: recordings of any length through an offline CTC model, hits in global time
    return p


def require_ctc(name: str):
    """Keyword spotting reads CTC log-probs: transducer and attention models are refused."""
    from .speech_align import model_kind

    try:
        kind = model_kind(name)
    except NotImplementedError:
        kind = "attention"
    if kind != "ctc":
        raise NotImplementedError(f"keyword spotting is implemented for encoder-only CTC models, not for the {kind} model '{name}'")


def check_args(args):
    if not 0.0 < args.threshold <= 1.0:
        raise ValueError(f"--threshold {args.threshold} is outside (0, 1]")
    if args.hold_ms < 0 or args.max_hits < 1:
        raise ValueError("--hold-ms must not be negative and --max-hits must be positive")
    if not args.streaming:
        for opt, v in (("--stream-chunk-ms", args.stream_chunk_ms), ("--streams", args.streams)):
            if v is not None:
                raise ValueError(f"{opt} configures --streaming: give --streaming too")
    chunk_ms = 400 if args.stream_chunk_ms is None else args.stream_chunk_ms
    streams = 16 if args.streams is None else args.streams
    if chunk_ms < 1 or streams < 1:
        raise ValueError("--stream-chunk-ms and --streams must be positive")
    return chunk_ms, streams


def hold_frames(hold_ms: float, seconds_per_frame: float) -> int:
    return max(0, int(round(hold_ms / 1000.0 / seconds_per_frame)))


def write_hits(results: Dict[str, List[Dict]], order, seconds_per_frame: float, out):
    """One line per hit, the utterances in `order`, an utterance's hits by start time (then end, then keyword index)."""
    from .tools.keyword_spotter import output_line

    for u in order:
        for h in sorted(results[u], key=lambda h: (h["start"], h["end"], h["keyword"])):
            print(output_line(u, h, seconds_per_frame), file=out)


def spot_streaming(task, model, spotter, utt_ids, waves, seconds_per_frame, chunk_ms=400, streams=16, out=None, rates=None):
    """utterance -> hits from a streamed pass: every utterance is read in pieces of `chunk_ms`, `streams` of them in flight; a
    finished utterance frees its slot for the next one (wav.scp order).  A `K-` line per hit as soon as it is read.
    rates: the sample rate of every entry of `waves` (None: the front-end's); pieces are cut at the utterance's own rate."""
    from .models.transformer.streaming_encoder import StreamingEncoder
    from .tools.keyword_spotter import hit_seconds

    out = sys.stdout if out is None else out
    se = StreamingEncoder(model, streams, frontend=task.frontend)
    rates = [task.frontend.sample_rate] * len(waves) if rates is None else [int(r) for r in rates]
    piece_of = [max(1, int(r * chunk_ms / 1000)) for r in rates]
    pending = list(range(len(utt_ids)))
    live = {}  # utterance index -> samples consumed
    results = {u: [] for u in utt_ids}

    def report(i, hits):
        for h in hits:
            s, e = hit_seconds(h, seconds_per_frame)
            print("K-{}\t{:.2f}\t{:.3f}\t{:.3f}\t{:.4f}\t{}".format(utt_ids[i], live[i] / float(rates[i]), s, e, h["confidence"], h["text"]),
                  file=out)
        results[utt_ids[i]] += hits

    while pending or live:
        while pending and len(live) < streams:
            i = pending.pop(0)
            live[i] = 0
            se.open([i], **({} if rates[i] == task.frontend.sample_rate else {"rates": [rates[i]]}))
            spotter.open([i])
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
            spotter.accept(ids, logits, counts)
            for i, hits in zip(ids, spotter.poll(ids)):
                report(i, hits)
        for i, f in zip(ids, final):
            if f:
                se.close([i])
                report(i, spotter.close(i))
                del live[i]
    return results


def main(argv=None):
    args = get_parser().parse_args(argv)
    chunk_ms, streams = check_args(args)
    from .tools import long_form as LF

    LF.check_long_form_args(args, tool="speech_kws")
    if args.model:  # refuse transducer and attention models before anything is loaded
        require_ctc(args.model)
    from .tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from .tools.forced_aligner import frame_seconds
    from .tools.keyword_spotter import CTCKeywordSpotter, read_keywords

    state = _load_file(args.path)
    model_name, model_cfg = resolve_model_config(args.model, args.model_config, state)
    require_ctc(model_name)
    dev = torch.device(args.device or "cuda:{}".format(int(os.environ.get("LOCAL_RANK", "0"))))
    if dev.type == "cuda":
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(dev)
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(
        dict=args.dict, autoregressive=False, global_cmvn_stats_path=args.global_cmvn_stats_path, criterion_name="ctc_loss",
        non_lang_syms=args.non_lang_syms, bpe=args.bpe, sentencepiece_model=args.sentencepiece_model))
    d = task.target_dictionary
    keywords = read_keywords(args.keywords, d, d.bos(), args.threshold)  # before the model: a malformed file fails fast
    if not keywords:
        raise ValueError(f"{args.keywords}: no keywords")
    if args.streaming:  # the encoder options streaming cannot reproduce exactly: refused before the model is built
        from . import registry
        from .models.transformer.streaming_encoder import check_streamable

        cfg_cls = getattr(registry.MODEL_REGISTRY[model_name], "config_class", None)
        cfg0 = cfg_cls.from_dict(model_cfg) if cfg_cls is not None else None
        if cfg0 is None or not hasattr(cfg0, "encoder") or not hasattr(cfg0.encoder, "chunk_size"):
            raise NotImplementedError(f"--streaming needs a chunk-streaming transformer or causal-conformer encoder model, not {model_name}")
        check_streamable(cfg0)
    model = load_member(state, model_name, model_cfg, task, dev)

    scp = read_scp(args.wav_scp)
    utt_ids = list(scp.keys())
    waves, rates = read_waves([scp[u] for u in utt_ids])
    task.build_frontend(dev)
    fo = task.frontend.sample_rate
    spf = frame_seconds(model, task.frontend.frame_shift / task.frontend.sample_rate)
    spotter = CTCKeywordSpotter(d, keywords, max_streams=streams if args.streaming else 1, hold_frames=hold_frames(args.hold_ms, spf),
                                max_hits=args.max_hits)

    t0 = time.perf_counter()
    if args.long_form:  # one recording at a time: its windows' stitched log-probs, then the offline scan
        lf = LF.LongFormModel(model, LF.LongFormCTC(task, LF.plan_from_args(args, task.frontend, model), d.bos(), args.max_tokens,
                                                    args.batch_size))
        results = {}
        for i in range(args.shard_id, len(utt_ids), args.num_shards):
            out = lf(waves[i], rates[i])
            results[utt_ids[i]] = spotter.spot_lprobs(out["_lprobs"], out["src_lengths"][0])[0]
        LF.log_worst(lf, sys.stderr)
    elif args.streaming:
        mine = [i for i in range(len(utt_ids)) if i % args.num_shards == args.shard_id]
        results = spot_streaming(task, model, spotter, [utt_ids[i] for i in mine], [waves[i] for i in mine], spf, chunk_ms, streams,
                                 rates=[rates[i] for i in mine])
    else:
        results = {}
        batches = shard_batches(make_batches(utt_ids, lengths_at(waves, rates, fo), args.max_tokens, args.batch_size), args.num_shards,
                                args.shard_id)
        for ids in batches:
            sample = collate(ids, utt_ids, waves, dev, rates, fo)
            s = task.prepare_sample(sample, train=False)
            results.update(zip(sample["utt_ids"], spotter.spot(model, s)))  # (one host copy per batch)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    t_spot = time.perf_counter() - t0

    order = [u for u in utt_ids if u in results]  # wav.scp order
    out = sys.stdout if args.output == "-" else open(args.output, "w", encoding="utf-8")
    try:
        write_hits(results, order, spf, out)
    finally:
        if out is not sys.stdout:
            out.close()
    audio_s = sum(len(w) / float(r) for u, w, r in zip(utt_ids, waves, rates) if u in results)
    print("| {} hits of {} keywords in {} utterances in {:.1f}s, RTF {:.4f}{}".format(
        sum(len(results[u]) for u in order), len(keywords), len(order), t_spot, t_spot / max(audio_s, 1e-9),
        " ({} hits lost to --max-hits)".format(spotter.overflowed) if spotter.overflowed else ""), file=sys.stderr)
    return results


if __name__ == "__main__":
    main()
