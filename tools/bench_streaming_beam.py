"""Cost of the streamed lexicon + n-gram CTC beam search (StreamingCTCLexiconBeamDecoder over ea_ctc_lexicon_stream_step)
next to the greedy StreamingCTCDecoder it replaces, to the offline search over the same frames, and as a share of a whole
streamed chunk.

Tables: those of tools/bench_ctc_lexicon_beam.py (V = 5004 in word-start mode, a generated trigram ARPA file, the lexicon that
spells every word as one word-start piece and 0-2 continuation pieces), beam `--beam`.

Per configuration (streams x chunk frames), on seeded peaked logits of `--frames` encoder frames per stream fed one chunk per
call, every stream ready in every call:
  step_ms / greedy_ms   median and p95 wall time of one `accept` (log-softmax included) ending in a device synchronise, of the
                        beam decoder and of StreamingCTCDecoder on the same rows;
  frame_us              the streamed search per frame and stream (all accepts of an utterance / frames), and offline_frame_us:
                        ea_ctc_lexicon_beam_search on the same [streams][frames] log-probs, one call (median of `--calls`);
  partial_ms, finish_ms one `partial` / `finish` + readback for all streams (median), at the end of the utterance;
with `--encoder`: enc_ms / dec_ms, the encoder (bench_streaming.py's model and loop) and the decoder of the same chunk timed
apart, and dec_share = dec / (enc + dec) of the medians.

Prints one JSON line per configuration, then one with the state bytes per stream.

`--endpoint`: instead, the streamed CTC prefix beam search (StreamingCTCPrefixBeamDecoder, no LM) per piece without times (the
baseline), with times, and endpointed (`accept` + the `endpoint` readback + the segment ends it asks for; rules of the command
line's defaults: 0.8 s / 5 s / 20 s), the three decoders fed the same pieces in the same loop; endpoint_ms is the probe and its
readback alone.  Then the bytes of device state per stream of a slot at the 20 s limit against one sized for 10 minutes."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(ts, name):
    return {f"{name}_median": round(float(np.median(ts)), 3), f"{name}_p95": round(float(np.percentile(ts, 95)), 3)}


def tables(args, dev):
    from espresso_amd.data.asr_dictionary import AsrDictionary
    from espresso_amd.models.ngram_lm import NGramLanguageModel
    from espresso_amd.tools.lexicon import LexiconTrie
    from tools.bench_ctc_lexicon_beam import write_arpa

    n_start = 2000
    d = AsrDictionary.from_symbols([f"▁p{i}" if i < n_start else f"p{i}" for i in range(args.V - 4)], enable_bos=True, add_space=False)
    assert len(d) == args.V
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "lm.arpa")
        words, _ = write_arpa(path, rng, args.words, args.bigrams, args.trigrams)
        ngram = NGramLanguageModel(path)
    ngram.to(dev)
    spell = {}
    for w in words:
        sp = (int(rng.integers(4, 4 + n_start)),) + tuple(int(t) for t in rng.integers(4 + n_start, args.V, rng.integers(0, 3)))
        spell.setdefault(sp, w)
    return d, ngram, LexiconTrie([(w, list(sp)) for sp, w in spell.items()], ngram, d)


def peaked_logits(streams, T, V, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    z = torch.randn(streams * T, V, generator=g) * 2.0
    peak = torch.where(torch.rand(streams * T, generator=g) < 0.5, torch.zeros(streams * T, dtype=torch.long),
                       torch.randint(1, V, (streams * T,), generator=g))
    z[torch.arange(streams * T), peak] += 8.0
    return z.view(streams, T, V).to(dev)


def run(streams, cs, args, dev, d, ngram, trie):
    from espresso_amd import kernels as K
    from espresso_amd.tools.ctc_lexicon_beam_search import CTCLexiconBeamSearchDecoder
    from espresso_amd.tools.streaming_ctc_decoder import StreamingCTCDecoder
    from espresso_amd.tools.streaming_ctc_lexicon_beam_decoder import StreamingCTCLexiconBeamDecoder

    T, V = args.frames, args.V
    z = peaked_logits(streams, T, V, dev)
    ids = list(range(streams))
    kw = dict(beam_size=args.beam, lm_weight=2.0, word_score=-1.0)
    beam = StreamingCTCLexiconBeamDecoder(d, ngram, trie, streams, T, **kw)
    greedy = StreamingCTCDecoder(d)
    pieces = [(a, min(T, a + cs)) for a in range(0, T, cs)]
    step, base, part, fin, utt = [], [], [], [], []
    for rnd in range(args.rounds + 1):  # round 0 warms every shape up
        beam.open(ids)
        greedy.open(ids)
        total = 0.0
        for a, b in pieces:
            rows = z[:, a:b].reshape(streams * (b - a), V)
            counts = [b - a] * streams
            t_beam, _ = _timed(lambda: beam.accept(ids, rows, counts))
            t_greedy, _ = _timed(lambda: greedy.accept(ids, rows, counts))
            total += t_beam
            if rnd:
                step.append(t_beam)
                base.append(t_greedy)
        t_part, _ = _timed(lambda: beam.partial(ids))
        t_fin, _ = _timed(lambda: [t.cpu() for t in beam.finish(ids)])
        if rnd:
            part.append(t_part)
            fin.append(t_fin)
            utt.append(total)
        for i in ids:
            beam.close(i)
            greedy.close(i)
    x = K.log_softmax(z.view(streams * T, V), streams * T, V, V).view(streams, T, V)
    off = CTCLexiconBeamSearchDecoder([None], d, ngram, trie, nbest=1, **kw)
    in_len = torch.full((streams,), T, dtype=torch.int32, device=dev)
    offline = [_timed(lambda: off.search(x, in_len))[0] for _ in range(args.calls + 1)][1:]
    res = {"streams": streams, "chunk_frames": cs, "frames": T, "beam": args.beam, "timed_accepts": len(step)}
    res.update(_stats(step, "step_ms"))
    res.update(_stats(base, "greedy_ms"))
    res["frame_us"] = round(float(np.median(utt)) * 1e3 / (streams * T), 3)
    res["offline_ms_median"] = round(float(np.median(offline)), 3)
    res["offline_frame_us"] = round(float(np.median(offline)) * 1e3 / (streams * T), 3)
    res["partial_ms_median"] = round(float(np.median(part)), 3)
    res["finish_ms_median"] = round(float(np.median(fin)), 3)
    if args.encoder:
        res.update(run_with_encoder(streams, cs, args, dev, beam))
    return res


def run_with_encoder(streams, cs, args, dev, beam):
    """bench_streaming.py's loop with the decoder behind the encoder: both timed per chunk."""
    from espresso_amd.models.transformer.streaming_encoder import StreamingEncoder
    from tools.bench_streaming import build

    model = build(cs, 3, 12, dev)
    T = args.frames * 4  # feature frames
    feats = torch.randn(streams, T, 80, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    se = StreamingEncoder(model, streams)
    ids = list(range(streams))
    piece = 4 * cs
    enc, dec = [], []
    with torch.no_grad():
        for rnd in range(2):
            se.open(ids)
            beam.open(ids)
            for a in range(0, T, piece):
                b = min(T, a + piece)
                t_enc, (y, counts) = _timed(lambda: se.accept_features(ids, feats[:, a:b], [b - a] * streams, b >= T))
                if y is None:
                    continue
                t_dec, _ = _timed(lambda: beam.accept(ids, y, counts))
                if rnd:
                    enc.append(t_enc)
                    dec.append(t_dec)
            se.close(ids)
            for i in ids:
                beam.close(i)
    e, dd = float(np.median(enc)), float(np.median(dec))
    return {"enc_ms_median": round(e, 3), "dec_ms_median": round(dd, 3), "dec_share": round(dd / (e + dd), 4), "chunks": len(enc)}


def run_endpoint(streams, cs, args, dev):
    from espresso_amd import kernels as K
    from espresso_amd.data.asr_dictionary import AsrDictionary
    from espresso_amd.tools.beam_common import EndpointRules
    from espresso_amd.tools.streaming_ctc_prefix_beam_decoder import StreamingCTCPrefixBeamDecoder

    T, V = args.frames, args.V
    d = AsrDictionary.from_symbols([f"p{i}" for i in range(V - 5)], enable_bos=True)
    assert len(d) == V
    x = K.log_softmax(peaked_logits(streams, T, V, dev).view(streams * T, V), streams * T, V, V).view(streams, T, V)
    ids = list(range(streams))
    rules = EndpointRules(20, 125, 500)  # 0.8 s, 5 s, 20 s in frames of 40 ms
    decs = {"step_ms": StreamingCTCPrefixBeamDecoder(d, streams, T, beam_size=args.beam),
            "times_step_ms": StreamingCTCPrefixBeamDecoder(d, streams, T, beam_size=args.beam, token_times=True),
            "endpointed_step_ms": StreamingCTCPrefixBeamDecoder(d, streams, rules.segment_frames + cs, beam_size=args.beam, endpoint=rules)}
    ts = {k: [] for k in decs}
    probe, ended = [], 0

    def endpointed(dec, rows, counts):
        n = 0
        for i in dec.room(ids, counts):
            dec.end_segment(i)
            n += 1
        dec.accept_lprobs(ids, rows, counts)
        for i, (rule, _, _, _) in zip(ids, dec.endpoint(ids)):
            if rule:
                dec.end_segment(i)
                n += 1
        return n

    for rnd in range(args.rounds + 1):  # round 0 warms every shape up
        for dec in decs.values():
            dec.open(ids)
        for a in range(0, T, cs):
            b = min(T, a + cs)
            rows, counts = x[:, a:b].reshape(streams * (b - a), V), [b - a] * streams
            for k, dec in decs.items():
                t, n = _timed((lambda: endpointed(dec, rows, counts)) if k == "endpointed_step_ms" else (lambda: dec.accept_lprobs(ids, rows, counts)))
                if rnd:
                    ts[k].append(t)
                    ended += n or 0
            t, _ = _timed(lambda: decs["endpointed_step_ms"].endpoint(ids))
            if rnd:
                probe.append(t)
        for dec in decs.values():
            for i in ids:
                dec.close(i)
    res = {"mode": "endpoint", "streams": streams, "chunk_frames": cs, "frames": T, "beam": args.beam, "timed_accepts": len(probe),
           "segments_ended": ended}
    for k, v in ts.items():
        res.update(_stats(v, k))
    res.update(_stats(probe, "endpoint_ms"))
    return res


def endpoint_state_bytes(lib_state, lib_times, beams, cs):
    """Device state per stream: a slot at the 20 s limit (500 frames + one piece, with its times slot) against the parent's slot
    for a 10-minute utterance (15000 frames, no times)."""
    return {"endpointed_20s_bytes_per_stream": {f"beam{b}": int(lib_state(500 + cs, b) + lib_times(500 + cs, b)) for b in beams},
            "slot_10min_bytes_per_stream": {f"beam{b}": int(lib_state(15000, b)) for b in beams}}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--streams", default="1,16,64")
    p.add_argument("--chunk-frames", default="16,32")
    p.add_argument("--frames", type=int, default=400, help="encoder frames per utterance (and max_frames of the decoder)")
    p.add_argument("--beam", type=int, default=10)
    p.add_argument("--V", type=int, default=5004)
    p.add_argument("--rounds", type=int, default=3, help="timed utterances per configuration, after one warm-up")
    p.add_argument("--calls", type=int, default=5, help="timed offline searches, after one warm-up")
    p.add_argument("--encoder", action="store_true", help="also time the decoder behind bench_streaming.py's encoder")
    p.add_argument("--endpoint", action="store_true", help="the CTC prefix beam search with and without endpointing instead (see above)")
    p.add_argument("--words", type=int, default=100000)
    p.add_argument("--bigrams", type=int, default=1500000)
    p.add_argument("--trigrams", type=int, default=2000000)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_streaming_beam.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    if args.endpoint:
        from espresso_amd import _lib

        for cs in [int(x) for x in args.chunk_frames.split(",")]:
            for s in [int(x) for x in args.streams.split(",")]:
                print(json.dumps(run_endpoint(s, cs, args, dev)), flush=True)
        L = _lib.lib()
        print(json.dumps(endpoint_state_bytes(L.ea_ctc_prefix_beam_stream_state_bytes, L.ea_ctc_prefix_beam_stream_times_state_bytes,
                                              (10, 64), 16)), flush=True)
        return
    d, ngram, trie = tables(args, dev)
    print(json.dumps({"lexicon_words": trie.num_words, "lexicon_nodes": len(trie), "V": args.V}), flush=True)
    for cs in [int(x) for x in args.chunk_frames.split(",")]:
        for s in [int(x) for x in args.streams.split(",")]:
            print(json.dumps(run(s, cs, args, dev, d, ngram, trie)), flush=True)
    from espresso_amd import _lib

    frames_30s = -(-(1 + (30 * 16000 - 400) // 160) // 4)  # encoder frames of 30 s: 25 ms / 10 ms fbank, sub-sampling 4
    print(json.dumps({"max_frames_30s": frames_30s,
                      "state_bytes_per_stream": {f"beam{b}": int(_lib.lib().ea_ctc_lexicon_stream_state_bytes(frames_30s, b))
                                                 for b in (10, 64)}}), flush=True)


if __name__ == "__main__":
    main()
