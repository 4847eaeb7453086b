"""Golden fixtures of the recognizer's output side, written by running the REFERENCE's own code: the attention alignments
(`hypo["attention"]`) of fairseq's SequenceGenerator, and the result strings of espresso's Scorer.

Runs only where the reference checkout exists (the path setup of oracle/gen_golden.py); the fixtures it writes are
committed and reproduced bit for bit by re-running it:

    python tools/gen_golden_alignment.py

  tests/golden/ref_alignment_attention.npz  beam 3 (max_len_b 12 / 10) with the weights of ref_transformer_encdec_trained.npz
                                            (all three groups) and of ref_speech_lstm_tiny.npz (make_generation_fast_(need_attn=
                                            True)); per hypothesis: tokens, score and attention [S][len]
  tests/golden/ref_alignment_scorer.json    the ref_wer_scorer.json pairs through the reference Scorer, plain and with the WER
                                            output filter, without and with add_ordered_utt_list (a permutation): the strings of
                                            print_results, print_char_results and print_aligned_results
"""
import argparse
import json
import os
import shutil
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import gen_golden as GG  # noqa: E402  (stub packages + reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = GG.OUT


def _store(out, prefix, hyps):
    for bi, hl in enumerate(hyps):
        for hi, hyp in enumerate(hl):
            out[f"{prefix}::{bi}::{hi}::tokens"] = hyp["tokens"].numpy()
            out[f"{prefix}::{bi}::{hi}::score"] = np.array(float(hyp["score"]))
            out[f"{prefix}::{bi}::{hi}::attention"] = hyp["attention"].float().numpy()


def _speech_lstm(sd):
    from espresso.data.asr_dictionary import AsrDictionary
    from espresso.models.speech_lstm import SpeechLSTMModel, base_architecture

    args = argparse.Namespace(dropout=0.0, encoder_conv_channels="[64, 64, 16, 16]", encoder_rnn_hidden_size=32, encoder_rnn_layers=2,
                              encoder_rnn_residual=True, decoder_embed_dim=24, decoder_hidden_size=32, decoder_layers=2,
                              decoder_out_embed_dim=48, attention_dim=40, criterion_name="label_smoothed_cross_entropy_v2",
                              scheduled_sampling_probs=[1.0], start_scheduled_sampling_epoch=1, max_source_positions=3600,
                              max_target_positions=200)
    base_architecture(args)

    class T:
        feat_dim, feat_in_channels = 80, 1
        cfg = argparse.Namespace(num_batch_buckets=0)
    dic = AsrDictionary()
    for i in range(40 - len(dic) - 1):
        dic.add_symbol(f"t{i}")
    dic.add_symbol("<space>")
    T.target_dictionary = dic
    model = SpeechLSTMModel.build_model(args, T)
    model.load_state_dict(sd, strict=True)
    return model.eval(), dic


def attention_fixture(name="ref_alignment_attention"):
    from fairseq.sequence_generator import SequenceGenerator

    out = {}
    g = np.load(os.path.join(OUT, "ref_transformer_encdec_trained.npz"))
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}
    model, dic = GG._build_ref_encdec(64, 4, 128, 40)
    model.load_state_dict(sd, strict=True)
    model.eval()
    for gi in range(int(g["groups"])):
        feats, lens = torch.from_numpy(g[f"g{gi}::feats"]), torch.from_numpy(g[f"g{gi}::lengths"])
        gen = SequenceGenerator([model], dic, beam_size=3, max_len_a=0.0, max_len_b=12)
        with torch.no_grad():
            hyps = gen.generate([model], {"net_input": {"src_tokens": feats, "src_lengths": lens}})
        _store(out, f"encdec::g{gi}", hyps)
        print("encdec", gi, [[h["tokens"].tolist() for h in hl][:1] for hl in hyps], [tuple(hl[0]["attention"].shape) for hl in hyps])
    out["encdec::groups"] = np.array(int(g["groups"]))

    g = np.load(os.path.join(OUT, "ref_speech_lstm_tiny.npz"))
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}
    model, dic = _speech_lstm(sd)
    model.make_generation_fast_(need_attn=True)
    gen = SequenceGenerator([model], dic, beam_size=3, max_len_a=0.0, max_len_b=10)
    with torch.no_grad():
        hyps = gen.generate([model], {"net_input": {"src_tokens": torch.from_numpy(g["feats"]), "src_lengths": torch.from_numpy(g["lengths"])}})
    _store(out, "lstm", hyps)
    print("lstm", [[h["tokens"].tolist() for h in hl][:1] for hl in hyps], [tuple(hl[0]["attention"].shape) for hl in hyps])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)


def scorer_fixture(name="ref_alignment_scorer"):
    from espresso.data.asr_dictionary import AsrDictionary
    from espresso.tools.wer import Scorer

    pairs = json.load(open(os.path.join(OUT, "ref_wer_scorer.json")))["pairs"]
    os.makedirs(os.path.join(GG.HERE, "_ref"), exist_ok=True)
    tmp = tempfile.mkdtemp(dir=os.path.join(GG.HERE, "_ref"))
    with open(os.path.join(tmp, "dict.txt"), "w") as f:
        f.write("".join(f"{c} 1\n" for c in "abcdefghijklmnopqrstuvwxyz'") + "<space> 1\n<noise> 1\n<laugh> 1\n")
    with open(os.path.join(tmp, "nlsyms.txt"), "w") as f:
        f.write("<noise>\n<laugh>\n")
    with open(os.path.join(tmp, "filter"), "w") as f:
        f.write("#!/bin/sed -f\ns/uh //g\ns: um::g\n")
    order = [p[0] for p in pairs][::-1]
    order = order[1:] + order[:1]
    out = {"order": order}
    for tag, filt in (("plain", None), ("filtered", os.path.join(tmp, "filter"))):
        for ordered in (False, True):
            dic = AsrDictionary.load(os.path.join(tmp, "dict.txt"), f_non_lang_syms=os.path.join(tmp, "nlsyms.txt"))
            dic.build_bpe(argparse.Namespace(bpe="characters_asr"))
            sc = Scorer(dic, wer_output_filter=filt)
            for utt, ref, hyp in pairs:
                sc.add_prediction(utt, hyp)
                sc.add_evaluation(utt, ref, hyp)
            if ordered:
                sc.add_ordered_utt_list(order)
            key = tag + ("_ordered" if ordered else "")
            out[key] = {"results": sc.print_results(), "char_results": sc.print_char_results(),
                        "aligned_results": sc.print_aligned_results()}
    shutil.rmtree(tmp)
    with open(os.path.join(OUT, name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    print(out["filtered"]["aligned_results"])


if __name__ == "__main__":
    scorer_fixture()
    attention_fixture()
