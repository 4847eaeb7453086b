"""Golden fixtures of the multi-level (sub-word + word) LM shallow fusion, written by running the REFERENCE's own
MultiLevelLanguageModel (espresso/models/external_language_model.py:306-567) on seeded tiny models.

Runs only where the reference checkout exists (the path setup of oracle/gen_golden.py); the fixtures it writes are
committed and reproduced bit for bit by re-running it:

    python tools/gen_golden_multilevel.py

  tests/golden/ref_multilevel_lm_tiny.npz      scripted hypotheses over the character lexicon of the look-ahead fixture
                                               (torch seed 2024), variants (0.8, open), (0.5, closed), (0.8, closed, 1e-7)
  tests/golden/ref_multilevel_fusion_tiny.npz  the reference SequenceGenerator with lm_model=MultiLevelLanguageModel on the
                                               enc-dec weights of ref_transformer_encdec_tiny.npz (torch seed 2025), beam 3,
                                               lm_weight 0.5 and lm_weight 1.0 + eos_factor 1.5

The reference's forward() cannot run these cases as shipped, so `_reference_multilevel()` recompiles it once in memory with
one line changed (nothing else of the reference is touched):
  - the closed-vocabulary branch keeps `batch_is_child_mask` as a Python list and applies `~` to it (TypeError): the list
    becomes a bool tensor right after it is filled;
  - a step on which no row adds a sub-word score (every row after <space>, which the tiny beam search reaches) gathers with
    an index of shape [0, 1] and fails: the index is built as [b, 1, 1] with view(-1, 1, 1) instead of unsqueeze(-1),
    the same tensor whenever b > 0.
"""
import argparse
import os
import string
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import gen_golden as GG  # noqa: E402  (stub packages + reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = GG.OUT

WORDS = sorted(["A", "AB", "ABC", "ABD", "B", "BA", "BAD", "BADE", "CAB", "DAD", "DEAD", "DEED", "E", "EBB", "ACE", "BEAD"])
CHARS = ["A", "B", "C", "D", "E", "F"]
VARIANTS = (("w08_open", 0.8, 1.0, True), ("w05_closed", 0.5, 1.0, False), ("w08_closed_oov", 0.8, 1e-7, False))


def _lm(task, dim, hidden, is_wordlm, scale):
    from espresso.models.lstm_lm import LSTMLanguageModelEspresso, base_lm_architecture

    args = argparse.Namespace(decoder_embed_dim=dim, decoder_hidden_size=hidden, decoder_layers=2, decoder_out_embed_dim=hidden,
                              dropout=0.0, share_embed=False, is_wordlm=is_wordlm, criterion_name="cross_entropy",
                              tokens_per_sample=64)
    base_lm_architecture(args)
    lm = LSTMLanguageModelEspresso.build_model(args, task)
    with torch.no_grad():
        for p_ in lm.parameters():
            p_.mul_(scale)
    return lm.eval()


def _dicts(words, chars):
    from espresso.data.asr_dictionary import AsrDictionary

    wd = AsrDictionary()
    for w in words:
        wd.add_symbol(w)
    wd.space_index = -1
    sd_ = AsrDictionary()
    for c in chars:
        sd_.add_symbol(c)
    sd_.add_symbol("<space>")
    sd_.space_index = sd_.indices["<space>"]  # AsrDictionary.load sets it (asr_dictionary.py:86)
    return wd, sd_


def _lms(wd, sd_, sub_dim, sub_hidden, sub_scale, word_dim, word_hidden, word_scale):
    from espresso.tasks.speech_recognition import SpeechRecognitionEspressoTask  # noqa: F401 (isinstance check in build_model)

    class TS:
        pass
    TS.source_dictionary = TS.target_dictionary = sd_

    class TW:
        pass
    TW.source_dictionary = TW.target_dictionary = TW.word_dictionary = wd
    sub_lm = _lm(TS, sub_dim, sub_hidden, False, sub_scale)
    word_lm = _lm(TW, word_dim, word_hidden, True, word_scale)
    return sub_lm, word_lm


def _reference_multilevel():
    """The reference MultiLevelLanguageModel with its closed-vocabulary mask made a tensor (see the module docstring)."""
    import inspect
    import textwrap

    import espresso.models.external_language_model as E

    cls = E._MultiLevelLanguageModel
    if not getattr(cls, "_mask_fixed", False):
        src = textwrap.dedent(inspect.getsource(cls.forward))
        anchor = "token_idx = prev_output_tokens.new(token_idx).unsqueeze(-1)"
        assert src.count(anchor) == 1
        fixed = "token_idx = prev_output_tokens.new(token_idx).view(-1, 1, 1)"
        src = src.replace(anchor, fixed + "; batch_is_child_mask = torch.tensor(batch_is_child_mask, dtype=torch.bool)")
        ns = {}
        exec(compile(src, inspect.getsourcefile(cls), "exec"), E.__dict__, ns)
        cls.forward = ns["forward"]
        cls._mask_fixed = True
    return E.MultiLevelLanguageModel


def _tree_summary(ml):
    """The reference's lexical prefix tree (the object the multi-level decoder walks): node count including the root, and
    every word end as (space-joined sub-word ids of its path, word index)."""
    count, paths, widx = 0, [], []
    stack = [((), ml.decoder.lexroot)]
    while stack:
        path, node = stack.pop()
        count += 1
        if node.word_idx >= 0:
            paths.append(" ".join(str(i) for i in path))
            widx.append(node.word_idx)
        for sidx, ch in node.children.items():
            stack.append((path + (sidx,), ch))
    order = np.argsort(widx)
    return {"tree_num_nodes": np.array(count), "tree_word_end_paths": np.array(paths)[order], "tree_word_end_idx": np.array(widx)[order]}


def scripted_fixture(name="ref_multilevel_lm_tiny"):
    """4 hypotheses, 9 steps after <eos>: a word end before <space>, an OOV first letter, leaving the tree mid-word,
    <space> after <space>, <eos> after <space>, and a beam reorder that duplicates a row."""
    MultiLevelLanguageModel = _reference_multilevel()
    torch.manual_seed(2024)
    wd, sd_ = _dicts(WORDS, CHARS)
    sub_lm, word_lm = _lms(wd, sd_, 16, 24, 3.0, 16, 24, 4.0)
    sp, eos = sd_.space(), sd_.eos()
    ci = {c: sd_.index(c) for c in CHARS}
    base_script = [
        [ci["A"], ci["B"], sp, ci["B"], ci["A"], ci["D"], sp, ci["E"], ci["B"]],  # word end (AB) then <space>; BAD
        [ci["D"], ci["A"], ci["C"], sp, sp, ci["A"], ci["C"], ci["E"], sp],     # leaves the tree at C; <space> after <space>
        [ci["F"], ci["F"], sp, ci["C"], ci["A"], ci["B"], sp, ci["B"], sp],     # OOV first letter
        [ci["B"], ci["E"], ci["A"], ci["D"], sp, ci["D"], ci["E"], sp, eos],    # BEAD; a prefix that ends no word; <eos> after <space>
    ]
    B, steps = len(base_script), len(base_script[0])
    out = {}
    for tag, weight, oov, open_vocab in VARIANTS:
        ml = MultiLevelLanguageModel(word_lm, sub_lm, subwordlm_weight=weight, oov_penalty=oov, open_vocab=open_vocab)
        ml.eval()
        script = [list(s) for s in base_script]
        inc = {}
        toks = torch.full((B, 1), eos, dtype=torch.long)
        outs, orders, last_tok = [], [], []
        with torch.no_grad():
            for step in range(steps + 1):
                lp, _ = ml.decoder(toks, incremental_state=inc)
                outs.append(lp.squeeze(1).numpy().copy())
                last_tok.append(toks[:, -1].numpy().copy())
                if step == steps:
                    break
                order = torch.arange(B)
                if step == 4:  # hypotheses 0 and 3 swap places, 1 is duplicated over 2
                    order = torch.tensor([3, 1, 1, 0])
                    script = [script[int(i)] for i in order]
                    toks = toks.index_select(0, order)
                    ml.decoder.reorder_incremental_state_scripting(inc, order)  # the generator's call: every submodule
                orders.append(order.numpy())
                toks = torch.cat([toks, torch.tensor([[script[b][step]] for b in range(B)])], 1)
        out[f"{tag}::lprobs"] = np.stack(outs)
        if tag == VARIANTS[0][0]:
            out["tokens"], out["orders"], out["last_tok"] = toks.numpy(), np.stack(orders), np.stack(last_tok)
            out.update(_tree_summary(ml))
        print(name, tag, "lprobs", np.stack(outs).shape, "logzero entries", int((np.stack(outs) == -10.0).sum()))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), words=np.array(WORDS), chars=np.array(CHARS),
                        variants=np.array([v[0] for v in VARIANTS]), weights=np.array([v[1] for v in VARIANTS]),
                        oov_penalties=np.array([v[2] for v in VARIANTS]), open_vocab=np.array([v[3] for v in VARIANTS]), **out,
                        **{"sub::" + k: v.numpy() for k, v in sub_lm.state_dict().items()},
                        **{"word::" + k: v.numpy() for k, v in word_lm.state_dict().items()})


def fusion_symbols(V=40):
    """The 36 `t{i}` symbols of the tiny enc-dec dictionary renamed to single characters (weights depend on indices only)."""
    return list(string.ascii_uppercase + string.digits)[: V - 4]


def fusion_fixture(name="ref_multilevel_fusion_tiny"):
    """Beam search of the reference SequenceGenerator with lm_model=MultiLevelLanguageModel on the enc-dec weights of
    ref_transformer_encdec_tiny.npz; the word lexicon is drawn from the characters the enc-dec model emits most."""
    from espresso.data.asr_dictionary import AsrDictionary
    from fairseq.sequence_generator import SequenceGenerator

    MultiLevelLanguageModel = _reference_multilevel()
    g = np.load(os.path.join(OUT, "ref_transformer_encdec_tiny.npz"))
    V = 40
    syms = fusion_symbols(V)
    model, dic0 = GG._build_ref_encdec(64, 4, 128, V)
    dic = AsrDictionary()
    for s in syms:
        dic.add_symbol(s)
    dic.add_symbol("<space>")
    dic.space_index = dic.indices["<space>"]
    assert len(dic) == V and all(dic.index(s) == dic0.index(f"t{i}") for i, s in enumerate(syms))
    model.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")})
    model.eval()
    # the lexicon: every word of 1-3 letters over the characters the b3 beams of the enc-dec fixture start with
    torch.manual_seed(2025)
    beam_tok = sorted({int(t) for k in g.files if k.startswith("beam::b3::") and k.endswith("::tokens") for t in g[k]})
    letters = sorted({syms[t - 3] for t in beam_tok if 3 <= t < V - 1})
    rng = np.random.RandomState(2025)
    words = set(letters[:4])
    while len(words) < 40:
        n = int(rng.randint(2, 4))
        words.add("".join(rng.choice(letters, n)))
    words = sorted(words)
    wd = AsrDictionary()
    for w in words:
        wd.add_symbol(w)
    wd.space_index = -1
    sub_lm, word_lm = _lms(wd, dic, 24, 32, 3.0, 16, 24, 4.0)
    feats, lengths = torch.from_numpy(g["feats"]), torch.from_numpy(g["lengths"])
    beams = _tree_summary(MultiLevelLanguageModel(word_lm, sub_lm))
    for tag, kw in (("lm05", dict(beam_size=3, max_len_a=0.0, max_len_b=12, lm_weight=0.5)),
                    ("lm10_eosf", dict(beam_size=3, max_len_a=0.0, max_len_b=12, lm_weight=1.0, eos_factor=1.5))):
        ml = MultiLevelLanguageModel(word_lm, sub_lm, subwordlm_weight=0.8, oov_penalty=1.0, open_vocab=True)
        gen = SequenceGenerator([model], dic, lm_model=ml, **kw)
        hyps = gen.generate([model], {"net_input": {"src_tokens": feats, "src_lengths": lengths}})
        for bi, hl in enumerate(hyps):
            for hi, hyp in enumerate(hl):
                beams[f"beam::{tag}::{bi}::{hi}::tokens"] = hyp["tokens"].numpy()
                beams[f"beam::{tag}::{bi}::{hi}::score"] = np.array(float(hyp["score"]))
                beams[f"beam::{tag}::{bi}::{hi}::pos"] = hyp["positional_scores"].numpy()
        print(tag, [[h["tokens"].tolist() for h in hl] for hl in hyps], [[round(float(h["score"]), 3) for h in hl] for hl in hyps])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), symbols=np.array(syms), words=np.array(words), **beams,
                        **{"sub::" + k: v.numpy() for k, v in sub_lm.state_dict().items()},
                        **{"word::" + k: v.numpy() for k, v in word_lm.state_dict().items()})


if __name__ == "__main__":
    scripted_fixture()
    fusion_fixture()
