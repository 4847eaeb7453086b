"""Multi-level (sub-word + word) LM shallow fusion (espresso/models/external_language_model.py:306-567): the recognition CLI's
option surface, the fixture LMs and prefix tree on the CPU, and the HIP step / beam search against the reference's own
outputs (fixtures written by tools/gen_golden_multilevel.py) on the GPU."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
LOGZERO = -10.0
# (embed, hidden) of the fixtures' LSTM LMs, as tools/gen_golden_multilevel.py built them
DIMS = {"ref_multilevel_lm_tiny": {"sub": (16, 24), "word": (16, 24)}, "ref_multilevel_fusion_tiny": {"sub": (24, 32), "word": (16, 24)}}


def _load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def _dicts(g, subword_symbols):
    from espresso_amd.data.asr_dictionary import AsrDictionary

    wd = AsrDictionary.from_symbols([str(w) for w in g["words"]], enable_bos=False, add_space=False)
    sd = AsrDictionary.from_symbols([str(c) for c in g[subword_symbols]], enable_bos=False)
    return wd, sd


def _lms(name, g, wd, sd):
    """Both fixture LMs as LSTMLanguageModelEspresso (CPU), loaded strict."""
    from espresso_amd.models.lstm_lm import LSTMLanguageModelEspresso

    out = {}
    for part, dic, is_wordlm in (("sub", sd, False), ("word", wd, True)):
        class T:
            target_dictionary = source_dictionary = word_dictionary = dic
        e, h = DIMS[name][part]
        lm = LSTMLanguageModelEspresso.build_model(dict(arch="lstm_lm_wsj", decoder_embed_dim=e, decoder_hidden_size=h, decoder_layers=2,
                                                        decoder_out_embed_dim=h, dropout=0.0, share_embed=False, is_wordlm=is_wordlm), T)
        lm.load_state_dict({k[len(part) + 2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(part + "::")}, strict=True)
        out[part] = lm.eval()
    return out["sub"], out["word"]


def _args(*extra):
    from espresso_amd import speech_recognize as sr

    return sr.get_parser().parse_args(["--path", "m.pt", "--dict", "d.txt", "--wav-scp", "wav.scp", *extra])


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_cli_resolves_lm_fusion_mode():
    """`--lm-path sub.pt:word.pt` + --word-dict = multi-level (espresso/speech_recognize.py:130-148); one path keeps the old
    sub-word LM / look-ahead paths; the new options carry the reference's defaults."""
    from espresso_amd import speech_recognize as sr

    two = os.pathsep.join(["sub.pt", "word.pt"])
    a = _args("--lm-path", two, "--word-dict", "words.txt")
    assert sr.lm_fusion_mode(a) == "multilevel"
    assert (a.subwordlm_weight, a.word_lm_arch, a.disable_open_vocab, a.lm_arch) == (0.8, "lstm_lm_wsj", False, "lstm_lm_librispeech")
    a = _args("--lm-path", two, "--word-dict", "words.txt", "--subwordlm-weight", "0.5", "--disable-open-vocab",
              "--word-lm-arch", "lstm_wordlm_wsj")
    assert (a.subwordlm_weight, a.disable_open_vocab, a.word_lm_arch) == (0.5, True, "lstm_wordlm_wsj")
    assert sr.lm_fusion_mode(_args("--lm-path", "lm.pt", "--word-dict", "words.txt")) == "lookahead"
    assert sr.lm_fusion_mode(_args("--lm-path", "lm.pt")) == "subword"
    assert sr.lm_fusion_mode(_args()) is None
    with pytest.raises(ValueError):  # two LMs need the word dictionary
        sr.lm_fusion_mode(_args("--lm-path", two))


@pytest.mark.parametrize("search", ["ctc", "transducer_greedy", "transducer_beam"])
def test_cli_refuses_multilevel_outside_beam_search(search):
    """the transducer decoders fuse one LSTM LM and the CTC decoder none: two LMs stop the CLI before anything is loaded"""
    from espresso_amd import speech_recognize as sr

    argv = ["--path", "missing.pt", "--dict", "missing.txt", "--wav-scp", "missing.scp", "--search", search,
            "--lm-path", os.pathsep.join(["sub.pt", "word.pt"]), "--word-dict", "words.txt"]
    with pytest.raises(NotImplementedError, match="multi-level"):
        sr.main(argv)
    assert sr.lm_fusion_mode(_args("--search", search, "--lm-path", "lm.pt")) == "subword"


@pytest.mark.parametrize("name,symbols", [("ref_multilevel_lm_tiny", "chars"), ("ref_multilevel_fusion_tiny", "symbols")])
def test_fixture_lms_load_strict(name, symbols):
    g = _load(name)
    wd, sd = _dicts(g, symbols)
    sub_lm, word_lm = _lms(name, g, wd, sd)
    assert len(sub_lm.decoder.dictionary) == len(sd) and len(word_lm.decoder.dictionary) == len(wd)
    assert word_lm.is_wordlm and not sub_lm.is_wordlm


@pytest.mark.parametrize("name,symbols", [("ref_multilevel_lm_tiny", "chars"), ("ref_multilevel_fusion_tiny", "symbols")])
def test_prefix_tree_matches_reference_lexical_tree(name, symbols):
    """node count and every word end of the reference's lexical_prefix_tree (the tree the multi-level decoder walks)"""
    from espresso_amd.tools.tensorized_prefix_tree import TensorizedPrefixTree, tokenize

    g = _load(name)
    wd, sd = _dicts(g, symbols)
    t = TensorizedPrefixTree.build(wd, sd, lambda x: tokenize(x).split(" "))
    assert t.children.shape[0] - 1 == int(g["tree_num_nodes"])  # minus the "none" node
    children, prev_sub, word_idx = t.children.numpy(), t.prev_subword_idx.numpy(), t.word_idx.numpy()
    for path, widx in zip(g["tree_word_end_paths"], g["tree_word_end_idx"]):
        node = TensorizedPrefixTree.root_id
        for s in str(path).split():
            nxt = [c for c in children[node] if c != TensorizedPrefixTree.none_id and prev_sub[c] == int(s)]
            assert len(nxt) == 1, (path, s)
            node = nxt[0]
        assert word_idx[node] == widx, (path, widx)
    assert int((word_idx >= 0).sum()) == len(g["tree_word_end_idx"])


# ---------------------------------------------------------------------------------------------------------------- GPU
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from espresso_amd import _lib

    _lib.lib()  # the HIP library must be the thing under test


def _multilevel(name, symbols, **kw):
    from espresso_amd.models.external_language_model import MultiLevelLanguageModel

    g = _load(name)
    wd, sd = _dicts(g, symbols)
    sub_lm, word_lm = _lms(name, g, wd, sd)
    return g, sd, MultiLevelLanguageModel(word_lm.to(DEV).eval(), sub_lm.to(DEV).eval(), **kw)


def _run_script(g, ml, sync_check=False):
    last, orders = g["last_tok"], g["orders"]
    B = last.shape[1]
    toks = [torch.from_numpy(last[k]).to(DEV).view(B, 1) for k in range(last.shape[0])]
    parents = [None] + [torch.from_numpy(orders[k]).to(DEV) for k in range(orders.shape[0])]
    ml.tree.device_tensors(torch.device(DEV))  # the one-time host -> device copy of the tree
    state = ml.init_incremental(B, 1)
    torch.cuda.synchronize()
    outs = []
    if sync_check:
        torch.cuda.set_sync_debug_mode("error")
    try:
        for k in range(len(toks)):
            outs.append(ml.step(state, toks[k], k, parents[k]))
    finally:
        if sync_check:
            torch.cuda.set_sync_debug_mode("default")
    return [o.cpu().numpy() for o in outs]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_multilevel_step_vs_reference(variant):
    """both LSTM LMs in bf16 MFMA GEMMs, everything after them fp32: the fused log-probs within 2e-2 of the reference's fp32
    run along the scripted hypotheses, and exactly the same entries set to logzero (-10)"""
    _need_gpu()
    g = _load("ref_multilevel_lm_tiny")
    tag = str(g["variants"][variant])
    _, _, ml = _multilevel("ref_multilevel_lm_tiny", "chars", subwordlm_weight=float(g["weights"][variant]),
                           oov_penalty=float(g["oov_penalties"][variant]), open_vocab=bool(g["open_vocab"][variant]))
    ref = g[tag + "::lprobs"]  # [calls][B][Vs]
    got = np.stack(_run_script(g, ml))
    assert got.shape == ref.shape
    zero_ref, zero_got = ref == LOGZERO, got == LOGZERO
    assert np.array_equal(zero_ref, zero_got), (tag, np.argwhere(zero_ref != zero_got))
    err = float(np.abs(got - ref)[~zero_ref].max())
    print(tag, "max_abs", err, "logzero entries", int(zero_ref.sum()))
    assert err < 2e-2, (tag, err)


@pytest.mark.gpu
def test_multilevel_step_does_not_synchronise():
    """a whole scripted decode (first call, reorder with a duplicated row, closed vocabulary) under sync debug mode `error`"""
    _need_gpu()
    g = _load("ref_multilevel_lm_tiny")
    _, _, ml = _multilevel("ref_multilevel_lm_tiny", "chars", subwordlm_weight=0.5, open_vocab=False)
    outs = _run_script(g, ml, sync_check=True)
    assert np.allclose(np.stack(outs), g["w05_closed::lprobs"], atol=2e-2)


@pytest.mark.gpu
def test_multilevel_fusion_beam_search_vs_reference():
    """SequenceGenerator with lm_model=MultiLevelLanguageModel vs the reference generator: acoustic + lm_weight * multi-level
    log-probs along the reference's best hypotheses within 0.1 per position (bf16 models, as for the sub-word LM fusion test);
    hypotheses found by both generators carry scores within 3e-2"""
    _need_gpu()
    from espresso_amd.sequence_generator import SequenceGenerator
    from tests.gpu_checks import build_tiny_encdec

    g = _load("ref_transformer_encdec_tiny")
    gl, d, ml = _multilevel("ref_multilevel_fusion_tiny", "symbols", subwordlm_weight=0.8, oov_penalty=1.0, open_vocab=True)
    model = build_tiny_encdec().to(DEV)
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}
    model.load_state_dict(model.upgrade_state_dict_named(dict(sd), ""), strict=False)
    model.eval()
    sample = {"net_input": {"src_tokens": torch.from_numpy(g["feats"]).to(DEV), "src_lengths": torch.from_numpy(g["lengths"]).to(DEV)}}
    for tag, kw in (("lm05", dict(beam_size=3, max_len_a=0.0, max_len_b=12, lm_weight=0.5)),
                    ("lm10_eosf", dict(beam_size=3, max_len_a=0.0, max_len_b=12, lm_weight=1.0, eos_factor=1.5))):
        hyps = SequenceGenerator([model], d, lm_model=ml, **kw).generate([model], sample)
        common, score_err = 0, 0.0
        for b, hl in enumerate(hyps):
            refset, hi = {}, 0
            while f"beam::{tag}::{b}::{hi}::tokens" in gl.files:
                refset[tuple(gl[f"beam::{tag}::{b}::{hi}::tokens"].tolist())] = float(gl[f"beam::{tag}::{b}::{hi}::score"])
                hi += 1
            for h in hl:
                k = tuple(h["tokens"].tolist())
                if k in refset:
                    common += 1
                    score_err = max(score_err, abs(float(h["score"]) - refset[k]))
        print(tag, "hypotheses in the reference beams", common, "score_abs", score_err)
        assert common > 0, tag
        assert score_err < 3e-2, (tag, score_err)
    # force-decode the reference's best fused hypotheses: per-position fused scores against its positional scores
    tag, lmw = "lm05", 0.5
    toks = torch.stack([torch.from_numpy(gl[f"beam::{tag}::{b}::0::tokens"]) for b in range(3)]).to(DEV)
    ref_pos = torch.stack([torch.from_numpy(gl[f"beam::{tag}::{b}::0::pos"]) for b in range(3)])
    with torch.no_grad():
        enc_out = model.forward_encoder(sample["net_input"]["src_tokens"], sample["net_input"]["src_lengths"])
        st = model.decoder.init_incremental(enc_out, 3, 1)
        lst = ml.init_incremental(3, 1)
        cur = torch.full((3, 1), d.eos(), dtype=torch.long, device=DEV)
        got = []
        for step in range(toks.shape[1]):
            par = None if step == 0 else torch.arange(3, device=DEV)
            lp = model.decoder.step(st, cur, step, par) + lmw * ml.step(lst, cur, step, par)
            got.append(lp.gather(-1, toks[:, step:step + 1]).squeeze(-1).cpu())
            cur = torch.cat([cur, toks[:, step:step + 1]], 1)
    got = torch.stack(got, 1)
    err = float((got[:, :-1] - ref_pos[:, :-1]).abs().max())  # the last position is the forced <eos> at max_len
    print("forced_decode_pos_score_abs", err)
    assert err < 0.1, err
