"""The recognizer's output side: attention alignments (`hypo["attention"]`) collected on the device, the reference's result
files (--results-path) and attention plots (--print-alignment).

CPU: the Scorer's result strings against the reference's (tests/golden/ref_alignment_scorer.json), the results writer, CLI
parsing, and the generator's slab-plus-parent alignment bookkeeping against a torch replay of fairseq's `attn` buffer.
GPU (-m gpu): the three kernels against torch, alignments against the reference's SequenceGenerator
(tests/golden/ref_alignment_attention.npz), bit-identical searches with alignment on / off, and the CLI end to end."""
import contextlib
import io
import json
import math
import os

import numpy as np
import pytest
import torch

from espresso_amd.sequence_generator import HipBeamSearch, SequenceGenerator
from oracle.search_ref import ScriptedDecoder, ScriptedModel, TorchRefSearch, scripted_setup

DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ Scorer and result files
def _scorer(tmp_path, filt):
    from espresso_amd.data.asr_dictionary import AsrDictionary
    from espresso_amd.tools.wer import Scorer

    (tmp_path / "dict.txt").write_text("".join(f"{c} 1\n" for c in "abcdefghijklmnopqrstuvwxyz'") + "<space> 1\n<noise> 1\n<laugh> 1\n")
    (tmp_path / "nlsyms.txt").write_text("<noise>\n<laugh>\n")
    (tmp_path / "filter").write_text("#!/bin/sed -f\ns/uh //g\ns: um::g\n")
    d = AsrDictionary.load(str(tmp_path / "dict.txt"), f_non_lang_syms=str(tmp_path / "nlsyms.txt"))
    d.build_bpe("characters_asr")
    return Scorer(d, wer_output_filter=str(tmp_path / "filter") if filt else None)


def _filled(tmp_path, golden_dir, filt):
    pairs = json.load(open(os.path.join(golden_dir, "ref_wer_scorer.json")))["pairs"]
    sc = _scorer(tmp_path, filt)
    for utt, ref, hyp in pairs:
        sc.add_prediction(utt, hyp)
        sc.add_evaluation(utt, ref, hyp)
    return sc


@pytest.mark.parametrize("tag", ["plain", "filtered"])
@pytest.mark.parametrize("ordered", [False, True])
def test_scorer_result_strings_match_the_reference(tmp_path, golden_dir, tag, ordered):
    g = json.load(open(os.path.join(golden_dir, "ref_alignment_scorer.json")))
    sc = _filled(tmp_path, golden_dir, tag == "filtered")
    if ordered:
        sc.add_ordered_utt_list(list(g["order"]))
    want = g[tag + ("_ordered" if ordered else "")]
    assert sc.print_results() == want["results"]
    assert sc.print_char_results() == want["char_results"]
    assert sc.print_aligned_results() == want["aligned_results"]


def test_ordered_utt_list_from_text_files(tmp_path, golden_dir):
    g = json.load(open(os.path.join(golden_dir, "ref_alignment_scorer.json")))
    sc = _filled(tmp_path, golden_dir, False)
    order = list(g["order"])
    (tmp_path / "a").write_text("".join(f"{u} x y\n" for u in order[:2]))
    (tmp_path / "b").write_text("".join(f"{u} z\n" for u in order[2:]))
    sc.add_ordered_utt_list(str(tmp_path / "a"), str(tmp_path / "b"))
    assert sc.print_results() == g["plain_ordered"]["results"]


def test_aligned_print_empty_and_counts_unchanged(tmp_path, golden_dir):
    from espresso_amd.tools.utils import aligned_print

    assert aligned_print([], [], []) == "REF: \nHYP: \nSTP: \nWER: 0.00%\n\n"
    g = json.load(open(os.path.join(golden_dir, "ref_wer_scorer.json")))
    sc = _filled(tmp_path, golden_dir, False)
    last = g["plain"][-1]
    assert (sc.tot_word_error(), sc.tot_word_count(), sc.tot_char_error(), sc.tot_char_count()) == (
        last["word_error"], last["word_count"], last["char_error"], last["char_count"])


def test_results_writer_files_and_formats(tmp_path, golden_dir):
    from espresso_amd.speech_recognize import write_results

    g = json.load(open(os.path.join(golden_dir, "ref_alignment_scorer.json")))
    sc = _filled(tmp_path, golden_dir, True)
    sc.add_ordered_utt_list(list(g["order"]))
    out = tmp_path / "res"
    write_results(str(out), sc, has_target=True)
    assert sorted(os.listdir(out)) == ["aligned_results.txt", "cer", "decoded_char_results.txt", "decoded_results.txt", "wer"]
    assert (out / "decoded_results.txt").read_text() == g["filtered_ordered"]["results"]
    assert (out / "decoded_char_results.txt").read_text() == g["filtered_ordered"]["char_results"]
    assert (out / "aligned_results.txt").read_text() == g["filtered_ordered"]["aligned_results"]
    w, c = sc.summary_lines()
    assert (out / "wer").read_text() == w + "\n" and w.startswith("WER=") and w.endswith(f"#words={sc.tot_word_count()}")
    assert (out / "cer").read_text() == c + "\n" and c.startswith("CER=")
    # without references: no wer / cer / aligned_results.txt
    sc2 = _scorer(tmp_path, False)
    sc2.add_prediction("a", "h i")
    sc2.add_prediction("b", "y o")
    out2 = tmp_path / "res2"
    write_results(str(out2), sc2, has_target=False)
    assert sorted(os.listdir(out2)) == ["decoded_char_results.txt", "decoded_results.txt"]
    assert (out2 / "decoded_results.txt").read_text() == "a hi\nb yo\n"


def test_cli_options(tmp_path, monkeypatch):
    from espresso_amd import speech_recognize as sr

    base = ["--path", "x.pt", "--dict", "d.txt", "--wav-scp", "w.scp"]
    a = sr.get_parser().parse_args(base)
    assert a.print_alignment is None and a.results_path is None and a.wer_output_filter is None and a.non_lang_syms is None
    assert sr.get_parser().parse_args(base + ["--print-alignment"]).print_alignment == "hard"
    assert sr.get_parser().parse_args(base + ["--print-alignment", "soft"]).print_alignment == "soft"
    a = sr.get_parser().parse_args(base + ["--results-path", "r", "--wer-output-filter", "f", "--non-lang-syms", "n"])
    assert (a.results_path, a.wer_output_filter, a.non_lang_syms) == ("r", "f", "n")

    def no_load(*a, **k):
        raise AssertionError("loaded something")
    monkeypatch.setattr(sr, "_load_file", no_load)
    with pytest.raises(ValueError, match="--results-path"):
        sr.main(base + ["--print-alignment"])


def test_cli_filter_and_non_lang_syms_reach_the_scorer(tmp_path, monkeypatch):
    """Everything up to decoding runs on the host; the scorer main() returns carries the filter and the dictionary the
    non-language symbols (the model / front-end steps are replaced by stubs)."""
    from espresso_amd import speech_recognize as sr

    (tmp_path / "dict.txt").write_text("".join(f"{c} 1\n" for c in "abc") + "<space> 1\n<noise> 1\n")
    (tmp_path / "nl").write_text("<noise>\n")
    (tmp_path / "filter").write_text("s/uh //g\n")
    (tmp_path / "wav.scp").write_text("")
    seen = {}

    def fake_recognize(task, model, gen, stream, dictionary, refs, **kw):
        seen["scorer"] = kw["scorer"]
        return kw["scorer"], {}

    class FakeModel:
        def to(self, dev):
            return self

        def eval(self):
            return self

    monkeypatch.setattr(sr, "_load_file", lambda p: {})
    monkeypatch.setattr(sr, "resolve_model_config", lambda *a: ("speech_transformer_base", {}))
    monkeypatch.setattr(sr, "recognize", fake_recognize)
    monkeypatch.setattr(sr, "build_generator", lambda *a, **k: None)
    from espresso_amd import registry
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoTask

    class FakeCls:
        @staticmethod
        def build_model(cfg, task):
            m = FakeModel()
            m.load_state_dict = lambda sd, strict=True: None
            return m
    monkeypatch.setitem(registry.MODEL_REGISTRY, "speech_transformer_base", FakeCls)
    monkeypatch.setattr(SpeechRecognitionEspressoTask, "build_frontend", lambda self, dev: None)
    sr.main(["--path", "x.pt", "--dict", str(tmp_path / "dict.txt"), "--wav-scp", str(tmp_path / "wav.scp"), "--device", "cpu",
             "--wer-output-filter", str(tmp_path / "filter"), "--non-lang-syms", str(tmp_path / "nl")])
    sc = seen["scorer"]
    assert sc.word_filters == [["uh ", ""]]
    assert sc.dictionary.non_lang_syms == ["<noise>"]


# ------------------------------------------------------------------------------------------------ generator bookkeeping
class AttnScriptedDecoder(ScriptedDecoder):
    """The scripted decoder of oracle/search_ref.py that also emits seeded attention rows [N][H][S] (zero past each
    sentence's length) and logs what it emitted together with the parent vector it was given."""

    def __init__(self, beam_probs, vocab, eos, seed, H=2, S=5, lens=(5, 3)):
        super().__init__(beam_probs, vocab, eos)
        self.seed, self.H, self.S, self.lens = seed, H, S, lens
        self.log = []

    def step(self, st, tokens, step, parent):
        lp = super().step(st, tokens, step, parent)
        if st.get("need_attn"):
            N = tokens.shape[0]
            g = torch.Generator().manual_seed(self.seed * 1000 + step)
            x = torch.randn(N, self.H, self.S, generator=g)
            sent = st["row_sent"] if parent is None else st["row_sent"][parent.cpu()]
            st["row_sent"] = sent
            mask = torch.arange(self.S).view(1, 1, -1) < torch.tensor([self.lens[int(s)] for s in sent]).view(-1, 1, 1)
            p = torch.softmax(x.masked_fill(~mask, -math.inf), -1).to(tokens.device)
            st["attn"] = {"probs": p, "s_row": self.H * self.S, "s_frame": 1, "s_head": self.S, "heads": self.H, "frames": self.S}
            self.log.append((step, None if parent is None else parent.cpu().clone(), p.cpu()))
        return lp

    def init_incremental(self, encoder_out, bsz, beam):
        return {"row_sent": torch.arange(bsz).repeat_interleave(beam)}


class TorchAttnSearch(TorchRefSearch):
    """TorchRefSearch plus the alignment history in torch (the HIP search's attn_put / attn_backtrace restated)."""

    def attn_put(self, attn, dst, accumulate, div):
        p = attn["probs"]
        N, S, H = dst.shape[0], attn["frames"], attn["heads"]
        src = torch.as_strided(p, (N, H, S), (attn["s_row"], attn["s_head"], attn["s_frame"]))
        v = src[:, 0].clone()
        for h in range(1, H):
            v = v + src[:, h]
        v = v / float(H)
        if accumulate:
            v = dst[:, :S] + v
        dst[:, :S] = v if div == 1.0 else v / div

    def attn_backtrace(self, hist, parents, bbsz_idx, step):
        rows = bbsz_idx.clone()
        cols = []
        for k in range(step, -1, -1):
            cols.append(hist[k].index_select(0, rows))
            if k > 0:
                rows = parents[k].long().index_select(0, rows)
        return torch.stack(cols[::-1], -1)  # [n][S][step+1]


def fairseq_replay(decoders, beam, finals):
    """fairseq's `attn` buffer (sequence_generator.py): column step+1 <- the ensemble mean of the head-mean attention; at a
    finalisation attn.index_select(0, bbsz_idx)[:, :, 1:step+2]; after the step, finished sentences are dropped
    (attn.view(bsz, -1)[batch_idxs]) and the rows reordered by active_bbsz_idx.  The parent vectors the decoders were given
    are decomposed back into batch_idxs / active_bbsz_idx.  Returns the expected attention of every (step, bbsz_idx)."""
    logs = [d.log for d in decoders]
    n_steps = len(logs[0])
    S = logs[0][0][2].shape[2]
    attn = None
    expect = {}
    fin = {}
    for step, idx in finals:
        fin.setdefault(step, []).append(idx)
    for k in range(n_steps):
        parent = logs[0][k][1]
        if k > 0:
            bsz_prev = attn.shape[0] // beam
            kept = sorted(set((parent // beam).tolist()))
            batch_idxs = torch.tensor(kept)
            corr = batch_idxs - torch.arange(len(kept))
            new_bsz = len(kept)
            active = parent - corr.repeat_interleave(beam) * beam
            if new_bsz < bsz_prev:
                attn = attn.view(bsz_prev, -1)[batch_idxs].view(new_bsz * beam, S, -1)
            attn[:, :, : k + 1] = attn[:, :, : k + 1].index_select(0, active)
        avg = None
        for lg in logs:
            p = lg[k][2]
            v = p[:, 0].clone()
            for h in range(1, p.shape[1]):
                v = v + p[:, h]
            v = v / float(p.shape[1])
            avg = v if avg is None else avg + v
        avg = avg / float(len(decoders)) if len(decoders) > 1 else avg
        if attn is None:
            attn = torch.zeros(avg.shape[0], S, n_steps + 2)
        attn[:, :, k + 1] = avg
        for idx in fin.get(k, []):
            expect[(k, tuple(idx.tolist()))] = attn.index_select(0, idx)[:, :, 1: k + 2]
    return expect


class RecordingAttnSearch(TorchAttnSearch):
    def __init__(self):
        self.calls = []

    def attn_backtrace(self, hist, parents, bbsz_idx, step):
        out = super().attn_backtrace(hist, parents, bbsz_idx, step)
        self.calls.append((step, bbsz_idx.cpu().clone(), out.cpu().clone()))
        return out


def _attn_setup(members, device, search, **kw):
    d, w1, w2, sample, model = scripted_setup()
    dec0 = model.decoder
    decs = [AttnScriptedDecoder(dec0.beam_probs, dec0.vocab, dec0.eos, seed=7 + i) for i in range(members)]
    models = [ScriptedModel(dc) for dc in decs]
    sample = {"net_input": {k: v.to(device) for k, v in sample["net_input"].items()}}
    gen = SequenceGenerator(models, d, beam_size=2, search=search, **kw)
    return decs, gen.generate(models, sample)


@pytest.mark.parametrize("members", [1, 2])
def test_slab_and_parent_alignments_equal_fairseq_attn_buffer(members):
    search = RecordingAttnSearch()
    decs, hypos = _attn_setup(members, "cpu", search, print_alignment=True)
    finals = [(step, idx) for step, idx, _ in search.calls]
    assert len({s for s, _ in finals}) > 1  # sentences / hypotheses finish at different steps
    expect = fairseq_replay(decs, 2, finals)
    for step, idx, got in search.calls:
        want = expect[(step, tuple(idx.tolist()))]
        assert got.shape == want.shape == (idx.numel(), 5, step + 1)
        assert torch.equal(got, want), (step, idx)
    n = 0
    for sent in hypos:
        for h in sent:
            a = h["attention"]
            assert a is not None and a.shape == (5, len(h["tokens"]))
            assert any(a.data_ptr() == o.data_ptr() or torch.equal(a, o[i]) for _, _, o in search.calls for i in range(o.shape[0]))
            n += 1
    assert n == 4


def test_alignment_off_by_default_and_on_through_need_attn():
    search = RecordingAttnSearch()
    decs, hypos = _attn_setup(1, "cpu", search)
    assert not search.calls and not decs[0].log and all(h["attention"] is None for s in hypos for h in s)
    # a decoder's need_attn (make_generation_fast_ / prepare_for_inference_) switches it on
    d, w1, w2, sample, model = scripted_setup()
    dec = AttnScriptedDecoder(model.decoder.beam_probs, model.decoder.vocab, model.decoder.eos, seed=3)
    dec.need_attn = True
    m = ScriptedModel(dec)
    hy = SequenceGenerator([m], d, beam_size=2, search=TorchAttnSearch()).generate([m], sample)
    assert all(h["attention"] is not None for s in hy for h in s)
    # the tokens and scores do not depend on it
    _, plain = _attn_setup(1, "cpu", TorchAttnSearch())
    for s0, s1 in zip(plain, hy):
        assert [h["tokens"].tolist() for h in s0] == [h["tokens"].tolist() for h in s1]
        assert [float(h["score"]) for h in s0] == [float(h["score"]) for h in s1]


def test_model_need_attn_hooks():
    from tests.gpu_checks import build_tiny_encdec, build_tiny_speech_lstm

    for m in (build_tiny_encdec(), build_tiny_speech_lstm()):
        assert not getattr(m.decoder, "need_attn", False)
        m.make_generation_fast_(need_attn=True)
        assert m.decoder.need_attn
        m.prepare_for_inference_({"generation": {"print_alignment": None}})
        assert not m.decoder.need_attn
        m.prepare_for_inference_({"generation": {"print_alignment": "hard"}})
        assert m.decoder.need_attn


# ------------------------------------------------------------------------------------------------ GPU: kernels
def _bf(x):
    return x.to(torch.bfloat16)


@pytest.mark.gpu
@pytest.mark.parametrize("dh,H,dedup", [(64, 4, True), (64, 2, False), (32, 4, True), (48, 2, True)])
def test_decode_attention_probs_kernel(dh, H, dedup):
    from espresso_amd import kernels as K

    torch.manual_seed(dh + H)
    C = dh * H
    B, beam, S = 3, 4, 77
    N = B * beam
    rows = B if dedup else N
    lens = torch.tensor([77, 40, 5][:rows] if dedup else [77 - 6 * i for i in range(N)], dtype=torch.int32, device=DEV)
    kv = _bf(torch.randn(rows, S, 2 * C, device=DEV))
    q = _bf(torch.randn(N, C, device=DEV) * 0.4)
    kv_row = torch.arange(B, device=DEV, dtype=torch.int32).repeat_interleave(beam) if dedup else None
    out_ref = K.decode_attention(q, kv, None, kv_row, lens, N, H, dh, S * 2 * C, 2 * C, 0, C, S)
    out, probs = K.decode_attention_probs(q, kv, None, kv_row, lens, N, H, dh, S * 2 * C, 2 * C, 0, C, S)
    assert torch.equal(out.view(torch.int16), out_ref.view(torch.int16))
    r = kv_row.long() if dedup else torch.arange(N, device=DEV)
    k = kv[r, :, :C].float().view(N, S, H, dh)
    sc = torch.einsum("nhd,nshd->nhs", q.float().view(N, H, dh), k)
    L = lens.long()[r]
    valid = torch.arange(S, device=DEV).view(1, 1, -1) < L.view(-1, 1, 1)
    want = torch.softmax(sc.masked_fill(~valid, -math.inf), -1)
    assert float((probs - want).abs().max()) < 2e-6
    assert bool((probs[~valid.expand_as(probs)] == 0).all())


@pytest.mark.gpu
def test_attn_history_put_and_backtrace_kernels():
    from espresso_amd import kernels as K

    torch.manual_seed(5)
    N, H, S = 12, 4, 37
    src = torch.rand(N, H, S, device=DEV)  # transformer layout [N][H][S]
    tm = torch.rand(S, N, device=DEV)  # speech_lstm's time-major [T][N], H = 1
    th = TorchAttnSearch()
    # the torch side runs on the CPU: torch's GPU division by a Python scalar multiplies by the reciprocal, the kernel divides
    for accumulate, div in ((False, 1.0), (True, 3.0)):
        init = torch.rand(N, S + 3, device=DEV)
        a, b = init.clone(), init.cpu()
        desc = {"probs": src.cpu(), "s_row": H * S, "s_frame": 1, "s_head": S, "heads": H, "frames": S}
        K.attn_history_put(src, H * S, 1, S, N, H, S, a[:, :S], accumulate, div)
        th.attn_put(desc, b[:, :S], accumulate, div)
        assert torch.equal(a.cpu(), b)
        desc = {"probs": tm.cpu(), "s_row": 1, "s_frame": N, "s_head": 0, "heads": 1, "frames": S}
        K.attn_history_put(tm, 1, N, 0, N, 1, S, a[:, :S], accumulate, div)
        th.attn_put(desc, b[:, :S], accumulate, div)
        assert torch.equal(a.cpu(), b)
    steps, rows, S = 70, 12, 83
    hist = torch.rand(steps, rows, S, device=DEV)
    parents = torch.randint(0, rows, (steps, rows), dtype=torch.int32, device=DEV)
    for step in (0, 1, 63, 64, 69):
        idx = torch.tensor([3, 0, 11, 3], device=DEV)
        got = K.attn_backtrace(hist, parents, idx, step, S)
        assert torch.equal(got, th.attn_backtrace(hist, parents, idx, step))


@pytest.mark.gpu
@pytest.mark.parametrize("members", [1, 2])
def test_hip_alignment_bookkeeping_matches_the_torch_search(members):
    class Rec(HipBeamSearch):
        calls = []

        def attn_backtrace(self, hist, parents, bbsz_idx, step):
            out = super().attn_backtrace(hist, parents, bbsz_idx, step)
            Rec.calls.append((step, bbsz_idx.cpu().clone(), out.cpu().clone()))
            return out
    search = RecordingAttnSearch()
    _attn_setup(members, "cpu", search, print_alignment=True)
    _attn_setup(members, DEV, Rec(), print_alignment=True)
    assert len(Rec.calls) == len(search.calls)
    for (s0, i0, o0), (s1, i1, o1) in zip(search.calls, Rec.calls):
        assert s0 == s1 and torch.equal(i0, i1) and torch.equal(o0, o1)


# ------------------------------------------------------------------------------------------------ GPU: against the reference
def _ref_hyps(g, prefix, b):
    out, hi = [], 0
    while f"{prefix}::{b}::{hi}::tokens" in g.files:
        out.append((g[f"{prefix}::{b}::{hi}::tokens"].tolist(), g[f"{prefix}::{b}::{hi}::attention"]))
        hi += 1
    return out


# Largest |attention - reference| over the columns of hypotheses whose tokens equal the reference's.  Measured on an MI355X:
# enc-dec 1.45e-2 (25 hypotheses, arg-max frame equal in 194 / 194 columns with a reference margin > 0.05), speech_lstm 1.3e-3
# (7 hypotheses; its random-weight attention is flat: no column has a margin > 0.05).  The bound leaves room for the bf16 operands of the decoder (bf16 GEMM
# inputs carry ~2^-9 relative error per operand; attention logits of the trained model span ~10, so probabilities move by
# up to ~1e-2 where the softmax is not saturated).
ATTN_BOUND = 2e-2


def _compare_alignments(hyps, g, prefix, enc_lens):
    n_cmp, worst, n_arg, n_arg_ok = 0, 0.0, 0, 0
    for b, hl in enumerate(hyps):
        ref = {tuple(t): a for t, a in _ref_hyps(g, prefix, b)}
        L = int(enc_lens[b])
        for h in hl:
            a = h["attention"].float().cpu().numpy()
            S = a.shape[0]
            col = a[:L].sum(0)
            assert np.abs(col - 1).max() < 1e-5
            assert (a[L:] == 0).all()
            r = ref.get(tuple(h["tokens"].tolist()))
            if r is None:
                continue
            assert r.shape == a.shape == (S, len(h["tokens"]))
            worst = max(worst, float(np.abs(a - r).max()))
            n_cmp += 1
            srt = np.sort(r[:L], axis=0)
            margin = srt[-1] - srt[-2]
            for j in np.nonzero(margin > 0.05)[0]:
                n_arg += 1
                n_arg_ok += int(a[:L, j].argmax() == r[:L, j].argmax())
    return n_cmp, worst, n_arg, n_arg_ok


@pytest.mark.gpu
def test_encdec_alignments_match_the_reference(golden_dir):
    from tests.gpu_checks import _TaskAR, build_tiny_encdec

    g = np.load(os.path.join(golden_dir, "ref_alignment_attention.npz"))
    t = np.load(os.path.join(golden_dir, "ref_transformer_encdec_trained.npz"))
    sd = {k[4:]: torch.from_numpy(t[k]) for k in t.files if k.startswith("sd::")}
    model = build_tiny_encdec(embed_dim=64, heads=4, ffn=128).to(DEV)
    model.load_state_dict(model.upgrade_state_dict_named(dict(sd), ""), strict=False)
    model.eval()
    d = _TaskAR(40).target_dictionary
    tot = [0, 0.0, 0, 0]
    for gi in range(int(g["encdec::groups"])):
        feats, lens = torch.from_numpy(t[f"g{gi}::feats"]).to(DEV), torch.from_numpy(t[f"g{gi}::lengths"]).to(DEV)
        sample = {"net_input": {"src_tokens": feats, "src_lengths": lens}}
        kw = dict(beam_size=3, max_len_a=0.0, max_len_b=12)
        off = SequenceGenerator([model], d, **kw).generate([model], sample)
        on = SequenceGenerator([model], d, print_alignment=True, **kw).generate([model], sample)
        for h0, h1 in zip(off, on):
            assert [x["tokens"].tolist() for x in h0] == [x["tokens"].tolist() for x in h1]
            assert [float(x["score"]) for x in h0] == [float(x["score"]) for x in h1]
            assert all(x["attention"] is None for x in h0)
        enc_lens = model.encoder.output_lengths(lens).tolist()
        r = _compare_alignments(on, g, f"encdec::g{gi}", enc_lens)
        tot = [tot[0] + r[0], max(tot[1], r[1]), tot[2] + r[2], tot[3] + r[3]]
    print("enc-dec alignments: compared", tot[0], "max abs", tot[1], "argmax", tot[3], "/", tot[2])
    assert tot[0] >= 9 and tot[1] < ATTN_BOUND and tot[2] > 0 and tot[3] == tot[2]


@pytest.mark.gpu
def test_speech_lstm_alignments_match_the_reference(golden_dir):
    from tests.gpu_checks import _TaskAR, build_tiny_speech_lstm

    g = np.load(os.path.join(golden_dir, "ref_alignment_attention.npz"))
    t = np.load(os.path.join(golden_dir, "ref_speech_lstm_tiny.npz"))
    sd = {k[4:]: torch.from_numpy(t[k]) for k in t.files if k.startswith("sd::")}
    model = build_tiny_speech_lstm().to(DEV)
    model.load_state_dict(model.upgrade_state_dict_named(dict(sd), ""), strict=False)
    model.eval()
    d = _TaskAR(40).target_dictionary
    lens = torch.from_numpy(t["lengths"]).to(DEV)
    sample = {"net_input": {"src_tokens": torch.from_numpy(t["feats"]).to(DEV), "src_lengths": lens}}
    kw = dict(beam_size=3, max_len_a=0.0, max_len_b=10)
    off = SequenceGenerator([model], d, **kw).generate([model], sample)
    model.make_generation_fast_(need_attn=True)
    on = SequenceGenerator([model], d, **kw).generate([model], sample)
    model.make_generation_fast_(need_attn=False)
    for h0, h1 in zip(off, on):
        assert [x["tokens"].tolist() for x in h0] == [x["tokens"].tolist() for x in h1]
        assert [float(x["score"]) for x in h0] == [float(x["score"]) for x in h1]
    r = _compare_alignments(on, g, "lstm", model.encoder.output_lengths(lens).tolist())
    print("speech_lstm alignments: compared", r[0], "max abs", r[1], "argmax", r[3], "/", r[2])
    assert r[0] >= 1 and r[1] < ATTN_BOUND and r[3] == r[2]


@pytest.mark.gpu
def test_alignment_off_never_calls_the_new_kernels(monkeypatch):
    from espresso_amd import kernels as K
    from tests.gpu_checks import _TaskAR, build_tiny_encdec

    def boom(*a, **k):
        raise AssertionError("alignment kernel called with alignment off")
    for name in ("decode_attention_probs", "attn_history_put", "attn_backtrace"):
        monkeypatch.setattr(K, name, boom)
    torch.manual_seed(1)
    model = build_tiny_encdec().to(DEV).eval()
    d = _TaskAR(40).target_dictionary
    feats = torch.randn(2, 60, 80, device=DEV)
    lens = torch.tensor([60, 41], device=DEV)
    hy = SequenceGenerator([model], d, beam_size=3, max_len_a=0.0, max_len_b=6).generate(
        [model], {"net_input": {"src_tokens": feats, "src_lengths": lens}})
    assert all(h["attention"] is None for s in hy for h in s)


# ------------------------------------------------------------------------------------------------ GPU: CLI end to end
def _cli_fixture(tmp_path, ctc):
    from espresso_amd import registry
    from espresso_amd.data import audio_utils
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask

    (tmp_path / "dict.txt").write_text("".join(f"{c} 1\n" for c in "abcdefghij") + "<space> 1\n")
    enc = {"embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4, "normalize_before": True,
           "relative_positional_embeddings": True, "layer_type": "transformer", "conv_channels": "[64, 64, 16, 16]"}
    if ctc:
        block = {"_name": "speech_transformer_encoder_model", "encoder": enc, "dropout": 0.0}
    else:
        block = {"_name": "speech_transformer_base", "encoder": enc, "dropout": 0.0, "layernorm_embedding": True,
                 "decoder": {"embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4, "normalize_before": True,
                             "input_dim": 64, "output_dim": 64}}
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(
        dict=str(tmp_path / "dict.txt"), autoregressive=not ctc, criterion_name="ctc_loss" if ctc else "label_smoothed_cross_entropy_v2"))
    cls = registry.MODEL_REGISTRY[block["_name"]]
    torch.manual_seed(11)
    m = cls.build_model(cls.config_class.from_dict(block), task)
    torch.save({"model": m.state_dict()}, str(tmp_path / "m.pt"))
    (tmp_path / "cfg.json").write_text(json.dumps(block))
    rng = np.random.default_rng(4)
    utts = [("u3", 0.9), ("u1", 0.5), ("u2", 1.2), ("u0", 0.7)]
    scp, text = [], []
    for u, sec in utts:
        x = np.round(rng.standard_normal(int(16000 * sec)) * 800).astype(np.float32)
        p = str(tmp_path / f"{u}.wav")
        audio_utils.write_wav(p, x)
        scp.append(f"{u} {p}\n")
        text.append(f"{u} a b <space> c\n")
    (tmp_path / "wav.scp").write_text("".join(scp))
    (tmp_path / "text").write_text("".join(text))
    return [u for u, _ in utts]


@pytest.mark.gpu
@pytest.mark.parametrize("ctc", [False, True])
def test_cli_results_path_and_print_alignment(tmp_path, ctc):
    from espresso_amd import speech_recognize

    order = _cli_fixture(tmp_path, ctc)
    res = tmp_path / "res"
    args = ["--path", str(tmp_path / "m.pt"), "--model-config", str(tmp_path / "cfg.json"), "--dict", str(tmp_path / "dict.txt"),
            "--wav-scp", str(tmp_path / "wav.scp"), "--text", str(tmp_path / "text"), "--beam", "3", "--batch-size", "2",
            "--results-path", str(res), "--print-alignment", "--search", "ctc" if ctc else "beam"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        scorer = speech_recognize.main(args)
    files = sorted(os.listdir(res))
    assert {"decode.log", "decoded_results.txt", "decoded_char_results.txt", "wer", "cer", "aligned_results.txt"} <= set(files)
    assert [l.split()[0] for l in (res / "decoded_results.txt").read_text().splitlines()] == order
    w = scorer.summary_lines()[0]
    assert (res / "wer").read_text() == w + "\n"
    out = buf.getvalue()
    assert w in out and "H-" not in out and "T-" not in out
    log = (res / "decode.log").read_text()
    assert sum(l.startswith("H-") for l in log.splitlines()) == len(order) and w in log
    if ctc:
        assert "attn_plots" not in files
        return
    pytest.importorskip("matplotlib")
    plots = sorted(os.listdir(res / "attn_plots"))
    assert plots == sorted(f"{u}.pdf" for u in order)
    for p in plots:
        assert (res / "attn_plots" / p).read_bytes()[:4] == b"%PDF"
