"""Keyword spotting on the device (csrc/kws.hip, tools/keyword_spotter.py, speech_kws): the kernel against its host twin
`ea_ctc_kws_host` bit for bit (which tests/test_keyword_spotting.py ties to the numpy reference), offline over packed
utterances in scattered slots, streamed in pieces of every kind, at real vocabulary widths, and through CTCKeywordSpotter and
the command line."""
import json

import numpy as np
import pytest
import torch

from tests import kws_ref
from tests.test_keyword_spotting import BLANK, assert_same, log_softmax, make_keywords, make_lprobs, tables

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from espresso_amd import _lib

    _lib.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _kw_tables(keywords, thetas, Lmax=None):
    tok, ln, tau = tables(keywords, thetas, Lmax)
    return (tok, ln, tau), tuple(_dev(a) for a in (tok, ln, tau))


def _pack(utts, ld, tail=4):
    """The utterances' rows one after the other (so another stream's rows follow every entry's) and `tail` NaN rows inside the
    allocation after the last: a look-ahead that is not clamped to the entry's rows changes the result instead of reading out
    of bounds.  Returns (x [rows][ld], row offsets)."""
    offs = np.cumsum([0] + [len(u) for u in utts])
    x = np.full((offs[-1] + tail, ld), np.nan, dtype=np.float32)
    for u, o in zip(utts, offs):
        x[o: o + len(u)] = u
    return x, [int(o) for o in offs[:-1]]


def _host_all(utts, host_tables, V, hold, max_hits):
    from espresso_amd import kernels as K

    outs = [K.ctc_kws_host(u, *host_tables, BLANK, hold, max_hits, V=V) for u in utts]
    return tuple(np.stack([o[i] for o in outs]) for i in range(4))


def _cpu(outputs):
    return tuple(t.cpu().numpy() for t in outputs)


# ------------------------------------------------------------------------------------------------ offline
OFFLINE = [  # (K, V, ld, long keyword)
    (1, 7, 11, False), (5, 7, 11, False), (9, 7, 11, False), (3, 70, 70, True)]


@pytest.mark.parametrize("Kk,V,ld,long_kw", OFFLINE)
@pytest.mark.parametrize("hold", [0, 3, 100])
def test_kernel_equals_host_twin_offline(Kk, V, ld, long_kw, hold):
    _need_gpu()
    from espresso_amd import kernels as K

    rng = np.random.default_rng(11 * Kk + V + hold)
    Ts = (0, 1, 7, 33, 70)
    if long_kw:  # V = 70: a keyword of 64 tokens planted in the longest utterance (one token per frame), beside two short ones
        y = [int(v) for v in rng.permutation(np.arange(1, V))[:64]]
        keywords = [y, y[3:6], [y[40]]]
        utts = []
        for T in Ts:
            z = rng.normal(0.0, 1.0, size=(T, V))
            for t in range(T if T == 70 else 0):  # (blank before and after the phrase)
                z[t, y[t - 2] if 2 <= t < 66 else BLANK] += 7.0
            u = np.full((T, ld), 9.0, dtype=np.float32)
            u[:, :V] = log_softmax(z).astype(np.float32)
            utts.append(u)
        thetas = [0.05, 0.5, 0.2]
    else:
        keywords = make_keywords(rng, Kk, V)
        utts = [make_lprobs(rng, T, V, ld) for T in Ts]
        thetas = [(0.05, 0.2, 0.5, 1.0)[int(i)] for i in rng.integers(0, 4, size=Kk)]
        if Kk == 9:
            keywords[4] = [3, BLANK, 2]  # inactive: it holds the blank
    max_hits, max_streams = 2, 8
    host_tables, dev_tables = _kw_tables(keywords, thetas)
    want = _host_all(utts, host_tables, V, hold, max_hits)
    if long_kw:
        assert want[3][4][0] == 1 and (want[0][4][0][0], want[1][4][0][0]) == (2, 65)  # the planted phrase, tight bounds

    x, offs = _pack(utts, ld)
    slots = [6, 1, 3, 0, 4]
    # a sixth entry with an out-of-range slot over valid rows: skipped
    meta = _dev(np.array([slots + [max_streams], list(Ts) + [7], offs + [offs[2]]], dtype=np.int32))
    state, nbytes = K.ctc_kws_state(max_streams, len(keywords), host_tables[0].shape[1], max_hits, DEV)
    state.copy_(torch.from_numpy(rng.integers(0, 256, size=(max_streams, nbytes), dtype=np.uint8)))
    before = state.cpu().numpy().copy()
    sl = _dev(np.array(slots, dtype=np.int32))
    K.ctc_kws_reset(state, sl, dev_tables, max_hits)
    rowmax = K.ctc_kws_step(_dev(x), meta, state, dev_tables, max_hits, V, BLANK, hold)
    got = _cpu(K.ctc_kws_hits(state, sl, dev_tables, max_hits, flush=True, clear=False))
    assert_same(got, want)
    rows = x.shape[0] - 4
    assert np.array_equal(rowmax.cpu().numpy()[:rows].view(np.int32), x[:rows, :V].max(axis=1).view(np.int32))
    after = state.cpu().numpy()
    for s in set(range(max_streams)) - set(slots):
        assert np.array_equal(after[s], before[s]), f"slot {s} is not listed and changed"
    # the frame counters: words [0] of the listed slots
    assert [int(after[s][:4].view(np.int32)[0]) for s in slots] == list(Ts)
    # a second read gives the same lists (flush found nothing open, nothing was cleared); clear empties them
    again = _cpu(K.ctc_kws_hits(state, sl, dev_tables, max_hits, flush=True, clear=True))
    assert_same(again, want)
    empty = _cpu(K.ctc_kws_hits(state, sl, dev_tables, max_hits))
    assert not empty[3].any() and (empty[0] == -1).all() and (empty[1] == -1).all()


def test_step_refuses_bad_arguments_and_skips_bad_entries():
    _need_gpu()
    from espresso_amd import kernels as K

    rng = np.random.default_rng(5)
    V, ld, T = 7, 11, 20
    keywords = make_keywords(rng, 3, V)
    host_tables, dev_tables = _kw_tables(keywords, [0.2] * 3)
    x, _ = _pack([make_lprobs(rng, T, V, ld)], ld)
    state, _ = K.ctc_kws_state(2, 3, host_tables[0].shape[1], 2, DEV)
    sl = _dev(np.array([0, 1], dtype=np.int32))
    K.ctc_kws_reset(state, sl, dev_tables, 2)
    fresh = state.cpu().numpy().copy()
    xd = _dev(x)
    # rows outside [0, total_rows): before the first, past the last; a negative count; a negative slot
    meta = _dev(np.array([[0, 1, 0, -1], [5, T, -3, 5], [-1, 10, 0, 0]], dtype=np.int32))
    K.ctc_kws_step(xd, meta, state, dev_tables, 2, V, BLANK, 3)
    assert np.array_equal(state.cpu().numpy(), fresh)
    for bad in (dict(V=12), dict(blank=7), dict(hold=-1)):
        kw = dict(V=V, blank=BLANK, hold=3)
        kw.update(bad)
        with pytest.raises((RuntimeError, AssertionError)):
            K.ctc_kws_step(xd, meta, state, dev_tables, 2, kw["V"], kw["blank"], kw["hold"])
    with pytest.raises(RuntimeError):
        K.ctc_kws_step(torch.from_numpy(x), meta.cpu(), state.cpu(), tuple(t.cpu() for t in dev_tables), 2, V, BLANK, 3)


# ------------------------------------------------------------------------------------------------ streamed
def _pieces(kind, T, rng):
    if kind == "ragged":
        out = []
        while sum(out) < T:
            out.append(min(int(rng.integers(0, 12)), T - sum(out)))
        return out + [0]
    n = int(kind)
    return [min(n, T - t) for t in range(0, T, n)]


@pytest.mark.parametrize("kind", ["1", "3", "7", "8", "9", "ragged"])
def test_chunking_invariance(kind):
    """The same frames in pieces of 1, of 3, of 7, 8 and 9 (shorter than, equal to and one past the look-ahead depth of 8) and
    of ragged counts with zero-frame pieces, two streams at once with different cuts: the polls (clear = 1 after every piece)
    plus the final flush are the offline lists."""
    _need_gpu()
    from espresso_amd import kernels as K

    rng = np.random.default_rng(3)
    V, ld, hold, max_hits = 7, 11, 3, 32
    Ts = (70, 61)
    utts = [make_lprobs(rng, T, V, ld) for T in Ts]
    keywords = make_keywords(rng, 6, V)
    thetas = [0.2, 0.5, 0.05, 0.2, 0.5, 0.2]
    host_tables, dev_tables = _kw_tables(keywords, thetas)
    want = _host_all(utts, host_tables, V, hold, max_hits)
    assert want[3].max() <= max_hits and want[3].sum() >= 20  # nothing overflows, so the polls can be concatenated
    cuts = [_pieces(kind, Ts[0], rng), _pieces("ragged" if kind == "ragged" else str(int(kind) + 1), Ts[1], rng)]
    # the cases the cuts must hold (conditions on the offline hits and the cuts alone): a hit that straddles a piece boundary
    # and a hold expiry (frame end + hold + 1) in a later piece than the hit's end
    bounds = np.cumsum(cuts[0])
    piece_of = lambda t: int(np.searchsorted(bounds, t, side="right"))  # noqa: E731
    hits0 = [(int(s), int(e)) for k in range(len(keywords)) for s, e in zip(want[0][0][k], want[1][0][k]) if s >= 0]
    assert any(piece_of(s) != piece_of(e) for s, e in hits0)
    assert any(e + hold + 1 < Ts[0] and piece_of(e) != piece_of(e + hold + 1) for s, e in hits0)

    slots = [2, 0]
    state, _ = K.ctc_kws_state(3, len(keywords), host_tables[0].shape[1], max_hits, DEV)
    sl = _dev(np.array(slots, dtype=np.int32))
    K.ctc_kws_reset(state, sl, dev_tables, max_hits)
    polled = [[[] for _ in keywords] for _ in Ts]

    def collect(outputs):
        st, en, sc, cnt = _cpu(outputs)
        for b in range(len(Ts)):
            for k in range(len(keywords)):
                assert cnt[b][k] <= max_hits
                polled[b][k] += [(int(st[b][k][h]), int(en[b][k][h]), sc[b][k][h]) for h in range(cnt[b][k])]

    pos = [0, 0]
    for j in range(max(len(c) for c in cuts)):
        n_new = [c[j] if j < len(c) else 0 for c in cuts]
        x, offs = _pack([u[p: p + n] for u, p, n in zip(utts, pos, n_new)], ld)
        meta = _dev(np.array([slots, n_new, offs], dtype=np.int32))
        K.ctc_kws_step(_dev(x), meta, state, dev_tables, max_hits, V, BLANK, hold)
        collect(K.ctc_kws_hits(state, sl, dev_tables, max_hits, clear=True))
        pos = [p + n for p, n in zip(pos, n_new)]
    assert pos == list(Ts)
    collect(K.ctc_kws_hits(state, sl, dev_tables, max_hits, flush=True, clear=True))
    got = kws_ref.as_arrays([(h, len(h)) for b in range(len(Ts)) for h in polled[b]], max_hits)
    assert_same(tuple(a.reshape(w.shape) for a, w in zip(got, want)), want)


# ------------------------------------------------------------------------------------------------ real vocabulary widths
@pytest.mark.parametrize("V,ld", [(5004, 5008), (5003, 5003), (5002, 5008)])
def test_real_vocabulary_widths(V, ld):
    """The row-max launch on its 16-byte path (ld a multiple of 4; with and without a tail of V) and on its 4-byte path, T = 40:
    rowmax is numpy's max bit for bit and the hits are the host's.  The keywords use the first and the last columns, and one
    of them is the greedy transcript of ea_ctc_greedy_decode, which must come back with e == 0."""
    _need_gpu()
    from espresso_amd import kernels as K

    rng = np.random.default_rng(V)
    T = 40
    special = [1, 2, 3, V - 3, V - 2, V - 1]
    z = rng.normal(0.0, 2.0, size=(T, V))
    peaks = [BLANK if rng.random() < 0.3 else special[int(rng.integers(0, 6))] for _ in range(T)]
    for t, p in enumerate(peaks):
        z[t, p] += 25.0
    x = np.full((T + 3, ld), np.nan, dtype=np.float32)
    x[:T, :] = 9.0
    x[:T, :V] = log_softmax(z).astype(np.float32)
    xd = _dev(x)
    tokens, out_len, _, _ = K.ctc_greedy_decode(xd[:T], torch.tensor([T], dtype=torch.int32, device=DEV), 1, T, V, BLANK, 0, ld=ld,
                                                want_align=False)
    greedy = tokens[0, : int(out_len[0])].tolist()
    assert 1 <= len(greedy) <= 64
    keywords = [greedy] + [[special[int(i)] for i in rng.integers(0, 6, size=int(rng.integers(1, 4)))] for _ in range(5)]
    thetas = [1.0, 0.5, 0.2, 0.05, 0.5, 0.2]
    host_tables, dev_tables = _kw_tables(keywords, thetas)
    max_hits, hold = 4, 2
    want = K.ctc_kws_host(x[:T], *host_tables, BLANK, hold, max_hits, V=V)
    state, _ = K.ctc_kws_state(1, len(keywords), host_tables[0].shape[1], max_hits, DEV)
    sl = _dev(np.array([0], dtype=np.int32))
    K.ctc_kws_reset(state, sl, dev_tables, max_hits)
    rowmax = K.ctc_kws_step(xd, _dev(np.array([[0], [T], [0]], dtype=np.int32)), state, dev_tables, max_hits, V, BLANK, hold)
    assert np.array_equal(rowmax.cpu().numpy()[:T].view(np.int32), x[:T, :V].max(axis=1).view(np.int32))
    got = _cpu(K.ctc_kws_hits(state, sl, dev_tables, max_hits, flush=True))
    assert_same(tuple(g[0] for g in got), want)
    nb = [t for t, p in enumerate(peaks) if p != BLANK]
    assert want[3][0] == 1 and (want[0][0][0], want[1][0][0]) == (nb[0], nb[-1]) and want[2][0][0] == 0.0
    assert want[3].sum() >= 4


# ------------------------------------------------------------------------------------------------ CTCKeywordSpotter
def _strip(hits):
    return [(h["keyword"], h["start"], h["end"], np.float32(h["score"]).view(np.int32).item()) for h in hits]


def test_spotter_offline_on_a_tiny_model_and_streamed():
    _need_gpu()
    from espresso_amd import kernels as K
    from espresso_amd.tools.keyword_spotter import CTCKeywordSpotter, keyword_lists, sort_hits
    from tests.gpu_checks import _Task, build_tiny_model, load_fixture, load_ref_state

    g, sd, _, _ = load_fixture("ref_conformer_ctc_tiny")
    model = build_tiny_model("conformer").to(DEV).eval()
    load_ref_state(model, sd)
    d = _Task(40).target_dictionary
    feats, lengths = torch.from_numpy(g["feats"]).to(DEV), torch.from_numpy(g["lengths"]).to(DEV)
    rng = np.random.default_rng(4)
    keywords = [([int(t)], 0.05) for t in range(5, 40)] + [([int(a), int(b)], 0.02) for a, b in rng.integers(5, 40, size=(12, 2))]
    hold, max_hits = 4, 64  # (max_hits: more than an utterance has frames, nothing overflows)
    sp = CTCKeywordSpotter(d, keywords, max_streams=len(g["lengths"]), hold_frames=hold, max_hits=max_hits)
    seen = {}
    orig = model.get_normalized_probs

    def grab(*a, **kw):  # the model's own log-probs: the tensor `spot` searches
        seen["lp"] = orig(*a, **kw)
        return seen["lp"]

    model.get_normalized_probs = grab
    try:
        with torch.no_grad():
            got = sp.spot(model, {"net_input": {"src_tokens": feats, "src_lengths": lengths}})
            enc = model(feats, lengths)["src_lengths"][0].cpu().numpy()
    finally:
        del model.get_normalized_probs
    lp = seen["lp"].transpose(0, 1).float().cpu().numpy()  # [B][T][V]
    V = lp.shape[2]
    assert V == len(d) and len(got) == lp.shape[0]
    tok, ln, tau = keyword_lists(sp.keywords)
    total = 0
    for b, hits in enumerate(got):
        ref = kws_ref.spot(lp[b][: int(enc[b])], [kw["tokens"] for kw in sp.keywords], tau, V, d.bos(), hold, max_hits)
        want = sort_hits([{"keyword": k, "start": s, "end": e, "score": float(sc)} for k, (hs, _) in enumerate(ref) for s, e, sc in hs])
        assert _strip(hits) == _strip(want)
        for h in hits:
            L = len(sp.keywords[h["keyword"]]["tokens"])
            assert h["text"] == sp.keywords[h["keyword"]]["text"] and h["confidence"] == pytest.approx(np.exp(h["score"] / L))
            assert 0.0 < h["confidence"] <= 1.0 and 0 <= h["start"] <= h["end"] < int(enc[b])
        total += len(hits)
    print("hits on the fixture model:", total)
    assert total >= 10 and sp.overflowed == 0

    # open / accept / poll / close over pieces == the offline search of the same frames (accept runs the log-softmax, so the
    # "logits" may be any rows: the model's log-probs scaled)
    B, T = lp.shape[:2]
    logits = (seen["lp"].transpose(0, 1).float() * 1.7).contiguous()  # [B][T][V]
    lens = [int(v) for v in enc]
    whole = K.log_softmax(logits.view(B * T, V), B * T, V, V).view(B, T, V)
    want = sp.spot_lprobs(whole, torch.tensor(lens, dtype=torch.int32, device=DEV))
    ids = [f"s{b}" for b in range(B)]
    live = list(ids)
    sp.open(live)
    polled = {sid: [] for sid in ids}
    pos = dict.fromkeys(ids, 0)
    step = 0
    while live:
        counts = [min((3, 0, 5, 1)[(step + i) % 4], lens[ids.index(sid)] - pos[sid]) for i, sid in enumerate(live)]
        rows = torch.cat([logits[ids.index(sid), pos[sid]: pos[sid] + c] for sid, c in zip(live, counts)])
        sp.accept(live, rows, counts)
        for sid, hits, c in zip(live, sp.poll(live), counts):
            polled[sid] += hits
            pos[sid] += c
        for sid in [s for s in live if pos[s] >= lens[ids.index(s)]]:
            polled[sid] += sp.close(sid)
            live.remove(sid)
        step += 1
    for b, sid in enumerate(ids):
        assert _strip(sort_hits(polled[sid])) == _strip(want[b])
    assert sum(len(w) for w in want) >= 10 and not sp.streams and sp.overflowed == 0


# ------------------------------------------------------------------------------------------------ the command line
def _write_keywords(path, n_tokens):
    lines = ["# every token alone, and a few pairs"] + [f"t{i}\t0.05" for i in range(n_tokens)] + ["t1 t2\t0.02", "t3 t3", "t0 t5 t7\t0.01"]
    path.write_text("\n".join(lines) + "\n")


def _check_output(path, results, order, spf):
    from espresso_amd.tools.keyword_spotter import output_line

    lines = path.read_text().splitlines()
    want = [output_line(u, h, spf) for u in order for h in sorted(results[u], key=lambda h: (h["start"], h["end"], h["keyword"]))]
    assert lines == want
    for l in lines:
        u, s, e, conf, text = l.split("\t")
        assert u in results and 0.0 <= float(s) < float(e) and 0.0 < float(conf) <= 1.0 and text


def test_cli_offline(tmp_path, capsys):
    _need_gpu()
    from espresso_amd import speech_kws
    from espresso_amd.data import audio_utils
    from tests.gpu_checks import load_fixture

    _, sd, _, _ = load_fixture("ref_conformer_ctc_tiny")
    (tmp_path / "dict.txt").write_text("".join(f"t{i} 1\n" for i in range(35)) + "<space> 1\n")  # (the fixture's V = 40)
    block = {"_name": "speech_transformer_encoder_model", "dropout": 0.0, "layernorm_embedding": True,
             "encoder": {"embed_dim": 64, "ffn_embed_dim": 128, "layers": 2, "attention_heads": 4, "normalize_before": True,
                         "relative_positional_embeddings": True, "layer_type": "conformer", "conv_channels": "[64, 64, 16, 16]"}}
    (tmp_path / "cfg.json").write_text(json.dumps(block))
    torch.save({"model": {"encoder." + k: v for k, v in sd.items()}}, str(tmp_path / "m.pt"))
    rng = np.random.default_rng(9)
    scp = []
    for u, sec in (("u0", 1.3), ("u1", 0.8), ("u2", 0.1)):
        p = str(tmp_path / f"{u}.wav")
        audio_utils.write_wav(p, np.round(rng.standard_normal(int(16000 * sec)) * 800).astype(np.float32))
        scp.append(f"{u} {p}\n")
    (tmp_path / "wav.scp").write_text("".join(scp))
    _write_keywords(tmp_path / "kw.txt", 35)
    base = ["--path", str(tmp_path / "m.pt"), "--model-config", str(tmp_path / "cfg.json"), "--dict", str(tmp_path / "dict.txt"),
            "--wav-scp", str(tmp_path / "wav.scp"), "--keywords", str(tmp_path / "kw.txt"), "--hold-ms", "120"]
    res = speech_kws.main(base + ["--output", str(tmp_path / "hits.txt"), "--batch-size", "2"])
    assert list(res) and set(res) == {"u0", "u1", "u2"} and sum(len(v) for v in res.values()) >= 5
    _check_output(tmp_path / "hits.txt", res, ["u0", "u1", "u2"], 0.04)  # 10 ms frame shift x the fixture's sub-sampling factor 4
    # without --output the hits go to stdout
    capsys.readouterr()
    res1 = speech_kws.main(base + ["--batch-size", "1"])
    out = [l for l in capsys.readouterr().out.splitlines() if l.count("\t") == 4]
    assert len(out) == sum(len(v) for v in res1.values()) >= 5


def test_cli_streaming(tmp_path, capsys, golden_dir):
    _need_gpu()
    from espresso_amd import speech_kws
    from tests.test_causal_conformer_streaming import _cli_checkpoint

    _, _, base = _cli_checkpoint(tmp_path, golden_dir, True)
    _write_keywords(tmp_path / "kw.txt", 20)
    capsys.readouterr()
    res = speech_kws.main(base + ["--keywords", str(tmp_path / "kw.txt"), "--hold-ms", "120", "--streaming", "--stream-chunk-ms", "170",
                                  "--streams", "2", "--output", str(tmp_path / "hits.txt")])
    out = capsys.readouterr().out.splitlines()
    order = ["flac", "utt0", "utt1"]
    assert set(res) == set(order) and sum(len(v) for v in res.values()) >= 5
    spf = 0.04
    _check_output(tmp_path / "hits.txt", res, order, spf)
    klines = [l.split("\t") for l in out if l.startswith("K-")]
    assert len(klines) == sum(len(v) for v in res.values())
    for u in order:
        mine = [l for l in klines if l[0] == "K-" + u]
        assert len(mine) == len(res[u])
        for l, h in zip(mine, res[u]):  # in the order in which they were reported
            assert (l[2], l[3], l[4], l[5]) == ("{:.3f}".format(h["start"] * spf), "{:.3f}".format((h["end"] + 1) * spf),
                                                "{:.4f}".format(h["confidence"]), h["text"])
            assert float(l[1]) + 0.05 >= float(l[3])  # reported no earlier than the audio that holds it was consumed
        reported = [float(l[1]) for l in mine]
        assert reported == sorted(reported)
