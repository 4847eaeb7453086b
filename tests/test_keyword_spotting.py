"""Keyword spotting (csrc/kws.hip, tools/keyword_spotter.py, speech_kws) -- the tests that need no GPU.

The rule is restated in numpy in tests/kws_ref.py from the header's text.  Here: known answers worked by hand, the host twin
`ea_ctc_kws_host` (the same __host__ __device__ functions as the kernel) against the fp32 reference bit for bit over seeded random
cases that reach every rare branch, the greedy transcript as a keyword, the fp32 reference against the fp64 one under the derived
rounding bound, and the host logic (keyword files, CLI refusals, hit order, frames to seconds).  The kernel itself is tested in
tests/test_keyword_spotting_gpu.py."""
import math

import numpy as np
import pytest

from tests import kws_ref

BLANK = 0
THETAS = (0.05, 0.2, 0.5, 1.0)


def log_softmax(z):
    z = z - z.max(axis=-1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=-1, keepdims=True))


def make_lprobs(rng, T, V, ld, sigma=2.0):
    """fp32 log-probs [T][ld] of logits N(0, sigma) over V; the columns from V on hold 9.0, above every log-prob: a row maximum
    that reads them is wrong."""
    x = np.full((T, ld), 9.0, dtype=np.float32)
    x[:, :V] = log_softmax(rng.normal(0.0, sigma, size=(T, V))).astype(np.float32)
    return x


def make_keywords(rng, n, V, Lmax=6):
    """n distinct-or-not token lists of 1 .. Lmax tokens over 1 .. V-1; every third one repeats a token on purpose."""
    out = []
    for i in range(n):
        L = int(rng.integers(1, Lmax + 1))
        y = [int(v) for v in rng.integers(1, V, size=L)]
        if i % 3 == 2 and L >= 2:
            j = int(rng.integers(1, L))
            y[j] = y[j - 1]
        out.append(y)
    return out


def tables(keywords, thetas, Lmax=None):
    Lmax = max(len(y) for y in keywords) if Lmax is None else Lmax
    tok = np.zeros((len(keywords), Lmax), dtype=np.int32)
    for k, y in enumerate(keywords):
        tok[k, : len(y)] = y
    ln = np.array([len(y) for y in keywords], dtype=np.int32)
    tau = np.array([kws_ref.tau_of(th, len(y)) for y, th in zip(keywords, thetas)], dtype=np.float32)
    return tok, ln, tau


def random_case(seed):
    """One seeded case: T 0 .. 70, V 7 with ld 7 or 11, five keywords of 1 .. 6 tokens (repeats among them), theta from THETAS,
    hold 0, 3 or past the end, max_hits 2 (so that lists overflow)."""
    rng = np.random.default_rng(1000 + seed)
    T = int(rng.integers(0, 71))
    V, ld = 7, (7, 11)[seed % 2]
    x = make_lprobs(rng, T, V, ld)
    kws = make_keywords(rng, 5, V)
    thetas = [THETAS[int(i)] for i in rng.integers(0, len(THETAS), size=len(kws))]
    hold = (0, 3, T + 5)[seed % 3]
    return dict(x=x, T=T, V=V, ld=ld, keywords=kws, thetas=thetas, hold=hold, max_hits=2)


N_CASES = 200


@pytest.fixture(scope="module")
def cases():
    """The random cases with their fp32 and fp64 reference results and the fp32 run's branch counters, computed once."""
    counters = dict.fromkeys(kws_ref.COUNTERS, 0)
    out = []
    for seed in range(N_CASES):
        c = random_case(seed)
        _, _, tau = tables(c["keywords"], c["thetas"])
        c["ref32"] = kws_ref.spot(c["x"], c["keywords"], tau, c["V"], BLANK, c["hold"], c["max_hits"], np.float32, counters)
        c["ref64"] = kws_ref.spot(c["x"], c["keywords"], tau, c["V"], BLANK, c["hold"], c["max_hits"], np.float64)
        out.append(c)
    return out, counters


def host(x, keywords, thetas, V, hold, max_hits, Lmax=None, blank=BLANK):
    from espresso_amd import kernels as K

    tok, ln, tau = tables(keywords, thetas, Lmax)
    return K.ctc_kws_host(x, tok, ln, tau, blank, hold, max_hits, V=V)


def assert_same(got, want):
    """starts, ends, counts and the scores' bits"""
    for g, w, name in zip(got, want, ("starts", "ends", "scores", "counts")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), name


# ------------------------------------------------------------------------------------------------ known answers
def table(rows, V=4):
    """Log-probs from per-frame probabilities (rows of V numbers)."""
    return np.log(np.asarray(rows, dtype=np.float64)).astype(np.float32)


A, B = 1, 2
HAND = table([[0.7, 0.1, 0.1, 0.1],   # 0: blank
              [0.1, 0.7, 0.1, 0.1],   # 1: a
              [0.1, 0.7, 0.1, 0.1],   # 2: a
              [0.1, 0.7, 0.1, 0.1],   # 3: a
              [0.7, 0.1, 0.1, 0.1],   # 4: blank
              [0.1, 0.7, 0.1, 0.1],   # 5: a
              [0.1, 0.1, 0.7, 0.1]])  # 6: b


@pytest.mark.parametrize("run", ["ref", "host"])
def test_known_answers(run):
    def spot(x, keywords, thetas, hold, max_hits=4, V=4):
        if run == "host":
            return host(x, keywords, thetas, V, hold, max_hits)
        _, _, tau = tables(keywords, thetas)
        return kws_ref.as_arrays(kws_ref.spot(x, keywords, tau, V, BLANK, hold, max_hits), max_hits)

    # a single token over a three-frame run reports [first, last]; the second run is a hit of its own (hold 0)
    st, en, sc, cnt = spot(HAND, [[A]], [0.9], hold=0)
    assert cnt[0] == 2 and list(st[0][:2]) == [1, 5] and list(en[0][:2]) == [3, 5] and np.all(sc[0][:2] == 0.0)
    # with a hold that covers the gap the second run is a candidate of its own too (it starts after the open hit's end)
    st, en, _, cnt = spot(HAND, [[A]], [0.9], hold=10)
    assert cnt[0] == 2 and list(st[0][:2]) == [1, 5] and list(en[0][:2]) == [3, 5]
    # `a a` needs the blank between the two: frames 1 .. 3 alone are one `a`; the hit runs from the first run to frame 5
    st, en, sc, cnt = spot(HAND, [[A, A]], [0.9], hold=10)
    assert cnt[0] == 1 and (st[0][0], en[0][0]) == (1, 5) and sc[0][0] == 0.0
    st, en, _, cnt = spot(HAND[:4], [[A, A]], [0.5], hold=10)
    assert cnt[0] == 0 and st[0][0] == -1 and en[0][0] == -1
    # `a b`: the skip move (no blank needed), tight bounds: the latest start on the greedy path is NOT taken, the tie stays
    st, en, sc, cnt = spot(HAND, [[A, B]], [0.9], hold=10)
    assert cnt[0] == 1 and (st[0][0], en[0][0]) == (5, 6) and sc[0][0] == 0.0
    # T < L and T == 0 give nothing
    _, _, _, cnt = spot(HAND[5:6], [[A, B]], [0.05], hold=0)
    assert cnt[0] == 0
    st, en, sc, cnt = spot(HAND[:0], [[A], [A, B]], [0.05, 0.05], hold=0)
    assert list(cnt) == [0, 0] and np.all(st == -1) and np.all(en == -1) and np.all(sc == 0.0)
    # max_hits 1: the second hit is counted, not stored
    st, en, _, cnt = spot(HAND, [[A]], [0.9], hold=0, max_hits=1)
    assert cnt[0] == 2 and list(st[0]) == [1] and list(en[0]) == [3]


def test_confidence_below_threshold_is_not_reported():
    # frame 1 gives `a` 0.3 against a greedy 0.4: exp(e / 1) = 0.75
    x = table([[0.4, 0.3, 0.2, 0.1]])
    for theta, n in ((0.7, 1), (0.8, 0)):
        _, _, sc, cnt = host(x, [[A]], [theta], 4, 0, 2)
        assert cnt[0] == n
        if n:
            assert math.exp(sc[0][0]) == pytest.approx(0.75, rel=1e-6)


def test_inactive_keywords_and_bad_arguments():
    from espresso_amd import kernels as K

    tok = np.array([[A, 0], [A, BLANK], [A, 7], [A, -1]], dtype=np.int32)
    ln = np.array([3, 2, 2, 2], dtype=np.int32)  # a length past Lmax, the blank, two ids outside [0, V)
    tau = np.full(4, -100.0, dtype=np.float32)
    _, _, _, cnt = K.ctc_kws_host(HAND, tok, ln, tau, BLANK, 0, 2)
    assert list(cnt) == [0, 0, 0, 0]
    assert K.ctc_kws_state_bytes(0, 4, 2) == K.ctc_kws_state_bytes(1, 0, 2) == K.ctc_kws_state_bytes(1, 65, 2) == 0
    assert K.ctc_kws_state_bytes(1, 4, 0) == 0
    assert K.ctc_kws_state_bytes(3, 4, 2) == 4 * (2 + 3 * (16 + 6 + 6))
    assert K.ctc_kws_state_bytes(1, 64, 1) == 4 * (2 + 256 + 6 + 3 + 1)  # (a keyword's words are rounded up to even)
    for bad in (dict(blank=4), dict(hold=-1), dict(max_hits=0)):
        kw = dict(blank=BLANK, hold=0, max_hits=2)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            K.ctc_kws_host(HAND, tok, ln, tau, **kw)


# ------------------------------------------------------------------------------------------------ host twin == fp32 reference
def test_host_twin_equals_fp32_reference_bit_for_bit(cases):
    cs, counters = cases
    hits = 0
    for c in cs:
        got = host(c["x"], c["keywords"], c["thetas"], c["V"], c["hold"], c["max_hits"])
        assert_same(got, kws_ref.as_arrays(c["ref32"], c["max_hits"]))
        hits += int(got[3].sum())
    print("hits:", hits, "keyword lists:", sum(len(c["keywords"]) for c in cs), "counters:", counters)
    assert all(counters[k] > 0 for k in kws_ref.COUNTERS), counters
    assert hits >= 300


def test_host_twin_long_keyword_wide_vocabulary():
    """V = 70 with a keyword of 64 tokens (every lane of the kernel's wave), planted with runs and blanks, beside short ones."""
    rng = np.random.default_rng(7)
    V, T = 70, 150
    y = [int(v) for v in rng.permutation(np.arange(1, V))[:64]]
    y[10] = y[9]  # a repeat: needs its blank
    path = []
    for u, tok in enumerate(y):
        if u > 0 and (y[u - 1] == tok or u % 5 == 0):
            path.append(BLANK)
        path += [tok] * (2 if u % 7 == 0 else 1)
    path = [BLANK] * 3 + path + [BLANK] * 4
    assert len(path) <= T
    z = rng.normal(0.0, 1.0, size=(T, V))
    for t, v in enumerate(path):
        z[t, v] += 6.0
    x = np.full((T, V + 2), 9.0, dtype=np.float32)
    x[:, :V] = log_softmax(z).astype(np.float32)
    kws = [y, y[:3], [y[5]]]
    thetas = [0.5, 0.5, 0.2]
    got = host(x, kws, thetas, V, 3, 2)
    _, _, tau = tables(kws, thetas)
    assert_same(got, kws_ref.as_arrays(kws_ref.spot(x, kws, tau, V, BLANK, 3, 2), 2))
    first = 3
    last = max(t for t, v in enumerate(path) if v != BLANK)
    assert got[3][0] == 1 and (got[0][0][0], got[1][0][0]) == (first, last)


# ------------------------------------------------------------------------------------------------ the greedy transcript
@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("hold", [0, 1000])
def test_greedy_transcript_is_found_with_e_zero(seed, hold):
    rng = np.random.default_rng(50 + seed)
    T, V = 60, 7
    x = make_lprobs(rng, T, V, V, sigma=3.0)
    x[rng.random(T) < 0.4, BLANK] += 8.0  # blank runs; x stays a table of finite scores, which is all the rule needs
    srt = np.sort(x, axis=1)
    assert np.all(srt[:, -1] > srt[:, -2])  # no argmax ties
    am = x.argmax(axis=1)
    y = [int(v) for t, v in enumerate(am) if v != BLANK and (t == 0 or am[t - 1] != v)]
    assert 1 <= len(y) <= 64
    nb = np.nonzero(am != BLANK)[0]
    for run in ("host", "ref"):
        if run == "host":
            st, en, sc, cnt = host(x, [y], [1.0], V, hold, 2)
        else:
            st, en, sc, cnt = kws_ref.as_arrays(kws_ref.spot(x, [y], [kws_ref.tau_of(1.0, len(y))], V, BLANK, hold, 2), 2)
        assert cnt[0] == 1
        assert (st[0][0], en[0][0]) == (nb[0], nb[-1])
        assert sc[0][0] == 0.0


# ------------------------------------------------------------------------------------------------ fp32 against fp64
def test_fp32_reference_against_fp64(cases):
    cs, _ = cases
    lists = differ = compared = 0
    for c in cs:
        for (h32, n32), (h64, n64) in zip(c["ref32"], c["ref64"]):
            lists += 1
            if n32 != n64 or [(s, e) for s, e, _ in h32] != [(s, e) for s, e, _ in h64]:
                differ += 1
                continue
            for (s, e, e32), (_, _, e64) in zip(h32, h64):
                D = e - s + 1
                assert abs(float(e32) - float(e64)) <= (D + 1) * 2.0 ** -24 * abs(float(e64)), (s, e, e32, e64)
                compared += 1
    print("keyword lists:", lists, "with different (start, end) lists:", differ, "hits compared:", compared)
    assert lists == 5 * N_CASES and differ <= lists // 100 and compared >= 300


# ------------------------------------------------------------------------------------------------ host logic
def _dict(tmp_path, symbols):
    from espresso_amd.data.asr_dictionary import AsrDictionary

    p = tmp_path / "dict.txt"
    p.write_text("".join(f"{s} 1\n" for s in symbols))
    return AsrDictionary.load(str(p), enable_bos=True)


def test_read_keywords_and_its_refusals(tmp_path):
    from espresso_amd.tools.keyword_spotter import keyword_tau, read_keywords

    d = _dict(tmp_path, ["x", "y", "z"])
    f = tmp_path / "kw.txt"
    f.write_text("# names\nx y\n\ny z x\t0.25\nz\t1\n")
    kws = read_keywords(str(f), d, d.bos(), 0.5)
    assert [k["tokens"] for k in kws] == [[d.index("x"), d.index("y")], [d.index("y"), d.index("z"), d.index("x")], [d.index("z")]]
    assert [k["threshold"] for k in kws] == [0.5, 0.25, 1.0] and [k["text"] for k in kws] == ["x y", "y z x", "z"]
    assert keyword_tau(3, 0.25) == np.float32(3) * np.float32(math.log(0.25)) and keyword_tau(1, 1.0) == 0.0

    def refused(text, match):
        f.write_text(text)
        with pytest.raises(ValueError, match=match):
            read_keywords(str(f), d, d.bos(), 0.5)

    refused("x\nx y\t1.5\n", r"kw.txt:2: threshold 1.5 is above 1")
    refused("x\n\n" + " ".join(["x"] * 65) + "\n", r"kw.txt:3: .* has 65 tokens, more than 64")
    refused("x y\n# c\nz\nx y\t0.3\n", r"kw.txt:4: phrase 'x y' repeats line 1")
    refused("x\ny\t0\n", r"kw.txt:2: .*not positive")
    refused("x\nq\n", r"kw.txt:2: .*<unk>")
    refused("x <s>\n", r"blank")
    f.write_text(" ".join(["x"] * 64) + "\n")
    assert len(read_keywords(str(f), d, d.bos(), 0.5)[0]["tokens"]) == 64
    with pytest.raises(ValueError, match="default threshold"):
        read_keywords(str(f), d, d.bos(), 1.5)


def test_spotter_refuses_bad_keywords(tmp_path):
    from espresso_amd.tools.keyword_spotter import CTCKeywordSpotter

    d = _dict(tmp_path, ["x", "y"])
    x = d.index("x")
    for kws, match in (([([x] * 65, 0.5)], "tokens"), ([([d.bos()], 0.5)], "blank"), ([([x], 1.5)], "threshold"), ([], "no keywords"),
                       ([([len(d)], 0.5)], "outside the dictionary")):
        with pytest.raises(ValueError, match=match):
            CTCKeywordSpotter(d, kws, 2, 5)
    with pytest.raises(ValueError, match="hold_frames"):
        CTCKeywordSpotter(d, [([x], 0.5)], 2, -1)
    sp = CTCKeywordSpotter(d, [([x, d.index("y")], 0.5)], 2, 5)
    assert sp.keywords[0]["text"] == "x y" and sp.Lmax == 2 and sp.blank == d.bos()


def test_hit_sorting_and_seconds():
    from espresso_amd.speech_kws import hold_frames
    from espresso_amd.tools.keyword_spotter import hit_seconds, output_line, sort_hits

    hits = [{"keyword": 2, "start": 3, "end": 9}, {"keyword": 0, "start": 8, "end": 9}, {"keyword": 1, "start": 0, "end": 4}]
    assert [h["keyword"] for h in sort_hits(hits)] == [1, 0, 2]
    h = {"keyword": 0, "text": "x y", "start": 5, "end": 9, "score": -0.5, "confidence": 0.7788}
    assert hit_seconds(h, 0.04) == (pytest.approx(0.2), pytest.approx(0.4))  # end is inclusive: (9 + 1) * 0.04
    assert output_line("utt1", h, 0.04) == "utt1\t0.200\t0.400\t0.7788\tx y"
    assert hold_frames(500, 0.04) == 12 and hold_frames(0, 0.04) == 0 and hold_frames(30, 0.04) == 1


def test_write_hits_orders_by_utterance_then_start(tmp_path):
    import io

    from espresso_amd.speech_kws import write_hits

    mk = lambda k, s, e: {"keyword": k, "text": f"k{k}", "start": s, "end": e, "score": 0.0, "confidence": 1.0}  # noqa: E731
    res = {"b": [mk(0, 7, 9), mk(1, 2, 9)], "a": [mk(0, 1, 1)]}
    out = io.StringIO()
    write_hits(res, ["b", "a"], 0.01, out)
    assert [l.split("\t")[0] + l.split("\t")[4] + l.split("\t")[1] for l in out.getvalue().splitlines()] == [
        "bk10.020", "bk00.070", "ak00.010"]


def test_cli_parser_defaults():
    from espresso_amd import speech_kws

    a = speech_kws.get_parser().parse_args(["--path", "m.pt", "--dict", "d.txt", "--wav-scp", "w.scp", "--keywords", "k.txt"])
    assert (a.threshold, a.hold_ms, a.max_hits, a.output, a.streaming, a.stream_chunk_ms, a.streams) == (0.5, 500.0, 64, "-", False,
                                                                                                         None, None)
    assert speech_kws.check_args(a) == (400, 16)
    with pytest.raises(SystemExit):
        speech_kws.get_parser().parse_args(["--path", "m.pt", "--dict", "d.txt", "--wav-scp", "w.scp"])  # --keywords required
    a = speech_kws.get_parser().parse_args(["--path", "m.pt", "--dict", "d.txt", "--wav-scp", "w.scp", "--keywords", "k", "--streams", "2"])
    with pytest.raises(ValueError, match="--streaming"):
        speech_kws.check_args(a)
    helps = speech_kws.get_parser().format_help()
    assert helps.count("unmeasured") >= 2


@pytest.mark.parametrize("name", ["speech_transformer_base", "speech_lstm", "speech_transformer", "speech_transformer_transducer_base"])
def test_cli_refuses_other_models_before_loading(tmp_path, name):
    from espresso_amd import speech_kws

    with pytest.raises(NotImplementedError, match="encoder-only CTC"):
        speech_kws.main(["--path", str(tmp_path / "missing.pt"), "--model", name, "--dict", "d.txt", "--wav-scp", "w.scp",
                         "--keywords", "k.txt"])
    speech_kws.require_ctc("speech_transformer_encoder_model")
