"""Float64 reference of hotword biasing for the tests: the bias expressed through the `lm_fn` hook of
tests.test_ctc_prefix_beam.prefix_beam_oracle, an independent statement of B(y), and the inputs the CPU and GPU tests share."""
import numpy as np

from tests.test_ctc_prefix_beam import _peaked, prefix_beam_oracle

BOOSTS = (0.73, 1.37)  # not multiples of each other: no ties between differently boosted hypotheses
# the (beam, K, seed) grid of tests.test_ctc_prefix_beam.test_search_vs_oracle_no_lm
GRID = [(1, 1, 0), (1, 4, 0), (4, 1, 0), (4, 4, 1), (16, 1, 0), (16, 4, 11)]
GRID_LENS = np.array([14, 0, 1, 9, 12], dtype=np.int32)


def locked_bonus(phrases, y):
    """B(y) stated on token tuples, without node tables or failure links: the state is the longest suffix of the consumed
    tokens that (extended by the next token) is a trie path, and whenever a phrase end is entered along its own trie edge the
    boosts on that path that are not yet locked become locked.  phrases: [(tokens, boost)].  Returns B(y) in float64."""
    paths = {}  # trie path -> edge boost e
    ends = set()
    for toks, s in phrases:
        toks = tuple(toks)
        for k in range(1, len(toks) + 1):
            paths[toks[:k]] = max(paths.get(toks[:k], 0.0), s)
        ends.add(toks)

    def w(path):
        return sum(paths[path[:k]] for k in range(1, len(path) + 1))

    def lock(path):
        return max([w(path[:k]) for k in range(1, len(path) + 1) if path[:k] in ends] + [0.0])

    total, cur = 0.0, ()  # cur: the suffix of the consumed tokens the automaton sits in
    for v in y:
        # the longest suffix m of cur (cur itself included) such that m + v is a trie path
        m = next((cur[k:] for k in range(len(cur) + 1) if cur[k:] + (v,) in paths), None)
        if m is None:
            cur = ()
            continue
        nxt = m + (v,)
        if nxt in ends:  # entered through its trie edge: everything pending on this path is locked
            total += w(nxt) - lock(m)
        cur = nxt
    return total


def bias_lm_fn(graph, V, lm_fn=None, lm_weight=0.0, eos=None):
    """The biased search as an `lm_fn` of prefix_beam_oracle used with lm_weight = 1 and eos = V: entry c < V is the increment of
    the score when token c is appended to y (lm_weight * log P_lm(c | y) + b' - b), entry V the final term
    (lm_weight * log P_lm(eos | y) - phi(q))."""
    cache = {}

    def fn(y):
        if y not in cache:
            q = graph.state(y)
            row = np.zeros(V + 1, dtype=np.float64)
            for c in range(V):
                row[c] = graph.step(q, c)[1]
            row[V] = -graph.pending(q)
            if lm_fn is not None:
                lrow = lm_fn(y)
                row[:V] += lm_weight * lrow[:V]
                row[V] += lm_weight * lrow[eos]
            cache[y] = row
        return cache[y]

    return fn


def biased_oracle(x, length, beam, K, blank, graph, lm_fn=None, lm_weight=0.0, bonus=0.0, eos=None, nbest=1):
    V = x.shape[1]
    return prefix_beam_oracle(x, length, beam, K, blank, lm_fn=bias_lm_fn(graph, V, lm_fn, lm_weight, eos), lm_weight=1.0, bonus=bonus,
                              eos=V, nbest=nbest)


def grid_inputs(seed, V):
    """The log-probs of test_search_vs_oracle_no_lm for a seed: float64 [5][14][V]."""
    rng = np.random.default_rng(seed)
    B, T = len(GRID_LENS), int(GRID_LENS.max())
    return _peaked(rng, B * T, V, sharp=4.0, scale=2.0).reshape(B, T, V)


def grid_phrases(x, lens, blank):
    """Phrases from token sequences that occur in the inputs: of every utterance the 2- and 3-grams of the second and third
    best unbiased hypotheses (beam 16, K 4), boosted alternately by BOOSTS.  [(tokens, boost)]."""
    phrases, n = [], 0
    for b in range(x.shape[0]):
        hyps, _ = prefix_beam_oracle(x[b], int(lens[b]), 16, 4, blank, nbest=3)
        for y, _ in hyps[1:]:
            for k in (2, 3):
                for i in range(len(y) - k + 1):
                    phrases.append((list(y[i : i + k]), BOOSTS[n % 2]))
                    n += 1
    return phrases
