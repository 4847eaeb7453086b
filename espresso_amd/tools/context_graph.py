"""ContextGraph — hotword (contextual phrase) biasing tables for the CTC prefix beam search (csrc/ctc_beam.hip, BIAS kernels)
and the frame-synchronous transducer beam search, offline and streamed (csrc/rnnt_beam.hip, kBias kernels).

Phrases p_1..p_P are non-empty token-id sequences with a per-token boost s_i > 0 (natural log, added to the hypothesis score
unweighted).  Over their trie, for a node n (root excluded): e(n) = max s_i over the phrases through n (boost of the edge into n),
w(n) = sum of e along root -> n, end(n) = some phrase ends at n, lock(n) = w of the deepest end node on root -> n (n included, 0
if none), phi(n) = w(n) - lock(n): the bonus that is pending while a hypothesis sits in n (0 at the root and at every end node).
fail(n) = the node of the longest proper suffix of path(n) that is a trie path (Aho-Corasick; fail(root) = root).

A hypothesis carries a node q and a running bias b (root, 0 for the empty prefix).  Appending token v:

    m = q
    while m != root and child(m, v) does not exist: m = fail(m)
    if child(m, v) exists:  q' = child(m, v);  b' = b + phi(m) + e(q') - phi(q)
    else:                   q' = root;         b' = b - phi(q)

and at the end b_final = b - phi(q).  The increments telescope: b_final = B(y), the boosts locked whenever an end node was
entered through its trie edge, so a finished score is the unbiased score of y plus B(y), while a half-matched phrase is kept
alive by its pending phi.  Deliberate limit: a phrase reached only through a failure link (one that ends inside a longer, still
pending phrase) is not credited — under-crediting only, never double counting.

`ContextGraph` holds the plain CSR trie (children sorted by token, the layout of tools/lexicon.py) with per-node `fail`, `phi`,
`edge_boost`, the packed tables the kernels walk (`nodes`, `edges`, `root`, see include/espresso_amd.h), and `score`, a float64
replay over a dict-of-nodes trie that shares no code with the packed walk."""
from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np

MAX_PHRASE_TOKENS = 64


class ContextGraph:
    def __init__(self, phrases: Iterable[Tuple[Sequence[int], float]], vocab_size: int):
        """phrases: (token ids, boost per token) pairs; duplicates keep the larger boost."""
        self.vocab_size = V = int(vocab_size)
        best: Dict[Tuple[int, ...], float] = {}
        for toks, boost in phrases:
            toks, boost = tuple(int(t) for t in toks), float(boost)
            if not 1 <= len(toks) <= MAX_PHRASE_TOKENS:
                raise ValueError(f"hotword phrase of {len(toks)} tokens: 1 to {MAX_PHRASE_TOKENS} are supported")
            if not boost > 0.0 or not np.isfinite(boost):
                raise ValueError(f"hotword boost {boost} of phrase {list(toks)}: boosts are positive and finite")
            if min(toks) < 0 or max(toks) >= V:
                raise ValueError(f"hotword phrase {list(toks)} has a token outside the vocabulary [0, {V})")
            best[toks] = max(boost, best.get(toks, 0.0))
        self.phrases: List[Tuple[Tuple[int, ...], float]] = sorted(best.items())
        # dict-of-nodes trie, nodes numbered breadth first (so that a fail link points to a lower number)
        children: List[Dict[int, int]] = [{}]
        e, end, depth, parent = [0.0], [False], [0], [0]
        for toks, boost in self.phrases:
            n = 0
            for t in toks:
                if t not in children[n]:
                    children[n][t] = len(children)
                    children.append({})
                    e.append(0.0)
                    end.append(False)
                    depth.append(depth[n] + 1)
                    parent.append(n)
                n = children[n][t]
                e[n] = max(e[n], boost)
            end[n] = True
        order, renum = [0], {0: 0}
        for n in order:  # breadth first, children by token
            for t in sorted(children[n]):
                renum[children[n][t]] = len(order)
                order.append(children[n][t])
        N = len(order)
        self._children = [{t: renum[c] for t, c in children[n].items()} for n in order]
        self._e = [e[n] for n in order]
        self._end = [end[n] for n in order]
        w, lock, fail = [0.0] * N, [0.0] * N, [0] * N
        for n in range(N):  # parents come first
            for t, c in self._children[n].items():
                w[c] = w[n] + self._e[c]
                lock[c] = w[c] if self._end[c] else lock[n]
                m = n
                while True:
                    if m == 0:
                        fail[c] = 0
                        break
                    m = fail[m]
                    if t in self._children[m]:
                        fail[c] = self._children[m][t]
                        break
        self._phi = [w[n] - lock[n] for n in range(N)]
        self._fail = fail
        if N >= 2 ** 31:
            raise ValueError("context graph: fewer than 2^31 nodes are supported")
        # plain CSR tables
        self.num_nodes = N
        self.off = np.zeros(N + 1, dtype=np.int32)
        for n in range(N):
            self.off[n + 1] = self.off[n] + len(self._children[n])
        E = int(self.off[N])
        self.tok = np.zeros(E, dtype=np.int32)
        self.child = np.zeros(E, dtype=np.int32)
        for n in range(N):
            for k, t in enumerate(sorted(self._children[n])):
                self.tok[self.off[n] + k] = t
                self.child[self.off[n] + k] = self._children[n][t]
        self.fail = np.asarray(fail, dtype=np.int32)
        self.phi = np.asarray(self._phi, dtype=np.float32)
        self.edge_boost = np.asarray(self._e, dtype=np.float32)
        # packed for the kernels: one 16-byte record per node and per edge, the root's edges by direct index
        self.nodes = np.zeros((N, 4), dtype=np.int32)
        self.nodes[:, 0], self.nodes[:, 1], self.nodes[:, 2] = self.off[:-1], self.off[1:], self.fail
        self.nodes[:, 3] = self.phi.view(np.int32)
        self.edges = np.zeros((E, 4), dtype=np.int32)
        self.edges[:, 0], self.edges[:, 1] = self.tok, self.child
        self.edges[:, 2] = self.edge_boost[self.child].view(np.int32)
        self.root = np.zeros((V, 2), dtype=np.int32)
        self.root[:, 0] = -1
        for t, c in self._children[0].items():
            self.root[t, 0] = c
            self.root[t, 1] = self.edge_boost[c : c + 1].view(np.int32)[0]
        self._dev = None

    @property
    def num_edges(self):
        return self.num_nodes - 1

    # ------------------------------------------------------------------------------------------ replays
    def step(self, q: int, v: int):
        """(q', b' - b) of appending token v in node q, over the dict-of-nodes trie (float64)."""
        m = q
        while m != 0 and v not in self._children[m]:
            m = self._fail[m]
        if v in self._children[m]:
            c = self._children[m][v]
            return c, self._phi[m] + self._e[c] - self._phi[q]
        return 0, -self._phi[q]

    def score(self, tokens: Sequence[int]):
        """(running bias after every token, B(tokens)) in float64 over the dict-of-nodes trie."""
        q, b, running = 0, 0.0, []
        for v in tokens:
            q, inc = self.step(q, v)
            b += inc
            running.append(b)
        return running, b - self._phi[q]

    def state(self, tokens: Sequence[int]) -> int:
        """The node after `tokens`."""
        q = 0
        for v in tokens:
            q, _ = self.step(q, v)
        return q

    def pending(self, q: int) -> float:
        """phi(q): the bonus a hypothesis in node q holds on credit."""
        return self._phi[q]

    def score_host(self, rows: Sequence[Sequence[int]]):
        """The packed tables replayed by ea_context_graph_score_host: (running fp32 [N][L], final fp32 [N], q int32 [N])."""
        import ctypes

        from .. import _lib

        N = len(rows)
        L = max([1] + [len(r) for r in rows])
        tokens = np.zeros((N, L), dtype=np.int32)
        lens = np.zeros(N, dtype=np.int32)
        for i, r in enumerate(rows):
            tokens[i, : len(r)] = r
            lens[i] = len(r)
        running = np.zeros((N, L), dtype=np.float32)
        final = np.zeros(N, dtype=np.float32)
        q = np.zeros(N, dtype=np.int32)

        def p(a):
            return a.ctypes.data_as(ctypes.c_void_p) if a.size else None

        _lib.check(_lib.lib().ea_context_graph_score_host(p(self.nodes), p(self.edges), p(self.root), self.num_nodes, self.num_edges,
                                                          self.vocab_size, p(tokens), p(lens), N, L, p(running), p(final), p(q)),
                   "ea_context_graph_score_host")
        return running, final, q

    def cuda(self, device=None):
        """Upload the packed tables once per device; returns (nodes, edges, root) device tensors.  No device, or a bare "cuda",
        is the current device: the cache is keyed on the resolved one."""
        import torch

        device = torch.device("cuda" if device is None else device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._dev is None or self._dev[0].device != device:
            self._dev = tuple(torch.from_numpy(a).to(device) for a in (self.nodes, self.edges, self.root))
        return self._dev


def read_hotwords(path: str, dictionary, blank: int, default_boost: float) -> List[Tuple[List[int], float]]:
    """A phrase file: one phrase per line, optionally `<TAB>boost`; `#` comments and blank lines are skipped.  The text is
    tokenised as transcripts are (speech_align.tokenize); a phrase that holds <unk> after that is refused with its line number."""
    from ..speech_align import tokenize

    out = []
    with open(path, encoding="utf-8") as f:
        for lineno, line in enumerate(f, 1):
            line = line.rstrip("\n").rstrip("\r")
            if not line.strip() or line.lstrip().startswith("#"):
                continue
            text, boost = line, default_boost
            if "\t" in line:
                text, col = line.split("\t", 1)
                try:
                    boost = float(col)
                except ValueError:
                    raise ValueError(f"{path}:{lineno}: boost {col.strip()!r} is not a number") from None
            if not boost > 0.0:
                raise ValueError(f"{path}:{lineno}: boost {boost} is not positive")
            ids = tokenize(dictionary, text.strip(), blank)
            if not ids:
                raise ValueError(f"{path}:{lineno}: phrase {text.strip()!r} has no tokens")
            if dictionary.unk() in ids:
                raise ValueError(f"{path}:{lineno}: phrase {text.strip()!r} contains {dictionary[dictionary.unk()]} after tokenisation")
            out.append((ids, boost))
    return out


def load_context_graph(path: str, dictionary, blank: int, default_boost: float) -> ContextGraph:
    return ContextGraph(read_hotwords(path, dictionary, blank, default_boost), len(dictionary))
