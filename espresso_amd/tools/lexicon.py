"""Lexicon of the lexicon-constrained CTC beam search (tools/ctc_lexicon_beam_search.py): which token sequences spell which
words, as a trie in CSR form for the device.

File format: wav2letter / Flashlight lexicon (the reference's `lexicon`, espresso/tools/ctc_decoder.py:24-71): one line per
spelling, `word tok1 tok2 ...`; several lines may spell one word; every token is a symbol of the model's dictionary.  Without
a file, and only in space mode (the dictionary has `<space>`), every ARPA unigram is spelled with the character tokenizer
(data/encoders.tokenize, as TensorizedPrefixTree.build does).  Word-start mode (no `<space>`, e.g. sentencepiece pieces that
start a word with U+2581) needs a file.

Per trie node: the LM word id that ends there (or -1) and the look-ahead S(node) = max ln P_1(w) over the words below it
(S(root) = 0).  Children are sorted by token id and found by binary search, so a root with thousands of children costs
nothing beyond its edges."""
import warnings
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

WORD_START = "▁"
_LM_SPECIAL = ("<s>", "</s>", "<unk>")


class LexiconError(ValueError):
    pass


def read_lexicon(path: str, dictionary) -> List[Tuple[str, List[int]]]:
    """[(word, token ids)] of a wav2letter-format lexicon file, in file order."""
    out = []
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            fields = line.split()
            if not fields:
                continue
            if len(fields) < 2:
                raise LexiconError(f"{path}: line {n}: '{line.strip()}' has no spelling")
            ids = []
            for t in fields[1:]:
                if t not in dictionary:
                    raise LexiconError(f"{path}: line {n}: token '{t}' is not in the dictionary")
                ids.append(dictionary.index(t))
            out.append((fields[0], ids))
    return out


def spell_words(words, dictionary) -> List[Tuple[str, List[int]]]:
    """Space mode without a lexicon file: each word spelled by the character tokenizer (with the dictionary's non-language
    symbols); words with a character outside the dictionary are left out."""
    from ..data.encoders import tokenize

    nls = getattr(dictionary, "non_lang_syms", None)
    out = []
    for w in words:
        if w in _LM_SPECIAL:
            continue
        toks = tokenize(w, non_lang_syms=nls).split(" ")
        if all(t in dictionary for t in toks):
            out.append((w, [dictionary.index(t) for t in toks]))
    return out


class LexiconTrie:
    """CSR trie: children of node n are tok[off[n]:off[n + 1]] (ascending) -> child[...]; word[n] = LM word id or -1;
    smear[n] = S(n) in natural log.  `word_start` uint8 [V]: 1 for tokens that start a word (word-start mode), None in
    space mode; `space` = the <space> token or -1."""

    def __init__(self, spellings: List[Tuple[str, List[int]]], lm, dictionary):
        self.space = dictionary.space()
        V = len(dictionary)
        if self.space >= 0:
            self.word_start = None
        else:
            self.word_start = np.array([1 if dictionary[i].startswith(WORD_START) else 0 for i in range(V)], dtype=np.uint8)
        uni = lm.unigram_logprobs().astype(np.float64)
        edges: Dict[Tuple[int, int], int] = {}
        word = [-1]
        names: List[Optional[str]] = [None]
        dropped = []
        for w, ids in spellings:
            wid = lm.index(w)
            if wid < 0:
                dropped.append(w)
                continue
            if not ids:
                raise LexiconError(f"lexicon: word '{w}' has an empty spelling")
            if self.space >= 0 and self.space in ids:
                raise LexiconError(f"lexicon: the spelling of '{w}' contains the word separator {dictionary[self.space]}")
            node = 0
            for t in ids:
                nxt = edges.get((node, t))
                if nxt is None:
                    nxt = edges[(node, t)] = len(word)
                    word.append(-1)
                    names.append(None)
                node = nxt
            if names[node] is not None and names[node] != w:
                raise LexiconError(f"lexicon: '{w}' and '{names[node]}' have the same spelling "
                                   f"'{' '.join(dictionary[t] for t in ids)}'")
            word[node], names[node] = wid, w
        if dropped:
            warnings.warn(f"lexicon: {len(dropped)} word(s) not in the ARPA file, which has no <unk>, are dropped "
                          f"(first: {dropped[:5]})")
        n = len(word)
        kids: List[List[Tuple[int, int]]] = [[] for _ in range(n)]
        parent = np.zeros(n, dtype=np.int64)
        for (p, t), c in edges.items():
            kids[p].append((t, c))
            parent[c] = p
        off, tok, child = [0], [], []
        for k in kids:
            k.sort()
            tok += [t for t, _ in k]
            child += [c for _, c in k]
            off.append(len(tok))
        smear = np.full(n, -np.inf)
        for i in range(n - 1, 0, -1):  # children have larger ids than their parents
            if word[i] >= 0:
                smear[i] = max(smear[i], uni[word[i]])
            smear[parent[i]] = max(smear[parent[i]], smear[i])
        smear[0] = 0.0
        self.off, self.tok, self.child = (np.asarray(a, dtype=np.int32) for a in (off, tok, child))
        self.word = np.asarray(word, dtype=np.int32)
        self.smear = smear.astype(np.float32)
        self.num_words = sum(1 for x in names if x is not None)

    def __len__(self):
        return len(self.word)

    def child_of(self, node: int, token: int) -> int:
        lo, hi = int(self.off[node]), int(self.off[node + 1])
        i = lo + int(np.searchsorted(self.tok[lo:hi], token))
        return int(self.child[i]) if i < hi and self.tok[i] == token else -1

    def is_boundary(self, token: int) -> bool:
        """Does `token` end the pending word (space mode: <space>) or start a new one (word-start mode)?"""
        return token == self.space if self.space >= 0 else bool(self.word_start[token])

    def to(self, device):
        """(off, tok, child, word, smear) device tensors and the word-start flags (None in space mode)."""
        trie = tuple(torch.from_numpy(a).to(device) for a in (self.off, self.tok, self.child, self.word, self.smear))
        ws = None if self.word_start is None else torch.from_numpy(self.word_start).to(device)
        return trie, ws


def build_lexicon(dictionary, lm, lexicon_path: Optional[str] = None) -> LexiconTrie:
    """The trie for `dictionary` and the n-gram LM `lm`: from a lexicon file, or in space mode from the ARPA unigrams."""
    if lexicon_path:
        spellings = read_lexicon(lexicon_path, dictionary)
    elif dictionary.space() >= 0:
        spellings = spell_words(lm.vocab, dictionary)
    else:
        raise LexiconError("the dictionary has no <space> symbol (word-start mode): words cannot be spelled from the ARPA "
                           "file, give --lexicon")
    return LexiconTrie(spellings, lm, dictionary)
