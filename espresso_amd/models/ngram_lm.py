"""NGramLanguageModel — a word n-gram LM read from a plain-text ARPA file (order <= 6; no gzip, no KenLM binary), the LM
the reference hands to Flashlight's lexicon decoder as `lm_model` (espresso/tools/ctc_decoder.py:24-71).

The library parses the file (csrc/ctc_lexicon_beam.hip: a sorted-array trie, natural-log values) and copies the tables to
the device once; this class holds that handle, the word vocabulary (word id = position among the unigrams) and the order.
`score` is the batched device query; tools.ctc_lexicon_beam_search fuses the LM into the CTC prefix beam search."""
import ctypes
from typing import List, Sequence

import numpy as np
import torch

from .. import _lib


class ArpaFormatError(ValueError):
    pass


class NGramLanguageModel:
    def __init__(self, path: str, device=None):
        """Parse `path`; with `device` (a CUDA device) the tables are copied there at once."""
        lib = _lib.lib()
        h, err = ctypes.c_void_p(), ctypes.create_string_buffer(1024)
        rc = lib.ea_ngram_create(path.encode(), ctypes.byref(h), err, len(err))
        if rc == -1:
            raise FileNotFoundError(err.value.decode(errors="replace"))
        if rc != 0:
            raise ArpaFormatError(err.value.decode(errors="replace"))
        self._h = h
        meta, counts = (ctypes.c_int * 4)(), (ctypes.c_long * 6)()
        _lib.check(lib.ea_ngram_info(h, meta, counts), "ea_ngram_info")
        self.order, self.unk, self.bos, self.eos = list(meta)
        self.counts = [int(c) for c in counts[: self.order]]
        n = lib.ea_ngram_vocab(h, None, 0)
        buf = ctypes.create_string_buffer(max(1, n))
        lib.ea_ngram_vocab(h, buf, n)
        self.vocab: List[str] = buf.raw[:n].decode("utf-8").split("\n")[:-1]
        self.word2id = {w: i for i, w in enumerate(self.vocab)}
        self.device = None
        if device is not None:
            self.to(device)

    def close(self):
        """Free the host and device tables."""
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            _lib.lib().ea_ngram_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: the library may already be gone
            pass

    @property
    def handle(self):
        if self.device is None:
            raise RuntimeError("NGramLanguageModel: call .to(device) before a device query")
        return self._h

    def to(self, device):
        device = torch.device(device)
        if self.device is not None and self.device != device:
            raise RuntimeError(f"NGramLanguageModel already lives on {self.device}")
        with torch.cuda.device(device):
            _lib.check(_lib.lib().ea_ngram_upload(self._h), "ea_ngram_upload")
        self.device = device
        return self

    def index(self, word: str) -> int:
        """Word id; a word the ARPA file lacks maps to <unk> (-1 without one)."""
        return self.word2id.get(word, self.unk)

    def records(self, order: int):
        """(ngrams int32 [count][order] word ids, logp fp32 [count], bow fp32 [count]) of one order, natural log, in table
        order (sorted by context record, then word id)."""
        n = self.counts[order - 1]
        ng = np.empty((n, order), dtype=np.int32)
        lp, bw = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.float32)
        got = _lib.lib().ea_ngram_records(self._h, order, ng.ctypes.data_as(ctypes.c_void_p), lp.ctypes.data_as(ctypes.c_void_p),
                                          bw.ctypes.data_as(ctypes.c_void_p))
        assert got == n, (got, n)
        return ng, lp, bw

    def unigram_logprobs(self) -> np.ndarray:
        """ln P_1(w) fp32 [vocabulary], indexed by word id."""
        return self.records(1)[1]

    def score_host(self, contexts: np.ndarray, words: np.ndarray) -> np.ndarray:
        """ln P(words[i] | contexts[i]) fp32 [N] on the host tables (ea_ngram_score_host); ids as for `score`."""
        ctx = np.ascontiguousarray(contexts, dtype=np.int32).reshape(len(words), self.order - 1)
        w = np.ascontiguousarray(words, dtype=np.int32)
        out = np.empty(len(w), dtype=np.float32)
        _lib.check(_lib.lib().ea_ngram_score_host(self._h, ctx.ctypes.data_as(ctypes.c_void_p), w.ctypes.data_as(ctypes.c_void_p),
                                                   len(w), out.ctypes.data_as(ctypes.c_void_p)), "ea_ngram_score_host")
        return out

    def encode_contexts(self, contexts: Sequence[Sequence[str]]) -> torch.Tensor:
        """int32 [N][order - 1]: the last order - 1 words of every context (oldest first), front-padded with -1."""
        W = self.order - 1
        out = np.full((len(contexts), W), -1, dtype=np.int32)
        for i, c in enumerate(contexts):
            # a context word the file lacks is <unk>, or without one an id that matches no n-gram
            ids = [self.word2id.get(w, self.unk if self.unk >= 0 else len(self.vocab)) for w in list(c)[len(c) - W:]] if W else []
            if ids:
                out[i, W - len(ids):] = ids
        return torch.from_numpy(out)

    @torch.no_grad()
    def score(self, contexts, words) -> torch.Tensor:
        """ln P(word | context) fp32 [N] on the device.  contexts: word lists (include "<s>" for a sentence start) or an
        int32 [N][order - 1] tensor of ids; words: strings or an int32 [N] tensor of ids."""
        from .. import kernels as K

        dev = self.device
        if not torch.is_tensor(contexts):
            contexts = self.encode_contexts(contexts)
        if not torch.is_tensor(words):
            words = torch.tensor([self.index(w) for w in words], dtype=torch.int32)
        return K.ngram_score(self.handle, contexts.to(dev, torch.int32).contiguous(), words.to(dev, torch.int32).contiguous())
