"""TokenNGramLM — an n-gram LM (plain-text ARPA, order <= 6) over the model's own sub-word units, fused by the four token-level
beam searches (ctc_beam, ctc_stream_beam, transducer_frame_beam, transducer_stream_beam) where they otherwise fuse the LSTM
LM.  The reference reaches an ARPA model only through Flashlight's KenLM lexicon decoder (espresso/tools/ctc_decoder.py:24-71),
word-level; this is the same kind of file trained on the tokenised text, with no lexicon.

It wraps models.ngram_lm.NGramLanguageModel (the parser, the tables, their upload) and adds `tok2word`, int32 [len(dictionary)]:
the dictionary's symbols, taken verbatim as ARPA words, as ARPA word ids.  The dictionary's eos is `</s>`; its `<unk>` is the
file's `<unk>` if there is one; pad and the blank / bos symbol are -2, columns that are always -inf; a symbol the file lacks
is -1 and scores as `<unk>` (-inf without one).  The state of a hypothesis is its context: the last order - 1 word ids, int32,
oldest first, front-padded with -1.  `start` and `update` are each one launch (csrc/ngram_rows.hip) that advances the contexts
from the (parent, token, keep) triple of a search step and writes the full rows ln P(. | context): what BeamDecoderMixin's
lm_start / lm_update return for this LM.  Every row is recomputed each frame, the rows of kept hypotheses too."""
import numpy as np
import torch

from .. import kernels as K
from .ngram_lm import NGramLanguageModel


class TokenNGramLM:
    def __init__(self, path: str, dictionary, blank=None, device=None):
        """blank: the id of the model's blank (default: the dictionary's bos when it has one of its own)."""
        self.ngram = lm = NGramLanguageModel(path)
        self.dictionary, self.order = dictionary, lm.order
        if lm.bos < 0 or lm.eos < 0:  # (the parser refuses such a file already)
            raise ValueError(f"{path}: a token n-gram LM needs the <s> and </s> unigrams")
        eos, pad, unk = dictionary.eos(), dictionary.pad(), dictionary.unk()
        if blank is None and dictionary.bos() != eos:
            blank = dictionary.bos()
        self.blank = blank
        t2w = np.empty(len(dictionary), dtype=np.int32)
        missing, plain = [], 0
        for i, sym in enumerate(dictionary.symbols):
            if i == eos:
                t2w[i] = lm.eos
            elif i == pad or i == blank:
                t2w[i] = -2
            elif i == unk:
                t2w[i] = lm.unk  # -1 without one
            else:
                t2w[i] = lm.word2id.get(sym, -1)
                if sym in ("<s>", "</s>", "<unk>"):  # these words belong to the special ids above
                    t2w[i] = -1
                plain += 1
                if t2w[i] < 0:
                    missing.append(sym)
        if 2 * len(missing) > plain:
            raise ValueError(f"{path}: {len(missing)} of the dictionary's {plain} symbols have no unigram (" +
                             ", ".join(repr(s) for s in missing[:10]) + (", ..." if len(missing) > 10 else "") +
                             "): is this the n-gram LM of this model's units?")
        self.tok2word = t2w
        self.device = self._map = None
        self._ctx = {}  # N -> the two context buffers that alternate between frames
        if device is not None:
            self.to(device)

    # ---- what the decoders ask of an LM ------------------------------------------------------------------------------------
    def eval(self):
        return self

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._map is None:
            self.ngram.to(device)
            self._map = K.NgramTokenMap(self.ngram.handle, self.tok2word, device)
            self.device = device
        elif self.device != device:
            raise RuntimeError(f"TokenNGramLM already lives on {self.device}")
        return self

    def cuda(self, device=None):
        return self.to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)

    # ---- the rows ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def start(self, N, device):
        """(ctx int32 [N][max(order - 1, 1)], rows fp32 [N][V]) of N empty hypotheses: <s> as the context."""
        self.to(device)
        return K.ngram_token_rows_start(self.ngram.handle, self._map, N, self.order - 1)

    def init_state(self, N, device):
        """Contexts of N rows to be filled by a reset (the streamed decoders' per-slot rows)."""
        return torch.full((N, max(self.order - 1, 1)), -1, dtype=torch.int32, device=device)

    @torch.no_grad()
    def update(self, ctx, parent, token, keep):
        """After one step: row i continues row parent[i] of ctx and, unless keep[i], appends token[i].  Returns (ctx, rows).
        The returned ctx is one of two buffers per row count N that this object owns and alternates (whichever `ctx` is not):
        it is valid until the next but one `update` with the same N, by whoever calls it.  A search loop hands it straight
        back, and the streamed decoders copy it into their slots after the loop; a caller that keeps a state longer clones
        it.  rows is a fresh tensor every call."""
        N = parent.numel()
        if N == 0:
            return ctx, torch.empty(0, len(self.dictionary), dtype=torch.float32, device=ctx.device)
        pair = self._ctx.get(N)
        if pair is None:
            pair = self._ctx[N] = [torch.empty_like(ctx), torch.empty_like(ctx)]
        out = pair[1] if ctx.data_ptr() == pair[0].data_ptr() else pair[0]
        rows = K.ngram_token_rows_step(self.ngram.handle, self._map, ctx, parent, token, keep, out)
        return out, rows

    def rows_host(self, ctx, parent, token, keep):
        """`update` on the host tables and numpy arrays (no device; tests)."""
        return K.ngram_token_rows_host(self.ngram._h, self.tok2word, ctx, parent, token, keep, self.order - 1)

    def start_host(self, N):
        return K.ngram_token_rows_host(self.ngram._h, self.tok2word, N, None, None, None, self.order - 1)
