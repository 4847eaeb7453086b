"""Sample-rate conversion in front of the fbank: audio of rate `fi` becomes audio of the front-end's rate `fo` on the device
(csrc/resample.hip), for ragged batches (`Resampler`) and for stream pieces (`StreamResampler`).

The filter is the Hann-windowed sinc of Kaldi's LinearResample (`torchaudio.compliance.kaldi.resample_waveform` restates it)
with num_zeros = 6 and roll-off 0.99:

    g = gcd(fi, fo), in_unit = fi / g, phases = fo / g, fc = 0.99 * 0.5 * min(fi, fo), W = 6 / (2 fc)
    output j (time j / fo): phase p = j mod phases, unit u = j div phases; with t_out = p / fo
      lo_p = ceil((t_out - W) fi), hi_p = floor((t_out + W) fi)
      weight of input i in [lo_p, hi_p] at t = i / fi - t_out:  h(t) / fi,
      h(t) = 0.5 (1 + cos(2 pi fc / 6 t)) sin(2 pi fc t) / (pi t)  for |t| < W,  h(0) = 2 fc,  0 otherwise
    K = max_p (hi_p - lo_p + 1);  taps[phases][K] (rows padded with zeros), first[p] = lo_p
    y[j] = sum_k taps[p][k] x[first[p] + u in_unit + k],  x = 0 outside [0, n);   n_out = ceil(n fo / fi)

The table is computed in numpy fp64 and rounded once to fp32.  Durations are preserved (n_out / fo covers n / fi), so every time
the decoders report stays in seconds of the original recording.  All bookkeeping here is exact integer arithmetic on the host;
the kernel evaluates one output the same way whether it is reached offline or piece by piece, so a streamed recording gives
the bits of the offline one."""
import math
from functools import lru_cache
from typing import Dict, List, Sequence

import numpy as np
import torch

from .. import kernels as K

NUM_ZEROS = 6
ROLLOFF = 0.99
MAX_TABLE_FLOATS = 1 << 20


class ResamplePlan:
    """The polyphase table of one (fi, fo) pair: `taps` fp32 [phases][K], `first` int32 [phases] (numpy), and device copies."""

    def __init__(self, fi: int, fo: int):
        fi, fo = int(fi), int(fo)
        if fi <= 0 or fo <= 0:
            raise NotImplementedError(f"cannot resample from {fi} Hz to {fo} Hz: sample rates must be positive")
        g = math.gcd(fi, fo)
        self.fi, self.fo = fi, fo
        self.in_unit, self.phases = fi // g, fo // g
        self._dev: Dict[str, tuple] = {}
        if fi == fo:  # identity: one phase, one tap of 1.0 (exact)
            self.K = 1
            self.first = np.zeros(1, dtype=np.int32)
            self.taps = np.ones((1, 1), dtype=np.float32)
            return
        fc = ROLLOFF * 0.5 * min(fi, fo)
        W = NUM_ZEROS / (2.0 * fc)
        t_out = np.arange(self.phases, dtype=np.float64) / fo
        lo = np.ceil((t_out - W) * fi).astype(np.int64)
        hi = np.floor((t_out + W) * fi).astype(np.int64)
        self.K = int((hi - lo + 1).max())
        if self.phases * self.K > MAX_TABLE_FLOATS:
            raise NotImplementedError(
                f"cannot resample from {fi} Hz to {fo} Hz: the filter table would hold {self.phases} x {self.K} weights "
                f"(more than {MAX_TABLE_FLOATS}); convert the audio to a rate with a larger common divisor first")
        i = lo[:, None] + np.arange(self.K, dtype=np.int64)[None, :]
        t = i.astype(np.float64) / fi - t_out[:, None]
        inside = (np.abs(t) < W) & (i <= hi[:, None])
        ts = np.where(t == 0.0, 1.0, t)
        h = 0.5 * (1.0 + np.cos(2.0 * np.pi * fc / NUM_ZEROS * t)) * np.sin(2.0 * np.pi * fc * t) / (np.pi * ts)
        h = np.where(t == 0.0, 2.0 * fc, h)
        self.taps = np.ascontiguousarray(np.where(inside, h / fi, 0.0).astype(np.float32))
        self.first = lo.astype(np.int32)

    def n_out(self, n: int) -> int:
        """Outputs with time < n / fi: ceil(n fo / fi)."""
        return (int(n) * self.phases + self.in_unit - 1) // self.in_unit

    def start(self, j: int) -> int:
        """Absolute index of the first input that output j reads."""
        return int(self.first[j % self.phases]) + (j // self.phases) * self.in_unit

    def ready(self, received: int, produced: int = 0) -> int:
        """How many outputs can be produced from the first `received` inputs alone: the smallest j >= produced whose last
        input, start(j) + K - 1, has not arrived yet (start is non-decreasing in j)."""
        lo, hi = produced, max(produced, self.n_out(received) + self.phases + 1)
        if self.start(lo) + self.K - 1 >= received:
            return lo
        while self.start(hi) + self.K - 1 < received:  # (the window reaches past t: never more than a step or two)
            hi += self.phases
        while hi - lo > 1:  # start(lo) is ready, start(hi) is not
            mid = (lo + hi) // 2
            if self.start(mid) + self.K - 1 < received:
                lo = mid
            else:
                hi = mid
        return hi

    def device(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.taps).to(device), torch.from_numpy(self.first).to(device))
        return self._dev[key]


@lru_cache(maxsize=64)
def resample_plan(fi: int, fo: int) -> ResamplePlan:
    return ResamplePlan(fi, fo)


def resampled_length(n: int, fi: int, fo: int) -> int:
    """Samples at fo that n samples at fi become (no table is built)."""
    fi, fo = int(fi), int(fo)
    if fi <= 0 or fo <= 0:
        raise NotImplementedError(f"cannot resample from {fi} Hz to {fo} Hz: sample rates must be positive")
    return int(n) if fi == fo else (int(n) * fo + fi - 1) // fi


def _to_device_async(arr: np.ndarray, device) -> torch.Tensor:
    src = torch.from_numpy(arr)
    if torch.device(device).type != "cuda":
        return src.to(device)
    pinned = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
    pinned.copy_(src)
    return pinned.to(device, non_blocking=True)


def _runs(rates: Sequence[int]):
    """(begin, end, rate) of each run of equal neighbours."""
    b = 0
    for e in range(1, len(rates) + 1):
        if e == len(rates) or rates[e] != rates[b]:
            yield b, e, rates[b]
            b = e


class Resampler:
    """Ragged batch at mixed rates -> the same batch at `fo`."""

    def __init__(self, device, fo: int):
        self.device, self.fo = device, int(fo)

    def __call__(self, wav: torch.Tensor, offsets: torch.Tensor, n_samples: Sequence[int], rates: Sequence[int]):
        """wav: device fp32 or int16 concatenated samples; offsets: device int64 [B+1]; n_samples, rates: host, per utterance.
        Returns (wav at fo, fp32), its offsets (device int64 [B+1]) and the host lengths at fo.  With every rate equal to fo
        the arguments come back untouched.  One launch per run of neighbours that share a rate (a batch of one rate: one
        launch), each writing its utterances' slots of the one output buffer; utterances already at fo take the identity plan."""
        rates = [int(r) for r in rates]
        assert len(rates) == len(n_samples)
        if all(r == self.fo for r in rates):
            return wav, offsets, n_samples
        plans = [resample_plan(r, self.fo) for r in rates]
        n_out = [p.n_out(int(n)) for p, n in zip(plans, n_samples)]
        off = np.zeros(len(n_out) + 1, dtype=np.int64)
        np.cumsum(n_out, out=off[1:])
        out_off = _to_device_async(off, self.device)
        out = torch.empty(int(off[-1]), dtype=torch.float32, device=self.device)
        for b, e, r in _runs(rates):
            plan = plans[b]
            taps, first = plan.device(self.device)
            K.resample_batch(wav, offsets[b:e + 1], out, out_off[b:e + 1], e - b, taps, first, plan.in_unit, max(n_out[b:e]))
        return out, out_off, n_out


class _RStream:
    __slots__ = ("plan", "received", "produced", "base", "tail")

    def __init__(self, plan):
        self.plan = plan
        self.received = 0   # input samples accepted so far
        self.produced = 0   # output samples handed out so far
        self.base = 0       # absolute index of tail[0]
        self.tail = None    # device fp32: the inputs from `base` on that a later output still reads


class StreamResampler:
    """Piece-by-piece resampling of many streams: the outputs of a stream, concatenated, are the bits `Resampler` gives for the
    whole recording.  Per stream it keeps three host integers and the device tail of inputs that later outputs still read
    (at most K + ceil(fi / fo) samples once a piece has been processed)."""

    def __init__(self, device, fo: int):
        self.device, self.fo = device, int(fo)
        self.streams: Dict[object, _RStream] = {}

    def open(self, ids: Sequence, rates: Sequence[int]):
        for sid, r in zip(ids, rates):
            if sid in self.streams:
                raise ValueError(f"stream {sid!r} is already open")
            self.streams[sid] = _RStream(resample_plan(int(r), self.fo))

    def close(self, ids: Sequence):
        for sid in ids:
            self.streams.pop(sid, None)

    def rate(self, sid) -> int:
        return self.streams[sid].plan.fi

    def held(self, sid) -> int:
        st = self.streams[sid]
        return 0 if st.tail is None else int(st.tail.numel())

    def _launch(self, plan, wav, in_off, in_base, out, out_off, out_base, B, max_out):
        taps, first = plan.device(self.device)
        K.resample_batch(wav, in_off, out, out_off, B, taps, first, plan.in_unit, max_out, in_base=in_base, out_base=out_base)

    def accept(self, ids: Sequence, pieces: Sequence[torch.Tensor], final) -> List[torch.Tensor]:
        """pieces: one 1-D tensor of new samples per stream, at the stream's own rate.  Returns one fp32 tensor per stream: the
        samples at fo that these pieces complete (all that remain when `final`).  Streams at fo pass through untouched."""
        final = [final] * len(ids) if isinstance(final, bool) else list(final)
        outs: List[torch.Tensor] = [None] * len(ids)
        groups: Dict[int, list] = {}
        for b, (sid, w, fin) in enumerate(zip(ids, pieces, final)):
            st = self.streams[sid]
            w = w.to(self.device, torch.float32)
            if st.plan.fi == self.fo:
                outs[b] = w
                continue
            st.tail = w if st.tail is None or st.tail.numel() == 0 else torch.cat([st.tail, w])
            st.received += int(w.numel())
            upto = st.plan.n_out(st.received) if fin else min(st.plan.ready(st.received, st.produced), st.plan.n_out(st.received))
            groups.setdefault(st.plan.fi, []).append((b, st, max(upto, st.produced)))
        for members in groups.values():
            plan = members[0][1].plan
            counts = [upto - st.produced for _, st, upto in members]
            B = len(members)
            if max(counts) > 0:
                meta = np.zeros((4, B + 1), dtype=np.int64)  # in_offsets, out_offsets, in_base, out_base
                np.cumsum([int(st.tail.numel()) for _, st, _ in members], out=meta[0, 1:])
                np.cumsum(counts, out=meta[1, 1:])
                meta[2, :B] = [st.base for _, st, _ in members]
                meta[3, :B] = [st.produced for _, st, _ in members]
                m = _to_device_async(meta, self.device)
                wav = members[0][1].tail if B == 1 else torch.cat([st.tail for _, st, _ in members])
                out = torch.empty(int(meta[1, -1]), dtype=torch.float32, device=self.device)
                self._launch(plan, wav, m[0], m[2], out, m[1], m[3], B, max(counts))
            for g, (b, st, upto) in enumerate(members):
                outs[b] = out[int(meta[1, g]):int(meta[1, g + 1])] if counts[g] > 0 else torch.empty(0, dtype=torch.float32, device=self.device)
                st.produced = upto
                keep = max(st.base, min(max(0, plan.start(st.produced)), st.received))  # first input a later output reads
                if keep > st.base:
                    st.tail = st.tail[keep - st.base:]
                    st.base = keep
        return outs
