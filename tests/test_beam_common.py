"""tools/beam_common.py on the host: the slot pool and the packing of an `accept`, the carried rows, the hypothesis lists, the
single readback of `partial` and the LM stepping.  No GPU: the tensors are CPU tensors, ea_gather_rows is stood in for by
index_select where a test needs it."""
import math

import pytest
import torch

from espresso_amd import kernels
from espresso_amd.tools.beam_common import BeamDecoderMixin, CarriedRows, StreamSlots, hyps_from_tensors, step_triple
from espresso_amd.tools.transducer_frame_beam_decoder import TransducerFrameBeamDecoder

CPU = torch.device("cpu")


# ---- the slot pool ---------------------------------------------------------------------------------------------------------
def test_slots_are_handed_out_in_order_and_reused():
    pool = StreamSlots("some search", 3, 8)
    pool.open(["a", "b", "c"])
    assert [pool.streams[s] for s in "abc"] == [[0, 0], [1, 0], [2, 0]] and pool._unreset == [0, 1, 2]
    with pytest.raises(RuntimeError, match="stream slots are in use"):
        pool.open(["d"])
    with pytest.raises(ValueError, match="already open"):
        pool.open(["a"])
    assert pool._unreset == [0, 1, 2] and set(pool.streams) == set("abc")
    pool._unreset = []  # what a decoder's _ensure does after its reset launch
    pool._release("b")
    assert "b" not in pool.streams
    pool.open(["d"])
    assert pool.streams["d"] == [1, 0] and pool._unreset == [1]
    assert pool._slots_of(["c", "d", "a"], CPU).tolist() == [2, 1, 0] and pool._slots_of(["a"], CPU).dtype == torch.int32


def test_constructor_names_the_search():
    with pytest.raises(ValueError, match="streaming CTC prefix beam search: max_streams 0 and max_frames 5 must be positive"):
        StreamSlots("streaming CTC prefix beam search", 0, 5)
    with pytest.raises(ValueError, match="must be positive"):
        StreamSlots("some search", 2, 0)


def test_check_room_refuses_one_frame_too_many():
    pool = StreamSlots("some search", 2, 8)
    pool.open(["a", "b"])
    pool.streams["a"][1] = 5
    pool._check_room(["a", "b"], [3, 8])  # 5 + 3 == 8 == 0 + 8: both fit
    with pytest.raises(ValueError, match=r"stream 'a': 5 \+ 4 encoder frames exceed max_frames 8"):
        pool._check_room(["a", "b"], [4, 1])
    assert pool._max_u(["a", "b"]) == 5 and pool._max_u(["b"]) == 1 and pool._max_u([]) == 1


# ---- the packing of an accept ----------------------------------------------------------------------------------------------
def test_pack_lists_the_streams_that_got_frames():
    pool = StreamSlots("some search", 5, 12)
    pool.open([9, 0, 1, 2, 3])  # stream 9 takes slot 0, so that slots and stream ids differ
    counts = [10, 0, 3, 10]
    ready, meta = pool._pack([0, 1, 2, 3], counts, torch.zeros(sum(counts), 7))
    assert meta.dtype == torch.int32 and tuple(meta.shape) == (3, 3) and meta.is_contiguous()
    assert meta[0].tolist() == [pool.streams[s][0] for s in (0, 2, 3)] == [1, 3, 4]
    assert meta[1].tolist() == [10, 3, 10]
    assert meta[2].tolist() == [0, 10, 13]  # the idle stream has no rows, the offsets are those into the packed rows
    assert [st for st, _, _ in ready] == [pool.streams[s] for s in (0, 2, 3)]
    assert all(pool.streams[s][1] == 0 for s in (0, 1, 2, 3))  # nothing is consumed before the launches
    pool._advance(ready)
    assert [pool.streams[s][1] for s in (0, 1, 2, 3, 9)] == [10, 0, 3, 10, 0]


def test_pack_with_nothing_to_do_and_with_too_much():
    pool = StreamSlots("some search", 4, 12)
    pool.open([0, 1, 2, 3])
    ready, meta = pool._pack([0, 1, 2, 3], [0, 0, 0, 0], torch.zeros(0, 7))
    assert not ready and meta is None
    with pytest.raises(ValueError, match="max_frames"):
        pool._pack([0, 1], [13, 1], torch.zeros(14, 7))
    with pytest.raises(AssertionError):
        pool._pack([0, 0], [1, 1], torch.zeros(2, 7))  # a stream listed twice
    with pytest.raises(AssertionError):
        pool._pack([0, 1], [1, 1], torch.zeros(3, 7))  # rows that are not the counts' sum
    assert all(st == [slot, 0] for slot, st in enumerate(pool.streams.values()))


# ---- the carried rows -------------------------------------------------------------------------------------------------------
BEAM, SLOTS, H, W = 3, 4, 5, 7


def _carried(monkeypatch):
    monkeypatch.setattr(kernels, "gather_rows", lambda src, rows: src.index_select(0, rows.long()))
    g = torch.Generator().manual_seed(3)
    R = SLOTS * BEAM
    state = {"h16": [torch.randn(R, H, generator=g).bfloat16() for _ in range(2)], "h32": [torch.randn(R, H, generator=g) for _ in range(2)],
             "c": [torch.randn(R, H, generator=g) for _ in range(2)]}
    start_state = {k: [torch.randn(1, H, generator=g).to(t.dtype) for t in v] for k, v in state.items()}
    row, start_row = torch.randn(R, W, generator=g), torch.randn(1, W, generator=g)
    rows = CarriedRows(BEAM, SLOTS, [(state, start_state), (row, start_row)])
    tensors = [t for v in state.values() for t in v] + [row]
    starts = [s for v in start_state.values() for s in v] + [start_row]
    return rows, tensors, starts


def test_carried_rows_reset_touches_the_slots_rows_only(monkeypatch):
    rows, tensors, starts = _carried(monkeypatch)
    assert rows.rows_of(torch.tensor([2, 0], dtype=torch.int32)).tolist() == [6, 7, 8, 0, 1, 2]
    before = [t.clone() for t in tensors]
    rows.reset(torch.tensor([2], dtype=torch.int32))
    for t, b, s in zip(tensors, before, starts):
        assert torch.equal(t[6:9], s.expand(3, -1))
        assert torch.equal(t[:6], b[:6]) and torch.equal(t[9:], b[9:])


def test_carried_rows_scatter_of_gather_is_the_identity(monkeypatch):
    rows, tensors, _ = _carried(monkeypatch)
    idx = rows.rows_of(torch.tensor([3, 1], dtype=torch.int32))
    before = [t.clone() for t in tensors]
    state, row = rows.gather(idx)
    assert set(state) == {"h16", "h32", "c"} and all(len(v) == 2 and tuple(v[0].shape) == (6, H) for v in state.values())
    assert torch.equal(row, before[-1][idx.long()]) and torch.equal(state["c"][1], before[5][idx.long()])
    rows.scatter(idx, [state, row])
    assert all(torch.equal(t, b) for t, b in zip(tensors, before))
    # new values land in the listed slots' rows, every other slot's rows stay bit-equal
    rows.scatter(idx, [{k: [t + 1 for t in v] for k, v in state.items()}, row + 1])
    for t, b in zip(tensors, before):
        assert torch.equal(t[idx.long()], b[idx.long()] + 1)
        assert torch.equal(t[0:3], b[0:3]) and torch.equal(t[6:9], b[6:9])


# ---- hypothesis lists and the triple ----------------------------------------------------------------------------------------
def test_hyps_from_tensors():
    tokens = torch.tensor([[[5, 6, 7, 1], [8, 1, 1, 1]], [[1, 1, 1, 1], [1, 1, 1, 1]], [[9, 9, 1, 1], [4, 3, 2, 2]]], dtype=torch.int32)
    lengths = torch.tensor([[3, 1], [0, 0], [0, 4]], dtype=torch.int32)
    scores = torch.tensor([[-1.5, -2.5], [0.0, 0.0], [-0.25, float("-inf")]])
    hyps = hyps_from_tensors(tokens, lengths, scores, torch.tensor([2, 0, 2], dtype=torch.int32))
    assert [len(h) for h in hyps] == [2, 0, 2] and hyps[1] == []
    assert [h["tokens"].tolist() for h in hyps[0] + hyps[2]] == [[5, 6, 7], [8], [], [4, 3, 2, 2]]
    assert all(h["tokens"].dtype == torch.long and h["attention"] is None and h["alignment"] is None for u in hyps for h in u)
    assert set(hyps[0][0]) == {"tokens", "score", "attention", "alignment"}
    for b, i in ((0, 0), (0, 1), (2, 0), (2, 1)):  # the very element of `scores`, not a copy
        assert hyps[b][i]["score"].data_ptr() == scores[b, i].data_ptr() and torch.equal(hyps[b][i]["score"], scores[b, i])


def test_step_triple():
    parent, token, keep = step_triple(6, CPU)
    assert parent.dtype == token.dtype == torch.int32 and keep.dtype == torch.uint8
    assert parent.shape == token.shape == keep.shape == (6,)


# ---- the readback of partial ------------------------------------------------------------------------------------------------
def test_partial_readback_keeps_the_score_bits():
    tokens = torch.tensor([[4, 5, 6, 1, 1], [7, 1, 1, 1, 1], [1, 1, 1, 1, 1]], dtype=torch.int32)
    lengths = torch.tensor([3, 1, 0], dtype=torch.int32)
    stable = torch.tensor([2, 1, 0], dtype=torch.int32)
    scores = torch.tensor([-3.1415927, float("-inf"), 0.0], dtype=torch.float32)
    got = StreamSlots._read_partial(tokens, lengths, scores, stable)
    assert [(t, k) for t, k, _ in got] == [([4, 5, 6], 2), ([7], 1), ([], 0)]
    assert all(isinstance(s, float) for _, _, s in got)
    back = torch.tensor([s for _, _, s in got], dtype=torch.float32)
    assert torch.equal(back.view(torch.int32), scores.view(torch.int32)) and math.isinf(got[1][2]) and got[1][2] < 0


# ---- the LM stepping --------------------------------------------------------------------------------------------------------
class _FakeLMDecoder:
    def __init__(self, calls):
        self.calls = calls

    def init_state(self, N, device):
        self.calls.append(("init_state", N))
        return {"n": 0}

    def reorder_state(self, state, parent):
        self.calls.append(("reorder_state", parent.tolist()))
        return {"n": state["n"], "parent": parent.tolist()}

    def advance(self, tokens, state, keep_row=None):
        self.calls.append(("advance", tokens.tolist(), None if keep_row is None else keep_row.tolist()))
        return torch.zeros(tokens.numel(), 2), {"n": state["n"] + 1}

    def output_layer(self, feat):
        return feat


class _FakeLM:
    def __init__(self, calls):
        self.decoder = _FakeLMDecoder(calls)


class _Decoder(BeamDecoderMixin):
    eos, blank = 2, 0

    def __init__(self, calls):
        self.lm_model = _FakeLM(calls)

    def _lm_rows(self, feat):  # the library's log-softmax needs the GPU
        return ("rows", tuple(feat.shape))


class _NoBlankDecoder(_Decoder):
    no_blank_in_lm = True
    _lm_tokens = TransducerFrameBeamDecoder._lm_tokens


@pytest.mark.parametrize("cls, shift", [(_Decoder, 0), (_NoBlankDecoder, 1)])
def test_lm_stepping(cls, shift):
    calls = []
    dec = cls(calls)
    state, rows = dec.lm_start(3, CPU)
    assert calls == [("init_state", 3), ("advance", [2 - shift] * 3, None)] and state == {"n": 1} and rows == ("rows", (3, 2))
    del calls[:]
    parent = torch.tensor([1, 1, 0], dtype=torch.int32)
    token = torch.tensor([5, 0, 1], dtype=torch.int32)  # above blank, blank, just above blank
    keep = torch.tensor([0, 1, 0], dtype=torch.uint8)
    state, rows = dec.lm_update(state, parent, token, keep)
    assert calls == [("reorder_state", [1, 1, 0]), ("advance", [5 - shift, 0, 1 - shift], [0, 1, 0])]
    assert state == {"n": 2} and rows == ("rows", (3, 2))


def test_decode_takes_the_best_hypothesis_up_to_its_length():
    class Dec(BeamDecoderMixin):
        def _generate(self, sample):
            tokens = torch.tensor([[[4, 5, 1, 1], [6, 6, 6, 6]], [[7, 1, 1, 1], [1, 1, 1, 1]]], dtype=torch.int32)
            return tokens, torch.tensor([[2, 4], [1, 0]], dtype=torch.int32), torch.tensor([[-1.0, -2.0], [-3.0, -4.0]]), None

    tokens, scores, extra = Dec().decode(None, {})
    assert tokens.dtype == torch.long and tokens.tolist() == [[4, 5], [7, 1]] and scores.tolist() == [-1.0, -3.0] and extra is None
