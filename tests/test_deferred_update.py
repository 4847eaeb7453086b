"""The deferred optimizer pass (FlatAdam.clip_and_step_split, Trainer.flush_update, the encoder's wait in front of its first layer):
the update of everything the model does not read before its first encoder layer runs on the Python-side stream, under the next
step's front-end and sub-sampler.

(a) split == whole, bit for bit, on a toy module whose declared early module lies in the middle of the flat buffer (two deferred
    ranges) or at its start (one).  The gradients are small integers, so that sumsq_kernel's atomic sum is exact in any order and
    the clip coefficient — hence every updated element — is reproducible between two launches.
(b) ordering (the pass is started from inside the next forward call, behind the sub-sampler's first layer), made deterministic by
    a bounded delay (torch.cuda._sleep) enqueued in front of every capped launch: whatever is not
    ordered behind the deferred pass then runs BEFORE it and reads the previous weights.
(c) a model that declares nothing keeps the single-launch path; flush_update clears a pending event."""
import numpy as np
import pytest
import torch
import torch.nn as nn

gpu = pytest.mark.gpu
DEV = "cuda:0"
DELAY_MS = 3.0
# |loss of the second step, delayed sequence - synchronised sequence| must stay within twice the largest difference seen between
# runs of the synchronised single-launch sequence itself (test_second_step_loss's docstring has the measurement)
LOSS_SPREAD = 0.19


def _bits_equal(what, a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    w = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[a.dtype]
    bad = a.view(w) != b.view(w)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {a.numel()} elements differ, first at {int(bad.flatten().nonzero()[0])}"


# ------------------------------------------------------------------ (a) split == whole
class Toy(nn.Module):
    def __init__(self, early):
        super().__init__()
        self.a, self.b, self.c = nn.Linear(257, 300), nn.Linear(64, 33), nn.Linear(1025, 700)
        self._early = early

    def early_update_modules(self):
        return [getattr(self, n) for n in self._early]


def _toy_pair(early):
    from espresso_amd.optim.adam import FlatAdam
    from espresso_amd.optim.flat import FlatParams

    pair = []
    for _ in range(2):
        torch.manual_seed(3)
        flat = FlatParams(Toy(early).to(DEV), DEV)
        pair.append((flat, FlatAdam(flat, lr=1e-2, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01)))
    return pair


@gpu
@pytest.mark.parametrize("early,ranges", [(("b",), 2), (("a",), 1), (("c",), None)], ids=["middle", "first", "too-large"])
def test_split_equals_whole(early, ranges):
    from espresso_amd import functional as F

    (f1, o1), (f2, o2) = _toy_pair(early)
    if ranges is None:  # c is 90 % of the buffer: not an early range
        assert f1.early_range is None
        return
    lo, hi = f1.early_range
    assert 0 <= lo < hi <= f1.numel and lo % 64 == 0 and hi % 64 == 0 and (hi - lo) <= 0.25 * f1.numel
    assert (lo > 0) + (hi < f1.numel) == ranges
    # every parameter of the early module inside, every other outside
    names = {id(p): n for n, p in zip("a.w a.b b.w b.b c.w c.b".split(), f1.params)}
    for p in f1.params:
        o = f1.offsets[id(p)]
        assert (lo <= o and o + p.numel() <= hi) == (names[id(p)][0] in early), names[id(p)]
    side, cur = F._side_stream(torch.device(DEV)), torch.cuda.current_stream(torch.device(DEV))
    gen = torch.Generator().manual_seed(11)
    denom = torch.full((1,), 4.0, device=DEV)
    for step in range(4):
        g = torch.randint(-3, 4, (f1.numel,), generator=gen).float()
        if step == 2:
            g[f1.numel // 2] = float("inf")  # an overflowed step: skipped by both, gradients dropped
        for f in (f1, f2):
            f.g32.copy_(g.to(DEV))
        hold = step % 2 == 1  # (held: nothing of the deferred part is launched before start() / wait())
        coef1, pend = o1.clip_and_step_split(side, pre_scale=1.0, max_norm=2.0, denom_dev=denom, hold=hold)
        assert pend.started != hold
        pend.wait(cur)
        assert pend.started and pend.start() is pend.start()
        coef2 = o2.clip_and_step(pre_scale=1.0, max_norm=2.0, denom_dev=denom)
        torch.cuda.synchronize()
        tag = f"early={early} step {step}: "
        assert bool(torch.isfinite(coef2).all()) == (step != 2)
        _bits_equal(tag + "coef", coef1, coef2)
        _bits_equal(tag + "p32", f1.p32, f2.p32)
        _bits_equal(tag + "p16", f1.p16, f2.p16)
        _bits_equal(tag + "exp_avg", o1.exp_avg, o2.exp_avg)
        _bits_equal(tag + "exp_avg_sq", o1.exp_avg_sq, o2.exp_avg_sq)
        assert not bool(f1.g32.any()) and not bool(f2.g32.any()), tag + "g32 not zero"
        assert float(o1._sumsq) == 0.0, tag + "the accumulator was not cleared"
        assert o1.step_count == o2.step_count == step + 1
    assert bool((f1.p32 != 0).any())


def test_early_range_on_the_cpu():
    """FlatParams.range_of: contiguity is verified, not assumed; padding is part of the range; frozen parameters do not count"""
    from espresso_amd.optim.flat import FlatParams

    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b, self.c, self.d = nn.Linear(100, 100), nn.Linear(3, 5), nn.Linear(100, 100), nn.Linear(7, 1)

    m = M()
    f = FlatParams(m, "cpu")
    assert f.early_range is None  # nothing declared
    o = lambda p: f.offsets[id(p)]
    assert f.range_of([m.b]) == (o(m.b.weight), o(m.c.weight)) and o(m.c.weight) - o(m.b.weight) == 128
    assert f.range_of([m.b, None]) == f.range_of([m.b])
    assert f.range_of([m.b, m.d]) is None       # c lies between them
    assert f.range_of([m.a]) is None            # 49 % of the buffer
    assert f.range_of([m.a], max_share=0.5) == (0, o(m.b.weight))
    assert f.range_of([]) is None and f.range_of([nn.Linear(2, 2)]) is None

    class Declares(M):
        def early_update_modules(self):
            return [self.d, self.b]

    assert FlatParams(Declares(), "cpu").early_range is None
    m = Declares()
    m.c.weight.requires_grad_(False)  # not in the flat buffer
    m.c.bias.requires_grad_(False)
    f = FlatParams(m, "cpu")
    assert f.early_range == (f.offsets[id(m.b.weight)], f.numel)


# ------------------------------------------------------------------ (b) ordering
def _sleep_cycles(ms):
    """torch.cuda._sleep counts device clock ticks: measure the tick once"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(100000)
    torch.cuda.synchronize()
    e0.record()
    torch.cuda._sleep(2000000)
    e1.record()
    torch.cuda.synchronize()
    return max(1, int(2000000 * ms / e0.elapsed_time(e1)))


def _tiny_trainer(defer_update=True):
    """the tiny Conformer-CTC of tests/gpu_checks.py (check_ddp_hooks: embed_dim 128, 2 heads, 2 layers) behind the real task,
    raw-audio batches of about one second"""
    from espresso_amd.data import synthetic
    from espresso_amd.tasks.speech_recognition import SpeechRecognitionEspressoConfig, SpeechRecognitionEspressoTask
    from espresso_amd.trainer import Trainer
    from tests.gpu_checks import _Task, build_tiny_model

    torch.manual_seed(0)
    d = _Task(40).target_dictionary
    task = SpeechRecognitionEspressoTask.setup_task(SpeechRecognitionEspressoConfig(criterion_name="ctc_loss"), tgt_dict=d)
    task.build_frontend(DEV)
    task.begin_epoch(1)
    model = build_tiny_model("conformer", embed_dim=128, heads=2)
    crit = task.build_criterion("ctc_loss", sentence_avg=True, zero_infinity=True)
    tr = Trainer(task, model, crit, torch.device(DEV), clip_norm=2.0, lr=1e-2, defer_update=defer_update,
                 lr_scheduler=("tri_stage", dict(warmup_steps=5, hold_steps=5, decay_steps=5)))
    n_samples = (np.array([1.0, 1.3, 0.8, 1.2, 0.9, 1.1]) * synthetic.SAMPLE_RATE).astype(np.int64)
    samples = [synthetic.make_sample(np.array(b), n_samples, 40, d.pad(), DEV, seed=1) for b in ([0, 1, 2], [3, 4, 5], [1, 2, 4])]
    tr.reserve(samples[:1])
    torch.cuda.synchronize()
    return tr, samples


def _synchronised_two_steps(split):
    """loss of the second of two update steps with a device synchronisation after each; split=False: the single-launch update"""
    tr, samples = _tiny_trainer()
    assert tr._split_update
    tr._split_update = split
    tr.train_step([samples[0]])
    torch.cuda.synchronize()
    out = tr.train_step([samples[1]])
    torch.cuda.synchronize()
    return float(out[1])


@pytest.fixture(scope="module")
def delayed():
    """two update steps back to back with every capped launch delayed by DELAY_MS on its stream, then the checks' raw material"""
    from espresso_amd import functional as F
    from espresso_amd import kernels as K

    tr, samples = _tiny_trainer()
    assert tr._split_update and tr.flat.early_range is not None
    cycles = _sleep_cycles(DELAY_MS)
    real = K.adam_step_capped
    calls = []

    snap = []

    def slow(*a, **kw):
        stream = a[13]
        calls.append(stream)
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
        rc = real(*a, **kw)
        if len(calls) == 2:  # the first step's pass is complete in the side stream's order, whatever the compute stream does
            with torch.cuda.stream(stream):
                snap.append(tr._flat.p16.clone())
        return rc

    logits = []
    hook = tr.model.encoder.register_forward_hook(lambda m, i, o: logits.append(o["_logits_bt"][0].detach().clone()))
    side = F._side_stream(torch.device(DEV))
    K.adam_step_capped = slow
    try:
        tr.train_step([samples[0]])
        first = tr._pending_update
        held_after_1 = not first.started and not calls  # held until the next forward pass has launched the sub-sampler's first layer
        out = tr.train_step([samples[1]])
        started_by_2 = first.started and len(calls) == 2
        pending_after_2 = not tr._pending_update.started
        loss2 = out[1:2].clone()
        del logits[:]
        tr.valid_step(samples[2])
        torch.cuda.synchronize()
        tr.valid_step(samples[2])
        torch.cuda.synchronize()
    finally:
        K.adam_step_capped = real
        hook.remove()
    return dict(tr=tr, calls=calls, side=side, p16_after_1=snap[0], pending_after_2=pending_after_2, loss2=float(loss2),
                logits=logits, held_after_1=held_after_1, started_by_2=started_by_2)


@gpu
def test_delay_was_in_effect(delayed):
    """both steps deferred two ranges to the side stream; the first step's pass was held until the second step's forward pass,
    the second step's until valid_step flushed it"""
    assert len(delayed["calls"]) == 4 and all(s == delayed["side"] for s in delayed["calls"])
    assert delayed["held_after_1"] and delayed["started_by_2"] and delayed["pending_after_2"]
    assert delayed["tr"]._pending_update is None and delayed["tr"].model.encoder.pending_update is None  # valid_step flushed


@gpu
def test_valid_step_waits_for_the_update(delayed):
    """eval logits right behind the delayed update == the same call after a device synchronisation (the eval forward has no atomics)"""
    a, b = delayed["logits"]
    _bits_equal("valid_step logits", a, b)
    assert bool(torch.isfinite(a.float()).all()) and bool((a != 0).any())


@gpu
def test_weight_transposes_follow_the_update(delayed):
    """the k-contiguous copies the second training forward left (csrc/engine.hip WT: ffn1.w_1 at 0, wqkv at 2 C F) are the
    transposes of the bf16 weights as the first step's update wrote them — w_1 lies behind the early range, wqkv in front of it"""
    tr, p16 = delayed["tr"], delayed["p16_after_1"]
    lo, hi = tr.flat.early_range
    for layer in tr.model.encoder.layers:
        bind = layer._ea_binding
        assert bind is not None
        C, Fd = layer.embed_dim, layer.ffn1.w_1.weight.shape[0]
        o1, oq = tr.flat.offsets[id(layer.ffn1.w_1.weight)], tr.flat.offsets[id(layer.self_attn.q_proj.weight)]
        assert o1 >= hi and oq + 3 * C * C <= lo
        assert not torch.equal(p16[o1:o1 + Fd * C], tr.flat.p16[o1:o1 + Fd * C])  # (the second update moved on: p16 itself is no reference)
        _bits_equal("w_1^T", bind.wt[:C * Fd].view(C, Fd), p16[o1:o1 + Fd * C].view(Fd, C).t().contiguous())
        _bits_equal("wqkv^T", bind.wt[2 * C * Fd:2 * C * Fd + 3 * C * C].view(C, 3 * C), p16[oq:oq + 3 * C * C].view(3 * C, C).t().contiguous())


@gpu
def test_second_step_loss(delayed):
    """the second step's loss == that of the same two steps with a device synchronisation between them, within 2 x LOSS_SPREAD.
    LOSS_SPREAD is the largest difference between runs of the synchronised SINGLE-LAUNCH sequence (the path before this change:
    BatchNorm statistics are summed with atomics, so two runs need not agree).  Measured on an MI355X over 8 runs of that sequence:
    the loss (a sum of about 260 over the batch) took the two values 260.3251037597656 (6 runs) and 260.1355285644531 (2 runs),
    spread 0.1896 -> LOSS_SPREAD = 0.19.  The delayed sequence gave 260.3251037597656 in both runs made of it."""
    ref = _synchronised_two_steps(split=False)
    print(f"second-step loss: delayed {delayed['loss2']!r} synchronised single-launch {ref!r} diff {abs(delayed['loss2'] - ref)!r}")
    assert abs(delayed["loss2"] - ref) <= 2 * LOSS_SPREAD


# ------------------------------------------------------------------ (c) fallback
@gpu
def test_fallback_and_flush():
    from espresso_amd.trainer import Trainer

    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = nn.Linear(8, 4), nn.Linear(4, 4)

        def forward(self, x):
            return self.b(self.a(x))

    class Task:
        def prepare_sample(self, sample, train=True):
            return sample

        def valid_step(self, sample, model, criterion):
            return criterion(model, sample)

    def crit(model, sample):
        return model(sample["x"]).pow(2).sum(), 2, {"ntokens": 5, "nsentences": 2}

    torch.manual_seed(0)
    t = Trainer(Task(), M(), crit, torch.device(DEV), lr=1e-3, defer_update=True,
                lr_scheduler=("tri_stage", dict(warmup_steps=10, hold_steps=10, decay_steps=10)))
    assert t.flat.early_range is None and not t._split_update  # asked for, but the model declares nothing
    t._optimizer.clip_and_step_split = None  # (a call would raise)
    before = t.flat.p32.clone()
    out = t.train_step([{"x": torch.randn(2, 8, device=DEV)}])
    assert out is not None and t._pending_update is None and t.num_updates == 1
    torch.cuda.synchronize()
    assert not torch.equal(before, t.flat.p32) and not bool(t.flat.g32.any())
    # not asked for: the single launch, whatever the model declares
    off, samples = _tiny_trainer(defer_update=False)
    assert off.flat.early_range is not None and not off._split_update
    off._optimizer.clip_and_step_split = None
    assert off.train_step([samples[0]]) is not None and off._pending_update is None and off.model.encoder.pending_update is None
    # a pending event is waited for and cleared, on a model with and without the hook
    tr, _ = _tiny_trainer()
    from espresso_amd.optim.adam import PendingUpdate

    for trainer in (tr, t):
        ev = torch.cuda.Event()
        ev.record()
        trainer._pending_update = pend = PendingUpdate(lambda: ev)
        if trainer is tr:
            tr.model.defer_update(pend)
        trainer.flush_update()
        assert trainer._pending_update is None and pend.started
        trainer.flush_update()  # nothing pending: a no-op
    # reading the trainer's buffers completes a held update
    tr._pending_update = pend = PendingUpdate(lambda: ev)
    assert tr.optimizer is tr._optimizer and pend.started and tr._pending_update is None
    tr._pending_update = pend = PendingUpdate(lambda: ev)
    assert tr.flat is tr._flat and pend.started and tr._pending_update is None
    tr.model.defer_update(PendingUpdate(lambda: ev))
    tr.model.state_dict()
    assert tr.model.encoder.pending_update is None
    assert tr.model.encoder.pending_update is None
