"""One-process-per-GPU trainer for the hot path: the update step of fairseq/trainer.py:780-1097
(micro-batches with no_sync -> grad sync -> multiply_grads(world/sample_size) -> clip_grad_norm ->
Adam -> lr schedule) re-scheduled for MI355X: gradient buckets are reduced by RCCL while backward is
still running, the per-step scalars (sample_size, loss, ntokens, nsentences) ride ONE small
all-reduce and stay on the device, and scaling + clipping + Adam + bf16 re-cast + grad zeroing are
a single streaming pass over the flat buffers.  No host synchronisation happens inside a step."""
import contextlib

import torch
import torch.distributed as dist

from . import functional as F
from . import kernels as K
from .distributed.overlapped_ddp import OverlappedDistributedDataParallel
from .optim.adam import FlatAdam
from .optim.flat import FlatParams
from .optim.noam_lr_scheduler import NoamSchedule


def grad_norms_inconsistent(norms: torch.Tensor) -> torch.Tensor:
    """1.0 (as a one-element tensor on `norms`' device) when the per-rank gradient norms differ — fairseq/trainer.py:1462-1475:
    consistent = max |g_r - g_0| / (g_0 + 1e-6) < 1e-6, or every norm is non-finite (all ranks overflowed alike)."""
    g0 = norms[0]
    close = ((norms - g0).abs().max() / (g0 + 1e-6)) < 1e-6
    all_bad = (~torch.isfinite(norms)).all()
    return (~(close | all_bad)).to(torch.float32).reshape(1)


class Trainer:
    def __init__(self, task, model, criterion, device, clip_norm=2.0, lr=5.0, warmup_steps=25000, adam_betas=(0.9, 0.98),
                 adam_eps=1e-8, weight_decay=0.0, final_lr=1e-6, seed=1, bucket_mb=64.0, lr_scheduler=None, defer_update=True):
        """`lr_scheduler`: optional `(name, kwargs)` resolved through the registry (default: the headline recipe's `noam`).
        `defer_update`: run most of the optimizer pass under the next step's sub-sampler when the model allows it (below)."""
        self.task, self.criterion, self.device = task, criterion, device
        self.model = model.to(device)
        self._flat = FlatParams(self.model, device)
        self._optimizer = FlatAdam(self._flat, lr=lr, betas=adam_betas, eps=adam_eps, weight_decay=weight_decay)
        if lr_scheduler is None:
            self.lr_scheduler = NoamSchedule(self._optimizer, lr=lr, warmup_steps=warmup_steps,
                                             model_size=model.cfg.encoder.embed_dim, final_lr=final_lr)
        else:
            from . import registry
            from .optim import lr_schedulers  # noqa: F401  (registers tri_stage / polynomial_decay_v2 / reduce_lr_on_plateau_v2)

            name, kw = lr_scheduler
            self.lr_scheduler = registry.LR_SCHEDULER_REGISTRY[name](self._optimizer, lr=lr, **kw)
        self.cfg = None
        self._optim_history = []
        self.world_size = dist.get_world_size() if dist.is_initialized() else 1
        self.ddp = OverlappedDistributedDataParallel(self.model, self._flat, bucket_mb=bucket_mb)
        self.clip_norm = clip_norm
        self.seed = seed
        self.num_updates = 0
        # [sample_size, loss, ntokens, nsentences] + one slot per rank for the cross-rank gradient-norm check (below)
        self._stats = torch.zeros(4 + (self.world_size if self.world_size > 1 else 0), dtype=torch.float32, device=device)
        self._gnorm_mismatch = torch.zeros(1, dtype=torch.float32, device=device)  # updates whose gradient norms differed across ranks
        self.last_coef = None
        self.ooms = 0  # updates skipped after an out-of-memory error (fairseq/trainer.py:797,850)
        self._train_mode_checked = False
        # defer_update: the optimizer pass over everything the model does not read before its first encoder layer (98 % of the
        # Conformer-CTC model) is HELD at the end of train_step and started by the model's next forward pass on the Python-side
        # stream, behind the sub-sampler's first layer, so that it runs beside the MFMA-bound gather convolutions; the model waits
        # for it in front of its first encoder layer (model.defer_update).  Until then the buffers outside the early range hold the
        # previous step's values: every other reader goes through flush_update() — the methods below, and the `flat` /
        # `optimizer` attributes themselves.  A model that does not declare its early modules, or a CPU run, keeps the single launch.
        self._split_update = (bool(defer_update) and torch.device(device).type == "cuda" and self._flat.early_range is not None
                              and hasattr(self.model, "defer_update"))
        self._pending_update = None

    @property
    def flat(self):
        """The flat parameter / gradient buffers, complete: reading this attribute (or `optimizer`) finishes a deferred update."""
        self.flush_update()
        return self._flat

    @property
    def optimizer(self):
        self.flush_update()
        return self._optimizer

    def flush_update(self):
        """The compute stream waits for a deferred optimizer pass (no-op when none is pending).  Called before anything but the
        model's own training forward touches parameters, gradients or optimizer state."""
        pending, self._pending_update = self._pending_update, None
        if pending is not None:
            pending.wait(torch.cuda.current_stream(self._flat.p32.device))
            if hasattr(self.model, "defer_update"):
                self.model.defer_update(None)

    def train_step(self, samples):
        """One optimizer update over a list of micro-batches (update_freq = len(samples))."""
        F.set_dropout_seed(self.seed + self.num_updates)  # trainer.py:782 _set_seed
        if not self._split_update:
            self.flush_update()
        if not self.model.training or not self._train_mode_checked:
            # nn.Module.train() walks every sub-module (2 300 of them: 1.1 ms of host time per update); once the whole tree is
            # in training mode the root flag tells (eval() / train() always set the tree as a whole)
            self.model.train()
            self._train_mode_checked = True
        self._stats.zero_()
        F.begin_step(self._stats.device)  # one fill for all the small zero-initialised accumulators of this update
        for i, sample in enumerate(samples):
            last = i == len(samples) - 1
            ctx = contextlib.nullcontext() if last else self.ddp.no_sync()
            dummy = bool(sample.get("_dummy", False))  # rank ran out of batches: same collectives, no contribution (trainer.py:873-877)
            try:
                with ctx:
                    sample = self.task.prepare_sample(sample, train=True)
                    loss, sample_size, log = self.criterion(self.ddp, sample)
                    if dummy:
                        loss = loss * 0.0
                    with F.accumulating_backward():  # (this trainer owns the flat gradient buffer the kernels write into)
                        loss.backward()
            except RuntimeError as e:
                if "out of memory" not in str(e).lower():
                    raise
                self._recover_from_oom(e)  # raises on more than one rank
                return None
            if dummy:
                continue
            if self._stats.is_cuda:
                # the four running sums in one launch (the loss is read from its device tensor: no host read)
                K.stats_add4(self._stats, float(sample_size), loss.detach().reshape(1).float(), float(log["ntokens"]),
                             float(log["nsentences"]))
            else:
                # (in-place adds on one-element views: `stats[i] += x` would be view + add + copy-back, two launches each)
                self._stats[0:1].add_(float(sample_size))
                self._stats[1:2].add_(loss.detach().reshape(1))
                self._stats[2:3].add_(float(log["ntokens"]))
                self._stats[3:4].add_(float(log["nsentences"]))
        if self.ddp.active:
            if self.world_size > 1 and self.last_coef is not None:
                # fairseq/trainer.py:1451-1488 _check_grad_norms: every rank must have clipped the SAME gradient norm (they
                # all-reduced the same buckets) — ranks that drifted apart train different models silently.  The reference
                # all-gathers the norms in their own collective; here rank r writes the norm of the PREVIOUS update into its
                # slot of the statistics vector, so the sum all-reduce that carries the step's scalars is also the gather
                # (4 more bytes per rank, no extra collective, no host read: the verdict accumulates on the device and is
                # read with the logging statistics, one update late).
                self._stats[4 + dist.get_rank():5 + dist.get_rank()].copy_(self.last_coef[1:2])
            dist.all_reduce(self._stats)  # C3 + sample_size (+ the gathered norms) in one small collective
            if self.world_size > 1 and self.last_coef is not None:
                self._gnorm_mismatch += grad_norms_inconsistent(self._stats[4:])
        self.ddp.all_reduce_grads()
        F.end_step()
        if self._split_update:
            self.last_coef, self._pending_update = self._optimizer.clip_and_step_split(
                F._side_stream(self._flat.p32.device), pre_scale=1.0, max_norm=self.clip_norm, denom_dev=self._stats[0:1], hold=True)
            self.model.defer_update(self._pending_update)
        else:
            self.last_coef = self._optimizer.clip_and_step(pre_scale=1.0, max_norm=self.clip_norm, denom_dev=self._stats[0:1])
        self.num_updates += 1
        if hasattr(self.model, "set_num_updates"):
            self.model.set_num_updates(self.num_updates)
        self.lr_scheduler.step_update(self.num_updates)
        return self._stats[:4]

    def _recover_from_oom(self, exc):
        """fairseq/trainer.py:842-857: a device out-of-memory error in the forward / backward pass of a micro-batch is logged, the
        gradients accumulated so far are dropped, the allocator cache is released and — with ONE worker — the update is skipped
        (`train_step` returns None, the loop carries on with the next batch).  With more workers the reference lets the worker
        contribute zeros to its end-of-backward all-reduce; here buckets of this update may already be in flight when the error
        arrives (that overlap is the point of the wrapper), so the update cannot be withdrawn on one rank only: the error is
        re-raised with that explanation."""
        import sys

        self.ooms += 1
        print(f"| WARNING: ran out of memory in the forward/backward pass of update {self.num_updates + 1} ({exc}); "
              f"{'skipping the update' if self.world_size == 1 else 'cannot skip on one rank of ' + str(self.world_size)}", file=sys.stderr)
        if self.world_size > 1:
            raise RuntimeError("out of memory on one data-parallel rank: gradient buckets of this update may already be in flight, "
                               "the update cannot be skipped consistently (lower max_tokens / batch_size)") from exc
        F.end_step()
        for m in self.model.modules():  # layers whose forward ran but whose backward never did: their saved-activation arenas are free again
            b = getattr(m, "_ea_binding", None)
            if b is not None:
                b.saved_busy = False
            m.__dict__.pop("_ea_chain_in", None)  # (a chained layer call whose successor never ran: drop its token and the tensors it holds)
            m.__dict__.pop("_ea_wt_fresh", None)
        self.flush_update()
        self._flat.zero_grad()
        self._stats.zero_()
        if self._stats.is_cuda:
            torch.cuda.synchronize(self._stats.device)
            torch.cuda.empty_cache()

    def check_grad_norm_consistency(self):
        """Host read (call it where the training statistics are read anyway): raises like fairseq/trainer.py:1477-1488 when any
        update since the last call saw different gradient norms on different ranks."""
        bad = float(self._gnorm_mismatch)
        self._gnorm_mismatch.zero_()
        if bad > 0:
            raise FloatingPointError(
                f"Fatal error: gradients are inconsistent between workers ({int(bad)} update(s) since the last check). "
                "Try --ddp-backend=legacy_ddp. Or are you mixing up different generation of GPUs in training?")

    def reserve(self, samples):
        """Size every grow-only arena (saved activations per layer, scratch, split-K slabs, allocator pools) for the largest
        batch shapes that will be seen: one forward + backward over each given sample with gradient reduction disabled,
        gradients and BatchNorm statistics restored afterwards; no optimizer update.  Called once at start-up (the reference's
        trainer does the same for the CUDA caching allocator with its dummy-batch / OOM-recovery logic, trainer.py:803-855)."""
        self.flush_update()
        bn = {n: b.clone() for n, b in self.model.named_buffers()}
        self.model.train()
        with self.ddp.no_sync():
            for sample in samples:
                sample = self.task.prepare_sample(sample, train=True)
                loss, _, _ = self.criterion(self.ddp, sample)
                with F.accumulating_backward():
                    loss.backward()
        self._flat.zero_grad()
        with torch.no_grad():
            for n, b in self.model.named_buffers():
                b.copy_(bn[n])
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    def valid_step(self, sample):
        self.flush_update()
        return self.task.valid_step(sample, self.model, self.criterion)

    # ---- configuration, learning-rate bookkeeping, checkpoints (fairseq/trainer.py:387-640, checkpoint_utils.py) ----

    @classmethod
    def from_cfg(cls, cfg, task, model, criterion, device):
        """Trainer from a recipe configuration (espresso_amd/config.py: groups optimization / optimizer / lr_scheduler / common)."""
        from .config import as_list, literal

        opt, optim = cfg["optimization"], cfg["optimizer"]
        if optim.get("_name", "adam") != "adam":
            raise NotImplementedError(f"optimizer {optim.get('_name')!r} (every ASR recipe of the reference uses adam)")
        sched = dict(cfg["lr_scheduler"])
        name = sched.pop("_name")
        sched.pop("lr", None)
        if name in ("reduce_lr_on_plateau_v2", "reduce_lr_on_plateau"):
            sched.setdefault("maximize_best_checkpoint_metric", cfg["checkpoint"]["maximize_best_checkpoint_metric"])
        if name == "tri_stage":
            sched.setdefault("max_update", opt["max_update"])
            if sched.get("phase_ratio") is not None:
                sched["phase_ratio"] = literal(sched["phase_ratio"])
        t = cls(task, model, criterion, device, clip_norm=float(opt["clip_norm"]), lr=float(as_list(opt["lr"])[0]),
                adam_betas=tuple(literal(optim["adam_betas"])), adam_eps=float(optim["adam_eps"]),
                weight_decay=float(optim["weight_decay"]), seed=int(cfg["common"]["seed"]), lr_scheduler=(name, sched))
        t.cfg = cfg
        return t

    def get_lr(self):
        return self._optimizer.get_lr()

    def lr_step_begin_epoch(self, epoch):
        if hasattr(self.lr_scheduler, "step_begin_epoch"):
            self.lr_scheduler.step_begin_epoch(epoch)
        return self.get_lr()

    def lr_step(self, epoch, val_loss=None):
        """End-of-epoch schedule hook (trainer.py:1134-1138)."""
        if hasattr(self.lr_scheduler, "step"):
            self.lr_scheduler.step(epoch, val_loss)
        return self.get_lr()

    def _optimizer_state(self):
        """torch.optim.Adam layout over `model.parameters()` order — what fairseq's FairseqAdam writes as
        `last_optimizer_state` (fairseq/optim/adam.py:159-240), so either side can resume the other's checkpoint."""
        self.flush_update()
        f, o = self._flat, self._optimizer
        state, ids = {}, []
        for i, p in enumerate(q for q in self.model.parameters() if q.requires_grad):
            off, n = f.offsets[id(p)], p.numel()
            state[i] = {"step": o.step_count, "exp_avg": o.exp_avg[off:off + n].view(p.shape).clone().cpu(),
                        "exp_avg_sq": o.exp_avg_sq[off:off + n].view(p.shape).clone().cpu()}
            ids.append(i)
        group = {"lr": o.lr, "betas": tuple(o.betas), "eps": o.eps, "weight_decay": o.weight_decay, "amsgrad": False, "params": ids}
        return {"state": state, "param_groups": [group]}

    def _load_optimizer_state(self, sd):
        self.flush_update()
        f, o = self._flat, self._optimizer
        params = [q for q in self.model.parameters() if q.requires_grad]
        if len(sd["state"]) not in (0, len(params)):
            raise ValueError(f"optimizer state holds {len(sd['state'])} parameters, the model has {len(params)}")
        for i, p in enumerate(params):
            st = sd["state"].get(i)
            if st is None:
                continue
            off, n = f.offsets[id(p)], p.numel()
            o.exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1))
            o.exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            o.step_count = int(st["step"])
        if sd.get("param_groups"):
            o.lr = sd["param_groups"][0].get("lr", o.lr)

    def state_dict(self, extra_state=None):
        """Checkpoint dictionary with the reference's top-level keys (fairseq/trainer.py:387-431)."""
        self.flush_update()
        sched = self.lr_scheduler.state_dict() if hasattr(self.lr_scheduler, "state_dict") else {}
        extra = {"previous_training_time": 0.0}
        extra.update(extra_state or {})
        no_optim = bool(((self.cfg or {}).get("checkpoint") or {}).get("no_save_optimizer_state", False))  # trainer.py:422
        sd = {
            "args": None,
            "cfg": self.cfg,
            "model": {k: v.detach().clone().cpu() for k, v in self.model.state_dict().items()},
            "criterion": None,
            "optimizer_history": self._optim_history + [{
                "criterion_name": type(self.criterion).__name__, "optimizer_name": type(self._optimizer).__name__,
                "lr_scheduler_state": sched, "num_updates": self.num_updates}],
            "task_state": {},
            "extra_state": extra,
        }
        if not no_optim:
            sd["last_optimizer_state"] = self._optimizer_state()
        return sd

    def save_checkpoint(self, filename, extra_state=None):
        """Rank 0 writes (data-parallel replicas hold identical state); atomically, like checkpoint_utils.torch_persistent_save."""
        import os

        self.flush_update()
        if dist.is_initialized() and dist.get_rank() != 0:
            return
        tmp = filename + ".tmp"
        torch.save(self.state_dict(extra_state), tmp)
        os.replace(tmp, filename)

    def load_checkpoint(self, filename, reset_optimizer=False, reset_lr_scheduler=False):
        """Restore model / optimizer / schedule / update count (trainer.py:454-640); returns `extra_state` or None when the file
        does not exist.  The bf16 shadow copies of the weights are refreshed from the restored fp32 masters."""
        import os

        self.flush_update()
        if not os.path.exists(filename):
            return None
        state = torch.load(filename, map_location="cpu", weights_only=False)
        sd = state["model"]
        if hasattr(self.model, "upgrade_state_dict_named"):
            sd = self.model.upgrade_state_dict_named(dict(sd), "")
        with torch.no_grad():  # parameters are views of the flat master buffer: copy in place
            own = self.model.state_dict()
            missing = [k for k in own if k not in sd]
            unexpected = [k for k in sd if k not in own]
            if missing or unexpected:
                raise RuntimeError(f"checkpoint does not match the model: missing {missing[:5]}, unexpected {unexpected[:5]}")
            for k, v in own.items():
                v.copy_(sd[k])
        self._flat.sync_bf16()
        hist = state.get("optimizer_history") or []
        self._optim_history = hist[:-1]
        last = hist[-1] if hist else None
        if last is not None and not reset_optimizer and state.get("last_optimizer_state") is not None:
            if last["criterion_name"] != type(self.criterion).__name__:
                raise RuntimeError("Criterion does not match; please reset the optimizer (--reset-optimizer)")
            self._load_optimizer_state(state["last_optimizer_state"])
            self.num_updates = int(last["num_updates"])
            if hasattr(self.model, "set_num_updates"):
                self.model.set_num_updates(self.num_updates)
            if not reset_lr_scheduler and hasattr(self.lr_scheduler, "load_state_dict") and last.get("lr_scheduler_state"):
                self.lr_scheduler.load_state_dict(last["lr_scheduler_state"])
            self.lr_scheduler.step_update(self.num_updates)
        return state.get("extra_state") or {}
