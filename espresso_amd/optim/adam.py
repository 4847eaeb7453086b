"""Adam on the flat buffers with fused gradient scaling/clipping — results equal to
fairseq/optim/adam.py:215-240 applied after Trainer's multiply_grads + clip_grad_norm
(fairseq/trainer.py:918-951, fairseq/utils.py:347-397)."""
import torch

from .. import kernels as K
from ..registry import register_optimizer
from .flat import FlatParams

# Workgroups of the deferred update's launches (clip_and_step_split): the side-queue kernel must leave the compute queue's
# kernels room.  256 stream at the full HBM rate already and measured best of 256 / 512 / 1024.
SIDE_MAX_BLOCKS = 256


class PendingUpdate:
    """The deferred part of an optimizer pass (FlatAdam.clip_and_step_split): `start()` issues its launches, once, and returns the
    event that marks their end.  Trainer and model hold the same object, whoever comes first starts it."""

    def __init__(self, launch):
        self._launch, self._event = launch, None

    @property
    def started(self):
        return self._event is not None

    def start(self):
        if self._event is None:
            self._event, self._launch = self._launch(), None
        return self._event

    def wait(self, stream):
        stream.wait_event(self.start())


@register_optimizer("adam")
class FlatAdam:
    def __init__(self, flat: FlatParams, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.flat = flat
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        dev = flat.p32.device
        self.exp_avg = torch.zeros_like(flat.p32)
        self.exp_avg_sq = torch.zeros_like(flat.p32)
        self.step_count = 0
        self._sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self._coef = torch.zeros(2, dtype=torch.float32, device=dev)

    def set_lr(self, lr):
        self.lr = lr

    def get_lr(self):
        return self.lr

    def clip_and_step(self, pre_scale=1.0, max_norm=0.0, denom_dev=None):
        """grad *= pre_scale/denom ; grad *= min(1, max_norm/(|grad|+1e-6)) ; Adam ; grads re-zeroed.
        Returns the device tensor coef = [applied scale, grad norm] (read it lazily for logging)."""
        f = self.flat
        self._sumsq.zero_()
        K.grad_sumsq(f.g32, self._sumsq)
        K.clip_coef(self._sumsq, pre_scale, max_norm, self._coef, denom_dev)
        self.step_count += 1
        K.adam_step(f.p32, f.g32, self.exp_avg, self.exp_avg_sq, f.p16, self._coef, self.lr, self.betas[0], self.betas[1],
                    self.eps, self.weight_decay, self.step_count, zero_grad=True)
        return self._coef

    def clip_and_step_split(self, side_stream, pre_scale=1.0, max_norm=0.0, denom_dev=None, hold=False):
        """clip_and_step with the update of everything outside `flat.early_range` on `side_stream`, from a grid of at most
        SIDE_MAX_BLOCKS workgroups: the norm, the coefficient and the early range's update run on the current stream as in
        clip_and_step; the rest follows on the side stream, behind whatever the current stream holds when it is started — at
        once, or with `hold` when the caller (or the model, in its next forward pass) calls `start()` of the PendingUpdate this
        returns.  Until the current stream has waited for it nothing on it may touch p32 / p16 / g32 / the moments outside the
        early range.  Same bits as clip_and_step.  -> (coef, PendingUpdate)"""
        f = self.flat
        lo, hi = f.early_range
        K.grad_sumsq(f.g32, self._sumsq)
        K.clip_coef_clear(self._sumsq, pre_scale, max_norm, self._coef, denom_dev)  # (leaves _sumsq zero for the next step)
        self.step_count += 1
        args = (self._coef, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.step_count)
        cut = lambda a, b: (f.p32[a:b], f.g32[a:b], self.exp_avg[a:b], self.exp_avg_sq[a:b], f.p16[a:b])
        K.adam_step(*cut(lo, hi), *args, zero_grad=True)

        def launch():
            side_stream.wait_stream(torch.cuda.current_stream(f.p32.device))
            for a, b in ((0, lo), (hi, f.numel)):
                if b > a:
                    K.adam_step_capped(*cut(a, b), *args, SIDE_MAX_BLOCKS, side_stream, zero_grad=True)
            return side_stream.record_event()

        pending = PendingUpdate(launch)
        if not hold:
            pending.start()
        return self._coef, pending

    def state_dict(self):
        return {"step": self.step_count, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "lr": self.lr}

    def load_state_dict(self, sd):
        self.step_count = sd["step"]
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.lr = sd.get("lr", self.lr)
