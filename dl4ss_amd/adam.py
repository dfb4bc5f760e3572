"""The guarded Adam of one flat parameter buffer and the host bookkeeping of its refused updates.

Every optimizer of a trainer shares the status word {hand-off timed out, refused updates}: an update is refused on
device when a hand-off of its step timed out or (clip_norm) its gradient holds an Inf or NaN.  The 2-int entry
points add the refusal to status[1] (``counted``), dl4ss_adam_guarded does not; check() turns status[1] into
timed-out steps (timed_out_steps) and takes each optimizer's refused updates out of its step count (settle), so
the bias corrections follow the updates applied.  DESIGN.md section 11, "Refusal accounting"."""
import torch

from . import _lib, ops


def delegate(holder, name, default=None):
    """A trainer's documented name for a host scalar (lr, a counter) of the GuardedAdam ``self.<holder>``, read /
    write; ``default``: what it reads on a trainer without that optimizer."""
    def get(self):
        opt = getattr(self, holder, None)
        return default if (opt is None and default is not None) else getattr(opt, name)

    return property(get, lambda self, x: setattr(getattr(self, holder), name, x))


def timed_out_steps(refused, optimizers):
    """The timed-out steps behind ``refused`` = status[1]; ``optimizers``: (GuardedAdam, updates per step) of all on
    that word.  Each update of a counted one counts a timed-out step; a non-finite refusal is counted once."""
    nonfinite = sum(opt.pending_nonfinite() for opt, _ in optimizers)
    return (refused - nonfinite) // sum(n for opt, n in optimizers if opt.counted)


class GuardedAdam:
    """m, v, step_count, lr, betas, eps of the flat fp32 ``flat`` under a shared ``status`` word and ``loss`` tensor.
    ``clip_norm``: every update clips its gradient's global norm (ops.grad_sumsq, dl4ss_adam_clipped) and the object
    owns the fp64 partials, ``grad_norm`` ({norm before clipping, coefficient}; ``norm_rows`` of them), the device
    counter ``nonfinite`` and the host count ``skipped_nonfinite``.  ``counted=False``: unclipped, the 1-int form."""

    def __init__(self, flat, status, loss, lr, betas=(0.9, 0.999), eps=1e-8, clip_norm=None, counted=True,
                 norm_rows=None):
        self.flat, self.status, self.loss = flat, status, loss
        self.lr, self.betas, self.eps, self.clip_norm = lr, betas, eps, clip_norm
        self.counted = counted or clip_norm is not None  # dl4ss_adam_clipped has the 2-int form only
        self.m, self.v = torch.zeros_like(flat), torch.zeros_like(flat)
        self.step_count = self.skipped_nonfinite = 0
        if clip_norm is not None:
            self.part = torch.zeros(ops.grad_sumsq_parts(flat.numel()), dtype=torch.float64, device=flat.device)
            self.grad_norm = torch.zeros(*([] if norm_rows is None else [norm_rows]), 2, device=flat.device)
            self.nonfinite = torch.zeros(1, dtype=torch.int32, device=flat.device)

    def step(self, grad, *, gnorm=None, dp_flag=None, gscale=1.0, shadow=None, step=None):
        """One update from ``grad`` (arguments as ops.adam_).  ``step``: another optimizer's count to step with,
        instead of this one's own, which then stays as it is; ``gnorm``: the row of grad_norm the update writes."""
        if step is None:
            self.step_count += 1
            step = self.step_count
        if not self.counted:
            _lib.call("dl4ss_adam_guarded", p=_lib.ptr(self.flat), g=_lib.ptr(grad), m=_lib.ptr(self.m),
                      v=_lib.ptr(self.v), n=self.flat.numel(), lr=float(self.lr), beta1=float(self.betas[0]),
                      beta2=float(self.betas[1]), eps=float(self.eps), step=step, status=_lib.ptr(self.status),
                      loss=_lib.ptr(self.loss), stream=_lib.stream_ptr())
            return
        clip = None
        if self.clip_norm is not None:
            ops.grad_sumsq(grad, self.part)
            clip = (self.part, self.clip_norm, self.grad_norm if gnorm is None else gnorm, self.nonfinite)
        ops.adam_(self.flat, grad, self.m, self.v, step, self.lr, self.betas, self.eps, status=self.status,
                  loss=self.loss, dp_flag=dp_flag, gscale=gscale, shadow=shadow, clip=clip)

    def pending_nonfinite(self):
        """The non-finite refusals since the last settle() (a device read)."""
        return int(self.nonfinite.item()) if self.clip_norm is not None else 0

    def settle(self, timed_out, updates_per_step=1):
        """Take the updates of ``timed_out`` steps and the non-finite refusals out of step_count and move the
        latter to skipped_nonfinite (device counter reset); returns them."""
        nonfinite = self.pending_nonfinite()
        if nonfinite:
            self.nonfinite.zero_()
        self.step_count -= timed_out * updates_per_step + nonfinite
        self.skipped_nonfinite += nonfinite
        return nonfinite
