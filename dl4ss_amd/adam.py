"""The guarded Adam (or Nadam) of one flat parameter buffer and the host bookkeeping of its refused updates.

Every optimizer of a trainer shares the status word {hand-off timed out, refused updates}: an update is refused on
device when a hand-off of its step timed out or (clip_norm) its gradient holds an Inf or NaN.  The 2-int entry
points add the refusal to status[1] (``counted``), dl4ss_adam_guarded does not; check() turns status[1] into
timed-out steps (timed_out_steps) and takes each optimizer's refused updates out of its step count (settle), so
the bias corrections follow the updates applied.  DESIGN.md section 11, "Refusal accounting".

Nadam (Keras 1's, GuardedAdam(kind="nadam")) takes its momentum schedule from the same count: nadam_schedule is a
pure function of it, so a settled count needs no further state.  DESIGN.md section 5, "Nadam and Keras's clipnorm"."""
import torch

from . import _lib, ops
from .params import check_tensor, mismatch


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


def require_settled(status, optimizers, what):
    """Training state is read and written on a settled trainer only: raise RuntimeError, telling the caller to run
    check() first, while the status word ``status`` is non-zero or one of ``optimizers`` has non-finite refusals
    that settle() has not yet taken out of its step count.  Synchronises first (a device read)."""
    if status.is_cuda:
        torch.cuda.synchronize()
    s = [int(x) for x in status.tolist()]
    pending = sum(opt.pending_nonfinite() for opt in optimizers)
    if any(s) or pending:
        raise RuntimeError(f"{what}: the trainer is not settled (status {s}, {pending} non-finite refusal(s) "
                           "pending): step_count still counts refused updates; run check() first")


_SCHEDULE = {}  # the default cache: (beta1, schedule_decay) -> [step, mu(step), P(step)]


def nadam_schedule(step, beta1=0.9, schedule_decay=0.004, cache=None):
    """(mu(step), mu(step + 1), P(step)) of Keras 1's Nadam momentum schedule, in Python floats:
    mu(i) = beta1 (1 - 0.5 0.96^(i schedule_decay)), P(t) = mu(1) mu(2) ... mu(t) multiplied in that order.  Pure
    functions of ``step``, the number of applied updates; the cache (per (beta1, schedule_decay)) advances by one
    factor per step, and a step behind it (settle() after a refusal, a borrowed count) recomputes from 1: the same
    multiplications in the same order, so the same bits with or without the cache.

    ``cache``: a dict of the caller's own.  Every optimizer passes one (GuardedAdam, compat.optim.Nadam): on the
    shared default two optimizers with the same hyper-parameters at different counts, stepped alternately, would
    send the trailing one back to 1 on every call, O(step) host work per update.

    P(t) is a product of factors near 0.5 and underflows in double: where mu stays below 0.5 (beta1 < ~0.87, or
    schedule_decay 0) it reaches exactly 0.0 after ~900 updates, elsewhere it sticks at the smallest denormal.  Both
    are the valid limit -- 1 - P is 1 to double precision long before -- and dl4ss_nadam takes 0 <= mu_prod < 1."""
    step, beta1, schedule_decay = int(step), float(beta1), float(schedule_decay)
    if step < 1:
        raise ValueError(f"nadam_schedule: step {step}, the first update is 1")
    cache = _SCHEDULE if cache is None else cache

    def mu(i):
        return beta1 * (1.0 - 0.5 * 0.96 ** (i * schedule_decay))

    c = cache.get((beta1, schedule_decay))
    if c is None or c[0] > step:
        c = cache[(beta1, schedule_decay)] = [1, mu(1), mu(1)]
    while c[0] < step:
        c[0] += 1
        c[1] = mu(c[0])
        c[2] *= c[1]
    return c[1], mu(step + 1), c[2]


class GuardedAdam:
    """m, v, step_count, lr, betas, eps of the flat fp32 ``flat`` under a shared ``status`` word and ``loss`` tensor.
    ``clip_norm``: every update clips its gradient's global norm (ops.grad_sumsq, dl4ss_adam_clipped) and the object
    owns the fp64 partials, ``grad_norm`` ({norm before clipping, coefficient}; ``norm_rows`` of them), the device
    counter ``nonfinite`` and the host count ``skipped_nonfinite``.  ``counted=False``: unclipped, the 1-int form.

    ``kind`` "nadam": Keras 1's Nadam (include/dl4ss_optim.h) with ``schedule_decay``, its schedule a function of
    the step count (nadam_schedule).  ``clipnorm``: the clip by Keras's rule (c = clipnorm / norm where norm >=
    clipnorm, else 1; no + 1e-6), everything else as with ``clip_norm``; the two together are refused.  ``parts``:
    (buffer, offset) -- a shared fp64 buffer of partials and where this optimizer's slice starts: sumsq() writes
    the slice, the update sums the whole buffer, so every optimizer on it clips by the one joint norm (a non-finite
    joint sum then also sets the sticky bit ops.STATUS_NONFINITE_GRAD of status[0]: the updates and the memory store
    behind it refuse too)."""

    def __init__(self, flat, status, loss, lr, betas=(0.9, 0.999), eps=1e-8, clip_norm=None, counted=True,
                 norm_rows=None, kind="adam", schedule_decay=0.004, clipnorm=None, parts=None):
        if kind not in ("adam", "nadam"):
            raise ValueError(f"optimizer {kind!r}: expected 'adam' or 'nadam'")
        if clip_norm is not None and clipnorm is not None:
            raise ValueError("clip_norm (torch's rule) and clipnorm (Keras's rule) are given together: choose one")
        if not float(schedule_decay) >= 0.0:
            raise ValueError(f"schedule_decay must not be negative, got {schedule_decay}")
        if parts is not None and clip_norm is None and clipnorm is None:
            raise ValueError("parts= (the joint norm's shared partials) needs clip_norm= or clipnorm=")
        self.flat, self.status, self.loss = flat, status, loss
        self.lr, self.betas, self.eps, self.clip_norm = lr, betas, eps, clip_norm
        self.kind, self.schedule_decay, self.clipnorm = kind, float(schedule_decay), clipnorm
        self.clip = clip_norm if clipnorm is None else clipnorm  # the threshold, by either rule
        # dl4ss_adam_clipped and dl4ss_nadam have the 2-int form only
        self.counted = counted or self.clip is not None or kind == "nadam"
        self.m, self.v = torch.zeros_like(flat), torch.zeros_like(flat)
        self.step_count = self.skipped_nonfinite = 0
        self._schedule = {}  # nadam_schedule's cache, this optimizer's own
        self.joint = parts is not None
        if self.clip is not None:
            n_part = ops.grad_sumsq_parts(flat.numel())
            if parts is None:
                self.part = self.part_all = torch.zeros(n_part, dtype=torch.float64, device=flat.device)
            else:
                self.part_all, off = parts
                if self.part_all.dtype != torch.float64 or not 0 <= off <= self.part_all.numel() - n_part:
                    raise ValueError(f"parts: a float64 buffer with {n_part} values from offset {off} on")
                self.part = self.part_all[off:off + n_part]
            self.grad_norm = torch.zeros(*([] if norm_rows is None else [norm_rows]), 2, device=flat.device)
            self.nonfinite = torch.zeros(1, dtype=torch.int32, device=flat.device)

    def sumsq(self, grad):
        """This optimizer's partial sums of squares of ``grad`` into its slice of the partials (the joint norm:
        every optimizer's before the first update)."""
        ops.grad_sumsq(grad, self.part)

    def step(self, grad, *, gnorm=None, dp_flag=None, gscale=1.0, shadow=None, step=None, summed=False):
        """One update from ``grad`` (arguments as ops.adam_).  ``step``: another optimizer's count to step with,
        instead of this one's own, which then stays as it is; ``gnorm``: the row of grad_norm the update writes;
        ``summed``: sumsq(grad) has been called already."""
        if step is None:
            self.step_count += 1
            step = self.step_count
        if not self.counted:
            _lib.call("dl4ss_adam_guarded", p=_lib.ptr(self.flat), g=_lib.ptr(grad), m=_lib.ptr(self.m),
                      v=_lib.ptr(self.v), n=self.flat.numel(), lr=float(self.lr), beta1=float(self.betas[0]),
                      beta2=float(self.betas[1]), eps=float(self.eps), step=step, status=_lib.ptr(self.status),
                      loss=_lib.ptr(self.loss), stream=_lib.stream_ptr())
            return
        clip, kw = None, {}
        if self.clip is not None:
            if not summed:
                self.sumsq(grad)
            clip = (self.part_all, self.clip, self.grad_norm if gnorm is None else gnorm, self.nonfinite)
            if self.joint:
                kw.update(n_part=self.part_all.numel(), sticky=True)
            if self.clipnorm is not None:
                kw.update(clip_rule=ops.CLIP_KERAS)
            elif self.kind == "nadam":
                kw.update(clip_rule=ops.CLIP_TORCH)
        if self.kind == "nadam":
            ops.nadam_(self.flat, grad, self.m, self.v, step, nadam_schedule(step, self.betas[0], self.schedule_decay, self._schedule),
                       self.lr, self.betas, self.eps, status=self.status, loss=self.loss, dp_flag=dp_flag,
                       gscale=gscale, shadow=shadow, clip=clip, **kw)
            return
        ops.adam_(self.flat, grad, self.m, self.v, step, self.lr, self.betas, self.eps, status=self.status,
                  loss=self.loss, dp_flag=dp_flag, gscale=gscale, shadow=shadow, clip=clip, **kw)

    def pending_nonfinite(self):
        """The non-finite refusals since the last settle() (a device read)."""
        return int(self.nonfinite.item()) if self.clip is not None else 0

    def settle(self, timed_out, updates_per_step=1):
        """Take the updates of ``timed_out`` steps and the non-finite refusals out of step_count and move the
        latter to skipped_nonfinite (device counter reset); returns them."""
        nonfinite = self.pending_nonfinite()
        if nonfinite:
            self.nonfinite.zero_()
        self.step_count -= timed_out * updates_per_step + nonfinite
        self.skipped_nonfinite += nonfinite
        return nonfinite

    # ---- training state (checkpoint.save_training_state)
    def hyper(self):
        """What a saved state is checked against, never restored: the update rule and its constants."""
        return {"kind": self.kind, "betas": [float(b) for b in self.betas], "eps": float(self.eps),
                "schedule_decay": self.schedule_decay,
                "clip_norm": None if self.clip_norm is None else float(self.clip_norm),
                "clipnorm": None if self.clipnorm is None else float(self.clipnorm)}

    def state_dict(self):
        """Host copies of m and v, the counts, lr (state: schedules assign it) and hyper().  Nadam's schedule is a
        pure function of step_count (nadam_schedule) and is not saved.  Of a settled optimizer only
        (require_settled): an unsettled step_count still counts refused updates."""
        return {"m": self.m.detach().to("cpu", copy=True), "v": self.v.detach().to("cpu", copy=True),
                "step_count": int(self.step_count), "skipped_nonfinite": int(self.skipped_nonfinite),
                "lr": float(self.lr), **self.hyper()}

    def check_state_dict(self, sd, where="optimizer"):
        """Raise ValueError naming the first field of ``sd`` this optimizer cannot take; nothing is written."""
        if not isinstance(sd, dict):
            raise ValueError(f"{where}: no optimizer state in the file")
        for k, own in self.hyper().items():
            if k not in sd or sd[k] != own:
                raise mismatch(f"{where}.{k}", sd.get(k), own)
        check_tensor(sd.get("m"), self.m, f"{where}.m")
        check_tensor(sd.get("v"), self.v, f"{where}.v")
        for k in ("step_count", "skipped_nonfinite"):
            if isinstance(sd.get(k), bool) or not isinstance(sd.get(k), int) or sd[k] < 0:
                raise mismatch(f"{where}.{k}", sd.get(k), "a count >= 0")
        if isinstance(sd.get("lr"), bool) or not isinstance(sd.get("lr"), (int, float)):
            raise mismatch(f"{where}.lr", sd.get("lr"), "a number")

    def load_state_dict(self, sd, checked=False):
        """In place: m and v by copy_ into the existing buffers (a captured graph and every view stay valid), the
        counts and lr assigned.  ``checked``: check_state_dict(sd) has passed already."""
        if not checked:
            self.check_state_dict(sd)
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.step_count, self.skipped_nonfinite, self.lr = sd["step_count"], sd["skipped_nonfinite"], float(sd["lr"])
