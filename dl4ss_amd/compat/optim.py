"""``torch.optim.Adam`` stand-in for the driver mirrors: the same constructor (a list of
``{'params': ...}`` groups, ``lr``, ``betas``, ``eps``), ``param_groups`` (so the reference's
LR-halving lines ``for ee in optimizer.param_groups: ee['lr'] /= 2`` work unchanged,
EvalVer.py:570-575), ``zero_grad`` and ``step`` -- with the update on the HIP Adam kernel
(dl4ss_adam: torch's Adam arithmetic, bias corrections in double on the host), one launch
per parameter.  Parameters without a gradient (the discarded classifier; the Linear_1/2/3
weights of an ATTENTION run in 'dot' mode, which only 'align' mode uses and trains) are
skipped, as torch skips them.

``Nadam``: the Keras trees' optimizer under Keras 1's constructor names (``lr``, ``beta_1``, ``beta_2``,
``epsilon``, ``schedule_decay``, ``clipnorm``; DL4SS_Keras/nnet.py:23,113: Nadam(clipnorm=200)) over the same
parameter groups, on dl4ss_nadam, one launch per parameter.  ``clipnorm`` is Keras's: global over every
parameter with a gradient, through one concatenated buffer of fp64 partial sums that every launch sums: at most
4096 of them (one per 4096 gradient elements of a parameter, at least one per parameter; a model that needs more
raises ValueError in ``step``).  A step whose global norm is not finite changes nothing, on device; there is no
status word to stop on, so ``step`` has counted it already: ``settle()`` (a device read) takes such steps back
out of ``step_count``, which the schedule and the bias correction follow, and returns how many there were.
"""
import torch

from dl4ss_amd import adam, ops


class Adam:
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        groups = list(params)
        if groups and not isinstance(groups[0], dict):
            groups = [{"params": groups}]
        self.param_groups = []
        for g in groups:
            g = dict(g)
            g["params"] = list(g["params"])
            g.setdefault("lr", lr)
            g.setdefault("betas", betas)
            g.setdefault("eps", eps)
            self.param_groups.append(g)
        self.state = {}

    def zero_grad(self):
        for g in self.param_groups:
            for p in g["params"]:
                p.grad = None

    @torch.no_grad()
    def step(self):
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state.get(p)
                if st is None:
                    st = self.state[p] = {"step": 0, "m": torch.zeros_like(p), "v": torch.zeros_like(p)}
                st["step"] += 1
                ops.adam_(p.data, p.grad.contiguous(), st["m"], st["v"], st["step"], g["lr"], g["betas"], g["eps"])


class Nadam:
    def __init__(self, params, lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=1e-8, schedule_decay=0.004,
                 clipnorm=None):
        groups = list(params)
        if groups and not isinstance(groups[0], dict):
            groups = [{"params": groups}]
        if not float(schedule_decay) >= 0.0:
            raise ValueError(f"schedule_decay must not be negative, got {schedule_decay}")
        self.clipnorm = None if clipnorm is None else ops.check_clip_norm(clipnorm, "clipnorm")
        self.schedule_decay = float(schedule_decay)
        self.param_groups = []
        for g in groups:
            g = dict(g)
            g["params"] = list(g["params"])
            g.setdefault("lr", lr)
            g.setdefault("betas", (beta_1, beta_2))
            g.setdefault("eps", epsilon)
            self.param_groups.append(g)
        self.state = {}
        self.step_count = 0  # one count for all parameters (Keras's `iterations`)
        self.skipped_nonfinite = 0
        self._clip = None
        self._schedule = {}  # adam.nadam_schedule's cache, this optimizer's own

    def zero_grad(self):
        for g in self.param_groups:
            for p in g["params"]:
                p.grad = None

    def _partials(self, grads):
        """One fp64 buffer [parts(g_0) | parts(g_1) | ...] of the gradients' sums of squares, with the norm's
        and the non-finite counter's buffers (kept while the sizes stay what they were)."""
        sizes = [ops.grad_sumsq_parts(g.numel()) for g in grads]
        if sum(sizes) > ops.CLIP_MAX_PARTS:
            raise ValueError(f"Nadam(clipnorm): {sum(sizes)} partial sums, at most {ops.CLIP_MAX_PARTS}")
        if self._clip is None or self._clip[0] != sizes:
            dev = grads[0].device
            self._clip = (sizes, torch.zeros(sum(sizes), dtype=torch.float64, device=dev),
                          torch.zeros(2, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
        _, part, gnorm, nonfinite = self._clip
        off = 0
        for g, k in zip(grads, sizes):
            ops.grad_sumsq(g, part[off:off + k])
            off += k
        return part, gnorm, nonfinite

    @property
    def grad_norm(self):
        """Device float[2] {the global norm before clipping, the coefficient} of the last step (clipnorm only)."""
        return None if self._clip is None else self._clip[2]

    @property
    def nonfinite(self):
        """Device int32[1]: the launches refused for a non-finite norm since the last settle() (clipnorm only; every
        parameter's launch of such a step counts one)."""
        return None if self._clip is None else self._clip[3]

    def settle(self):
        """Take the steps refused for a non-finite global norm since the last call out of step_count (a device
        read); returns their number, also added to skipped_nonfinite.  Without clipnorm: 0, nothing is refused."""
        if self._clip is None:
            return 0
        launches = int(self._clip[3].item())
        if not launches:
            return 0
        self._clip[3].zero_()
        steps = launches // max(1, len(self._clip[0]))  # (every parameter of a refused step counted it)
        self.step_count -= steps
        self.skipped_nonfinite += steps
        return steps

    @torch.no_grad()
    def step(self):
        todo = [(g, p, p.grad.contiguous()) for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not todo:
            return
        self.step_count += 1
        kw = {}
        if self.clipnorm is not None:
            part, gnorm, nonfinite = self._partials([grad for _, _, grad in todo])
            kw = dict(clip=(part, self.clipnorm, gnorm, nonfinite), n_part=part.numel())
        for g, p, grad in todo:
            st = self.state.get(p)
            if st is None:
                st = self.state[p] = {"m": torch.zeros_like(p), "v": torch.zeros_like(p)}
            sched = adam.nadam_schedule(self.step_count, g["betas"][0], self.schedule_decay, self._schedule)
            ops.nadam_(p.data, grad, st["m"], st["v"], self.step_count, sched, g["lr"], g["betas"], g["eps"], **kw)
