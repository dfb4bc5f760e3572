"""The adversarial term of the separation step (SepTrainer(adversary=DiscNet)): the Discriminator over [true;
predicted] magnitude maps, its two gradients, the prediction's adversarial gradient and its Adam."""
import torch

from . import _lib, ops
from .adam import GuardedAdam


class AdvStep:
    """Buffers and launches of the adversarial step (TDAA_beta/main_run_sstune_dis.py:613-647 with detach_fake, the
    adversarial term weighted by ``adv_weight``) for B K sources: the Discriminator's activations over the 2 B K
    maps [true; predicted], their gradients, the scores and loss heads, gext, the split-K workspace, its Adam.
    ``mag``: the trainer's magnitudes [mixtures | sources | predictions]; ``status``, ``loss``: the trainer's (itself
    not referenced: SepTrainer._ws_slot).  fp32 for precision 'fp32', the bf16 activation mode otherwise."""

    def __init__(self, disc, batch, k, mag, precision, status, loss, lr, betas, eps, adv_weight=1.0,
                 disc_adv_update=True, clip_norm=None):
        D, B, N, (T, F) = disc, batch, batch * k, mag.shape[1:]
        self.disc, self.N, self.adv_weight = D, N, float(adv_weight)
        self.updates = 2 if disc_adv_update else 1  # Adam updates per step: on grad_dis, then on grad_adv
        self.prec = ops.PREC["fp32" if precision == "fp32" else "bf16"]
        dt = torch.float32 if self.prec == 0 else torch.bfloat16
        f32 = dict(device=D.device, dtype=torch.float32)
        self.pred = mag[B + N:].view(B, k, T, F)  # mask |X|, written by the COST pass (pred_out)
        self.maps = mag[B:]  # (2 B K, T, F): the sources' magnitudes, then the predictions
        self.y = [torch.empty(2 * N, D.hw[2 * l], D.hw[2 * l + 1], 64, device=D.device, dtype=dt) for l in range(3)]
        self.dy = [torch.empty_like(y) for y in self.y]
        self.scores, self.logit, self.dz, self.ds_dis = (torch.empty(2 * N, **f32) for _ in range(4))
        self.ds_adv = torch.empty(N, **f32)
        self.adv_loss = torch.zeros(3, **f32)  # [L_dt, L_df, L_adv] (L_adv unweighted)
        self.gext = torch.empty(B, k, T, F, **f32)
        self.ws_bytes = _lib.query("dl4ss_disc_ws_bytes", 2 * N, T, F)
        if self.ws_bytes < 0:
            raise RuntimeError(f"Discriminator shape unsupported (N={2 * N}, T={T}, F={F})")
        self.ws = torch.empty((self.ws_bytes + 3) // 4, **f32)
        # one Adam state for both gradients; its unclipped updates go through the 1-int status form
        self.opt = GuardedAdam(D.flat, status, loss, lr, betas, eps, clip_norm=clip_norm, counted=False, norm_rows=2)

    def disc_grads(self):
        """Scores of the 2 B K maps (one forward), the loss heads, then two backwards: all maps without the
        input gradient -> grad_dis = d(L_dt + L_df), the predicted maps with conv1's dX -> grad_adv =
        d(lambda L_adv) and gext = d(lambda L_adv)/dpred.  All on the current stream, at the pre-step weights."""
        D, N = self.disc, self.N
        ops.disc_forward(self.prec, self.maps, [D.view(name) for name, _ in D.specs], self.y, self.logit, self.scores)
        _lib.call("dl4ss_disc_adv_heads", _lib.ptr(self.scores), N, self.adv_weight, _lib.ptr(self.adv_loss),
                  _lib.ptr(self.ds_dis), _lib.ptr(self.ds_adv), _lib.stream_ptr())
        for a, n, ds, g, dx in ((0, 2 * N, self.ds_dis, D.grad_dis, None), (N, N, self.ds_adv, D.grad_adv, self.gext)):
            ops.disc_backward(self.prec, self.maps[a:a + n], [D.view(name) for name, _ in D.specs[0::2]],
                              [y[a:a + n] for y in self.y], [d[:n] for d in self.dy], self.scores[a:a + n], ds, 0.0,
                              None, self.dz, [D.view(name, g) for name, _ in D.specs], dx, self.ws, self.ws_bytes)

    def optimizer_step(self):
        """The Discriminator's updates in the reference's order (dis.py:627-628, 646-647): Adam on grad_dis, then
        (disc_adv_update) on grad_adv -- each a step of the one Adam state, clipped on its own gradient."""
        for i, g in enumerate((self.disc.grad_dis, self.disc.grad_adv)[:self.updates]):
            self.opt.step(g, gnorm=self.opt.grad_norm[i] if self.opt.clip_norm is not None else None)

    # ---- training state (checkpoint.save_training_state; the trainer checks that it is settled)
    def state_dict(self):
        """The Discriminator's flat buffer with its layout, and its Adam (moments, both updates' one count, lr)."""
        return {"net": self.disc.flat_state(), "opt": self.opt.state_dict()}

    def check_state_dict(self, sd, where="adversary"):
        if not isinstance(sd, dict):
            raise ValueError(f"{where}: no adversary section in the file")
        self.disc.check_flat_state(sd.get("net"), f"{where}.net")
        self.opt.check_state_dict(sd.get("opt"), f"{where}.optimizer")

    def load_state_dict(self, sd, checked=False):
        if not checked:
            self.check_state_dict(sd)
        self.disc.load_flat_state(sd["net"])
        self.opt.load_state_dict(sd["opt"], checked=True)
