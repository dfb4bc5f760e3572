"""Training step of the speaker classifier on the HIP kernels.

``MIX_SPEECH_classifier`` (BiLSTM(129, 600, 3 layers) -> mean over t -> Linear(1200, N_lab) -> sigmoid,
``Torch_multi/test_multi_labels_speech.py:240-263``) is trained by the reference with
``nn.MultiLabelSoftMarginLoss`` on the sigmoid output and Adam (``:389-445``); ``ClassifierTrainer`` is that
step on a ``ClassifierNet`` (``dl4ss_amd.infer``), whose weights the inference paths then read directly
(``ClassifierForward``, ``RecursiveExtractor``, the drivers' ``load_params(classifier=...)``).

Per step: mixing + STFT magnitude kernels (``features``), per layer the input-projection GEMM and the
persistent recurrence with its saved ``out / hprev / act / cs`` (``forward``), ``dl4ss_time_mean`` and the
head kernels of ``cls_head.hip`` (``loss_and_grad``), then top-down the large-hidden BPTT
(``dl4ss_birnn_bwd_ex``; the top layer takes only the head's ``dOut_bcast``) with the weight / bias / input
gradient GEMMs unsplit, so a step on B * T <= 256 rows is reproducible bit for bit (``backward``), and the
guarded Adam (``optimizer_step``).  Single GPU, eager launches (no HIP-graph capture).
"""
import torch

from . import _lib, adam, ops, plan

LSTM = 0


class ClassifierTrainer:
    """``precision``: "fp32" -- fp32 GEMMs, exact fp32 recurrence (precision 0); "bf16" -- bf16 GEMM
    operands, bf16 MFMA recurrent matvec (precision 1), fp32 accumulate and state everywhere.
    ``lr``: what the reference's optimizer is built with (1e-5, ``:395``); ``schedule.classifier()`` halves
    it from epoch 0 on.
    ``clip_norm``: clip the gradient's global L2 norm to it on device (torch.nn.utils.clip_grad_norm_'s
    arithmetic; +inf: measure and guard only), and refuse an update whose gradient holds an Inf or NaN;
    ``grad_norm`` (device float[2], valid after optimizer_step(), not synced) then holds the norm before
    clipping and the coefficient.  None: no extra launch, the unclipped step.
    ``optimizer`` "nadam": Keras 1's Nadam with ``schedule_decay`` instead of Adam; ``clipnorm``: the clip by
    Keras's rule (c = clipnorm / norm where norm >= clipnorm, else 1), otherwise as ``clip_norm``; the two
    together are refused (SepTrainer has the same three arguments)."""

    def __init__(self, cnet, batch, k, n_samples, precision="fp32", lr=1e-5, betas=(0.9, 0.999), eps=1e-8,
                 clip_norm=None, optimizer="adam", schedule_decay=0.004, clipnorm=None):
        if precision not in ops.PREC:
            raise ValueError(f"precision {precision!r}: expected one of {sorted(ops.PREC)}")
        self.clipnorm = plan.check_optimizer(optimizer, schedule_decay, clip_norm, clipnorm)
        self.optimizer, self.schedule_decay = optimizer, float(schedule_decay)
        self.clip_norm = None if clip_norm is None else ops.check_clip_norm(clip_norm)
        self.net, self.B, self.K, self.N = cnet, batch, k, n_samples
        self.precision = precision
        B, K, N, H, L, C = batch, k, n_samples, cnet.H, cnet.L, cnet.num_labels
        self.T = T = ops.n_frames(n_samples)
        self.F = F = cnet.F
        dev = cnet.device
        f32 = dict(device=dev, dtype=torch.float32)
        self._sig = torch.empty(B + B * K, N, **f32)  # [mixtures | sources]: the mixing kernel's outputs
        self.mix = self._sig[:B]
        self.src = self._sig[B:].view(B, K, N)
        self.stats = torch.empty(32 * B * K, **f32)
        self.feats = torch.empty(B, T, F, **f32)
        self.G = torch.empty(B * T, 2 * 4 * H, **f32)  # input projections, then dG of the same layer
        self.out = [torch.empty(B, T, 2 * H, **f32) for _ in range(L)]
        self.hprev = [torch.empty(B, T, 2 * H, **f32) for _ in range(L)]
        self.act = [torch.empty(B, T, 2, 4 * H, **f32) for _ in range(L)]
        self.cs = [torch.empty(B, T, 2, H, **f32) for _ in range(L)]
        self.dH = [torch.empty(B * T, 2 * H, **f32) for _ in range(min(2, L - 1))]
        self.mean = torch.empty(B, 2 * H, **f32)
        self.logits = torch.empty(B, C, **f32)
        self.prob = torch.empty(B, C, **f32)
        self.y = torch.zeros(B, C, **f32)
        self.dz = torch.empty(B, C, **f32)
        self.dmb = torch.empty(B, 2 * H, **f32)  # d(mean_t h) / T: the top BPTT's dOut_bcast
        # the top layer's dOut is identically zero: NULL for the generic BPTT kernel; the packed bf16
        # kernels of the small nets (H <= 320) read a dOut, a zero buffer that nothing writes
        self._zero_dout = torch.zeros(B * T, 2 * H, **f32) if (precision == "bf16" and H <= 320) else None
        self.loss = torch.zeros(1, **f32)
        ws = _lib.query("dl4ss_birnn_workspace_bytes", LSTM, B, H)
        if ws < 0:
            raise RuntimeError(f"BiRNN shape unsupported (B={B}, H={H})")
        self.ws_bytes = ws
        self.rnn_ws = torch.zeros((ws + 7) // 8, device=dev, dtype=torch.int64)
        self.status = torch.zeros(2, device=dev, dtype=torch.int32)  # {hand-off timed out, refused updates}
        self._feed = None  # corpus.CorpusFeed, made by the first features_corpus()
        cnet.grad = torch.zeros_like(cnet.flat)
        self.opt = adam.GuardedAdam(cnet.flat, self.status, self.loss, lr, betas, eps, clip_norm=self.clip_norm,
                                    kind=optimizer, schedule_decay=schedule_decay, clipnorm=self.clipnorm)
        self.m, self.v = self.opt.m, self.opt.v
        if self.opt.clip is not None:
            self.grad_norm = self.opt.grad_norm

    # the documented scalars live in the optimizer, read / write (schedule.classifier() assigns lr)
    lr = adam.delegate("opt", "lr")
    step_count = adam.delegate("opt", "step_count")
    skipped_nonfinite = adam.delegate("opt", "skipped_nonfinite")  # counted by check()

    # ------------------------------------------------------------------ training state (as SepTrainer's)
    def require_settled(self, what="state_dict()"):
        """Synchronise; RuntimeError unless check() has settled every refused update (adam.require_settled)."""
        adam.require_settled(self.status, [self.opt], what)

    def state_dict(self):
        """Host copies in plain containers of the net's flat buffer with its layout and of the optimizer (moments,
        applied-update count, lr, skipped count); batch size and precision are not part of it.  Of a settled trainer
        only (RuntimeError: run check() first).  DESIGN.md section 5, "Training state"."""
        self.require_settled()
        return {"net": self.net.flat_state(), "opt": self.opt.state_dict()}

    def check_state_dict(self, sd):
        """Everything that refuses a load, before anything is written: ValueError naming the field and both values."""
        self.require_settled("load_state_dict()")
        if not isinstance(sd, dict):
            raise ValueError("trainer: no trainer state in the file")
        extra = sorted(set(sd) - {"net", "opt"})
        if extra:  # a SepTrainer's parts
            raise ValueError(f"{extra[0]}: the file has it, a ClassifierTrainer has no such part")
        self.net.check_flat_state(sd.get("net"), "net")
        self.opt.check_state_dict(sd.get("opt"), "optimizer")

    def load_state_dict(self, sd, checked=False):
        """Load a state_dict() in place (copy_ into the existing buffers)."""
        if not checked:
            self.check_state_dict(sd)
        self.net.load_flat_state(sd["net"])
        self.opt.load_state_dict(sd["opt"], checked=True)

    # ------------------------------------------------------------------ features
    def features(self, raw=None, gains=None, feats=None):
        """raw (B, K, N) sources + gains (B, K) -> |STFT| of the mixtures (B, T, F); or precomputed
        ``feats`` (B, T, F)."""
        if feats is not None:
            self.feats.copy_(feats)
            return self.feats
        ops.mix_sources(raw, gains, out_src=self.src, out_mix=self.mix, stats_ws=self.stats)
        ops.stft(self.mix, complex_out=False, mag_out=True, out_mag=self.feats)
        return self.feats

    def features_corpus(self, corpus, clips, gains, shifts=None):
        """features() with the sources gathered from a device-resident corpus (corpus.DeviceCorpus) by clip id: host
        arrays clips, gains, shifts (B, Ks), copied into trainer-owned device buffers, one mixing launch.  An
        out-of-range clip id is a silent source, reported by check()."""
        if self._feed is None:
            from .corpus import CorpusFeed
            self._feed = CorpusFeed(self.B, self.net.device)
        self._feed.mix(corpus, clips, gains, shifts, self.K, self.N, self.src, self.mix)
        ops.stft(self.mix, complex_out=False, mag_out=True, out_mag=self.feats)
        return self.feats

    # ------------------------------------------------------------------ forward
    def forward(self):
        net, B, T, H = self.net, self.B, self.T, self.net.H
        st = _lib.stream_ptr()
        x = self.feats.view(B * T, -1)
        for l in range(net.L):
            ops.gemm(x, net.cat_view("weight_ih", l), transB=True, bias=net.cat_view("bias_ih", l), out=self.G,
                     precision=self.precision)
            ops.birnn_fwd("lstm", B, T, H, G=self.G, w_hh=net.cat_view("weight_hh", l), b_hh=net.cat_view("bias_hh", l),
                          out=self.out[l], hprev=self.hprev[l], act=self.act[l], cs=self.cs[l], ws=self.rnn_ws,
                          ws_bytes=self.ws_bytes, status=self.status, precision=self.precision)
            x = self.out[l].view(B * T, 2 * H)
        _lib.call("dl4ss_time_mean", _lib.ptr(self.out[-1]), B, T, 2 * H, _lib.ptr(self.mean), st)
        _lib.call("dl4ss_cls_head_fwd", _lib.ptr(self.mean), _lib.ptr(net.view("Linear.weight")),
                  _lib.ptr(net.view("Linear.bias")), B, 2 * H, net.num_labels, _lib.ptr(self.logits),
                  _lib.ptr(self.prob), st)
        return self.prob

    # ------------------------------------------------------------------ loss + head backward
    def loss_and_grad(self, y_map=None):
        """y_map (B, N_lab): the multi-hot of ``multi_label_vector``.  Writes the loss, the Linear's
        gradients and the top layer's ``dOut_bcast``; returns the loss tensor (not synced)."""
        net = self.net
        if y_map is not None:
            self.y.copy_(y_map)
        g = net.grad
        _lib.call("dl4ss_cls_head_loss_bwd", p=_lib.ptr(self.prob), y=_lib.ptr(self.y), m=_lib.ptr(self.mean),
                  W=_lib.ptr(net.view("Linear.weight")), B=self.B, D=2 * net.H, C=net.num_labels, T=self.T,
                  loss=_lib.ptr(self.loss), dz=_lib.ptr(self.dz), dW=_lib.ptr(net.view("Linear.weight", g)),
                  db=_lib.ptr(net.view("Linear.bias", g)), dOut_bcast=_lib.ptr(self.dmb), stream=_lib.stream_ptr())
        return self.loss

    # ------------------------------------------------------------------ backward
    def backward(self):
        net, B, T, H = self.net, self.B, self.T, self.net.H
        BT, NGH = B * T, 4 * H
        g = net.grad
        dH = self._zero_dout
        for l in range(net.L - 1, -1, -1):
            top = l == net.L - 1
            dG = self.G
            ops.birnn_bwd("lstm", B, T, H, dOut=dH, dOut_bcast=self.dmb if top else None,
                          w_hh=net.cat_view("weight_hh", l), act=self.act[l], cs=self.cs[l], hprev=self.hprev[l], dG=dG,
                          ws=self.rnn_ws, ws_bytes=self.ws_bytes, status=self.status, precision=self.precision)
            xl = self.feats.view(BT, -1) if l == 0 else self.out[l - 1].view(BT, 2 * H)
            # unsplit (splitk = 1): no float atomics, the step repeats bit for bit
            ops.gemm(dG, xl, transA=True, out=net.cat_view("weight_ih", l, g), precision=self.precision)
            db = net.cat_view("bias_ih", l, g)
            db.zero_()
            ops.colsum(dG, db)
            net.cat_view("bias_hh", l, g).copy_(db)  # LSTM: dGh == dG
            whh_g = net.cat_view("weight_hh", l, g)
            hp = self.hprev[l].view(BT, 2 * H)
            for d in range(2):
                ops.gemm(dG[:, d * NGH:(d + 1) * NGH], hp[:, d * H:(d + 1) * H], transA=True,
                         out=whh_g[d * NGH:(d + 1) * NGH], precision=self.precision)
            if l > 0:
                dH = self.dH[l % 2] if len(self.dH) > 1 else self.dH[0]
                ops.gemm(dG, net.cat_view("weight_ih", l), out=dH, precision=self.precision)

    # ------------------------------------------------------------------ Adam
    def optimizer_step(self):
        """Adam on the flat buffers; refused on device (parameters untouched, loss[0] = NaN, status[1]
        counts it) when a recurrence hand-off of this step timed out.  With clip_norm: one sum-of-squares
        launch first, then the clipped Adam, which also refuses a gradient that holds an Inf or NaN."""
        self.opt.step(self.net.grad)

    def step(self, raw=None, gains=None, y_map=None, feats=None):
        """One training step on device-resident inputs; returns the loss tensor (not synced)."""
        self.features(raw, gains, feats)
        self.forward()
        loss = self.loss_and_grad(y_map)
        self.backward()
        self.optimizer_step()
        return loss

    def check(self):
        """Raise if a recurrence hand-off timed out since the last check (the guarded Adam already
        refused every update from then on); the refused steps leave step_count, the status word and the
        hand-off workspace are reset, so training can continue.  Updates refused only because the gradient
        held an Inf or NaN (clip_norm) leave step_count too, are added to skipped_nonfinite, and do not
        raise.  Until this runs, the bias corrections of later steps count a refused step, time-out or
        non-finite alike."""
        torch.cuda.synchronize()
        s, refused = (int(x) for x in self.status.tolist())
        if s or refused:
            self.status.zero_()
            timed_out = adam.timed_out_steps(refused, [(self.opt, 1)])
            self.opt.settle(timed_out)
            if s or timed_out:
                self.rnn_ws.zero_()
                raise RuntimeError(f"BiRNN hand-off timed out (status {s}): {timed_out} update(s) refused")
        if self._feed is not None:
            self._feed.check()
