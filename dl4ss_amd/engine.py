"""The separation training step on the HIP path (host orchestration).

One step (``TDAA_beta/main_run_sstune_EvalVer.py:586-675``,
``main_run_sstune_cRM_EvalVer.py:639-752``, ``Torch_multi/main_run.py:453-522``):

    raw sources -> normalise/gain/mix (R1) -> STFT of mixture and sources (R2-R4)
    -> stacked BiLSTM/BiGRU (R8/R9) -> Linear + tanh -> V (B,T,F,E)
    -> speaker queries (embedding + ADDJUST, R7/R10)
    -> fused mask attention + label-ordered / PIT / cRM loss + backward (R11-R14)
    -> BPTT, weight gradients -> (optional DP all-reduce) -> Adam (R15)

Every arithmetic step is a C-ABI call into ``libdl4ss_hip.so``; torch only owns
device memory, streams and (for DP) the collective.  All parameters live in one
flat fp32 buffer (views carry the reference ``state_dict`` key names, so a
reference / oracle state dict loads directly) and all gradients in a second
flat buffer: one all-reduce and one Adam launch per step.
"""
import ctypes

import torch

from . import _lib, adam, dp, ops
from .adversarial import AdvStep
from .ops import CELLS, DEFER_BIAS, DGH_PAD8, DOUT_SLABS, WS_ZEROED, pad8  # noqa: F401 (re-exported)
from .params import DiscNet, FlatParams, SepNet, _ngate, mismatch  # noqa: F401 (re-exported)
from .plan import RETIRED_KNOBS, check_args, step_plan  # noqa: F401 (re-exported)
from .imagequery import ImageQueryStep
from .voiceprint import VoiceprintStep


class SepTrainer:
    """Buffers and the step schedule for one (B, K, N) workload.

    ``clip_norm``: clip the global L2 norm of the global-batch mean gradient to it inside optimizer_step()
    (torch.nn.utils.clip_grad_norm_'s arithmetic, on device; +inf measures and guards only) and refuse an update
    whose gradient holds an Inf or NaN; ``grad_norm`` (device float[2]) then holds the norm before clipping and the
    coefficient, ``skipped_nonfinite`` what check() has counted.  ``adv_clip_norm``: the same for each of the
    Discriminator's updates (``adv_grad_norm``, float[2, 2]).  None (the default): no launch is added.

    ``optimizer`` "nadam": the mask net and the query encoder (voiceprint= / image_query=) train with Keras 1's
    Nadam (DL4SS_Keras/nnet.py:23,113; ``schedule_decay``, default 0.004) instead of Adam -- eager and in
    step_graph(), fp32 and bf16 (the shadows come from the same launch), data parallel; the Discriminator keeps
    Adam, as the reference trains it.  ``clipnorm``: the global-norm clip by Keras's rule (c = clipnorm / norm where
    norm >= clipnorm, else 1), with either optimizer, otherwise as ``clip_norm`` (``grad_norm``,
    ``skipped_nonfinite``); the two together are refused.  With voiceprint= / image_query= it is the JOINT norm
    over the net's and the encoder's gradients, as Keras takes it: both ``grad_norm`` and ``vp_opt.grad_norm``
    hold it, and a joint norm that is not finite refuses both updates and the memory store (check() raises).

    ``voiceprint`` (a ``voiceprint.VoiceprintNet``) with ``memory`` (a ``voiceprint.SpeakerMemory``): the queries
    are not rows of ``emb.layer.weight`` but voiceprints -- the masked encoder over the step's own clean
    magnitudes, accumulated into and read back from the speaker memory (DL4SS_Keras/nnet.py:64-92); the encoder
    trains with the mask net (its own guarded Adam at ``voiceprint_lr``, default ``lr``) and the memory rows of
    the batch's speakers are rewritten after every applied update: ``memory_refresh`` "reference" re-encodes
    with the updated weights first (nnet.py:131-135), "reuse" stores the step's own queries.  fp32, mode
    "label", single GPU, eager only; everything else is refused (plan.check_args).  None (the default): no launch is
    added and no line of the step changes.

    ``image_query`` (an ``imagequery.ImageQueryNet``) with ``memory``: the same step with the target named by a
    picture (Multi_modal/software/DL4SS_Keras/nnet.py:70-94) -- the queries are the image-query CNN over the step's
    ``images`` (B, K, h, w), given to step(images=), accumulated into and read back from the speaker memory; the
    encoder trains at ``image_query_lr`` (default ``lr``), ``memory_refresh`` as above.  A step whose loss is not
    finite is refused on device (no parameter, moment or memory row changes; check() raises).  The refusal is
    sticky, as a time-out's is: the status word keeps bit 1 and every step enqueued behind it is refused too, until
    check() has been called.  The voiceprint
    step's limits (fp32, mode "label", single GPU, eager only) and refusals apply.

    ``splitk_reduce`` "fixed" (precision "fp32" only): every backward GEMM of the step splits K through fp32 slabs
    that are added in a fixed order (ops.gemm(reduce="fixed"), one trainer-owned workspace) -- 'align', which runs
    them unsplit otherwise, too -- the bias gradients are fixed-order column sums (ops.vp_colsum), and with
    ``voiceprint`` the encoder's weight gradients split the same way: losses, gradients and parameters repeat bit
    for bit from run to run, eager or replayed.  "atomic" (the default): the step as it was."""

    def __init__(self, net, batch, k, n_samples, mode="label", precision="fp32", lr=2e-4, sum_weight=0.5,
                 loss_channels=None, betas=(0.9, 0.999), eps=1e-8, process_group=None, rnn_precision=None,
                 adversary=None, adv_weight=1.0, adv_lr=None, disc_adv_update=True, clip_norm=None,
                 adv_clip_norm=None, voiceprint=None, memory=None, voiceprint_lr=None, memory_refresh="reference",
                 splitk_reduce="atomic", image_query=None, image_query_lr=None, optimizer="adam",
                 schedule_decay=0.004, clipnorm=None):
        self.clip_norm, self.adv_clip_norm = check_args(  # every refusal, before any device call
            net, batch, k, n_samples, mode, precision, rnn_precision, loss_channels, process_group, adversary,
            clip_norm, adv_clip_norm, voiceprint, memory, memory_refresh, splitk_reduce=splitk_reduce,
            inet=image_query, optimizer=optimizer, schedule_decay=schedule_decay, clipnorm=clipnorm)
        self.optimizer, self.schedule_decay = optimizer, float(schedule_decay)
        self.clipnorm = None if clipnorm is None else float(clipnorm)
        self.inet = image_query
        self.vnet, self.memory, self.memory_refresh, self.adversary = voiceprint, memory, memory_refresh, adversary
        self.align = getattr(net, "attention", "dot") == "align"
        # rnn_precision, fast, split, split_x2, grouped, _ws_fill, dh_split, dh_slabs, xw, xw_kmax, xw_split0, buckets,
        # dp_layer, side, dw_splits, zero_free, _gbeta, _shadow_on
        vars(self).update(vars(step_plan(net, batch, n_samples, precision, rnn_precision, process_group)))
        self.net, self.B, self.K, self.N = net, batch, k, n_samples
        self.mode, self.precision = mode, precision
        # split-K of the fp32 step's backward GEMMs (gemm.hip: fp32 atomics, the order of the partial sums
        # varies from launch to launch).  The 'align' step keeps every GEMM in one piece instead, so that its
        # gradients are bitwise reproducible, eager or replayed.  (The bf16 steps never read _sk: their gemm_gl
        # split-K is deterministic, and an align net keeps the usual split factors there.)
        self._sk = 1 if (self.align and not self.fast) else "auto"
        # splitk_reduce "fixed" (fp32): every backward GEMM splits ("auto", 'align' too) through fp32 slabs added
        # in a fixed order (ops.gemm(reduce="fixed")) and the bias gradients are fixed-order column sums
        # (ops.vp_colsum): the whole step repeats bit for bit.  Both workspaces are allocated below
        self.splitk_reduce = splitk_reduce
        self._gk = {}
        if splitk_reduce == "fixed":
            self._sk = "auto"
        self.pg = process_group
        # data parallel: the gradient is all-reduced with SUM and Adam applies 1 / world
        self.world = dp.world(process_group) if process_group is not None else 1
        self.T = ops.n_frames(n_samples)
        self.F = net.F
        dev = net.device
        B, K, N, T, F, H = batch, k, n_samples, self.T, net.F, net.H
        NGH = _ngate(net.cell) * H
        BT, FE = B * T, F * net.E
        f32 = dict(device=dev, dtype=torch.float32)
        # mixtures and scaled sources in ONE signal buffer [B + B K, N] (magnitude modes: one STFT
        # launch over both, their magnitudes likewise adjacent)
        self._sig = torch.empty(B + B * K, N, **f32)
        self.mix = self._sig[:B]
        self.src = self._sig[B:].view(B, K, N)
        self.stats = torch.empty(32 * B * K, **f32)  # mixing partials (dl4ss_mix_sources)
        if mode == "crm":
            self.mag_mix = torch.empty(B, T, F, **f32)
            self.Xc_mix = torch.empty(B, T, F, 2, **f32)
            self.Xc_src = torch.empty(B, K, T, F, 2, **f32)
        else:
            self.Xc_mix = None
            # (adversarial step: B K more maps behind the sources' for the predictions, so that one Discriminator
            # forward runs over [true; predicted]; the STFT launch still covers the first B + B K only)
            self._mag = torch.empty(B + B * K * (2 if adversary is not None else 1), T, F, **f32)
            self.mag_mix = self._mag[:B]
            self.mag_src = self._mag[B:B + B * K].view(B, K, T, F)
        self.out = [torch.empty(B, T, 2 * H, **f32) for _ in range(net.L)]
        self.hprev = [torch.empty(B, T, 2 * H, **f32) for _ in range(net.L)]
        self.act = [torch.empty(B, T, 2, 4 * H, **f32) for _ in range(net.L)]
        self.cs = [torch.empty(B, T, 2, H, **f32) for _ in range(net.L)] if net.cell == "lstm" else None
        self.G = torch.empty(BT, 2 * NGH, **f32)  # input projection, reused as dG
        self.dGh = torch.empty(BT, 2 * NGH, **f32) if net.cell == "gru" else None
        self.dH = [torch.empty(BT, 2 * H, **f32), torch.empty(BT, 2 * H, **f32)]
        self.V = torch.empty(BT, FE, **f32)  # tanh output; overwritten in place by dPre
        if splitk_reduce == "fixed":
            # one slab workspace for the largest request of the backward's GEMMs (dW_lin, dH, every layer's dW_ih,
            # dW_hh and dX), allocated here so that capture() never allocates
            shapes = [(FE, 2 * H, BT), (BT, 2 * H, FE), (NGH, H, BT), (BT, 2 * H, 2 * NGH)]
            shapes += [(2 * NGH, F if l == 0 else 2 * H, BT) for l in range(net.L)]
            nb = max(ops.gemm_fixed_ws_bytes(*s, "auto") for s in shapes)
            self.fixed_ws = torch.empty(max(nb, 4) // 4, **f32)
            self.cs_part = ops.vp_colsum_part(BT, max(FE, 2 * NGH), dev)
            self._gk = dict(reduce="fixed", ws=self.fixed_ws)
        W = net.W
        self.q = torch.empty(B, K, W, **f32)
        self.mean = torch.empty(B, 2 * H, **f32)
        self.dq = torch.empty(B, K, W, **f32)
        self.dh_bcast = torch.empty(B, 2 * H, **f32)
        self.nblk = _lib.query("dl4ss_attn_align_nblk", T * F) if self.align else _lib.query("dl4ss_attn_nblk", T, F)
        self.part_loss = torch.empty(B, self.nblk, K * K + 1, **f32)
        self.part_dq = torch.empty(B, self.nblk, K, W, **f32)
        if self.align:  # the align GRAD pass's partial records (dW1, dp, dw3 per block) + finalize scratch
            self.part_att = torch.empty(_lib.query("dl4ss_attn_align_part_floats", B, K, self.nblk), **f32)
        self.perm = torch.empty(B, K, device=dev, dtype=torch.int32)
        self.loss = torch.zeros(3, **f32)
        self.eval_out = torch.zeros(3, **f32)  # eval_loss()'s result: the step's loss stays the last step's
        ws = _lib.query("dl4ss_birnn_workspace_bytes", CELLS[net.cell], B, H)
        if ws < 0:
            raise RuntimeError("unsupported BiRNN configuration")
        self.ws_bytes = ws
        self.rnn_ws = torch.empty((ws + 7) // 8, device=dev, dtype=torch.int64)
        # bf16 fast path: one workspace per (layer, pass) (DL4SS_RNN_WS_ZEROED), zeroed here once instead of a
        # memset in front of every recurrence launch; check() zeroes them again after a timed-out launch
        w8 = (ws + 255) // 256 * 32
        self.rnn_ws_all = torch.zeros(2, net.L * w8, device=dev, dtype=torch.int64)  # [fwd | bwd][layer]
        self._w8 = w8
        # {hand-off timed out, refused-update count} (the recurrence kernels set [0]; the guarded
        # Adam counts its refusals in [1])
        self.status = torch.zeros(2, device=dev, dtype=torch.int32)
        okw = dict(kind=optimizer, schedule_decay=schedule_decay, clipnorm=self.clipnorm)
        query_net = voiceprint if voiceprint is not None else image_query
        if self.clipnorm is not None and query_net is not None:
            # the joint norm: one fp64 buffer [parts(net.flat) | parts(encoder.flat)], each optimizer writes its
            # slice and sums the whole (the same sum, bit for bit, and the same coefficient in both updates)
            n0 = ops.grad_sumsq_parts(net.flat.numel())
            joint = torch.zeros(n0 + ops.grad_sumsq_parts(query_net.flat.numel()), dtype=torch.float64, device=dev)
            okw.update(parts=(joint, 0))
        self.opt = adam.GuardedAdam(net.flat, self.status, self.loss, lr, betas, eps, clip_norm=self.clip_norm, **okw)
        if okw.get("parts"):
            okw.update(parts=(joint, n0))  # (the query encoder's optimizer, below)
        self.m, self.v = self.opt.m, self.opt.v
        if self.opt.clip is not None:
            self.grad_norm, self._nonfinite = self.opt.grad_norm, self.opt.nonfinite  # (_nonfinite: the tests read it)
        nch = loss_channels if loss_channels else K
        self.s1 = 1.0 / (B * nch * T * F)
        self.s2 = 0.0 if (mode == "crm" or loss_channels) else sum_weight / (B * T * F)
        self.spk = torch.empty(B, K, device=dev, dtype=torch.int32)
        self._works = []
        self._feed = None  # corpus.CorpusFeed, made by the first corpus step
        self._in_chain = False
        self._side_stream = self._side_gemm = self._fork_ev = None
        self._wb_ver = None
        self.adv = self.adv_opt = self.vp = None
        if adversary is not None:
            self.adv = AdvStep(adversary, B, K, self._mag, precision, self.status, self.loss,
                               lr if adv_lr is None else adv_lr, betas, eps, adv_weight, disc_adv_update,
                               self.adv_clip_norm)
            a = self.adv  # the documented names, and the two private ones the tests read (_dmaps, _dy)
            self.adv_opt, self.adv_m, self.adv_v, self.adv_weight = a.opt, a.opt.m, a.opt.v, a.adv_weight
            self.adv_loss, self.adv_scores, self.gext, self._dmaps, self._dy = a.adv_loss, a.scores, a.gext, a.maps, a.y
            if self.adv_clip_norm is not None:
                self.adv_grad_norm = self.adv_opt.grad_norm  # [grad_dis | grad_adv]
        if voiceprint is not None:
            self.vp = VoiceprintStep(voiceprint, memory, memory_refresh, self.mag_src, self.spk, self.q, self.dq,
                                     self.status, self.loss, lr if voiceprint_lr is None else voiceprint_lr, betas, eps,
                                     wgrad_split="auto" if splitk_reduce == "fixed" else 1, opt_kw=okw)
            self.vp_enc, self.vp_opt = self.vp.enc, self.vp.opt
        self.images = None
        if image_query is not None:  # the same slot: the trainer calls queries / backward / optimizer_step on either
            self.images = torch.zeros(B, K, image_query.h, image_query.w, **f32)
            self.vp = ImageQueryStep(image_query, memory, memory_refresh, self.images, self.spk, self.q, self.dq,
                                     self.status, self.loss, lr if image_query_lr is None else image_query_lr, betas,
                                     eps, opt_kw=okw)
            self.vp_enc, self.vp_opt = self.vp.enc, self.vp.opt
        if not self.fast:
            return
        # the bf16 step's operands, each produced directly as bf16 by the kernel that forms it (the BiRNN
        # kernels' h / h_{t-1} / dG / dGh, the attention's dPre, Adam's weight copies, the STFT's features);
        # rows padded to multiples of 8 (16-B aligned operand rows)
        bf = dict(device=dev, dtype=torch.bfloat16)
        self.xb0 = torch.zeros(BT, pad8(F), **bf)  # (row padding zero: the STFT writes columns < F only)
        self.outb = [torch.empty(BT, pad8(2 * H), **bf) for _ in range(net.L)]
        self.hprevb = [torch.empty(BT, 2 * pad8(H), **bf) for _ in range(net.L)]
        # every layer's bf16 dG (and GRU dGh) stays until the end of backward: the weight
        # gradients of all layers run as one grouped GEMM launch after the last BPTT
        self.dGb_l = [torch.empty(BT, 2 * NGH, **bf) for _ in range(net.L)]
        # GRU dGh: each direction's gate columns start 16-B aligned (900 -> 904,
        # DL4SS_RNN_DGH_PAD8): 16-B aligned LDS-DMA operand rows for each direction's dW_hh
        self.ngh_p8 = pad8(NGH)
        self.dGhb_l = [torch.empty(BT, 2 * self.ngh_p8, **bf) for _ in range(net.L)] if net.cell == "gru" else None
        self._dw_group = None
        # zero row padding (never written): gemm_gl reads k-contiguous rows in 8-element chunks
        self.dPreb = torch.zeros(BT, pad8(FE), **bf)
        # gemm_gl split-K slabs (the largest split of the backward: dH, dX, dW_lin, dW_ih, dW_hh)
        gl_need = max(_lib.query("dl4ss_gemm_bf16_gl_ws_bytes", BT, 2 * H, FE, max(1, self.dh_split), 1),
                      _lib.query("dl4ss_gemm_bf16_gl_ws_bytes", BT, 2 * H, 2 * NGH, 1, 1),
                      _lib.query("dl4ss_gemm_bf16_gl_ws_bytes", FE, 2 * H, BT, 2, 1),
                      _lib.query("dl4ss_gemm_bf16_gl_ws_bytes", 2 * NGH, 2 * H, BT, 4, 1),
                      _lib.query("dl4ss_gemm_bf16_gl_ws_bytes", NGH, H, BT, 8, 2))
        self.gl_ws = torch.empty(max(gl_need, 1), device=dev, dtype=torch.uint8)
        if self.dh_slabs > 1:
            # the slabs' own workspace: other split-K GEMMs between dH and the BPTT (dW_lin off the side
            # stream) must not overwrite them
            self.dh_ws = torch.empty(self.dh_slabs * BT * 2 * H * 4, device=dev, dtype=torch.uint8)
        # partial sums of the deterministic Linear-bias colsum (dl4ss_colsum_bf16_det)
        pb = _lib.query("dl4ss_colsum_bf16_part_bytes", BT, FE)
        self.colsum_part = torch.empty(max(1, pb // 4), device=dev, dtype=torch.float32)
        # V = tanh(Linear) in bf16 (even row length); bf16s keeps V in fp32 (self.V)
        self.Vb = None if self.split else torch.empty(BT, FE, **bf)
        self.wb_ih = [torch.empty(2 * NGH, pad8(F if l == 0 else 2 * H), **bf) for l in range(net.L)]
        self.wb_lin = torch.empty(FE, pad8(2 * H), **bf)
        if self.split:  # split-precision forward operands (K' = 3 segments of pad8(K) each)
            self.seg = [pad8(F if l == 0 else 2 * H) for l in range(net.L)]
            self.xs0 = torch.empty(BT, 3 * self.seg[0], **bf)
            self.xs = torch.empty(BT, 3 * pad8(2 * H), **bf)
            self.ws_ih = [torch.empty(2 * NGH, 3 * self.seg[l], **bf) for l in range(net.L)]
            self.ws_lin = torch.empty(FE, 3 * pad8(2 * H), **bf)
        if net.cell == "lstm":  # the LSTM BPTT never reads the fp32 h_{t-1}
            self.hprev = [None] * net.L

    # the documented scalars live in the optimizers, read / write (a schedule assigns lr, tests restore the counts)
    lr, adv_lr, vp_lr = (adam.delegate(o, "lr") for o in ("opt", "adv_opt", "vp_opt"))
    step_count = adam.delegate("opt", "step_count")
    skipped_nonfinite = adam.delegate("opt", "skipped_nonfinite")
    adv_step_count = adam.delegate("adv_opt", "step_count")
    adv_skipped_nonfinite = adam.delegate("adv_opt", "skipped_nonfinite", default=0)

    # ------------------------------------------------------------------ training state
    def _sections(self):
        """The trainer's optional parts by their name in a saved state (None: this trainer has none)."""
        return {"adversary": self.adv, "voiceprint": self.vp if self.vnet is not None else None,
                "image_query": self.vp if self.inet is not None else None}

    def require_settled(self, what="state_dict()"):
        """Synchronise; RuntimeError unless check() has settled every refused update (adam.require_settled)."""
        opts = [self.opt] + [s.opt for s in (self.adv, self.vp) if s is not None]
        adam.require_settled(self.status, opts, what)

    def state_dict(self):
        """Everything a continued run needs, as host copies in plain containers: the net's flat buffer with its
        layout, the optimizer (moments, applied-update count, lr, skipped count), and of the parts this trainer has
        the Discriminator and its Adam, or the query encoder, its optimizer and the speaker memory.  Batch size,
        precision, mode, eager or graph and world size are not part of it: a run may continue under others.  Of a
        settled trainer only (RuntimeError: run check() first).  DESIGN.md section 5, "Training state"."""
        self.require_settled()
        sd = {"net": self.net.flat_state(), "opt": self.opt.state_dict()}
        sd.update({name: part.state_dict() for name, part in self._sections().items() if part is not None})
        return sd

    def check_state_dict(self, sd):
        """Everything that refuses a load, before anything is written: ValueError naming the field and both values
        (layout, optimizer kind and hyper-parameters, a part on one side only, the memory's shape)."""
        self.require_settled("load_state_dict()")
        if not isinstance(sd, dict):
            raise ValueError("trainer: no trainer state in the file")
        self.net.check_flat_state(sd.get("net"), "net")
        self.opt.check_state_dict(sd.get("opt"), "optimizer")
        for name, part in self._sections().items():
            if (part is None) != (name not in sd):
                raise mismatch(name, "present" if name in sd else "absent", "absent" if part is None else "present")
            if part is not None:
                part.check_state_dict(sd[name], name)

    def load_state_dict(self, sd, checked=False):
        """Load a state_dict() in place: copy_ into the existing buffers, so a graph captured before stays valid and
        replays on the loaded state; every net written declares the change and the bf16 weight copies are marked
        stale (the next step, eager or replayed, converts them again)."""
        if not checked:
            self.check_state_dict(sd)
        self.net.load_flat_state(sd["net"])
        self.opt.load_state_dict(sd["opt"], checked=True)
        for name, part in self._sections().items():
            if part is not None:
                part.load_state_dict(sd[name], checked=True)
        self.params_changed()

    # ------------------------------------------------------------------ features
    def features(self, raw, gains, lengths=None):
        ops.mix_sources(raw, gains, out_src=self.src, out_mix=self.mix, stats_ws=self.stats, lengths=lengths)
        self._stfts()

    def _mix_corpus(self, corpus, clips, gains, shifts, spk_idx=None):
        """The step's sources and mixtures from a device-resident corpus (corpus.DeviceCorpus) in one launch: host
        index arrays clips, gains, shifts (B, Ks), K <= Ks (a source behind the K targets is in the mixture only),
        copied into trainer-owned device buffers in one asynchronous upload; spk_idx (B, K) goes with them when it is
        a host array (a device tensor is copied as step() copies it).  An out-of-range clip id is a silent source,
        reported by check()."""
        if self._feed is None:
            from .corpus import CorpusFeed  # (corpus imports the compat loaders' rules; not needed otherwise)
            self._feed = CorpusFeed(self.B, self.net.device)
        host_spk = None
        if isinstance(spk_idx, torch.Tensor) and spk_idx.is_cuda:
            self.spk.copy_(spk_idx)
        elif spk_idx is not None:
            host_spk = spk_idx.numpy() if isinstance(spk_idx, torch.Tensor) else spk_idx
        self._feed.mix(corpus, clips, gains, shifts, self.K, self.N, self.src, self.mix, spk=host_spk,
                       spk_out=self.spk)

    def features_corpus(self, corpus, clips, gains, shifts=None):
        """features() with the sources gathered from ``corpus`` by clip id instead of uploaded (``_mix_corpus``)."""
        self._mix_corpus(corpus, clips, gains, shifts)
        self._stfts()

    def _stfts(self):
        """The step's STFTs: cRM, the mixtures' complex + magnitude and the sources' complex
        spectra (two launches); magnitude modes, mixtures and sources in one launch over the
        shared signal buffer."""
        B, K, N = self.B, self.K, self.N
        # bf16 step: the mixtures' magnitudes also land in bf16 in the recurrence's input rows (xb0)
        xb = dict(out_bf16=self.xb0, n_bf16=B) if self.fast else {}
        if self.mode == "crm":
            ops.stft(self.mix, complex_out=True, mag_out=True, out_c=self.Xc_mix, out_mag=self.mag_mix, **xb)
            ops.stft(self.src.view(B * K, N), complex_out=True, mag_out=False, out_c=self.Xc_src.view(B * K, self.T,
                                                                                                     self.F, 2))
        else:
            ops.stft(self._sig, complex_out=False, mag_out=True, out_mag=self._mag, **xb)
        self._xb0_fresh = self.fast

    # ------------------------------------------------------------------ forward
    def _to_bf16_rows(self, x, out):
        """out[:, :cols] = bf16(x), zero row padding (dl4ss_f32_to_bf16_2d)."""
        _lib.call("dl4ss_f32_to_bf16_2d", _lib.ptr(x, True), x.stride(0), x.shape[0], x.shape[1], _lib.ptr(out),
                  out.stride(0), _lib.stream_ptr())

    def params_changed(self):
        """Tell the trainer that net.flat was rewritten by means that may bypass torch's version
        counter (a raw-pointer kernel, a collective, `.data`): the next step of every trainer on
        this net re-derives the bf16 weight copies instead of trusting the ones Adam keeps."""
        self.net.params_changed()
        self._wb_ver = None

    def _wb_key(self):
        return (self.net.generation, self.net.flat._version)

    def _wb_stale(self):
        return self._wb_ver is None or self._wb_ver != self._wb_key()

    def _weights_to_bf16(self, force=False):
        """The bf16 copies of every layer's W_ih and the Linear weight, one launch
        (dl4ss_f32_to_bf16_2d_multi) -- only when the parameters changed by other means than this
        trainer's Adam, which writes the copies itself (dl4ss_adam_guarded_dp_scaled_bf16, round 5):
        a torch in-place op on net.flat (a checkpoint load, the DP broadcast, a test's state restore)
        bumps its version counter, the device-side Adam does not -- it bumps the net's generation,
        so another trainer on the same net sees the change."""
        net = self.net
        if not hasattr(self, "_cvt_args"):
            pairs = [(net.cat_view("weight_ih", l), self.wb_ih[l]) for l in range(net.L)]
            pairs.append((net.view("mix.Linear.weight"), self.wb_lin))
            n = len(pairs)
            P = ctypes.c_void_p
            self._cvt_args = (n, (P * n)(*[x.data_ptr() for x, _ in pairs]),
                              (ctypes.c_longlong * n)(*[x.stride(0) for x, _ in pairs]),
                              (ctypes.c_int * n)(*[x.shape[0] for x, _ in pairs]),
                              (ctypes.c_int * n)(*[x.shape[1] for x, _ in pairs]),
                              (P * n)(*[y.data_ptr() for _, y in pairs]),
                              (ctypes.c_longlong * n)(*[y.stride(0) for _, y in pairs]))
            base = net.flat.data_ptr()
            assert all(x.is_contiguous() for x, _ in pairs)
            self._shadow = (n, (ctypes.c_longlong * n)(*[(x.data_ptr() - base) // 4 for x, _ in pairs]),
                            self._cvt_args[3], self._cvt_args[4], self._cvt_args[5], self._cvt_args[6])
        if not force and self._shadow_on and not self._wb_stale():
            return
        _lib.call("dl4ss_f32_to_bf16_2d_multi", *self._cvt_args, _lib.stream_ptr())
        self._wb_ver = self._wb_key()

    def _forward_prepare(self, x):
        """The bf16 steps' work in front of the first layer: the optional workspace fill, the bf16 weight
        copies, (bf16s) the split images of every weight, then the features' bf16 rows and split image."""
        net = self.net
        if self._ws_fill:
            self.rnn_ws_all.zero_()  # every layer's forward AND BPTT hand-off workspaces, one fill per step
        self._weights_to_bf16()
        if self.split:
            for l in range(net.L):  # bf16s2, layers >= 1: two terms [hi | hi] . [hi | lo]
                pat, nseg = (ops.W_SPLIT2, 2) if (l >= 1 and self.split_x2) else (ops.W_SPLIT, 3)
                ops.hilo(net.cat_view("weight_ih", l), self.ws_ih[l], self.seg[l], pat, nseg)
            ops.hilo(net.view("mix.Linear.weight"), self.ws_lin, pad8(2 * net.H), ops.W_SPLIT)
        if not self._xb0_ok:
            self._to_bf16_rows(x, self.xb0)
        if self.split:
            ops.hilo(x, self.xs0, self.seg[0], ops.A_SPLIT)

    def _split_input(self, l):
        """Layer l's output as the split A image of the next GEMM: [hi | lo | hi] (three terms), or
        [hi | hi] (bf16s2, into layers >= 1: two terms, K' = 2 pad8(2H)); the Linear's is three."""
        H, w = self.net.H, pad8(2 * self.net.H)
        src = self.out[l].view(self.B * self.T, 2 * H)
        if self.split_x2 and l < self.net.L - 1:
            ops.hilo(src, self.xs, w, ops.A_SPLIT2, 2)
            return self.xs[:, :2 * w]
        ops.hilo(src, self.xs, w, ops.A_SPLIT)
        return self.xs

    def _fwd_operands(self, l, x):
        """(input rows, weight) of layer l's input projection, l == L: of the Linear -- fp32, the bf16 rows
        and weight copies, or (bf16s: formed here from the layer below's fp32 output) the split images."""
        net, H = self.net, self.net.H
        if not self.fast:
            w = net.view("mix.Linear.weight") if l == net.L else net.cat_view("weight_ih", l)
            return (x if l == 0 else self.out[l - 1].view(-1, 2 * H)), w
        if self.split:
            xin, w = (self.xs0 if l == 0 else self._split_input(l - 1)), (self.ws_lin if l == net.L else self.ws_ih[l])
        else:
            xin = self.xb0[:, :x.shape[1]] if l == 0 else self.outb[l - 1][:, :2 * H]
            w = self.wb_lin if l == net.L else self.wb_ih[l]
        return xin, w[:, :xin.shape[1]]

    def _gemm_fwd(self, x, w, bias, out, epilogue=ops.EPI_NONE):
        """out = x w^T + bias (epilogue): the input projections and the Linear (+ tanh -> bf16 V)"""
        ops.gemm_bf16_gl(x, w, transB=True, bias=bias, epilogue=epilogue, out=out)

    def forward(self, feats=None):
        """Per layer the input projection fused into the packed recurrence (bf16 steps, where it is built),
        or a GEMM and then the recurrence; the Linear + tanh -> V; the speaker queries."""
        net, B, T, H = self.net, self.B, self.T, self.net.H
        x = (self.mag_mix if feats is None else feats).reshape(B * T, -1)
        # the STFT of this step already wrote x's bf16 rows (self.xb0) unless the features came from elsewhere
        self._xb0_ok = feats is None and getattr(self, "_xb0_fresh", False)
        self._xb0_fresh = False
        fast, bf16v = self.fast, self.fast and not self.split
        if fast:
            self._forward_prepare(x)
        for l in range(net.L):
            xin, w = self._fwd_operands(l, x)
            kw = dict(w_hh=net.cat_view("weight_hh", l), b_hh=net.cat_view("bias_hh", l), hprev=self.hprev[l],
                      act=self.act[l], cs=self.cs[l] if self.cs else None, ws=self.rnn_ws, ws_bytes=self.ws_bytes,
                      status=self.status)
            if fast:  # the bf16 layer outputs; the last layer forms the time mean of ADDJUST / the query (h_mean)
                kw.update(out_bf16=self.outb[l], hprev_bf16=self.hprevb[l], ws=self._ws_slot(l, False),
                          h_mean=self.mean if (bf16v and l == net.L - 1) else None)
            K = xin.shape[1]
            if ((self.xw and K <= self.xw_kmax) or (self.xw_split0 and l == 0)) and \
                    _lib.query("dl4ss_birnn_fwd_xw_supported", CELLS[net.cell], B, T, H, K) == 1:
                # (bf16: no fp32 layer output, the next layer and the GEMMs read the bf16 one)
                ops.birnn_fwd_xw(net.cell, B, T, H, x=xin, w_ih=w, b_ih=net.cat_view("bias_ih", l),
                                 out=self.out[l] if self.split else None, **kw)
                continue
            if fast:
                self._gemm_fwd(xin, w, net.cat_view("bias_ih", l), self.G)
            else:
                ops.gemm(xin, w, transB=True, bias=net.cat_view("bias_ih", l), out=self.G, precision=self.precision)
            ops.birnn_fwd(net.cell, B, T, H, G=self.G, out=self.out[l], precision=self.rnn_precision,
                          flags=(WS_ZEROED if fast else 0) | self.rnn_flags, **kw)
        xin, w = self._fwd_operands(net.L, x)
        if fast:  # bf16: V itself is bf16 (the EPI_TANH_BF16 epilogue); bf16s keeps it fp32
            self._gemm_fwd(xin, w, net.view("mix.Linear.bias"), self.Vb if bf16v else self.V,
                           ops.EPI_TANH_BF16 if bf16v else ops.EPI_TANH)
        else:
            ops.gemm(xin, w, transB=True, bias=net.view("mix.Linear.bias"), epilogue=ops.EPI_TANH, out=self.V,
                     precision=self.precision)
        if self.vp is not None:  # the queries are voiceprints read back from the speaker memory
            self.vp.queries(self.q)
            return
        wadj = net.view("adj.layer.weight") if net.adjust else None
        # (bf16: the time mean is already in self.mean, the query kernel reads no layer output)
        _lib.call("dl4ss_query_fwd", h=None if bf16v else _lib.ptr(self.out[-1]), B=B, T=T, D=2 * H,
                  idx=_lib.ptr(self.spk), emb=_lib.ptr(net.view("emb.layer.weight")), w_adj=_lib.ptr(wadj), K=self.K,
                  W=net.W, q=_lib.ptr(self.q), mean_out=_lib.ptr(self.mean), stream=_lib.stream_ptr())

    def _attn_args(self):
        B, K, T, F = self.B, self.K, self.T, self.F
        TF = T * F
        if self.mode == "crm":
            return self.Xc_mix, TF, self.Xc_src, K * TF, TF
        return self.mag_mix, TF, self.mag_src, K * TF, TF

    def attn(self, pass_, perm=None, mask_out=None, pred_out=None, gext=None):
        """One pass of the fused attention + loss kernels.  ``gext`` (GRAD pass of an adversarial step): a
        second gradient at the prediction, (B, K, T, F) -- the adversarial form of the same kernel."""
        X, xs, Y, ys, yks = self._attn_args()
        grad, ptr = pass_ == 1, _lib.ptr
        # what the four entry points share, by the header's parameter names
        kw = dict(B=self.B, K=self.K, T=self.T, F=self.F, E=self.net.E, q=ptr(self.q), X=ptr(X), x_bstride=xs,
                  Y=ptr(Y), y_bstride=ys, y_kstride=yks, perm=ptr(perm), s1=self.s1, s2=self.s2,
                  part_loss=ptr(self.part_loss), mask_out=ptr(mask_out), pred_out=ptr(pred_out),
                  stream=_lib.stream_ptr())
        # bf16 path: V itself is bf16 (the Linear's EPI_TANH_BF16 epilogue); bf16s: fp32 V, bf16 dPre
        bf16v = self.fast and not self.split
        if self.align and gext is None:
            net = self.net
            akw = dict(pass_=pass_, W1=ptr(net.view("att.Linear_1.weight")), W2=ptr(net.view("att.Linear_2.weight")),
                       w3=ptr(net.view("att.Linear_3.weight")), part=ptr(self.part_att) if grad else None,
                       part_floats=self.part_att.numel(), **kw)
            if self.fast:  # the same kernel text on bf16 V (bf16) or fp32 V (bf16s), dPre into the GEMMs' bf16 rows
                _lib.call("dl4ss_mask_attn_align_loss_ex", V=None if bf16v else ptr(self.V),
                          V_bf16=ptr(self.Vb) if bf16v else None, dPre=None, dPre_bf16=ptr(self.dPreb),
                          dpre_bf16_ld=self.dPreb.stride(0), **akw)
            else:
                _lib.call("dl4ss_mask_attn_align_loss", V=ptr(self.V), dPre=ptr(self.V) if grad else None, **akw)
            return
        kw["V_bf16" if bf16v else "V"] = ptr(self.Vb if bf16v else self.V)
        # (the COST pass gets dPre_bf16 too: it selects the same attention kernel as the GRAD pass)
        kw.update(dPre_bf16=ptr(self.dPreb) if self.fast else None,
                  dpre_bf16_ld=self.dPreb.stride(0) if self.fast else 0)
        if gext is not None:
            _lib.call("dl4ss_mask_attn_loss_adv_bf16v" if bf16v else "dl4ss_mask_attn_loss_adv", dpred_extra=ptr(gext),
                      dPre=None if self.fast else ptr(self.V), part_dq=ptr(self.part_dq), **kw)
            return
        _lib.call("dl4ss_mask_attn_loss_bf16v" if bf16v else "dl4ss_mask_attn_loss_ex", pass_=pass_,
                  crm=int(self.mode == "crm"), dPre=ptr(self.V) if grad and not self.fast else None,
                  part_dq=ptr(self.part_dq) if grad else None, **kw)

    def loss_and_grad(self):
        """Fused attention + loss + dPre (in place over V) + dq; returns loss (device)."""
        st = _lib.stream_ptr()
        perm = None
        adv = self.adv is not None
        if self.mode == "pit" or adv:  # (an adversary in label order: a COST pass only for the predictions)
            self.attn(0, pred_out=self.adv.pred if adv else None)
        if self.mode == "pit":
            _lib.call("dl4ss_pit_select", _lib.ptr(self.part_loss), self.B, self.K, self.nblk, _lib.ptr(self.perm), st)
            perm = self.perm
        if adv:  # the Discriminator on [true; predicted], its two gradients and gext = d(lambda L_adv)/dpred
            self.adv.disc_grads()
        self.attn(1, perm, gext=self.adv.gext if adv else None)
        if self.align:
            # the loss from the same partials; dq and the three attention-weight gradients from the align
            # partials, straight into their views of the flat gradient (backward_early zeroes only the
            # range in front of them; the bf16 steps zero nothing: each of the four has this one writer)
            net, g = self.net, self.net.grad
            _lib.call("dl4ss_loss_finalize", part_loss=_lib.ptr(self.part_loss), B=self.B, K=self.K, nblk=self.nblk,
                      perm=_lib.ptr(perm), s1=self.s1, s2=self.s2, loss_out=_lib.ptr(self.loss), part_dq=None, qw=net.W,
                      dq=None, stream=st)
            _lib.call("dl4ss_attn_align_finalize", part=_lib.ptr(self.part_att), part_floats=self.part_att.numel(),
                      B=self.B, K=self.K, T=self.T, F=self.F, q=_lib.ptr(self.q),
                      W2=_lib.ptr(net.view("att.Linear_2.weight")), dq=_lib.ptr(self.dq),
                      dW1=_lib.ptr(net.view("att.Linear_1.weight", g)),
                      dW2=_lib.ptr(net.view("att.Linear_2.weight", g)),
                      dw3=_lib.ptr(net.view("att.Linear_3.weight", g)), stream=st)
            return self.loss
        _lib.call("dl4ss_loss_finalize", part_loss=_lib.ptr(self.part_loss), B=self.B, K=self.K, nblk=self.nblk,
                  perm=_lib.ptr(perm), s1=self.s1, s2=self.s2, loss_out=_lib.ptr(self.loss),
                  part_dq=_lib.ptr(self.part_dq), qw=self.net.W, dq=_lib.ptr(self.dq), stream=st)
        return self.loss

    # ------------------------------------------------------------------ backward
    def _weight_grad_group(self):
        """The step's weight gradients (dW_lin, then every layer's dW_ih and both directions'
        dW_hh) as one grouped gemm_gl launch + one split-K combine (ops.GroupedGemm), after the last
        BPTT: one at a time they under-fill the chip (dW_ih 95 tiles x 4 splits, dW_hh 2 x 30 tiles
        x 8 splits, each with its own ramp and tail).  Each gradient is bitwise what a single
        launch with the same split factor produces (tests/test_gemm_grouped_gpu.py).  The weight gradients
        accumulate (beta 1) onto the zeroed flat gradient: the reference's loss.backward()
        (TDAA_beta/main_run_sstune_EvalVer.py:673).  Returns the list of launches: one, or with three
        data-parallel buckets two -- the layers >= dp_layer, then the rest -- each gradient bitwise the
        one-launch form's (same split factors; step_plan's dw_splits)."""
        if self._dw_group is not None:
            return self._dw_group
        net, H = self.net, self.net.H
        NGH = _ngate(net.cell) * H
        FE = self.F * net.E
        g = net.grad
        hp8 = pad8(H)
        gru = self.dGhb_l is not None
        ldgh = self.ngh_p8 if gru else NGH
        s_lin, s_ih, s_hh = self.dw_splits

        def layer_probs(layers):
            # longest k-ranges first (dW_lin 63 k-tiles per workgroup, dW_ih 32, dW_hh 16): the short
            # ones fill the tail
            probs = []
            for l in layers:
                xb = self.xb0[:, :self.F] if l == 0 else self.outb[l - 1][:, :2 * H]
                probs.append(dict(A=self.dGb_l[l], B=xb, out=net.cat_view("weight_ih", l, g), transA=True,
                                  transB=False, beta=self._gbeta, splitk=s_ih))
            for l in layers:
                src = self.dGhb_l[l] if gru else self.dGb_l[l]
                whh = net.cat_view("weight_hh", l, g)
                for d in range(2):
                    probs.append(dict(A=src[:, d * ldgh:d * ldgh + NGH], B=self.hprevb[l][:, d * hp8:d * hp8 + H],
                                      out=whh[d * NGH:(d + 1) * NGH], transA=True, transB=False, beta=self._gbeta,
                                      splitk=s_hh))
            return probs

        lin = [] if (self.buckets or self.side) else [dict(A=self.dPreb[:, :FE], B=self.outb[-1][:, :2 * H],
                                             out=net.view("mix.Linear.weight", g), transA=True, transB=False,
                                             beta=self._gbeta, splitk=s_lin)]
        Ls = self.dp_layer if self.dp_layer is not None else 0
        self._dw_group = [ops.GroupedGemm(lin + layer_probs(range(net.L - 1, Ls - 1, -1)), net.device)]
        if Ls:
            self._dw_group.append(ops.GroupedGemm(layer_probs(range(Ls - 1, -1, -1)), net.device))
        return self._dw_group

    def _backward_fast_early(self):
        """The bf16 backward up to the first BPTT: the Linear's input gradient dH (all the BPTT chain
        waits on), its bias gradient, and -- ungrouped or data-parallel bucketed -- its weight
        gradient."""
        net, H = self.net, self.net.H
        FE = self.F * net.E
        g = net.grad
        dPreb = self.dPreb[:, :FE]
        # gemm_gl split-K factors, measured per shape at C2 (tools/gemm_gl_bench.py --sweep): dH
        # 8032x600x6450 -> 3, dW_lin 6450x600x8032 -> 2, dX 8032x600x2400 -> 1, dW_ih
        # 2400x600x8032 -> 4, dW_hh 2 x 1200x300x8032 -> 8 (slabs + a fixed-order reduce)
        if self.dh_slabs > 1:  # the slabs stay in dh_ws: the top layer's BPTT sums them (DL4SS_RNN_DOUT_SLABS)
            ops.gemm_bf16_gl(dPreb, self.wb_lin[:, :2 * H], out=self.dH[0], splitk=self.dh_split, ws=self.dh_ws,
                             epilogue=ops.EPI_SPLIT_SLABS)
        else:
            ops.gemm_bf16_gl(dPreb, self.wb_lin[:, :2 * H], out=self.dH[0], splitk=self.dh_split, ws=self.gl_ws)
        if self.side:
            # the fork point.  The side launch itself is enqueued after the first BPTT, so that a captured
            # graph keeps the chain on the main queue and puts the side GEMM on the second
            if self._fork_ev is None:
                self._fork_ev = torch.cuda.Event()
            self._fork_ev.record()
            return
        if not self.grouped or self.buckets:  # (bitwise the grouped launch's dW_lin at the same split)
            ops.gemm_bf16_gl(dPreb, self.outb[-1][:, :2 * H], transA=True, out=net.view("mix.Linear.weight", g),
                             beta=self._gbeta, splitk=2, ws=self.gl_ws)
        self._colsum_lin_bias()

    def _colsum_lin_bias(self):
        """The Linear's bias gradient as the deterministic column sums of dPre."""
        net, g = self.net, self.net.grad
        _lib.call("dl4ss_colsum_bf16_det_ex", _lib.ptr(self.dPreb), self.dPreb.stride(0), self.B * self.T,
                  self.F * net.E, _lib.ptr(net.view("mix.Linear.bias", g)), _lib.ptr(self.colsum_part),
                  self.colsum_part.numel() * 4, self._gbeta, _lib.stream_ptr())

    def _side_launch(self):
        """Fork: the side stream waits for the fork event (the work enqueued up to the dH GEMM), then runs
        the persistent dW_lin (+ bias row sums) launch beside the BPTT chain.  The gradient zeroing and the
        query backward stay on the main stream, before dH (DESIGN.md section 11 has the measured
        alternatives)."""
        net, H = self.net, self.net.H
        g = net.grad
        FE = self.F * net.E
        if self._side_stream is None:
            grid, cfg, split, one = self.side
            self._side_stream = torch.cuda.Stream(device=net.device)
            self._side_gemm = ops.GroupedGemm(
                [dict(A=self.dPreb[:, :FE], B=self.outb[-1][:, :2 * H], out=net.view("mix.Linear.weight", g),
                      transA=True, transB=False, beta=self._gbeta, splitk=split,
                      rowsum=net.view("mix.Linear.bias", g) if split == 1 else None)],
                net.device, grid=grid, cfg=cfg, one_per_cu=one)
        self._side_stream.wait_event(self._fork_ev)
        with torch.cuda.stream(self._side_stream):
            if self.side[2] != 1:  # split dW_lin: no row sums, the bias gradient by colsum
                self._colsum_lin_bias()
            self._side_gemm.run()

    def _backward_chain(self):
        """The bf16 BPTT / dX chain down the layers, the side stream joined at its end.  No collective may
        start while it is being enqueued (_allreduce)."""
        self._in_chain = True
        try:
            self._enqueue_chain()
        finally:
            self._in_chain = False

    def _enqueue_chain(self):
        net, B, T, H = self.net, self.B, self.T, self.net.H
        BT = B * T
        NGH = _ngate(net.cell) * H
        g = net.grad
        gru = self.dGhb_l is not None
        if self.grouped:
            self._weight_grad_group()  # (built by the first step, in front of its chain)
        # (the BPTT hand-off workspaces were zeroed with the forward's, in the step's one fill)
        dH = self.dH[0]
        hp8 = pad8(H)
        ldgh = self.ngh_p8 if gru else NGH  # dW_hh operand: direction d at column d * ldgh
        for l in range(net.L - 1, -1, -1):
            top = l == net.L - 1
            dGb = self.dGb_l[l]
            dGhb = self.dGhb_l[l] if gru else dGb
            # the top layer reads dH as the dH GEMM's split-K slabs (summed as it loads them); the bias
            # partials stay in the workspace until the one reduce after the last BPTT (_bias_reduce)
            slabs = self.dh_slabs if top else 1
            ops.birnn_bwd(net.cell, B, T, H, precision="bf16",
                          flags=WS_ZEROED | DEFER_BIAS | (DGH_PAD8 if gru else 0) | DOUT_SLABS(slabs),
                          dOut=self.dh_ws if slabs > 1 else dH,
                          dOut_bcast=self.dh_bcast if (top and net.adjust) else None,
                          w_hh=net.cat_view("weight_hh", l), act=self.act[l], cs=self.cs[l] if self.cs else None,
                          hprev=self.hprev[l], dG_bf16=dGb, dGh_bf16=dGhb if gru else None,
                          db_ih=net.cat_view("bias_ih", l, g), db_hh=net.cat_view("bias_hh", l, g),
                          ws=self._ws_slot(l, True), ws_bytes=self.ws_bytes, status=self.status)
            if self.side and top:
                self._side_launch()
            if l > 0:  # the input gradient: all the next BPTT waits on
                dH_next = self.dH[1] if dH is self.dH[0] else self.dH[0]
                ops.gemm_bf16_gl(dGb, self.wb_ih[l][:, :2 * H], out=dH_next, splitk=1, ws=self.gl_ws)
            if not self.grouped:
                xb = self.xb0[:, :self.F] if l == 0 else self.outb[l - 1][:, :2 * H]
                ops.gemm_bf16_gl(dGb, xb, transA=True, out=net.cat_view("weight_ih", l, g), beta=1.0, splitk=4,
                                 ws=self.gl_ws)
                # both directions' dW_hh in one launch: member d = columns d*ldgh of dGh, d*pad8(H) of h_{t-1}
                ops.gemm_bf16_gl(dGhb[:, :NGH], self.hprevb[l][:, :H], transA=True,
                                 out=net.cat_view("weight_hh", l, g)[:NGH], beta=1.0, splitk=8, batch=2, strideA=ldgh,
                                 strideB=hp8, strideC=NGH * H, M=NGH, N=H, K=BT, ws=self.gl_ws)
            if l > 0:
                dH = dH_next
        # the side stream joins at the end of the chain (it ends inside the last BPTT): a join after the
        # grouped launch cost ~9 us more per step (the cross-queue wait in front of Adam; A/B x3, round 5)
        if self.side:
            torch.cuda.current_stream().wait_stream(self._side_stream)

    def _backward_wgrad(self, which="all"):
        """The recurrent layers' bias reduce and grouped weight-gradient launch(es) (after the chain).
        Three data-parallel buckets: "upper" (the bias reduce + the layers >= dp_layer) and "lower"."""
        if which != "lower":
            self._bias_reduce()
        if self.grouped:
            groups = self._weight_grad_group()
            for grp in (groups if which == "all" else groups[:1] if which == "upper" else groups[1:]):
                grp.run()

    def _bias_reduce(self):
        """Every layer's BPTT bias partials (DL4SS_RNN_DEFER_BIAS) into db_ih / db_hh, one launch."""
        net, g = self.net, self.net.grad
        if not hasattr(self, "_bias_args"):
            n = net.L
            P = ctypes.c_void_p
            self._bias_args = (n, (P * n)(*[self._ws_slot(l, True).data_ptr() for l in range(n)]),
                               (P * n)(*[net.cat_view("bias_ih", l, g).data_ptr() for l in range(n)]),
                               (P * n)(*[net.cat_view("bias_hh", l, g).data_ptr() for l in range(n)]))
        _lib.call("dl4ss_birnn_bias_reduce_ex", CELLS[net.cell], self.B, net.H, *self._bias_args, self._gbeta,
                  _lib.stream_ptr())

    def backward(self):
        self.backward_early()
        self.backward_late()

    def backward_early(self):
        """The backward up to the first BPTT: the query / embedding / ADDJUST gradients and the
        Linear's.  Every gradient of the data-parallel early bucket (the flat range from
        SepNet.bucket_split on) is complete when this returns (in stream order)."""
        net, H = self.net, self.net.H
        g = net.grad
        # (zero_free, the grouped bf16 backward: every gradient has one writer per step, 'align' included -- the
        # finalize in loss_and_grad WRITES dq and the three attention-weight gradients -- so nothing is zeroed)
        if self.zero_free:
            pass
        elif self.align:  # the attention-weight gradients behind this range were written by loss_and_grad
            g[:net.offsets["att.Linear_1.weight"][0]].zero_()
        else:
            g.zero_()
        self._query_bwd()
        if self.fast:
            self._backward_fast_early()
            return
        dPre = self.V
        hL = self.out[-1].view(self.B * self.T, 2 * H)
        # grads were zeroed above: weight gradients accumulate (beta 1) with split-K
        # (splitk_reduce "fixed": _gk selects the fixed-order reduce and the trainer's slab workspace)
        ops.gemm(dPre, hL, transA=True, out=net.view("mix.Linear.weight", g), beta=1.0, splitk=self._sk,
                 precision=self.precision, **self._gk)
        self._colsum(dPre, net.view("mix.Linear.bias", g))
        ops.gemm(dPre, net.view("mix.Linear.weight"), out=self.dH[0], splitk=self._sk, precision=self.precision,
                 **self._gk)

    def _colsum(self, A, out):
        """A bias gradient: the column sums of A added into the zeroed gradient (ops.colsum: row blocks added
        atomically), or (splitk_reduce "fixed") written over it in a fixed order (ops.vp_colsum): the same values."""
        if self._gk:
            ops.vp_colsum(A, out, self.cs_part)
        else:
            ops.colsum(A, out)

    def _query_bwd(self):
        """SPEECH_EMBEDDING / ADDJUST backward: the embedding and ADDJUST gradients (added into the
        zeroed flat gradient, or written over it when zero_free) and dh_bcast, ADDJUST's share of the
        last layer's output gradient."""
        net, B, T, H = self.net, self.B, self.T, self.net.H
        g = net.grad
        if self.vp is not None:  # emb.layer.weight's gradient stays zero (backward_early zeroed it)
            self.vp.backward()
            return
        wadj = net.view("adj.layer.weight") if net.adjust else None
        _lib.call("dl4ss_query_bwd_ex", dq=_lib.ptr(self.dq), B=B, T=T, D=2 * H, idx=_lib.ptr(self.spk),
                  emb=_lib.ptr(net.view("emb.layer.weight")), w_adj=_lib.ptr(wadj), mean=_lib.ptr(self.mean), K=self.K,
                  W=net.W, d_emb=_lib.ptr(net.view("emb.layer.weight", g)),
                  d_wadj=_lib.ptr(net.view("adj.layer.weight", g)) if net.adjust else None,
                  dh_bcast=_lib.ptr(self.dh_bcast) if net.adjust else None, n_labels=net.num_labels, beta=self._gbeta,
                  stream=_lib.stream_ptr())

    def backward_late(self):
        """The BPTT chain and the recurrent layers' weight / bias gradients, then the status flag."""
        net, B, T, H = self.net, self.B, self.T, self.net.H
        BT = B * T
        NGH = _ngate(net.cell) * H
        g = net.grad
        if self.fast:
            self._backward_chain()
            self._backward_wgrad()
            self._status_flag()
            return
        dH = self.dH[0]
        for l in range(net.L - 1, -1, -1):
            dG = self.G
            dGh = self.dGh if self.dGh is not None else dG
            ops.birnn_bwd(net.cell, B, T, H, precision=self.rnn_precision, dOut=dH,
                          dOut_bcast=self.dh_bcast if (l == net.L - 1 and net.adjust) else None,
                          w_hh=net.cat_view("weight_hh", l), act=self.act[l], cs=self.cs[l] if self.cs else None,
                          hprev=self.hprev[l], dG=dG, dGh=self.dGh, ws=self.rnn_ws, ws_bytes=self.ws_bytes,
                          status=self.status, flags=self.rnn_flags)
            xl = self.mag_mix.view(BT, -1) if l == 0 else self.out[l - 1].view(BT, 2 * H)
            ops.gemm(dG, xl, transA=True, out=net.cat_view("weight_ih", l, g), splitk=self._sk, beta=1.0,
                     precision=self.precision, **self._gk)
            self._colsum(dG, net.cat_view("bias_ih", l, g))
            whh_g = net.cat_view("weight_hh", l, g)
            hp = self.hprev[l].view(BT, 2 * H)
            for d in range(2):
                ops.gemm(dGh[:, d * NGH:(d + 1) * NGH], hp[:, d * H:(d + 1) * H], transA=True,
                         out=whh_g[d * NGH:(d + 1) * NGH], splitk=self._sk, beta=1.0, precision=self.precision,
                         **self._gk)
            self._colsum(dGh, net.cat_view("bias_hh", l, g))
            if l > 0:
                dH_next = self.dH[1] if dH is self.dH[0] else self.dH[0]
                ops.gemm(dG, net.cat_view("weight_ih", l), out=dH_next, splitk=self._sk, precision=self.precision,
                         **self._gk)
                dH = dH_next
        self._status_flag()

    def _status_flag(self):
        """Data parallel: this rank's hand-off status as the float behind the flat gradient
        (rewritten every step), combined by the all-reduce (allreduce()).  Without a process
        group the slot stays zero."""
        if self.pg is not None:
            _lib.call("dl4ss_status_flag", _lib.ptr(self.status), _lib.ptr(self.net.dp_flag), _lib.stream_ptr())

    def allreduce(self):
        """START the RCCL all-reduce (SUM) of the whole flat gradient, asynchronously; Adam applies the 1 / world of
        the mean (no separate pass over the buffer).  The slot in front of the gradient carries this rank's hand-off
        status flag (dl4ss_status_flag, written at the end of backward()): after the sum it is non-zero on every
        rank iff a hand-off timed out on any rank, and the guarded Adam reads it (a timed-out rank's
        incomplete gradient must not reach the healthy ranks' weights either).  Bucketed steps (self.buckets) use
        allreduce_early / _late.

        Contract: net.grad is complete only after wait_allreduce() (optimizer_step()
        calls it), and it then holds the SUM over ranks, not the mean -- grad_mean() is the mean."""
        if self.pg is not None:
            self._allreduce(None, None)

    def _allreduce(self, lo, hi):
        """Start the asynchronous SUM all-reduce of net.grad_ext[lo:hi].  Invariant: no collective starts
        while the BPTT chain is being enqueued.  The persistent recurrence needs all its workgroups co-resident, and
        the side-stream dW_lin holds every CU the recurrence plan leaves free for the whole chain; a collective
        kernel placed beside the chain could keep a recurrence workgroup off the device (a hand-off timeout, then a
        refused step).  Every all-reduce of the step therefore starts after the chain."""
        if self._in_chain:
            raise RuntimeError("a gradient all-reduce was started inside the BPTT chain")
        self._works.append(dp.allreduce_sum_async(self.net.grad_ext[lo:hi], self.pg))

    def allreduce_early(self):
        """Start the SUM all-reduce of the early bucket (Linear -- formed on the side stream, joined at the end of the
        chain --, embedding, ADDJUST gradients): asynchronous, on the process group's stream after the work enqueued
        so far.  The bucketed step starts it after the BPTT chain, beside the recurrent layers' weight gradients."""
        self._allreduce(self.net.bucket_split(), None)

    def allreduce_mid(self):
        """Three buckets: start the SUM all-reduce of the upper recurrent layers (>= dp_layer), complete
        after the first weight-gradient launch, beside the second."""
        self._allreduce(self.net.bucket_mid(self.dp_layer), self.net.bucket_split())

    def allreduce_late(self):
        """Start the SUM all-reduce of the late bucket: the status flag and every recurrent layer (two
        buckets), or the layers below dp_layer (three)."""
        self._allreduce(None, self.net.bucket_split() if self.dp_layer is None else self.net.bucket_mid(self.dp_layer))

    def wait_allreduce(self):
        """The current stream waits for every all-reduce started this step: net.grad then holds the
        gradient SUM over ranks (for callers that inspect it before optimizer_step(), which calls this
        itself; grad_mean() gives the mean).  To clip the global norm, build the trainer with clip_norm:
        the clip then runs on device inside optimizer_step(), with no pass over the gradient of its own."""
        for w in self._works:
            if w is not None:
                w.wait()
        self._works = []

    def grad_mean(self):
        """The global-batch mean gradient (a new tensor): the all-reduced SUM x 1 / world, the
        arithmetic the guarded Adam applies (gscale).  For inspection: clip_norm clips this gradient's
        global norm without forming it, and leaves the norm in grad_norm."""
        self.wait_allreduce()
        return self.net.grad * (1.0 / self.world)

    def optimizer_step(self):
        """Adam on device; refused (parameters untouched, loss[0] = NaN) when a recurrence
        hand-off of this step timed out on this rank or (data parallel) on any rank -- a
        timed-out step never reaches the weights.  A refused step is counted on device
        (status[1]); check() takes the refused steps back out of step_count, so the bias
        corrections follow the updates actually applied, as torch.optim.Adam's do.  Data
        parallel: the gradient is the SUM over ranks, scaled by 1 / world inside the update.

        clip_norm: one sum-of-squares launch over net.grad (the all-reduced SUM, so every rank forms the
        same coefficient), then the clipped Adam: the global-batch mean gradient's L2 norm is clipped to
        clip_norm as torch.nn.utils.clip_grad_norm_ does, the factor folded into the 1 / world scale (no pass
        that writes the gradient, no host sync); grad_norm holds {the norm before clipping, the coefficient}
        afterwards (device, not synced).  A gradient with an Inf or NaN is refused like a timed-out step and
        counted; check() rolls it out of step_count and adds it to skipped_nonfinite without raising.  The
        Discriminator's updates run first and are guarded by adv_clip_norm alone: a non-finite separation
        gradient does not undo them.

        optimizer="nadam": the same launch sequence with dl4ss_nadam, its momentum schedule taken from the step
        count on the host (adam.nadam_schedule).  clipnorm: the clip by Keras's rule; with a query encoder both
        sums of squares go into one shared buffer before either update, so the net's and the encoder's updates
        clip by the one joint norm, and a joint norm that is not finite sets the sticky bit that stops the
        encoder's update and the memory store behind it (check() raises)."""
        self.wait_allreduce()
        if self.inet is not None:  # a non-finite loss refuses this step's updates and memory store
            self.vp.guard()
        if self.adv is not None:  # the Discriminator's updates first (the reference's order)
            self.adv.optimizer_step()
        shadow = self._shadow if (self._shadow_on and hasattr(self, "_shadow")) else None
        joint = self.opt.joint  # the joint norm: both sums of squares before either update
        if joint:
            self.opt.sumsq(self.net.grad)
            self.vp.opt.sumsq(self.vp.net.grad)
        self.opt.step(self.net.grad, dp_flag=self.net.dp_flag, gscale=1.0 / self.world, shadow=shadow, summed=joint)
        # the update bypasses torch's version counter: a new generation of the parameters, whose bf16
        # copies only this trainer holds (written by the same launch), and only if they were current
        # before it -- copies stale before the update stay stale after it
        fresh = shadow is not None and not self._wb_stale()
        self.net.params_changed()
        self._wb_ver = self._wb_key() if fresh else None
        if self.vp is not None:  # the encoder steps with the net's count, then the memory refresh
            self.vp.optimizer_step(self.opt.step_count)

    def set_images(self, images):
        """The step's images (B, K, h, w) into the trainer's buffer: required with image_query=, refused without."""
        if self.inet is None:
            if images is not None:
                raise ValueError("images= needs a trainer built with image_query= (an imagequery.ImageQueryNet)")
            return
        if images is None:
            raise ValueError("image_query: step() needs images= (B, K, h, w), one picture per source")
        if tuple(images.shape) != tuple(self.images.shape):
            raise ValueError(f"images {tuple(images.shape)}, expected {tuple(self.images.shape)}")
        self.images.copy_(images)

    def step(self, raw, gains, spk_idx, lengths=None, images=None):
        """One full training step on device-resident inputs; returns the loss tensor (not synced).  lengths (B, K)
        int32: each source's own length in samples (zero beyond: ops.mix_sources).  images (B, K, h, w): the
        pictures that name the sources (image_query= only)."""
        self.set_images(images)
        self.spk.copy_(spk_idx)
        self.features(raw, gains, lengths)
        return self._step_tail()

    def step_corpus(self, corpus, clips, gains, spk_idx, shifts=None, images=None):
        """step() on a batch named by clip ids of a device-resident corpus: clips, gains, shifts host arrays
        (B, Ks) (features_corpus); spk_idx (B, K) a device tensor or a host array (then it rides in the same upload:
        nothing of the step waits for the device); everything behind the mixing launch is step()'s."""
        self.set_images(images)
        self._mix_corpus(corpus, clips, gains, shifts, spk_idx)
        self._stfts()
        return self._step_tail()

    def _step_tail(self):
        """step() behind its features: forward, loss, backward, all-reduce, update."""
        self.forward()
        loss = self.loss_and_grad()
        if self.buckets:
            self.backward_early()
            self._backward_chain()
            self.allreduce_early()
            if self.dp_layer is not None:
                self._backward_wgrad("upper")
                self.allreduce_mid()
                self._backward_wgrad("lower")
            else:
                self._backward_wgrad()
            self._status_flag()
            self.allreduce_late()
        else:
            self.backward()
            self.allreduce()
        self.optimizer_step()
        return loss

    def eval_loss(self, raw, gains, spk_idx, lengths=None):
        """The trainer's own separation loss of one batch, forward only (a validation loss: what
        DL4SS_Keras/nnet.py:149-153 takes after every epoch): features(), forward(), the attention COST pass,
        dl4ss_pit_select in PIT mode and dl4ss_loss_finalize without dq.  Returns ``eval_out`` (device float[3]
        {total, MSE term, weighted sum-to-one term}, not synced; the next call overwrites it).  No parameter,
        gradient, optimizer moment, step count, status counter, memory row or parameter generation changes, and
        ``loss`` keeps the last step's; the step's scratch buffers are overwritten, as the next step overwrites them.
        An adversary is ignored: only the separation loss is reported.  Eager launches, also on a trainer that
        holds a captured graph.  A voiceprint= / image_query= trainer validates the target alone:
        targeteval.TargetEvaluator.eval_loss."""
        self._eval_refusals()
        self.spk.copy_(spk_idx)
        self.features(raw, gains, lengths)
        return self._eval_tail()

    def eval_loss_corpus(self, corpus, clips, gains, spk_idx, shifts=None):
        """eval_loss() on a batch named by clip ids of a device-resident corpus (features_corpus)."""
        self._eval_refusals()
        self._mix_corpus(corpus, clips, gains, shifts, spk_idx)
        self._stfts()
        return self._eval_tail()

    def _eval_refusals(self):
        if self.vp is not None or self.vnet is not None or self.inet is not None:
            raise ValueError("eval_loss(): a voiceprint= / image_query= trainer is validated on the target alone, by "
                             "targeteval.TargetEvaluator.eval_loss")

    def _eval_tail(self):
        """eval_loss() behind its features: forward, the attention COST pass, the loss."""
        self.forward()
        self.attn(0)
        st, perm = _lib.stream_ptr(), None
        if self.mode == "pit":
            _lib.call("dl4ss_pit_select", _lib.ptr(self.part_loss), self.B, self.K, self.nblk, _lib.ptr(self.perm), st)
            perm = self.perm
        _lib.call("dl4ss_loss_finalize", part_loss=_lib.ptr(self.part_loss), B=self.B, K=self.K, nblk=self.nblk,
                  perm=_lib.ptr(perm), s1=self.s1, s2=self.s2, loss_out=_lib.ptr(self.eval_out), part_dq=None,
                  qw=self.net.W, dq=None, stream=st)
        return self.eval_out

    # ------------------------------------------------------------------ HIP graph
    def _graph_body(self):
        """The launch sequence recorded into the step graph: STFT features of the mixed
        batch, forward, loss + its gradient, backward (everything between the mixing
        kernel and the all-reduce; no host synchronisation inside)."""
        self._stfts()
        self.forward()
        return self.loss_and_grad()

    def _ws_slot(self, l, bwd):
        """Layer l's hand-off workspace of the forward (bwd False) or BPTT pass.  (A method, not a
        lambda holding self: a reference cycle leaves a dropped trainer to the garbage collector,
        which could then free its device buffers in the middle of another trainer's graph capture.)"""
        return self.rnn_ws_all[int(bwd), l * self._w8:(l + 1) * self._w8]

    def capture(self):
        """Record STFT -> forward -> loss -> backward (~70 launches: persistent BiRNN
        kernels, gemm_gl GEMMs, attention, small kernels) as one HIP graph, replayed by
        step_graph() (not with voiceprint=: that step is eager only, NotImplementedError).  The mixing kernel (its
        input pointer changes per batch), the RCCL
        all-reduce and Adam (its bias correction is a per-step host scalar) stay eager launches
        around the replay.  Bucketed data parallel: two graphs, split where the early bucket's
        all-reduce starts -- after the BPTT chain, which the side-stream dW_lin (forked and joined
        inside the first graph) runs beside; the second graph (the recurrent layers' weight-gradient
        launch) then runs beside that all-reduce.  Three buckets: a third graph -- the second graph holds
        the bias reduce and the upper layers' weight gradients, the third the lower layers' and the status
        flag, with the middle bucket's all-reduce started between them.  Call after at least one eager
        step(), so every workspace exists before the capture."""
        import gc

        if self.vnet is not None:
            raise NotImplementedError("capture(): the voiceprint step is not built for HIP-graph capture; use step()")
        if self.inet is not None:
            raise NotImplementedError("capture(): the image-query step is not built for HIP-graph capture; use step()")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        g2 = torch.cuda.CUDAGraph() if self.buckets else None
        g3 = torch.cuda.CUDAGraph() if (self.buckets and self.dp_layer is not None) else None
        # no garbage collection while the stream is being captured: a collection that frees another
        # object's device memory mid-capture aborted the process (round 4, a dropped trainer's buffers)
        gc.collect()
        was_enabled = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g):
                self._graph_loss = self._graph_body()
                if g2 is None:
                    self.backward()
                else:
                    self.backward_early()
                    self._backward_chain()
            if g2 is not None and g3 is None:
                with torch.cuda.graph(g2, pool=g.pool()):
                    self._backward_wgrad()
                    self._status_flag()
            elif g3 is not None:
                with torch.cuda.graph(g2, pool=g.pool()):
                    self._backward_wgrad("upper")
                with torch.cuda.graph(g3, pool=g.pool()):
                    self._backward_wgrad("lower")
                    self._status_flag()
        finally:
            if was_enabled:
                gc.enable()
        torch.cuda.synchronize()
        self.graph, self.graph_late, self.graph_lower = g, g2, g3
        return g

    def step_graph(self, raw, gains, spk_idx):
        """step() with the captured graph: mixing, graph replay, all-reduce, Adam (bucketed: the
        early bucket's all-reduce between the first two replays, the middle one's between the second
        and the third)."""
        self._graph_ready()
        self.spk.copy_(spk_idx)
        ops.mix_sources(raw, gains, out_src=self.src, out_mix=self.mix, stats_ws=self.stats)
        return self._graph_tail()

    def step_graph_corpus(self, corpus, clips, gains, spk_idx, shifts=None):
        """step_corpus() with the captured graph: the one mixing launch stays an eager launch ahead of the replay,
        so ragged lengths and shifts -- which step_graph() does not take -- run through the replayed step."""
        self._graph_ready()
        self._mix_corpus(corpus, clips, gains, shifts, spk_idx)
        return self._graph_tail()

    def _graph_ready(self):
        if self.vnet is not None:
            raise NotImplementedError("step_graph(): the voiceprint step is not built for HIP-graph capture; "
                                      "use step()")
        if self.inet is not None:
            raise NotImplementedError("step_graph(): the image-query step is not built for HIP-graph capture; "
                                      "use step()")
        if getattr(self, "graph", None) is None:
            self.capture()

    def _graph_tail(self):
        """step_graph() behind its mixing launch: replay, all-reduce, update."""
        if self.fast and self._wb_stale():
            # parameters changed outside Adam since the capture
            self._weights_to_bf16()
        self.graph.replay()
        if self.graph_late is not None:
            self.allreduce_early()
            self.graph_late.replay()
            if self.graph_lower is not None:
                self.allreduce_mid()
                self.graph_lower.replay()
            self.allreduce_late()
        else:
            self.allreduce()
        self.optimizer_step()
        return self._graph_loss

    def check(self):
        """Raise if a recurrence hand-off timed out, here or (data parallel) on a peer rank, since
        the last check: the guarded Adam already refused every update computed from then on.
        The refused steps are taken back out of step_count and the status word is reset, so the
        trainer can continue after the caller has handled it.

        clip_norm / adv_clip_norm: updates refused only because their gradient held an Inf or NaN are
        taken out of step_count (adv_step_count) in the same way and added to skipped_nonfinite
        (adv_skipped_nonfinite); the device counters are reset and check() returns without raising.  As with
        time-outs, the bias corrections of the steps enqueued before this check count the skipped step.

        image_query: bit 1 of status[0] is the step's loss guard (dl4ss_imgq_guard: a loss that is not finite).
        The steps it refused -- the one with that loss and every one enqueued behind it -- are taken out of the
        step counts in the same way, the status word is reset and check() raises RuntimeError("non-finite loss
        ...") when bit 1 alone is set; with bit 0 set as well, the time-out's message.

        clipnorm with voiceprint= / image_query= (the joint norm): a joint sum of squares that is not finite sets
        bit 2 of status[0] (ops.STATUS_NONFINITE_GRAD), sticky in the same way, so that neither optimizer nor the
        memory store runs; the refused steps leave the step count, are added to skipped_nonfinite, the word is
        reset and check() raises RuntimeError("non-finite gradient ...").  Without a query encoder clipnorm is
        counted and skipped exactly as clip_norm is, with no raise.  The bits are tested one by one: a time-out
        (bit 0) comes first whatever else is set, then bit 2 (also with bit 1 beside it: a step enqueued behind
        the refusal whose loss was not finite either), then bit 1."""
        torch.cuda.synchronize()
        self._check_status()
        if self._feed is not None:
            self._feed.check()

    def _check_status(self):
        s, refused = (int(x) for x in self.status.tolist())
        if s or refused:
            self.status.zero_()
            # (optimizer, updates per step) on this status word; the voiceprint encoder's steps with the net's count
            opts = [(self.opt, 1)] + ([(self.adv_opt, self.adv.updates)] if self.adv is not None else [])
            timed_out = adam.timed_out_steps(refused, opts + ([(self.vp.opt, 1)] if self.vp is not None else []))
            skipped = self.opt.skipped_nonfinite
            for opt, n in opts:  # a timed-out step refused the Discriminator's updates too
                opt.settle(timed_out, n)
            if not (s or timed_out):
                return
            # status[0] by its bits: 0 a hand-off time-out (first: its workspaces need the reset below), 2 the
            # non-finite joint gradient norm (sticky), 1 the image-query step's loss guard (dl4ss_imgq_guard)
            if not s & 1 and s & ops.STATUS_NONFINITE_GRAD:
                # opt.settle has moved the step with that gradient to skipped_nonfinite; the steps enqueued behind
                # it, refused by the sticky bit (a later one's loss guard may have added bit 1), are skipped for
                # the same reason
                self.opt.skipped_nonfinite += timed_out
                self.vp.opt.settle(0)
                raise RuntimeError(f"non-finite gradient: {self.opt.skipped_nonfinite - skipped} update(s) refused")
            if not s & 1 and s & 2:
                raise RuntimeError(f"non-finite loss: {timed_out} update(s) refused")
            self.rnn_ws_all.zero_()  # a timed-out launch's half-written hand-offs must not reach the next
            if self.vp is not None:
                self.vp.reset_workspaces()
            where = "on this rank" if s else "on a data-parallel peer"
            raise RuntimeError(f"BiRNN hand-off timed out {where} (status {s}): {timed_out} update(s) refused")
