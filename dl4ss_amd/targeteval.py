"""Target-speaker evaluation of the Keras trees on the HIP path: the test pass ``predict.eval_separation``
(``Cocktail/software/DL4SS_Keras/predict.py:46-336``, ``main_run.py:40-50``) and the validation loss
``predict.eval_loss`` (``predict.py:339-``) that ``nnet.py:149-172`` stops early on.

One target speaker is extracted from a mixture of ``spk_num`` speakers, optionally with background noise; the speaker
is either seen (a row of the speaker memory) or unseen (enrolled from clean speech, or from a picture); every mixture
is scored with ``BSS_EVAL.m`` -- BSS Eval 2.0's gain decomposition of the prediction on [noise; target]
(``bss.bss_eval_target``) -- and the run is reported as the plain means GSDR / GSIR / GSAR / GNSDR.

Reading and resampling wav files, MATLAB and ``.h5`` weights stay outside: ``evaluate`` takes the raw, cropped
sources on the device.  The metric is pinned to the published formulae (include/dl4ss_eval.h), parity with the
reference's MATLAB run unpinned.
"""
import numpy as np
import torch

from . import _lib, ops
from .bss import bss_eval_target
from .infer import EnrolledExtractor

METRICS = ("SDR", "SIR", "SAR", "NSDR")
PRECISIONS = ("fp32", "bf16", "bf16s")


def read_eval_list(path, unk_spk=False):
    """The Keras trees' evaluation lists (predict.py:81-93, 361-372), one mixture per line, fields separated by
    white space: seen speakers ``target.wav bg1.wav,bg2.wav spk``; unseen speakers (``unk_spk``) ``target.wav bg.wav
    spk supp1.wav,supp2.wav``.  Returns a list of dicts ``target``, ``bg`` (a list), ``spk`` and ``supp`` (a list;
    empty for seen speakers).  A line with fewer than two fields raises, as the reference does, and so does one
    that does not have exactly the format's fields (where the reference's tuple assignment fails)."""
    want = 4 if unk_spk else 3
    out = []
    with open(path) as f:
        for no, raw in enumerate(f, 1):
            line = raw.strip().split()
            if len(line) < 2:
                raise ValueError(f"{path}:{no}: wrong audio list record {raw.strip()!r}")
            if len(line) != want:
                raise ValueError(f"{path}:{no}: {len(line)} fields, the {'unseen' if unk_spk else 'seen'}-speaker "
                                 f"format has {want}")
            target, bg, spk = line[:3]
            out.append(dict(target=target, bg=[bg] if unk_spk else bg.strip().split(","), spk=spk,
                            supp=line[3].strip().split(",") if unk_spk else []))
    return out


def assemble(srcs, lengths=None, bgd=None, spk_num=2, out=None):
    """``dl4ss_te_assemble``: srcs (B, S, N) normalised sources -> (mix, noise, target (B, N) each, mix_len (B)
    int32), fp32 adds in the reference's order over the first ``spk_num`` slots (+ ``bgd`` (N))."""
    ops._f32c(srcs, "assemble")
    B, S, N = srcs.shape
    if bgd is not None:
        ops._f32c(bgd, "assemble(bgd)")
        if tuple(bgd.shape) != (N,):
            raise RuntimeError("assemble: bgd must be (N)")
    if lengths is not None and (lengths.dtype != torch.int32 or tuple(lengths.shape) != (B, S)
                                or not lengths.is_cuda or not lengths.is_contiguous()):
        raise RuntimeError("assemble: lengths must be a contiguous (B, S) int32 CUDA tensor")
    if out is None:
        out = tuple(torch.empty(B, N, device=srcs.device, dtype=torch.float32) for _ in range(3)) + \
            (torch.empty(B, device=srcs.device, dtype=torch.int32),)
    mix, noise, target, mix_len = out
    _lib.call("dl4ss_te_assemble", srcs=_lib.ptr(srcs), lengths=_lib.ptr(lengths), bgd=_lib.ptr(bgd), B=B, S=S, N=N,
              spk_num=int(spk_num), mix=_lib.ptr(mix), noise=_lib.ptr(noise), target=_lib.ptr(target),
              mix_len=_lib.ptr(mix_len), stream=_lib.stream_ptr())
    return mix, noise, target, mix_len


def prepare_background(clip, N):
    """The background clip as predict.py:153-155 prepares it: cropped to N, mean-removed, peak-normalised (in
    float64, as numpy does there), as a float32 numpy array (N).  A clip shorter than N or without any variation
    is refused."""
    x = np.asarray(clip.detach().cpu().numpy() if isinstance(clip, torch.Tensor) else clip, dtype=np.float64)
    if x.ndim != 1 or x.shape[0] < N:
        raise ValueError(f"bgd_noise: a 1-D clip of at least N = {N} samples, got shape {x.shape}")
    x = x[:N] - np.mean(x[:N])
    peak = np.max(np.abs(x))
    if not (np.isfinite(peak) and peak > 0):
        raise ValueError("bgd_noise: the clip is constant or not finite over its first N samples")
    return (x / peak).astype(np.float32)


class TargetEvaluator:
    """``predict.eval_separation`` / ``predict.eval_loss`` for batches of up to B mixtures of N samples.

    ``net``: the mask net (SepNet, 'dot' or 'align', E = 50); ``vnet``: a ``VoiceprintNet`` or ``ImageQueryNet``, as
    ``infer.EnrolledExtractor`` takes them (what it refuses is refused here); ``memory``: the ``SpeakerMemory`` of
    the seen speakers (None: unseen speakers only).  ``spk_num`` < 2 becomes 2 (predict.py:51-52).  ``bgd_noise``:
    the background clip, prepared once (prepare_background).  ``log_features``: the net reads log magnitudes
    (IS_LOG_SPECTRAL), the mask still multiplies the magnitudes.  ``precision``: the mask net's, as
    ``MaskNetForward``; with "bf16" the attention reads V rounded to bf16, as the bf16 training step's does (not
    with 'align': the evaluator feeds its kernel the fp32 V, where the bf16 training step feeds it bf16 V).

    ``evaluate`` and ``eval_loss`` enqueue launches only: nothing synchronises with the host.  ``check()`` does,
    and raises if a recurrence hand-off timed out; ``summary()`` reads the running sums."""

    def __init__(self, net, vnet, memory, B, N, spk_num=2, bgd_noise=None, log_features=False, precision="fp32"):
        if isinstance(B, bool) or not isinstance(B, int) or B < 1:
            raise ValueError(f"TargetEvaluator: B {B!r}, expected an int >= 1")
        if isinstance(N, bool) or not isinstance(N, int) or N < 256:
            raise ValueError(f"TargetEvaluator: N {N!r}, expected an int >= 256 (two frames)")
        if isinstance(spk_num, bool) or not isinstance(spk_num, int):
            raise ValueError(f"TargetEvaluator: spk_num {spk_num!r}, expected an int")
        if precision not in PRECISIONS:
            raise ValueError(f"TargetEvaluator: precision {precision!r}, expected one of {PRECISIONS}")
        if net.E != 50:
            raise ValueError(f"TargetEvaluator: the fused attention kernels are built for E = 50, the net has {net.E}")
        if memory is not None and memory.E != net.E:
            raise ValueError(f"TargetEvaluator: the memory holds rows of {memory.E}, the net takes queries of {net.E}")
        self.spk_num = max(2, spk_num)
        if self.spk_num > 16:
            raise ValueError("TargetEvaluator: spk_num <= 16")
        bgd = None if bgd_noise is None else prepare_background(bgd_noise, N)
        T = ops.n_frames(N)
        # (its refusals come before its first allocation; K = 1: one target per mixture)
        self.ext = EnrolledExtractor(net, vnet, B, T, 1, precision)
        self.net, self.vnet, self.memory = net, vnet, memory
        self.B, self.N, self.T, self.F = B, N, T, net.F
        self.L = ops.HOP * (T - 1)  # the iSTFT's length
        self.log_features, self.precision = bool(log_features), precision
        self.align = self.ext.align
        dev = net.device
        f32 = dict(device=dev, dtype=torch.float32)
        i32 = dict(device=dev, dtype=torch.int32)
        self.bgd = None if bgd is None else torch.as_tensor(bgd).to(dev)
        self._slots = {}  # S -> (raw, lengths, gains, srcs, scratch mix, stats)
        self.mix, self.noise, self.target = (torch.empty(B, N, **f32) for _ in range(3))
        self.mix_len = torch.empty(B, **i32)
        self.n_eff = torch.empty(B, **i32)
        self.Xc = torch.empty(B, T, self.F, 2, **f32)
        self._mag = torch.empty(2 * B, T, self.F, **f32)  # [mixtures | targets]
        self.mag_mix, self.mag_tgt = self._mag[:B], self._mag[B:]
        self.feat = torch.empty(B, T, self.F, **f32) if self.log_features else self.mag_mix
        self.V = self.ext.V
        self.Vb = torch.empty(B * T, self.F * net.E, device=dev, dtype=torch.bfloat16) \
            if (precision == "bf16" and not self.align) else None
        self.ids = torch.zeros(B, 1, **i32)
        self.q = torch.zeros(B, 1, net.E, **f32)
        self.nblk = _lib.query("dl4ss_attn_align_nblk", T * self.F) if self.align else \
            _lib.query("dl4ss_attn_nblk", T, self.F)
        self.part_loss = torch.empty(B, self.nblk, 2, **f32)
        self.pred = torch.empty(B, T, self.F, **f32)  # mask . |X|
        self.pred_wav = torch.empty(B, self.L, **f32)
        self.loss = torch.zeros(3, **f32)
        self._sum = torch.zeros(2 * len(METRICS), device=dev, dtype=torch.float64)
        self.count = 0

    # ------------------------------------------------------------------ the shared pipeline
    def _buffers(self, S):
        b = self._slots.get(S)
        if b is None:
            dev, B, N = self.net.device, self.B, self.N
            f32 = dict(device=dev, dtype=torch.float32)
            b = self._slots[S] = dict(raw=torch.zeros(B, S, N, **f32),
                                      lengths=torch.full((B, S), N, device=dev, dtype=torch.int32),
                                      gains=torch.ones(B, S, **f32), srcs=torch.empty(B, S, N, **f32),
                                      mix=torch.empty(B, N, **f32), stats=torch.empty(32 * B * S, **f32))
        return b

    def _check_batch(self, raw, lengths, ids, enrol, enrol_lengths, spk_num):
        if raw.dim() != 3 or raw.shape[2] != self.N or raw.dtype != torch.float32 or not raw.is_cuda:
            raise ValueError(f"raw {tuple(raw.shape)}: expected float32 (n, S, {self.N}) on the device")
        n, S = raw.shape[:2]
        if not 1 <= n <= self.B:
            raise ValueError(f"raw holds {n} mixtures, the evaluator was built for 1..{self.B}")
        if not spk_num <= S <= 16:
            raise ValueError(f"raw has {S} source slots, expected {spk_num}..16")
        if lengths is not None and (tuple(lengths.shape) != (n, S) or lengths.dtype != torch.int32):
            raise ValueError(f"lengths: expected int32 {(n, S)}")
        if (ids is None) == (enrol is None):
            raise ValueError("give ids= (seen speakers: rows of the memory) or enrol= (unseen speakers), not both")
        if ids is not None:
            if self.memory is None:
                raise ValueError("ids= needs the evaluator built with a SpeakerMemory")
            if ids.numel() != n or ids.dtype != torch.int32:
                raise ValueError(f"ids: expected int32 ({n})")
        elif enrol.shape[0] != n:
            raise ValueError(f"enrol holds {enrol.shape[0]} entries for {n} mixtures")
        if enrol_lengths is not None and (enrol is None or tuple(enrol_lengths.shape) != (n,)
                                          or enrol_lengths.dtype != torch.int32):
            raise ValueError(f"enrol_lengths: int32 ({n}), with enrol= only")
        return n, S

    def _query(self, n, ids, enrol, enrol_lengths):
        if ids is not None:  # the all-masked clean input of predict.py:231-233 adds nothing to the memory row
            self.ids[:n, 0].copy_(ids.view(-1))
            self.q.copy_(self.ext.queries_of(self.memory, self.ids))
            return
        for b in range(n):  # batch size 1, as the reference forces it for unseen speakers (predict.py:48-50)
            le = None if enrol_lengths is None else enrol_lengths[b:b + 1]
            kw = {} if self.ext.by_image else dict(lengths=le, check=False)
            self.q[b].copy_(self.ext.enrol(enrol[b:b + 1], **kw))

    def _forward(self, raw, lengths, ids, enrol, enrol_lengths, spk_num, bgd):
        """mixing -> assembly -> STFTs -> query -> mask net -> one COST pass (K = 1); returns n."""
        n, S = self._check_batch(raw, lengths, ids, enrol, enrol_lengths, spk_num)
        B, T, F, net = self.B, self.T, self.F, self.net
        bf = self._buffers(S)
        bf["raw"][:n].copy_(raw)
        if lengths is None:
            bf["lengths"][:n].fill_(self.N)
        else:
            bf["lengths"][:n].copy_(lengths)
        ops.mix_sources(bf["raw"], bf["gains"], out_src=bf["srcs"], out_mix=bf["mix"], stats_ws=bf["stats"],
                        lengths=bf["lengths"])
        assemble(bf["srcs"], bf["lengths"], bgd, spk_num, out=(self.mix, self.noise, self.target, self.mix_len))
        ops.stft(self.mix, complex_out=True, mag_out=True, out_c=self.Xc, out_mag=self.mag_mix)
        ops.stft(self.target, complex_out=False, mag_out=True, out_mag=self.mag_tgt)
        if self.log_features:
            ops.stft(self.mix, complex_out=False, mag_out=True, log=True, out_mag=self.feat)
        self._query(n, ids, enrol, enrol_lengths)
        self.ext.mask_net(self.feat, self.V)
        ptr, TF = _lib.ptr, T * F
        kw = dict(pass_=0, B=B, K=1, T=T, F=F, E=net.E, q=ptr(self.q), X=ptr(self.mag_mix), x_bstride=TF,
                  Y=ptr(self.mag_tgt), y_bstride=TF, y_kstride=TF, perm=None, s1=1.0 / (n * TF), s2=0.0, dPre=None,
                  part_loss=ptr(self.part_loss), mask_out=None, pred_out=ptr(self.pred), stream=_lib.stream_ptr())
        if self.align:
            _lib.call("dl4ss_mask_attn_align_loss", V=ptr(self.V), W1=ptr(net.view("att.Linear_1.weight")),
                      W2=ptr(net.view("att.Linear_2.weight")), w3=ptr(net.view("att.Linear_3.weight")), part=None,
                      part_floats=0, **kw)
        elif self.Vb is not None:
            _lib.call("dl4ss_f32_to_bf16", _lib.ptr(self.V), _lib.ptr(self.Vb), self.V.numel(), _lib.stream_ptr())
            _lib.call("dl4ss_mask_attn_loss_bf16v", crm=0, V_bf16=ptr(self.Vb), dPre_bf16=None, dpre_bf16_ld=0,
                      part_dq=None, **kw)
        else:
            _lib.call("dl4ss_mask_attn_loss_ex", crm=0, V=ptr(self.V), dPre_bf16=None, dpre_bf16_ld=0, part_dq=None,
                      **kw)
        # the mean over the n mixtures' T F bins (the partials of the rows behind n are not read)
        _lib.call("dl4ss_loss_finalize", part_loss=ptr(self.part_loss), B=n, K=1, nblk=self.nblk, perm=None,
                  s1=1.0 / (n * TF), s2=0.0, loss_out=ptr(self.loss), part_dq=None, qw=net.E, dq=None,
                  stream=_lib.stream_ptr())
        return n

    # ------------------------------------------------------------------ the two passes
    def evaluate(self, raw, lengths, ids=None, enrol=None, enrol_lengths=None):
        """raw (n, S, N) float32 on the device, n <= B: slot 0 the target, then the interferers, each cropped to N
        and otherwise as read (the normalisation is done here); lengths (n, S) int32 their lengths (None: N).
        ``ids`` (n) int32: seen speakers, the rows of the memory; or ``enrol``: unseen speakers, clean features
        (n, T', F) (``enrol_lengths`` (n) int32 frames: a plain prefix) or images (n, h, w).  Returns a dict of (n)
        float64 device tensors: ``SDR, SIR, SAR, NSDR`` of the prediction and ``SDR_0, SIR_0, SAR_0, NSDR_0`` of
        the mixture as its own estimate (the reference's epoch-0 figures), and adds them to the running sums."""
        n = self._forward(raw, lengths, ids, enrol, enrol_lengths, self.spk_num, self.bgd)
        _lib.call("dl4ss_istft_apply", X_mix_c64=_lib.ptr(self.Xc), aux=_lib.ptr(self.pred), n_sig=self.B,
                  k_per_mix=1, T=self.T, mode=0, conj=0, y=_lib.ptr(self.pred_wav), stream=_lib.stream_ptr())
        L = self.L
        torch.clamp(self.mix_len, max=L, out=self.n_eff)  # min(len(target), len(pred), mix_len), predict.py:248
        tgt, noi, mix = (x[:n, :L].contiguous() for x in (self.target, self.noise, self.mix))
        ne = self.n_eff[:n].contiguous()
        res = bss_eval_target(tgt, noi, self.pred_wav[:n].contiguous(), mix, ne)
        res0 = bss_eval_target(tgt, noi, mix, mix, ne)
        out = {k: res[k] for k in METRICS}
        out.update({k + "_0": res0[k] for k in METRICS})
        self._sum += torch.stack([out[k].sum() for k in METRICS] + [out[k + "_0"].sum() for k in METRICS])
        self.count += n
        return out

    def eval_loss(self, raw, lengths, ids=None, enrol=None, enrol_lengths=None):
        """The Keras validation loss of one batch (predict.py:339-, ``model.evaluate`` of the 'mse' model): the
        target plus the FIRST interferer only, no background; the mean over n T F of (mask |X_mix| - |X_target|)^2,
        from the COST pass's own partials.  A 1-element device tensor (a copy); the caller sums over batches."""
        self._forward(raw, lengths, ids, enrol, enrol_lengths, 2, None)
        return self.loss[:1].clone()

    def summary(self):
        """The plain means over everything evaluated since reset() (np.mean of predict.py:288-291): ``GSDR, GSIR,
        GSAR, GNSDR``, the same four of the unprocessed mixtures (``*_0``) and ``count``.  Reads the device."""
        s = (self._sum / max(self.count, 1)).tolist()
        nan = float("nan")
        out = {"G" + k: (s[i] if self.count else nan) for i, k in enumerate(METRICS)}
        out.update({"G" + k + "_0": (s[4 + i] if self.count else nan) for i, k in enumerate(METRICS)})
        out["count"] = self.count
        return out

    def reset(self):
        self._sum.zero_()
        self.count = 0

    def check(self):
        """Synchronise and raise if a recurrence hand-off of the mask net or of an enrolment encoder timed out."""
        self.ext.mask_net.stack.check()
        for enc in self.ext._enc.values():
            if hasattr(enc, "check"):
                enc.check()
