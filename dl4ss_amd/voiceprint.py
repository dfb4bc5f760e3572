"""Voiceprint encoder and life-long speaker memory on the HIP path.

The model this code base descends from takes its speaker query from clean speech of the target
(``Cocktail/software/DL4SS_Keras/nnet.py:64-92``): a small BiLSTM over the target's features with silent
frames masked (``Masking`` / ``MaskingGt``, ``:44-47``), the mean over the unmasked frames (``MeanPool``,
``extend_layers.py:105-125``), an L2 normalisation and a speaker memory the unit vectors accumulate in
(``SpkLifeLongMemory`` / ``SelectSpkMemory`` / ``update_memory``, ``extend_layers.py:132-228``).

Contract of the masked encoder (``pack_padded_sequence`` generalised to any frame mask): utterance b's valid
frames are compacted to a prefix of length len[b]; every layer's forward direction runs over 0 .. len-1 and
its reverse direction over len-1 .. 0, both from a zero state; the voiceprint is the sum of the top layer's
len frames / (len + eps).  The full-length recurrence kernels give exactly that when the reverse direction's
rows are right-aligned (``dl4ss_vp_shift``): DESIGN.md section 5, "Voiceprint memory".

The cell is this project's LSTM (torch gate order); ``VoiceprintNet(gates="hard")`` makes its i / f / o gates
Keras 1's ``hard_sigmoid`` (the ``LSTM`` default ``inner_activation`` those lines run with;
``DL4SS_RNN_HARD_GATES``), the default ``"logistic"`` torch's.  fp32, single GPU, eager launches.
"""
import math

import torch

from . import _lib, ops
from .adam import GuardedAdam
from .params import FlatParams, check_gates, check_tensor

EPS = 2.220446049250313e-16  # np.spacing(1)


class VoiceprintNet(FlatParams):
    """Parameters of the voiceprint BiLSTM, flat fp32 under ``spk.layer.{kind}_l{l}[_reverse]``; ``grad`` is the
    flat gradient of the same layout (VoiceprintEncoder.backward writes it).  ``gates``: "logistic" or "hard"
    (Keras 1's LSTM cell), independent of the mask net's; layout and initialisation are the same."""

    layer_prefix = "spk.layer."

    def __init__(self, input_fre=129, emb=50, hidden=None, num_layers=2, cell="lstm", device="cuda", seed=1,
                 gates="logistic"):
        hidden = emb // 2 if hidden is None else hidden
        if cell != "lstm":
            raise ValueError(f"VoiceprintNet: cell {cell!r}, the voiceprint encoder is a BiLSTM")
        self.gates = check_gates(gates, cell, "VoiceprintNet")
        if 2 * hidden != emb:
            raise ValueError(f"VoiceprintNet: 2 * hidden ({hidden}) must equal emb ({emb})")
        if num_layers < 1:
            raise ValueError("VoiceprintNet: num_layers >= 1")
        self.cell, self.F, self.E, self.H, self.L = cell, input_fre, emb, hidden, num_layers
        self._allocate(self._layer_specs(num_layers, input_fre, hidden, 4 * hidden), device)
        self.grad = torch.zeros_like(self.flat)
        self.reset_parameters(seed)

    def named_parameters(self):
        for name, _ in self.specs:
            yield name, self.view(name)

    def grad_view(self, name):
        return self.view(name, self.grad)

    def reset_parameters(self, seed=1):
        """torch's nn.LSTM default: U(+-1 / sqrt(H)) for every tensor."""
        g = torch.Generator().manual_seed(seed)
        k = 1.0 / math.sqrt(self.H)
        for name, shape in self.specs:
            self.view(name).copy_(torch.empty(shape).uniform_(-k, k, generator=g))


class SpeakerMemory:
    """The life-long speaker memory: ``mem`` (num_speakers, emb) fp32, zero at start, one row per speaker
    (extend_layers.py:132-147; trainable=False: it gets no gradient, update_memory rewrites its rows)."""

    def __init__(self, num_speakers, emb=50, device="cuda"):
        if num_speakers < 1 or not 1 <= emb <= 128:
            raise ValueError("SpeakerMemory: num_speakers >= 1 and 1 <= emb <= 128")
        self.M, self.E = int(num_speakers), int(emb)
        self.device = torch.device(device)
        self.mem = torch.zeros(self.M, self.E, device=self.device, dtype=torch.float32)

    def reset(self):
        self.mem.zero_()

    def state_dict(self):
        return {"mem": self.mem.detach().clone()}

    def load_state_dict(self, sd):
        m = sd["mem"]
        if tuple(m.shape) != (self.M, self.E):
            raise ValueError(f"SpeakerMemory: mem has shape {tuple(m.shape)}, expected {(self.M, self.E)}")
        self.mem.copy_(m.to(torch.float32))


class VoiceprintEncoder:
    """Buffers and launches of the masked encoder for n utterances of T frames.

    Per layer: the input projection (``ops.gemm``, unsplit), a row shift that right-aligns the reverse
    direction's columns of G, the full-length recurrence (``ops.birnn_fwd``), and a shift back that assembles the
    next layer's compact input; then the masked mean.  ``backward`` runs the same moves in reverse around
    ``ops.birnn_bwd``; every GEMM is unsplit and the bias gradient is ``ops.vp_colsum`` (two fixed-order stages;
    ``ops.colsum`` adds its row blocks atomically), so every sum has a fixed order for any n * T and a repeated
    call gives the same bits.  ``status``: a caller's recurrence status word (2 ints) to share; default: its own.
    ``wgrad_split`` (an int or "auto", default 1: unsplit): the six weight-gradient GEMMs of ``backward`` (per
    layer dW_ih and both directions' dW_hh, K = n * T) split over K with the fixed-order reduce
    (``ops.gemm(reduce="fixed")``) out of one workspace allocated here: still the same bits on every call, not
    the unsplit GEMMs' bits.  The forward, the dX GEMM and the bias gradients are the same either way."""

    def __init__(self, vnet, n, T, status=None, wgrad_split=1):
        if not isinstance(vnet, VoiceprintNet):
            raise ValueError("VoiceprintEncoder: expected a VoiceprintNet")
        if n < 1 or not 1 <= T <= 2048:
            raise ValueError("VoiceprintEncoder: n >= 1 and 1 <= T <= 2048")
        if wgrad_split != "auto" and (isinstance(wgrad_split, bool) or not isinstance(wgrad_split, int)
                                      or wgrad_split < 1):
            raise ValueError(f"VoiceprintEncoder: wgrad_split {wgrad_split!r}, expected an int >= 1 or 'auto'")
        self.net, self.n, self.T, self.wgrad_split = vnet, int(n), int(T), wgrad_split
        self.rnn_flags = ops.gate_flags(getattr(vnet, "gates", "logistic"))  # the fp32 recurrence: either form
        H, L, F, dev = vnet.H, vnet.L, vnet.F, vnet.device
        f32 = dict(device=dev, dtype=torch.float32)
        i32 = dict(device=dev, dtype=torch.int32)
        self.xc = torch.empty(n, T, F, **f32)
        self.len = torch.zeros(n, **i32)
        self.idx = torch.empty(n, T, **i32)
        self.Gc = torch.empty(n, T, 8 * H, **f32)  # compact frame: x W_ih^T + b, then dG moved back
        self.G = torch.empty(n, T, 8 * H, **f32)  # the recurrence's frame (reverse columns right-aligned), then dG
        self.out = [torch.empty(n, T, 2 * H, **f32) for _ in range(L)]
        self.hprev = [torch.empty(n, T, 2 * H, **f32) for _ in range(L)]
        self.act = [torch.empty(n, T, 2, 4 * H, **f32) for _ in range(L)]
        self.cs = [torch.empty(n, T, 2, H, **f32) for _ in range(L)]
        self.xin = [None] + [torch.empty(n, T, 2 * H, **f32) for _ in range(L - 1)]  # compact inputs of layers >= 1
        self.dH = torch.empty(n, T, 2 * H, **f32)  # dOut of the layer at hand (the recurrence's frame)
        self.dX = torch.empty(n, T, 2 * H, **f32)  # compact frame
        self.vec = torch.empty(n, 2 * H, **f32)
        self.cs_part = ops.vp_colsum_part(n * T, 8 * H, dev)
        ws = _lib.query("dl4ss_birnn_workspace_bytes", ops.CELLS["lstm"], n, H)
        if ws < 0:
            raise RuntimeError(f"BiRNN shape unsupported (B={n}, H={H})")
        self.ws_bytes = ws
        self.rnn_ws = torch.zeros((ws + 7) // 8, device=dev, dtype=torch.int64)
        self.status = torch.zeros(2, **i32) if status is None else status
        # the weight gradients' shapes (M, N, K): dW_hh per direction, dW_ih of layer 0 and of the layers above
        shapes = [(4 * H, H, n * T), (8 * H, F, n * T)] + ([(8 * H, 2 * H, n * T)] if L > 1 else [])
        self.wgrad_ws = None
        if wgrad_split != 1:
            nb = max(ops.gemm_fixed_ws_bytes(*s, wgrad_split) for s in shapes)
            self.wgrad_ws = torch.empty(max(nb, 4) // 4, **f32)
        self._wg = {} if wgrad_split == 1 else dict(splitk=wgrad_split, reduce="fixed", ws=self.wgrad_ws)

    def forward(self, feats, rule="nonzero", thr=None, lengths=None):
        """feats (n, T, F) -> vec (n, E) (a buffer the next call reuses).  ``lengths`` (n) int32: a plain prefix
        per utterance instead of the frame rule."""
        net, n, T, H = self.net, self.n, self.T, self.net.H
        if tuple(feats.shape) != (n, T, net.F):
            raise RuntimeError(f"VoiceprintEncoder: feats {tuple(feats.shape)}, expected {(n, T, net.F)}")
        ops.vp_compact(feats, rule, thr, lengths, xc=self.xc, len_out=self.len, idx=self.idx)
        x = self.xc.view(n * T, -1)
        for l in range(net.L):
            ops.gemm(x, net.cat_view("weight_ih", l), transB=True, bias=net.cat_view("bias_ih", l),
                     out=self.Gc.view(n * T, 8 * H))
            ops.vp_shift(self.Gc, self.G, self.len, 4 * H, 8 * H, +1, other=2)
            ops.birnn_fwd("lstm", n, T, H, G=self.G, w_hh=net.cat_view("weight_hh", l), b_hh=net.cat_view("bias_hh", l),
                          out=self.out[l], hprev=self.hprev[l], act=self.act[l], cs=self.cs[l], ws=self.rnn_ws,
                          ws_bytes=self.ws_bytes, status=self.status, flags=self.rnn_flags)
            if l + 1 < net.L:  # the reverse half back to the compact frame, both halves zero behind len
                ops.vp_shift(self.out[l], self.xin[l + 1], self.len, H, 2 * H, -1, other=1)
                x = self.xin[l + 1].view(n * T, 2 * H)
        return ops.vp_mean_fwd(self.out[-1], self.len, self.vec)

    def backward(self, dvec):
        """dvec (n, E) -> net.grad, every element written (of the forward this follows)."""
        net, n, T, H = self.net, self.n, self.T, self.net.H
        nT, NGH = n * T, 4 * H
        g = net.grad
        ops.vp_mean_bwd(dvec, self.len, self.dH)
        G2, Gc2 = self.G.view(nT, 2 * NGH), self.Gc.view(nT, 2 * NGH)
        for l in range(net.L - 1, -1, -1):
            ops.birnn_bwd("lstm", n, T, H, dOut=self.dH, w_hh=net.cat_view("weight_hh", l), act=self.act[l],
                          cs=self.cs[l], hprev=self.hprev[l], dG=self.G, ws=self.rnn_ws, ws_bytes=self.ws_bytes,
                          status=self.status, flags=self.rnn_flags)
            # dG is exactly zero on the padded rows: the bias and W_hh gradients are taken in the recurrence's frame
            db = net.cat_view("bias_ih", l, g)
            ops.vp_colsum(G2, db, self.cs_part)
            net.cat_view("bias_hh", l, g).copy_(db)  # LSTM: dGh == dG
            whh_g = net.cat_view("weight_hh", l, g)
            hp = self.hprev[l].view(nT, 2 * H)
            for d in range(2):
                ops.gemm(G2[:, d * NGH:(d + 1) * NGH], hp[:, d * H:(d + 1) * H], transA=True,
                         out=whh_g[d * NGH:(d + 1) * NGH], **self._wg)
            # the reverse columns back to the compact frame, where the layer's input lives
            ops.vp_shift(self.G, self.Gc, self.len, NGH, 2 * NGH, -1, other=2)
            xl = self.xc.view(nT, -1) if l == 0 else self.xin[l].view(nT, 2 * H)
            ops.gemm(Gc2, xl, transA=True, out=net.cat_view("weight_ih", l, g), **self._wg)
            if l > 0:
                ops.gemm(Gc2, net.cat_view("weight_ih", l), out=self.dX.view(nT, 2 * H))
                ops.vp_shift(self.dX, self.dH, self.len, H, 2 * H, +1, other=2)
        return g

    def check(self):
        """Raise if a recurrence hand-off timed out since the last check; the status word and the hand-off
        workspace are reset (as ClassifierTrainer.check does for its own)."""
        torch.cuda.synchronize()
        s = int(self.status[0].item())
        if s:
            self.status.zero_()
            self.rnn_ws.zero_()
            raise RuntimeError(f"BiRNN hand-off timed out (status {s})")


class MemoryQueryStep:
    """What the query steps of a trainer share (the voiceprint step below, imagequery.ImageQueryStep): the speaker
    memory forward / backward around an encoder, the encoder's guarded Adam and the memory refresh.  A subclass
    builds ``enc`` (``forward(x) -> vec (n, E)``, ``backward(dvec) -> net.grad``, ``vec`` the forward's output)
    and says what it reads (``encoder_input``).  ``spk``, ``q``, ``dq``, ``status``, ``loss``: the trainer's
    buffers (the trainer itself is not referenced: _ws_slot)."""

    def __init__(self, net, memory, refresh, enc, spk, q, dq, status, loss, lr, betas, eps, opt_kw=None):
        n = spk.numel()
        f32 = dict(device=net.device, dtype=torch.float32)
        self.net, self.memory, self.refresh, self.enc, self.status = net, memory, refresh, enc, status
        self.spk, self.q, self.dq = spk.view(-1), q, dq.view(n, -1)
        self.u, self.dv, self.q2 = (torch.empty(n, net.E, **f32) for _ in range(3))  # q2: the refreshed rows
        # opt_kw: the trainer's optimizer= / schedule_decay= / clipnorm= (with parts=: the joint norm's buffer)
        self.opt = GuardedAdam(net.flat, status, loss, lr, betas, eps, **(opt_kw or {}))

    def encoder_input(self):
        raise NotImplementedError

    def queries(self, q):
        """q (B, K, E) = the memory rows of the step's speakers with this batch's unit vectors accumulated: the
        encoder over its input, then the memory forward."""
        ops.spk_memory_fwd(self.enc.forward(self.encoder_input()), self.spk, self.memory.mem, u=self.u,
                           q=q.view(self.u.shape))

    def backward(self):
        """dq -> the vectors' gradient through the memory, then the encoder's backward into net.grad (all written)."""
        ops.spk_memory_bwd(self.dq, self.enc.vec, self.u, self.spk, self.memory.mem, dv=self.dv)
        self.enc.backward(self.dv)

    def optimizer_step(self, step):
        """The encoder's guarded Adam at the mask net's count ``step`` (refused with the net's), then the memory
        refresh, skipped on device with a refused update: "reference" re-encodes first (nnet.py:131-135)."""
        self.opt.step(self.net.grad, step=step, summed=self.opt.joint)
        q = self.q
        if self.refresh == "reference":
            q = self.q2
            self.queries(q)
        ops.spk_memory_store(q.view(self.u.shape), self.spk, self.memory.mem, status=self.status)

    def reset_workspaces(self):
        """After a timed-out hand-off: nothing to reset unless the encoder has recurrences."""

    # ---- training state (checkpoint.save_training_state; the trainer checks that it is settled).  Both
    # subclasses hold nothing beyond this: their buffers are rewritten by every step
    def state_dict(self):
        """The encoder net's flat buffer with its layout, its optimizer (stepped at the mask net's count: its own
        step_count stays what it was) and the speaker memory's rows."""
        return {"net": self.net.flat_state(), "opt": self.opt.state_dict(),
                "memory": {"mem": self.memory.mem.detach().to("cpu", copy=True)}}

    def check_state_dict(self, sd, where="query"):
        if not isinstance(sd, dict):
            raise ValueError(f"{where}: no query-encoder section in the file")
        self.net.check_flat_state(sd.get("net"), f"{where}.net")
        self.opt.check_state_dict(sd.get("opt"), f"{where}.optimizer")
        mem = sd["memory"].get("mem") if isinstance(sd.get("memory"), dict) else None
        check_tensor(mem, self.memory.mem, f"{where}.memory.mem")

    def load_state_dict(self, sd, checked=False):
        if not checked:
            self.check_state_dict(sd)
        self.net.load_flat_state(sd["net"])
        self.opt.load_state_dict(sd["opt"], checked=True)
        self.memory.mem.copy_(sd["memory"]["mem"])


class VoiceprintStep(MemoryQueryStep):
    """The voiceprint queries of a training step (SepTrainer(voiceprint=, memory=)): the encoder over the step's clean
    magnitudes ``mag_src`` (B, K, T, F), the memory, the encoder's guarded Adam and the memory refresh.

    The masked encoder reads the clean magnitudes the step's STFT wrote (silent frames, e.g. the zero tail of
    a short source, are masked: rule 'nonzero').  (The STFT transforms frames in
    pairs: a silent frame that shares its transform with a voiced one -- the first silent frame behind an odd
    number of voiced ones -- carries that neighbour's rounding residue, ~1e-8 of it, and counts as valid.)"""

    def __init__(self, vnet, memory, refresh, mag_src, spk, q, dq, status, loss, lr, betas, eps, wgrad_split=1,
                 opt_kw=None):
        B, K, T, F = mag_src.shape
        self.maps = mag_src.view(B * K, T, F)
        # its recurrences share the step's status word
        enc = VoiceprintEncoder(vnet, B * K, T, status=status, wgrad_split=wgrad_split)
        super().__init__(vnet, memory, refresh, enc, spk, q, dq, status, loss, lr, betas, eps, opt_kw)

    def encoder_input(self):
        return self.maps

    def reset_workspaces(self):
        self.enc.rnn_ws.zero_()


def unit(vec):
    """u = v / |w(v)| of voiceprints (n, E): the memory's vector normalisation alone (what enrolment returns)."""
    n, E = vec.shape
    ids = torch.full((n,), -1, device=vec.device, dtype=torch.int32)
    mem = torch.zeros(1, E, device=vec.device, dtype=torch.float32)
    return ops.spk_memory_fwd(vec, ids, mem)[1]
