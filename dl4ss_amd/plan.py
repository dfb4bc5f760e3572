"""From a SepTrainer's arguments, before any buffer exists: check_args() every refusal, step_plan() the schedule."""
import os
import types

import torch

from . import _lib, ops
from .imagequery import ImageQueryNet
from .params import DiscNet, _ngate
from .voiceprint import SpeakerMemory, VoiceprintNet


def _same_device(net, other):
    return (other.device.type, other.device.index or 0) == (net.device.type, net.device.index or 0)


def check_optimizer(optimizer, schedule_decay, clip_norm, clipnorm):
    """The optimizer's arguments of a trainer (SepTrainer, ClassifierTrainer): returns clipnorm as a float or None."""
    if optimizer not in ("adam", "nadam"):
        raise ValueError(f"optimizer {optimizer!r}: expected 'adam' or 'nadam'")
    if not float(schedule_decay) >= 0.0:  # also NaN
        raise ValueError(f"schedule_decay must not be negative, got {schedule_decay}")
    if clipnorm is None:
        return None
    if clip_norm is not None:
        raise ValueError("clip_norm (torch.nn.utils.clip_grad_norm_'s rule) and clipnorm (Keras's rule) are given "
                         "together: choose one")
    return ops.check_clip_norm(clipnorm, "clipnorm")


def check_args(net, batch, k, n_samples, mode, precision, rnn_precision, loss_channels, process_group, adversary,
               clip_norm, adv_clip_norm, vnet, memory, memory_refresh, splitk_reduce="atomic", inet=None,
               optimizer="adam", schedule_decay=0.004, clipnorm=None):
    """Every combination of SepTrainer's arguments it is not built for, each refused with its reason: host checks
    only, run in front of the first device call.  Returns the clip thresholds as floats (or None); ``clipnorm``
    (Keras's rule) is checked here and stays the caller's."""
    if mode not in ("label", "pit", "crm"):
        raise ValueError(mode)
    check_optimizer(optimizer, schedule_decay, clip_norm, clipnorm)
    if splitk_reduce not in ("atomic", "fixed"):
        raise ValueError(f"splitk_reduce {splitk_reduce!r}: expected 'atomic' or 'fixed'")
    if splitk_reduce == "fixed" and precision != "fp32":
        raise ValueError(f"splitk_reduce='fixed' is the fp32 step's fixed-order split-K (precision {precision!r}: "
                         "the bf16 steps' split-K is already deterministic)")
    if inet is not None:  # everything the image-query step is not built for (the voiceprint step's list)
        if vnet is not None:
            raise ValueError("image_query: given together with voiceprint=, a step has one query encoder")
        if memory is None:
            raise ValueError("image_query: the encoder needs memory= (a voiceprint.SpeakerMemory)")
        if not isinstance(inet, ImageQueryNet):
            raise ValueError("image_query: expected an imagequery.ImageQueryNet")
        if not isinstance(memory, SpeakerMemory):
            raise ValueError("memory: expected a voiceprint.SpeakerMemory")
        if mode != "label":
            raise ValueError(f"image_query: mode {mode!r} is unsupported, the query by image belongs to its own "
                             "source (mode 'label')")
        if net.crm:
            raise ValueError("image_query: a cRM net (query width 2E) is unsupported")
        if net.adjust:
            raise ValueError("image_query: net.adjust is unsupported (ADDJUST adds to an embedding row, not to a "
                             "memory row); build the SepNet with adjust=False")
        if net.E != inet.E:
            raise ValueError(f"image_query: the encoder's vectors have {inet.E} elements, the net's queries {net.E}")
        if memory.E != inet.E:
            raise ValueError(f"memory: rows of {memory.E} elements, the encoder's vectors have {inet.E}")
        if precision != "fp32":
            raise ValueError(f"image_query: precision {precision!r} is unsupported, the image-query path is fp32")
        if loss_channels:
            raise ValueError("image_query: loss_channels is unsupported")
        if adversary is not None:
            raise ValueError("image_query: an adversary is unsupported")
        if process_group is not None:
            raise ValueError("image_query: no data-parallel image-query step (process_group; the encoder's "
                             "gradient and the memory are not all-reduced)")
        if clip_norm is not None:
            raise ValueError("image_query: clip_norm is unsupported (one global norm over the two flat gradients "
                             "needs a kernel change)")
        if memory_refresh not in ("reference", "reuse"):
            raise ValueError(f"memory_refresh {memory_refresh!r}: expected 'reference' or 'reuse'")
        if batch * k > 1024:
            raise ValueError(f"image_query: {batch * k} sources per step, the memory kernels take at most 1024")
        for what, other in (("image_query", inet), ("memory", memory)):
            if not _same_device(net, other):
                raise ValueError(f"{what}: lives on another device than the net")
    elif vnet is not None or memory is not None:  # everything the voiceprint step is not built for
        if vnet is None:
            raise ValueError("memory: a SpeakerMemory needs voiceprint= (the encoder whose vectors it accumulates)")
        if memory is None:
            raise ValueError("voiceprint: the encoder needs memory= (a voiceprint.SpeakerMemory)")
        if not isinstance(vnet, VoiceprintNet):
            raise ValueError("voiceprint: expected a voiceprint.VoiceprintNet")
        if not isinstance(memory, SpeakerMemory):
            raise ValueError("memory: expected a voiceprint.SpeakerMemory")
        if mode != "label":
            raise ValueError(f"voiceprint: mode {mode!r} is unsupported, the enrolled query belongs to its own "
                             "source (mode 'label')")
        if net.crm:
            raise ValueError("voiceprint: a cRM net (query width 2E) is unsupported")
        if net.adjust:
            raise ValueError("voiceprint: net.adjust is unsupported (ADDJUST adds to an embedding row, not to a "
                             "memory row); build the SepNet with adjust=False")
        if net.E != vnet.E:
            raise ValueError(f"voiceprint: the encoder's vectors have {vnet.E} elements, the net's queries {net.E}")
        if memory.E != vnet.E:
            raise ValueError(f"memory: rows of {memory.E} elements, the encoder's vectors have {vnet.E}")
        if net.F != vnet.F:
            raise ValueError(f"voiceprint: the encoder reads {vnet.F} bins, the step's magnitudes have {net.F}")
        if precision != "fp32":
            raise ValueError(f"voiceprint: precision {precision!r} is unsupported, the voiceprint path is fp32")
        if loss_channels:
            raise ValueError("voiceprint: loss_channels is unsupported")
        if adversary is not None:
            raise ValueError("voiceprint: an adversary is unsupported")
        if process_group is not None:
            raise ValueError("voiceprint: no data-parallel voiceprint step (process_group; the encoder's gradient "
                             "and the memory are not all-reduced)")
        if clip_norm is not None:
            raise ValueError("voiceprint: clip_norm is unsupported (one global norm over the two flat gradients "
                             "needs a kernel change)")
        if memory_refresh not in ("reference", "reuse"):
            raise ValueError(f"memory_refresh {memory_refresh!r}: expected 'reference' or 'reuse'")
        if batch * k > 1024:
            raise ValueError(f"voiceprint: {batch * k} sources per step, the memory kernels take at most 1024")
        for what, other in (("voiceprint", vnet), ("memory", memory)):
            if not _same_device(net, other):
                raise ValueError(f"{what}: lives on another device than the net")
    clip_norm = None if clip_norm is None else ops.check_clip_norm(clip_norm)
    adv_clip_norm = None if adv_clip_norm is None else ops.check_clip_norm(adv_clip_norm, "adv_clip_norm")
    if adv_clip_norm is not None and adversary is None:
        raise ValueError("adv_clip_norm needs an adversary")
    if (mode == "crm") != net.crm:
        raise ValueError("cRM mode needs a cRM net (query width 2E) and vice versa")
    check_hard_gates(net, resolve_rnn_precision(precision, rnn_precision))
    align = getattr(net, "attention", "dot") == "align"
    if adversary is not None:
        T = ops.n_frames(n_samples)
        if not isinstance(adversary, DiscNet):
            raise ValueError("adversary: expected an engine.DiscNet")
        if mode == "crm":
            raise ValueError("adversary: the adversarial term is built for the magnitude modes, not 'crm'")
        if loss_channels:
            raise ValueError("adversary: loss_channels is unsupported with an adversary")
        if align:
            raise ValueError("adversary: attention='align' is unsupported with an adversary")
        if process_group is not None:
            raise ValueError("adversary: no data-parallel adversarial step (the Discriminator's gradients are "
                             "not all-reduced)")
        if T < 15:
            raise ValueError(f"adversary: {T} frames, the Discriminator needs maps of at least 15 x 15")
        if (adversary.T, adversary.F) != (T, net.F):
            raise ValueError(f"adversary: a DiscNet for ({adversary.T}, {adversary.F}) maps, this trainer's "
                             f"are ({T}, {net.F})")
        if not _same_device(net, adversary):
            raise ValueError("adversary: the DiscNet lives on another device than the net")
    if align:
        if mode == "crm":
            raise ValueError("attention='align' supports the modes 'label' and 'pit', not 'crm'")
        if loss_channels:
            raise ValueError("attention='align' does not support loss_channels")
        # precision "bf16" / "bf16s" / "bf16s2" on the bf16 recurrence: the fast step, with the align kernel's
        # bf16-V / bf16-dPre forms (dl4ss_mask_attn_align_loss_ex) -- built and verified for the BiLSTM nets, the
        # cell of the Keras model that builds 'align'; a BiGRU align net stays on the fp32 step
        fast = precision in ("bf16s", "bf16s2") or (precision == "bf16" and (rnn_precision or precision) == "bf16")
        if fast and net.cell != "lstm":
            raise ValueError(f"attention='align' on the bf16 / bf16s fast paths is built for cell 'lstm', not "
                             f"{net.cell!r} (precision={precision!r}, rnn_precision={rnn_precision!r}); use "
                             "precision='fp32'")
        if net.E != 50:
            raise ValueError("attention='align' is built for embedding size 50")
    return clip_norm, adv_clip_norm


# settled A/B knobs (DESIGN.md section 11 keeps their last figures): the default of each is the only path now
RETIRED_KNOBS = ("DL4SS_DX_SPLIT", "DL4SS_DEFER_BIAS", "DL4SS_SIDE_LATE", "DL4SS_DW_SPLITS", "DL4SS_DW_CFG") + \
    _lib.RETIRED_ENV  # (the three the library itself read: _lib._load refuses them for every consumer)


def resolve_rnn_precision(precision, rnn_precision=None):
    """The recurrent matvec's precision a step resolves to (defaults to the GEMM precision; the split-operand steps
    run the bf16 recurrence): "fp32" the exact VALU kernels, "bf16" the packed MFMA ones."""
    if precision in ("bf16s", "bf16s2") and rnn_precision in (None, precision):
        return "bf16"
    return rnn_precision or precision


def check_hard_gates(net, rnn_precision):
    """Refuse a hard-gates net on anything but the fp32 recurrence (host check, before any device call; the
    refusal is ops.gate_flags', which the inference paths raise too).  Returns the recurrence's flag."""
    gates = getattr(net, "gates", "logistic")
    return ops.gate_flags(gates, net.cell, rnn_precision) if gates != "logistic" else 0


def step_plan(net, batch, n_samples, precision, rnn_precision=None, process_group=None):
    """Every schedule decision of a SepTrainer, derived once from its arguments, the recurrence's plan,
    the CU count and the environment knobs -- each knob is read and validated here and nowhere else.
    DESIGN.md section 11 has the table of knobs and the measurement behind every default.  The fields
    of the result become the trainer's attributes of the same names."""
    env = os.environ
    for name in RETIRED_KNOBS:
        if name in env:
            raise ValueError(f"{name} is retired, its default is the only path (DESIGN.md section 11): unset it")
    p = types.SimpleNamespace()
    B, T, F, H, L = batch, ops.n_frames(n_samples), net.F, net.H, net.L
    BT, FE, NGH = B * T, F * net.E, _ngate(net.cell) * H
    # precision "bf16": every GEMM on the LDS-DMA MFMA kernel over bf16 operands; "bf16s": the forward GEMMs over
    # split (hi + lo) operands, three terms; "bf16s2": two terms into the layers >= 1.  The recurrence (bf16 MFMA
    # matvec, fp32 state) and the whole backward are the bf16 step's in all three
    p.split = precision in ("bf16s", "bf16s2")
    p.split_x2 = precision == "bf16s2"
    # recurrent matvec precision (defaults to the GEMM precision): "fp32" exact VALU, "bf16" MFMA
    p.rnn_precision = resolve_rnn_precision(precision, rnn_precision)
    # the recurrence's gate form as a launch constant (ops.HARD_GATES: Keras 1's cell, fp32 recurrence only)
    p.rnn_flags = check_hard_gates(net, p.rnn_precision)
    if p.split and p.rnn_precision != "bf16":
        raise ValueError(f"precision '{precision}' runs the bf16 recurrence (rnn_precision bf16)")
    p.fast = precision in ("bf16", "bf16s", "bf16s2") and p.rnn_precision == "bf16"
    p.grouped = L <= 5  # <= 16 problems per grouped weight-gradient launch; deeper nets: a GEMM per gradient
    # one hand-off workspace per (layer, pass), zeroed once: a completed launch leaves it fit for the next
    # (T >= 4).  DL4SS_WS_FILL=1: a fill per step
    p._ws_fill = T < 4 or env.get("DL4SS_WS_FILL", "0") == "1"
    p.dh_split = int(env.get("DL4SS_DH_SPLIT", "3"))  # dH split-K
    # input projections fused into the packed recurrence: "1" every layer, "l0" the first only, "0" none
    xw = env.get("DL4SS_RNN_XW", "1")
    if xw not in ("0", "1", "l0"):
        raise ValueError(f"DL4SS_RNN_XW={xw}: expected 0, 1 or l0")
    p.xw = p.fast and xw != "0" and not p.split
    p.xw_kmax = 160 if xw == "l0" else 640
    # bf16s: the first layer's split-operand projection (K' = 3 pad8(F) = 408 <= 640) is fused too
    p.xw_split0 = p.split and xw != "0"
    # data parallel: "2" the gradient leaves in two buckets around the grouped launch, "3" three (the upper
    # layers >= dp_layer in the middle), "0" one flat all-reduce
    nb = env.get("DL4SS_DP_BUCKETS", "2")
    if nb not in ("0", "1", "2", "3"):
        raise ValueError(f"DL4SS_DP_BUCKETS={nb}: expected 0, 1 (alias of 2), 2 or 3")
    p.buckets = process_group is not None and p.fast and p.grouped and nb != "0"
    p.dp_layer = L // 2 if (p.buckets and nb == "3" and L >= 2) else None
    # grouped bf16 backward: every gradient has exactly one writer (beta 0), so no zeroing pass over the
    # flat gradient.  DL4SS_GRAD_ZERO=1 restores it
    p.zero_free = p.fast and p.grouped and env.get("DL4SS_GRAD_ZERO", "0") != "1"
    p._gbeta = 0.0 if p.zero_free else 1.0
    # Adam writes the bf16 weight copies itself.  DL4SS_ADAM_SHADOW=0: a conversion launch every step
    p._shadow_on = p.fast and env.get("DL4SS_ADAM_SHADOW", "1") != "0"
    cuda = net.device.type == "cuda"
    rnn = ops.birnn_plan(net.cell, B, H) if (p.fast and cuda) else None
    # dW_lin (+ the Linear's bias gradient as row sums) on a side stream beside the BPTT chain, one persistent
    # workgroup per CU the recurrence leaves free, when a cost model says it fits inside the chain.
    # DL4SS_SIDE_DWLIN: "0" off, "1" on, "grid,cfg,split[,one_per_cu]" a forced shape
    p.side = None
    side = env.get("DL4SS_SIDE_DWLIN", "")
    if p.fast and p.grouped and side != "0" and cuda:
        if side and side != "1":
            v = [int(x) for x in side.split(",")]
            p.side = (v[0], v[1], v[2], bool(v[3]) if len(v) > 3 else True)
        else:
            cus = torch.cuda.get_device_properties(net.device).multi_processor_count
            free = cus - (rnn["grid"] if rnn else 1 << 30)
            flops = 2.0 * FE * (2 * H) * BT
            if free >= 8 and (flops / (free * 2.75e12) < L * T * 1.75e-6 * 0.85 or side == "1"):
                p.side = (free, 2, 1, False)
    # the top layer's BPTT sums the dH GEMM's split-K slabs as it loads dOut (no combine launch): three slabs
    # and batch chunks of 4 only, the instance that measured no slower.  DL4SS_DH_SLABS=0: the combine launch
    p.dh_slabs = 1
    if p.fast and env.get("DL4SS_DH_SLABS", "1") != "0" and rnn is not None and rnn["BC"] == 4:
        nsl = _lib.query("dl4ss_gemm_bf16_gl_ws_bytes", BT, 2 * H, FE, max(1, p.dh_split), 1) // (BT * 2 * H * 4)
        p.dh_slabs = 3 if nsl == 3 else 1

    # split-K of the grouped weight-gradient launch (dW_lin, dW_ih, dW_hh): dW_ih goes unsplit when the group
    # fills >= 3 waves of the 512 workgroup slots without it (C2: 1793 workgroups; the BiGRU-2L nets: 999)
    def tiles(m, n):
        return ((m + 127) // 128) * ((n + 127) // 128)

    wg1 = 2 * tiles(FE, 2 * H) + sum(tiles(2 * NGH, F if l == 0 else 2 * H) for l in range(L)) + \
        4 * 2 * L * tiles(NGH, H)
    p.dw_splits = (2, 1 if wg1 >= 3 * 512 else 2, 4)
    return p
