"""The masked voiceprint encoder's contract with Keras 1's LSTM cell, in fp64: tests/voiceprint_ref.encoder_ref with
the hard-gates layer of tests/keras_cell_ref.py in place of nn.LSTM -- each utterance's valid prefix through the
stacked bidirectional layers from a zero state, the voiceprint = the sum of the top layer's frames / (len + eps), and
the gradients of sum(vec * dvec) by autograd through keras_cell_ref.HardLSTMLayer (the reference's own saturation
pattern: the tests choose inputs whose gates keep a margin to every kink and assert it)."""
import torch

import keras_cell_ref as K
from voiceprint_ref import EPS


def stack(x, P, L, prefix, margins=None, acts=None):
    """x (n, T, D) fp64 through L hard-gates layers with the parameters P {name: fp64 tensor}; ``margins``: a list
    that receives each layer's smallest | |z| - 2.5 | over the i, f, o gates; ``acts``: one that receives each
    layer's gate activations (n, T, 2, 4H)."""
    for l in range(L):
        p = lambda kind, r: P[f"{prefix}{kind}_l{l}{'_reverse' if r else ''}"]  # noqa: E731
        G = torch.stack([x @ p("weight_ih", r).T + p("bias_ih", r) for r in (0, 1)], 2)
        w_hh = torch.stack([p("weight_hh", 0), p("weight_hh", 1)])
        b_hh = torch.stack([p("bias_hh", 0), p("bias_hh", 1)])
        if margins is not None or acts is not None:
            fw = K.forward(G.detach(), w_hh.detach(), b_hh.detach())
            if margins is not None:
                margins.append(min((g.abs() - K.EDGE).abs().min().item() for g in K.gate_blocks(fw["z"])))
            if acts is not None:
                acts.append(fw["act"])
        x = K.HardLSTMLayer.apply(G, w_hh, b_hh, None)
    return x


def encoder_ref(xc, lens, sd, H, L, dvec, prefix="spk.layer."):
    """(vec (n, 2H) fp64, {name: grad}, the smallest kink margin over every utterance, layer and gate)."""
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in sd.items()}
    vec, margins = [], []
    for b in range(xc.shape[0]):
        Lb = int(lens[b])
        if Lb == 0:
            vec.append(torch.zeros(2 * H, dtype=torch.float64))
            continue
        o = stack(xc[b:b + 1, :Lb].double(), P, L, prefix, margins)
        vec.append(o[0].sum(0) / (Lb + EPS))
    vec = torch.stack(vec)
    (vec * dvec.double()).sum().backward()
    return vec.detach(), {k: p.grad.clone() for k, p in P.items()}, min(margins)
