"""Flat fp32 parameter buffers with named views under the reference's ``state_dict`` key names, and their gradients."""
import ctypes
import math

import torch

from . import _lib


def _ngate(cell):
    return 4 if cell == "lstm" else 3


def check_gates(gates, cell, who):
    """A net's ``gates`` setting: "logistic" (torch's cell) or "hard" (Keras 1's LSTM cell, whose i / f / o gates are
    hard_sigmoid: DL4SS_RNN_HARD_GATES), the latter for cell "lstm" only.  Returns it."""
    if gates not in ("logistic", "hard"):
        raise ValueError(f"{who}: gates {gates!r}, expected 'logistic' or 'hard'")
    if gates == "hard" and cell != "lstm":
        raise ValueError(f"{who}: gates='hard' is Keras 1's LSTM cell and needs cell='lstm', got cell {cell!r} "
                         "(Keras's GRU is a different cell from this one and is not built)")
    return gates


class FlatParams:
    """Parameters in one flat fp32 buffer with named views (16-B aligned) under the reference's
    ``state_dict`` key names; ``layer_prefix`` + ``{kind}_l{l}[_reverse]`` names the recurrent layers'."""

    layer_prefix = "layer."

    def _layer_specs(self, num_layers, input_fre, hidden, NGH):
        specs = []
        for l in range(num_layers):
            D = input_fre if l == 0 else 2 * hidden
            for kind, shape in (("weight_ih", (NGH, D)), ("weight_hh", (NGH, hidden)), ("bias_ih", (NGH,)),
                                ("bias_hh", (NGH,))):
                specs.append((f"{self.layer_prefix}{kind}_l{l}", shape))
                specs.append((f"{self.layer_prefix}{kind}_l{l}_reverse", shape))
        return specs

    def _allocate(self, specs, device):
        self.specs = specs
        self.offsets = {}
        off = 0
        for name, shape in specs:
            self.offsets[name] = (off, shape)
            off += (math.prod(shape) + 3) // 4 * 4  # 16-B aligned views
        self.numel = off
        self.device = torch.device(device)
        self.flat = torch.zeros(off, device=self.device, dtype=torch.float32)

    def view(self, name, buf=None):
        """The parameter ``name``, or its counterpart in ``buf`` (a flat buffer of the same layout:
        the gradient, an Adam moment)."""
        off, shape = self.offsets[name]
        return (self.flat if buf is None else buf)[off:off + math.prod(shape)].view(shape)

    def cat_view(self, kind, l, buf=None):
        """[fwd; reverse] of layer l (adjacent in the flat buffer by construction)."""
        off, shape = self.offsets[f"{self.layer_prefix}{kind}_l{l}"]
        v = (self.flat if buf is None else buf)[off:off + 2 * math.prod(shape)]
        return v.view(2 * shape[0], *shape[1:])

    def load_state_dict(self, sd):
        for name, _ in self.specs:
            self.view(name).copy_(sd[name].to(torch.float32))

    def state_dict(self):
        return {name: self.view(name).detach().clone() for name, _ in self.specs}

    # ---- training state (checkpoint.save_training_state): the flat buffer as one tensor beside its layout
    def layout(self):
        """What the flat buffer's bits mean, in plain containers: the parameter names and shapes in order, and the
        net's ``cell``, ``gates``, ``attention``, ``crm``, ``adjust`` (None where a net has no such setting)."""
        fp = {"params": [[name, [int(d) for d in shape]] for name, shape in self.specs]}
        fp.update({k: getattr(self, k, None) for k in LAYOUT_FIELDS})
        return fp

    def flat_state(self):
        """{"flat": a host copy of the whole flat buffer, "layout": layout()}."""
        return {"flat": self.flat.detach().to("cpu", copy=True), "layout": self.layout()}

    def check_flat_state(self, sd, where):
        """Raise ValueError naming the first field in which ``sd`` (a flat_state()) is not this net's; nothing is
        written."""
        if not isinstance(sd, dict) or not isinstance(sd.get("layout"), dict):
            raise ValueError(f"{where}: no flat buffer with a layout in the file")
        saved, own = sd["layout"], self.layout()
        for k in LAYOUT_FIELDS:
            if saved.get(k) != own[k]:
                raise mismatch(f"{where}.layout.{k}", saved.get(k), own[k])
        ps, po = [(n, tuple(s)) for n, s in saved.get("params", [])], [(n, tuple(s)) for n, s in own["params"]]
        for i in range(max(len(ps), len(po))):
            a, b = (ps[i] if i < len(ps) else None), (po[i] if i < len(po) else None)
            if a != b:
                raise mismatch(f"{where}.layout.params[{i}] (of {len(ps)} in the file, {len(po)} here)", a, b)
        check_tensor(sd.get("flat"), self.flat, f"{where}.flat")

    def load_flat_state(self, sd):
        """Copy a checked flat_state() into the existing buffer and declare the change (params_changed, where the
        net has it)."""
        self.flat.copy_(sd["flat"])
        if hasattr(self, "params_changed"):
            self.params_changed()


LAYOUT_FIELDS = ("cell", "gates", "attention", "crm", "adjust")


def mismatch(field, saved, own):
    """The ValueError of a training-state field that differs: its name and both values."""
    return ValueError(f"{field}: the file has {saved!r}, this trainer has {own!r}")


def check_tensor(t, like, field):
    """``t`` must be a tensor of ``like``'s dtype and shape (a saved buffer against the one it is copied into)."""
    if not isinstance(t, torch.Tensor):
        raise mismatch(field, type(t).__name__, f"a {like.dtype} tensor of shape {tuple(like.shape)}")
    if t.dtype != like.dtype or tuple(t.shape) != tuple(like.shape):
        raise mismatch(field, f"{t.dtype} {tuple(t.shape)}", f"{like.dtype} {tuple(like.shape)}")


class SepNet(FlatParams):
    """Trainable parameters of the mask network, flat fp32 with named views.  ``gates``: "logistic" (torch's
    LSTM / GRU) or "hard", Keras 1's LSTM cell (hard_sigmoid i / f / o gates; cell "lstm", the fp32 recurrence):
    a setting that travels with the net -- parameter layout and initialisation are the same."""

    layer_prefix = "mix.layer."

    def __init__(self, cell="lstm", num_layers=4, hidden=300, emb=50, num_labels=101, input_fre=129, crm=False,
                 adjust=True, device="cuda", seed=1, attention="dot", gates="logistic"):
        self.gates = check_gates(gates, cell, "SepNet")
        if attention not in ("dot", "align"):
            raise ValueError(f"attention={attention!r}: expected 'dot' or 'align'")
        if attention == "align" and crm:
            raise ValueError("attention='align' with a cRM net is unsupported (the reference never ran that pair)")
        # 'dot': mask = sigmoid(V . q); 'align': sigmoid(w3 . tanh(W1 V + W2 q)) on the three extra
        # ATTENTION weights (EvalVer.py:228-239; DL4SS_Keras/extend_layers.py:50-64)
        self.attention = attention
        self.cell, self.L, self.H, self.E = cell, num_layers, hidden, emb
        self.F, self.num_labels, self.crm, self.adjust = input_fre, num_labels, crm, adjust
        self.W = 2 * emb if crm else emb
        specs = self._layer_specs(num_layers, input_fre, hidden, _ngate(cell) * hidden)
        specs += [("mix.Linear.weight", (input_fre * emb, 2 * hidden)), ("mix.Linear.bias", (input_fre * emb,)),
                  ("emb.layer.weight", (num_labels, self.W))]
        if adjust:
            specs.append(("adj.layer.weight", (self.W, 2 * hidden + self.W)))
        if attention == "align":  # behind every 'dot' parameter: the default layout does not move
            specs += [("att.Linear_1.weight", (emb, emb)), ("att.Linear_2.weight", (emb, emb)),
                      ("att.Linear_3.weight", (1, emb))]
        self._allocate(specs, device)
        off = self.numel
        # the flat gradient behind one 16-B slot: slot 0 carries each rank's hand-off status flag
        # through the gradient all-reduce (SepTrainer.allreduce), so every rank's guarded Adam
        # refuses the same steps.  Layout [flag | layers | Linear, emb, adj]: the data-parallel
        # step's two buckets are the contiguous ranges in front of and behind the Linear weight
        # (bucket_split)
        self.grad_ext = torch.zeros(off + 4, device=self.device, dtype=torch.float32)
        self.grad = self.grad_ext[4:]
        self.dp_flag = self.grad_ext[0:1]
        # generation of `flat` for writers torch's version counter does not see (the device-side
        # Adam of any trainer on this net, a raw-pointer kernel, a collective): every such write
        # bumps it (params_changed()), and a trainer trusts its bf16 weight copies only while
        # (generation, flat._version) is what it was when the copies were made
        self.generation = 0
        self.reset_parameters(seed)

    def params_changed(self):
        """Declare that `flat` was rewritten by means that may bypass torch's version counter:
        every trainer on this net re-derives its bf16 weight copies on its next step."""
        self.generation += 1

    def bucket_split(self):
        """Index into grad_ext between the data-parallel buckets: [0, split) = the status flag and
        every recurrent layer (complete after the last BPTT), [split, end) = the Linear, the speaker
        embedding, ADDJUST and the 'align' attention weights (complete before the first BPTT)."""
        return 4 + self.offsets["mix.Linear.weight"][0]

    def bucket_mid(self, layer):
        """Index into grad_ext where the recurrent layers >= ``layer`` start (layers are contiguous in
        order): the three-bucket step's middle bucket is [bucket_mid(layer), bucket_split())."""
        return 4 + self.offsets[f"mix.layer.weight_ih_l{layer}"][0]

    def named_parameters(self):
        return {name: self.view(name) for name, _ in self.specs}

    def reset_parameters(self, seed=1):
        """torch default initialisers (nn.LSTM/GRU, nn.Linear, nn.Embedding)."""
        g = torch.Generator().manual_seed(seed)
        for name, shape in self.specs:
            if name.startswith("mix.layer."):
                k = 1.0 / math.sqrt(self.H)
                t = torch.empty(shape).uniform_(-k, k, generator=g)
            elif name == "emb.layer.weight":
                t = torch.randn(shape, generator=g)
            elif name.endswith("bias"):
                k = 1.0 / math.sqrt(2 * self.H)
                t = torch.empty(shape).uniform_(-k, k, generator=g)
            else:
                k = 1.0 / math.sqrt(shape[1])
                t = torch.empty(shape).uniform_(-k, k, generator=g)
            self.view(name).copy_(t)


class DiscNet(FlatParams):
    """Parameters of the adversarial Discriminator (TDAA_beta/main_run_sstune_dis.py:318-336) for (T, F)
    maps, flat fp32 under the reference's eight ``state_dict`` keys with the shapes of
    ``compat.myNet.Discriminator`` (a ``_dislayer_`` file or that module's state_dict loads unchanged;
    ``checkpoint.load_reference_discriminator`` / ``save_reference_discriminator`` take a DiscNet as their
    module), and the two flat gradients of the adversarial step: ``grad_dis`` = d(L_dt + L_df) and
    ``grad_adv`` = d(lambda L_adv) (SepTrainer(adversary=...))."""

    def __init__(self, T, F=129, device="cuda", seed=1):
        hw = (ctypes.c_int * 6)()
        feat = _lib.query("dl4ss_disc_dims", int(T), int(F), hw)
        if feat < 0:
            raise ValueError(f"DiscNet: a ({T}, {F}) map is smaller than the 15 x 15 minimum")
        self.T, self.F, self.hw, self.feat = int(T), int(F), list(hw), feat
        self._allocate([("cnn.weight", (64, 1, 3, 3)), ("cnn.bias", (64,)), ("cnn1.weight", (64, 64, 3, 3)),
                        ("cnn1.bias", (64,)), ("cnn2.weight", (64, 64, 3, 3)), ("cnn2.bias", (64,)),
                        ("final.weight", (1, feat)), ("final.bias", (1,))], device)
        self.grad_dis = torch.zeros_like(self.flat)
        self.grad_adv = torch.zeros_like(self.flat)
        self.reset_parameters(seed)

    def load_state_dict(self, sd):
        """The eight keys, each with this net's shape (a file saved at another map size raises)."""
        for name, shape in self.specs:
            if tuple(sd[name].shape) != tuple(shape):
                raise ValueError(f"DiscNet: {name} has shape {tuple(sd[name].shape)}, expected {tuple(shape)}")
        super().load_state_dict(sd)

    def reset_parameters(self, seed=1):
        """torch's default initialisers of nn.Conv2d / nn.Linear: uniform +-1/sqrt(fan_in), weight and bias."""
        g = torch.Generator().manual_seed(seed)
        fan = {"cnn": 9, "cnn1": 576, "cnn2": 576, "final": self.feat}
        for name, shape in self.specs:
            k = 1.0 / math.sqrt(fan[name.split(".")[0]])
            self.view(name).copy_(torch.empty(shape).uniform_(-k, k, generator=g))
