"""Keras 1's LSTM cell through the upper layers: one SepTrainer step on a SepNet(gates="hard") against an fp64 torch
restatement (oracle.model's pieces around tests/keras_cell_ref.py's layer), the captured-graph step, the voiceprint
encoder and a voiceprint training step with hard nets, and MaskNetForward.

The mask net is SepNet(cell="lstm", num_layers=2, hidden=40, gates="hard", adjust=False) at B = 2, K = 2, N = 4000
(32 frames), fp32, label order, 'dot' and 'align'.  With default weights the cell never leaves hs's linear region, so
the first layer's input biases are drawn from N(0, 9): the fp64 reference then has each of its i, f, o gates at
exactly 0 and at exactly 1 for >= 10 % of the values and strictly inside for >= 20 % (asserted).  The seed is the
first whose fp64 pre-activations all keep >= 1e-4 from the kinks at +-2.5 (chosen on the CPU from the reference
alone, asserted), so fp32 and fp64 saturate alike -- checked on the device's act -- and the reference's own BPTT
pattern applies.  Bounds: those of the logistic step tests (tests/test_step_gpu.py, tests/test_align_api_gpu.py):
loss 1e-4 relative, every gradient 2e-3 of its largest element; the voiceprint encoder's are
tests/test_voiceprint_encoder_gpu.py's (2e-5 absolute, 1e-4 of the largest element).

The parameters after the first Adam step (_assert_adam_step): that step moves a weight by lr f(g), f(g) = g / (|g| +
eps), which is increasing in g.  A gradient within E = 2e-3 of its tensor's largest element of the fp64 one (the
bound just asserted) therefore moves its weight by something in [lr f(g - E), lr f(g + E)], up to the fp32 rounding
of the update (one rounding of the parameter, 2^-24 |w|, doubled, and 1e-5 of lr for the moments' few roundings).
Every weight must lie in that interval -- also the many whose gradient is zero or below E (columns of silent
bins, gates on the clip), which the logistic tests' helper counts as rare exceptions and the hard cell has more of.
The fp64 torch.optim.Adam step of the restatement is checked against the same lr f(g)."""
import functools

import numpy as np
import pytest
import torch

import keras_cell_ref as K
import keras_voiceprint_ref as KV
import voiceprint_ref as vr
from oracle import model as om
from dl4ss_amd import engine, infer, ops, synth
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintEncoder, VoiceprintNet
from test_align_api_gpu import AlignSepModel
from test_step_gpu import _oracle_features

L, H, B, NK, N = 2, 40, 2, 2, 4000
MARGIN = 1e-4


def _saturating_biases(net, prefix, seed):
    """the first layer's input biases ~ N(0, 9), both directions"""
    g = torch.Generator().manual_seed(1000 + seed)
    for sfx in ("", "_reverse"):
        b = net.view(f"{prefix}bias_ih_l0{sfx}")
        b.copy_(torch.randn(b.shape, generator=g) * 3.0)


def _net(device, seed, attention):
    net = engine.SepNet(cell="lstm", num_layers=L, hidden=H, gates="hard", adjust=False, device=device, seed=seed,
                        attention=attention)
    _saturating_biases(net, "mix.layer.", seed)
    return net


def _ref_model(net, rec):
    """oracle.model.SepModel ('align': test_align_api_gpu's) in fp64 on net's parameters, its nn.LSTM forward
    replaced by the hard-gates layers; rec collects the layers' kink margins and activations."""
    base = AlignSepModel if net.attention == "align" else om.SepModel
    ref = base(cell="lstm", num_layers=L, hidden=H, adjust=False)
    ref.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    ref.double()
    mix = ref.mix

    def forward(x):
        h = KV.stack(x, dict(mix.layer.named_parameters()), L, "", rec["margins"], rec["acts"])
        n, T, _ = h.shape
        return torch.tanh(mix.Linear(h.reshape(n * T, -1))).view(n, T, mix.input_fre, -1), h

    mix.forward = forward
    return ref


def _assert_adam_step(net, w0, ref, grads_ref, tol_grad, lr=2e-4, eps=1e-8):
    """net's parameters after its first Adam step from w0 (see the module docstring)."""
    f = lambda g: g / (g.abs() + eps)  # noqa: E731
    for name, p in ref.named_parameters():
        g = grads_ref[name]
        before, after = net.view(name, w0).cpu().double(), net.view(name).cpu().double()
        assert (before - lr * f(g) - p.detach()).abs().max().item() < 1e-12, name  # the restatement's own step
        E = tol_grad * g.abs().max().item()
        moved = before - after
        r = 2 * 2.0 ** -24 * torch.maximum(before.abs(), after.abs()) + 1e-5 * lr
        assert bool((moved >= lr * f(g - E) - r).all()) and bool((moved <= lr * f(g + E) + r).all()), name


def _data(seed):
    src, spk, u = synth.SyntheticMixtures(n_samples=N, k=NK, seed=seed).batch(B)
    return src, spk, synth.gains_for(u, NK)


@functools.lru_cache(maxsize=None)
def _seed(attention):
    """The first seed whose fp64 reference keeps every i / f / o pre-activation >= MARGIN from a kink (CPU only)."""
    for seed in range(3, 40):
        rec = dict(margins=[], acts=[])
        ref = _ref_model(_net("cpu", seed, attention), rec)
        src, spk, gains = _data(seed)
        with torch.no_grad():
            ref.mix(_oracle_features(src, gains, False)[0].double())
        if min(rec["margins"]) >= MARGIN:
            return seed
    raise AssertionError("no seed with a kink margin of 1e-4")


def test_reference_case_saturates_with_a_margin():
    """(no GPU) the properties of the step test's reference: chosen seed, margin, saturation shares"""
    for attention in ("dot", "align"):
        seed = _seed(attention)
        rec = dict(margins=[], acts=[])
        ref = _ref_model(_net("cpu", seed, attention), rec)
        src, spk, gains = _data(seed)
        with torch.no_grad():
            ref.mix(_oracle_features(src, gains, False)[0].double())
        print(attention, "seed", seed, "margins", rec["margins"], K.saturation_shares(rec["acts"][0]))
        assert min(rec["margins"]) >= MARGIN
        K.assert_saturates(rec["acts"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("attention", ["dot", "align"])
def test_hard_step_matches_fp64(dev, attention):
    tol_loss, tol_grad = 1e-4, 2e-3
    seed = _seed(attention)
    net = _net(dev, seed, attention)
    tr = engine.SepTrainer(net, B, NK, N, mode="label")
    assert tr.rnn_flags == ops.HARD_GATES
    rec = dict(margins=[], acts=[])
    ref = _ref_model(net, rec)
    src, spk, gains = _data(seed)
    feats, X, Y = (t.double() for t in _oracle_features(src, gains, False))
    opt = om.make_adam(ref)
    opt.zero_grad()
    mask = ref(feats, torch.from_numpy(spk))[0]
    assert min(rec["margins"]) >= MARGIN, rec["margins"]
    K.assert_saturates(rec["acts"][0])
    loss_ref, _ = om.loss_label_ordered(mask, X, Y)
    loss_ref.backward()
    grads_ref = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    opt.step()
    # --- the HIP step
    tr.spk.copy_(torch.from_numpy(spk.astype(np.int32)).to(dev))
    tr.features(torch.from_numpy(src.astype(np.float32)).to(dev), torch.from_numpy(gains.astype(np.float32)).to(dev))
    tr.forward()
    w0 = net.flat.clone()
    for l in range(L):  # fp32 saturates exactly where fp64 does (the margin): the reference's pattern is the device's
        assert torch.equal(K.inside(tr.act[l].cpu().double()), K.inside(rec["acts"][l])), l
        err = (tr.act[l].cpu().double() - rec["acts"][l]).abs().max().item()
        print(f"{attention}: layer {l} act max abs err {err:.3e}")
    loss = tr.loss_and_grad()
    tr.backward()
    tr.optimizer_step()
    tr.check()
    l_, lr_ = float(loss[0].cpu()), float(loss_ref.detach())
    print(f"{attention}: loss {l_:.8e} vs fp64 {lr_:.8e} (rel {abs(l_ - lr_) / abs(lr_):.3e})")
    assert abs(l_ - lr_) / abs(lr_) < tol_loss, (l_, lr_)
    errs = {}
    for name, gr in grads_ref.items():
        ours = net.view(name, net.grad).cpu().double()
        denom = gr.abs().max().item()
        errs[name] = (ours - gr).abs().max().item() / denom if denom > 0 else ours.abs().max().item()
    print(f"{attention}: gradient errors (of the largest element)", {k: f"{v:.2e}" for k, v in errs.items()})
    assert set(errs) == {n for n, _ in net.specs}
    bad = {k: v for k, v in errs.items() if v > tol_grad}
    assert not bad, (bad, errs)
    _assert_adam_step(net, w0, ref, grads_ref, tol_grad)


@pytest.mark.gpu
@pytest.mark.parametrize("attention", ["dot", "align"])
def test_hard_graph_step_equals_eager_bitwise(dev, attention):
    gen = synth.SyntheticMixtures(n_samples=N, k=NK, seed=5)
    batches = []
    for _ in range(3):
        src, spk, u = gen.batch(B)
        batches.append((torch.from_numpy(src.astype(np.float32)).to(dev),
                        torch.from_numpy(synth.gains_for(u, NK).astype(np.float32)).to(dev),
                        torch.from_numpy(spk.astype(np.int32)).to(dev)))
    runs = []
    for graph in (False, True):
        net = _net(dev, 7, attention)
        tr = engine.SepTrainer(net, B, NK, N, mode="label", splitk_reduce="fixed")
        if graph:
            tr.capture()
        losses = [(tr.step_graph(*b) if graph else tr.step(*b)).clone() for b in batches]
        tr.check()
        act0 = tr.act[0]
        assert bool((act0 == 0).any()) and bool((act0 == 1).any())  # the hard cell ran: gates on the clip
        runs.append((torch.stack(losses), net.grad.clone(), net.flat.clone(), tr.m.clone(), tr.v.clone()))
    assert runs[0][0].isfinite().all()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- the voiceprint encoder ----------------------------------------------------------------------------------------
VN, VT, VF, VH = 4, 9, 23, 25
VLENS = [9, 4, 0, 1]


def _vp_feats():
    x = vr.inputs(51, VN, VT, VF)
    for b, n in enumerate(VLENS):
        x[b, n:] = 0
    return x


@functools.lru_cache(maxsize=None)
def _vp_case():
    """(seed, fp64 voiceprints, gradients): the first seed whose reference keeps MARGIN from every kink (CPU only)."""
    x = _vp_feats()
    xc, lens, _ = vr.compact(x, vr.frame_mask(x))
    dvec = vr.inputs(52, VN, 2 * VH)
    for seed in range(3, 40):
        vnet = VoiceprintNet(input_fre=VF, emb=2 * VH, hidden=VH, num_layers=2, device="cpu", seed=seed, gates="hard")
        _saturating_biases(vnet, "spk.layer.", seed)
        vec, grads, margin = KV.encoder_ref(xc, lens, vnet.state_dict(), VH, 2, dvec)
        if margin >= MARGIN:
            return seed, vec, grads, margin
    raise AssertionError("no seed with a kink margin of 1e-4")


def test_voiceprint_reference_case_has_a_margin():
    seed, vec, grads, margin = _vp_case()
    assert margin >= MARGIN and vec.isfinite().all()


@pytest.mark.gpu
def test_hard_voiceprint_encoder_matches_per_utterance_fp64(dev):
    seed, want, grads, margin = _vp_case()
    assert margin >= MARGIN
    vnet = VoiceprintNet(input_fre=VF, emb=2 * VH, hidden=VH, num_layers=2, device=dev, seed=seed, gates="hard")
    _saturating_biases(vnet, "spk.layer.", seed)
    enc = VoiceprintEncoder(vnet, VN, VT)
    assert enc.rnn_flags == ops.HARD_GATES
    x = _vp_feats()
    dvec = vr.inputs(52, VN, 2 * VH)
    vec = enc.forward(x.to(dev)).clone()
    vnet.grad.fill_(float("nan"))
    enc.backward(dvec.to(dev))
    enc.check()
    assert enc.len.tolist() == VLENS
    assert bool((enc.act[0] == 0).any()) and bool((enc.act[0] == 1).any())  # gates on the clip
    err = (vec.cpu().double() - want).abs().max().item()
    print(f"hard voiceprint: max abs err {err:.3e}")
    assert err < 2e-5, err
    assert (vec[2] == 0).all() and not vnet.grad.isnan().any()
    for name, _ in vnet.specs:
        g, w = vnet.grad_view(name).cpu().double(), grads[name]
        rel = ((g - w).abs().max() / w.abs().max()).item()
        print(f"  {name}: {rel:.3e} of the largest element")
        assert rel < 1e-4, (name, rel)
    # the logistic encoder on the same parameters gives another vector: the setting is not ignored
    soft = VoiceprintNet(input_fre=VF, emb=2 * VH, hidden=VH, num_layers=2, device=dev, seed=seed)
    soft.flat.copy_(vnet.flat)
    assert (VoiceprintEncoder(soft, VN, VT).forward(x.to(dev)) - vec).abs().max().item() > 1e-2


@pytest.mark.gpu
def test_voiceprint_training_step_with_both_nets_hard(dev):
    net = _net(dev, 7, "align")
    vnet = VoiceprintNet(device=dev, seed=3, gates="hard")
    _saturating_biases(vnet, "spk.layer.", 3)
    memory = SpeakerMemory(101, 50, device=dev)
    tr = engine.SepTrainer(net, B, NK, N, voiceprint=vnet, memory=memory)
    assert tr.rnn_flags == ops.HARD_GATES and tr.vp_enc.rnn_flags == ops.HARD_GATES
    g = torch.Generator().manual_seed(1)
    raw = torch.randn(B, NK, N, generator=g).to(dev)
    gains = (torch.rand(B, NK, generator=g) * 0.5 + 0.75).to(dev)
    spk = torch.tensor([[17, 4], [4, 99]], dtype=torch.int32, device=dev)
    w0, v0 = net.flat.clone(), vnet.flat.clone()
    losses = [float(tr.step(raw, gains, spk)[0].cpu()) for _ in range(2)]
    tr.check()
    assert all(np.isfinite(losses)), losses
    assert not torch.equal(net.flat, w0) and not torch.equal(vnet.flat, v0)  # both nets trained
    assert net.flat.isfinite().all() and vnet.flat.isfinite().all() and memory.mem.isfinite().all()
    for act in (tr.act[0], tr.vp_enc.act[0]):
        assert bool((act == 0).any()) and bool((act == 1).any())


@pytest.mark.gpu
def test_mask_net_forward_equals_the_trainers_forward(dev):
    """infer.MaskNetForward on the hard net: V, the forward output every mask is formed from, bit for bit the
    trainer's; and the logistic forward of the same parameters differs."""
    net = _net(dev, 7, "dot")
    tr = engine.SepTrainer(net, B, NK, N, mode="label")
    src, spk, gains = _data(7)
    tr.spk.copy_(torch.from_numpy(spk.astype(np.int32)).to(dev))
    tr.features(torch.from_numpy(src.astype(np.float32)).to(dev), torch.from_numpy(gains.astype(np.float32)).to(dev))
    tr.forward()
    mask = torch.empty(B, NK, tr.T * tr.F, device=dev)
    tr.attn(0, mask_out=mask)
    tr.check()
    fwd = infer.MaskNetForward(net, B, tr.T)
    V = fwd(tr.mag_mix, torch.empty_like(tr.V))
    fwd.stack.check()
    assert torch.equal(V.view(-1), tr.V.view(-1))
    # the masks of the inference path from that V and the trainer's queries (another attention kernel: the bound
    # of tests/test_voiceprint_step_gpu.py for it)
    ex = infer.EnrolledExtractor(net, VoiceprintNet(device=dev, gates="hard"), B, tr.T, NK)
    masks = ex.run(tr.mag_mix, tr.q.view(B, NK, -1))
    assert (masks.view(B, NK, -1) - mask).abs().max().item() < 1e-4
    soft = engine.SepNet(cell="lstm", num_layers=L, hidden=H, adjust=False, device=dev, seed=7)
    soft.flat.copy_(net.flat)
    Vs = infer.MaskNetForward(soft, B, tr.T)(tr.mag_mix, torch.empty_like(tr.V))
    assert (Vs.view(-1) - V.view(-1)).abs().max().item() > 1e-2
