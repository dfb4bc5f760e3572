"""ATTENTION 'align' through the public layers: the autograd Function and the dl4ss::attention_align
op, compat.myNet.ATTENTION(mode='align'), and one SepNet(attention="align") / SepTrainer training
step (eager and as a HIP graph) against the CPU oracle extended, in this file, with the reference's
additive attention (TDAA_beta/main_run_sstune_EvalVer.py:228-239: Linear_1 / Linear_2 / Linear_3 without
bias, tanh, sigmoid).  The step test follows tests/test_step_gpu._compare_step and uses its fp32
tolerances: loss 1e-4, masked-magnitude rel-L2 1e-3, every gradient 2e-3 of its max, the Adam check of
_assert_adam_params_close with the attention weights included."""
import functools
import itertools

import numpy as np
import pytest
import torch
from torch import nn

from oracle import model as om
from dl4ss_amd import autograd as ag, engine, library, synth  # noqa: F401  (library registers the ops)
from test_step_gpu import _assert_adam_params_close, _oracle_features

pytestmark = pytest.mark.gpu
E = 50


class AlignAttention(nn.Module):
    """The reference ATTENTION's three 'align' Linears (EvalVer.py:207-213), state_dict keys as there."""

    def __init__(self, emb=E):
        super().__init__()
        self.Linear_1 = nn.Linear(emb, emb, bias=False)
        self.Linear_2 = nn.Linear(emb, emb, bias=False)
        self.Linear_3 = nn.Linear(emb, 1, bias=False)

    def forward(self, V, q):
        """V (B,T,F,E), q (B,K,E) -> mask (B,K,T,F) (EvalVer.py:228-239 per query)."""
        s = torch.tanh(self.Linear_1(V)[:, None] + self.Linear_2(q)[:, :, None, None])
        return torch.sigmoid(self.Linear_3(s).squeeze(-1))


class AlignSepModel(om.SepModel):
    """oracle.model.SepModel with att.Linear_1/2/3 and the additive attention in place of 'dot'."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.att = AlignAttention()

    def forward(self, feats, spk_idx):
        V, h = self.mix(feats)
        q = self.queries(h, spk_idx)
        return self.att(V, q), V, h, q


def _inputs(dev, Bq, R, seed=0, double=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    k = 1.0 / E ** 0.5
    t = [torch.tanh(torch.randn(Bq, R, E, generator=g)), torch.randn(Bq, E, generator=g),
         torch.empty(E, E).uniform_(-k, k, generator=g), torch.empty(E, E).uniform_(-k, k, generator=g),
         torch.empty(1, E).uniform_(-k, k, generator=g)]
    dm = torch.randn(Bq, R, generator=g)
    if double:
        return [x.double().requires_grad_(True) for x in t], dm.double()
    return [x.to(dev).requires_grad_(True) for x in t], dm.to(dev)


def test_function_and_op_agree_bitwise(dev):
    (a, dm), (b, _) = _inputs(dev, 3, 700), _inputs(dev, 3, 700)
    ma = ag.AttentionAlignFn.apply(*a)
    mb = torch.ops.dl4ss.attention_align(*b)
    assert torch.equal(ma, mb)
    ga = torch.autograd.grad(ma, a, dm)
    gb = torch.autograd.grad(mb, b, dm)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)
    # needs_input_grad is honoured: no gradient for a frozen input
    c, _ = _inputs(dev, 3, 700)
    c[0].requires_grad_(False)
    c[3].requires_grad_(False)
    mc = ag.AttentionAlignFn.apply(*c)
    gc_ = torch.autograd.grad(mc, [c[1], c[2], c[4]], dm)
    for x, y in zip(gc_, (ga[1], ga[2], ga[4])):
        assert torch.equal(x, y)


def test_op_opcheck(dev):
    a, _ = _inputs(dev, 2, 300)
    torch.library.opcheck(torch.ops.dl4ss.attention_align.default, tuple(a),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    dm = torch.randn(2, 300, device=dev)
    torch.library.opcheck(torch.ops.dl4ss.attention_align_bwd.default, (dm, *[x.detach() for x in a], True),
                          test_utils=("test_schema", "test_faketensor"))


def test_compat_attention_align_matches_fp64(dev):
    from dl4ss_amd.compat import myNet

    B, T, F = 2, 5, 129
    g = torch.Generator(device="cpu").manual_seed(4)
    att = myNet.ATTENTION(E, 'align', crm=False).to(dev)
    V = torch.tanh(torch.randn(B, T, F, E, generator=g))
    q = torch.randn(B, E, generator=g)
    dm = torch.randn(B, T, F, generator=g)
    Vd, qd = V.to(dev).requires_grad_(True), q.to(dev).requires_grad_(True)
    mask = att(Vd, qd)
    assert mask.shape == (B, T, F)
    params = [att.Linear_1.weight, att.Linear_2.weight, att.Linear_3.weight]
    got = torch.autograd.grad(mask, [Vd, qd] + params, dm.to(dev))
    # fp64 torch autograd of the reference formula on the same weights
    leaves = [V.double().requires_grad_(True), q.double().requires_grad_(True)] + \
        [p.detach().double().cpu().requires_grad_(True) for p in params]
    V64, q64, W1, W2, w3 = leaves
    s = torch.tanh(V64 @ W1.t() + (q64 @ W2.t())[:, None, None])
    ref = torch.sigmoid((s @ w3.t()).squeeze(-1))
    want = torch.autograd.grad(ref, leaves, dm.double())
    assert torch.allclose(mask.double().cpu(), ref.detach(), rtol=1e-5, atol=1e-6)
    for n, x, y, tol in zip(("dV", "dq", "dW1", "dW2", "dw3"), got, want, (1e-5, 1e-4, 1e-4, 1e-4, 1e-4)):
        err = float((x.double().cpu() - y).abs().max()) / float(y.abs().max())
        assert err <= tol, (n, err)


def test_compat_attention_dot_unchanged(dev):
    from dl4ss_amd.compat import myNet

    g = torch.Generator(device="cpu").manual_seed(5)
    V = torch.tanh(torch.randn(2, 5, 129, E, generator=g)).to(dev)
    q = torch.randn(2, E, generator=g).to(dev)
    att = myNet.ATTENTION(E, 'dot', crm=False).to(dev)
    assert torch.equal(att(V, q), ag.AttentionDotFn.apply(V.reshape(2, -1, E), q, False).view(2, 5, 129))


def test_compat_align_with_crm_raises(dev):
    from dl4ss_amd.compat import myNet

    att = myNet.ATTENTION(E, 'align', crm=True).to(dev)
    with pytest.raises(NotImplementedError, match="align"):
        att(torch.zeros(1, 2, 129, E, device=dev), torch.zeros(1, 2 * E, device=dev))


def test_trainer_rejects_unsupported_align_combinations(dev):
    with pytest.raises(ValueError, match="cRM"):
        engine.SepNet(cell="gru", num_layers=1, crm=True, attention="align", device=dev)
    net = engine.SepNet(cell="gru", num_layers=1, attention="align", device=dev)
    with pytest.raises(ValueError, match="loss_channels"):
        engine.SepTrainer(net, 1, 2, 2000, loss_channels=101)
    for prec in ("bf16", "bf16s", "bf16s2"):
        with pytest.raises(ValueError, match="bf16"):
            engine.SepTrainer(net, 1, 2, 2000, precision=prec)
    with pytest.raises(ValueError):
        engine.SepTrainer(net, 1, 2, 2000, mode="crm")


# ------------------------------------------------------------------ one training step
def _margin(ref, feats, X, Y, idx):
    """The oracle's per-utterance relative margin between its best and second-best PIT cost."""
    with torch.no_grad():
        mask = ref(feats, idx)[0]
    K = mask.shape[1]
    pred = mask * X[:, None]
    C = ((pred[:, :, None] - Y[:, None, :]) ** 2).sum(dim=(-1, -2))
    costs = torch.stack([sum(C[:, k, p[k]] for k in range(K)) for p in itertools.permutations(range(K))], 1)
    srt = costs.sort(1).values
    return ((srt[:, 1] - srt[:, 0]) / srt[:, 0]).min().item()


@functools.lru_cache(maxsize=None)
def _pit_seed(cell, L, B, K, N):
    """The first seed whose oracle PIT decision has a relative margin above 1e-3 in every utterance
    (CPU only: the reference alone decides, before any GPU work)."""
    for seed in range(3, 40):
        net = engine.SepNet(cell=cell, num_layers=L, device="cpu", seed=seed, attention="align")
        ref = AlignSepModel(cell=cell, num_layers=L)
        ref.load_state_dict(net.state_dict())
        src, spk, u = synth.SyntheticMixtures(n_samples=N, k=K, seed=seed).batch(B)
        feats, X, Y = _oracle_features(src, synth.gains_for(u, K), False)
        if _margin(ref, feats, X, Y, torch.from_numpy(spk)) > 1e-3:
            return seed
    raise AssertionError("no seed with a PIT margin above 1e-3")


@pytest.mark.parametrize("cell,L,B,K,N,mode", [("lstm", 2, 2, 2, 3000, "label"), ("gru", 2, 3, 2, 3000, "pit")])
def test_align_step_matches_oracle(dev, cell, L, B, K, N, mode):
    tol_loss, tol_pred, tol_grad = 1e-4, 1e-3, 2e-3
    seed = _pit_seed(cell, L, B, K, N) if mode == "pit" else 3
    net = engine.SepNet(cell=cell, num_layers=L, device=dev, seed=seed, attention="align")
    tr = engine.SepTrainer(net, B, K, N, mode=mode)
    src, spk, u = synth.SyntheticMixtures(n_samples=N, k=K, seed=seed).batch(B)
    gains = synth.gains_for(u, K)
    ref = AlignSepModel(cell=cell, num_layers=L)
    ref.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    assert set(ref.state_dict()) == set(net.state_dict())
    feats, X, Y = _oracle_features(src, gains, False)
    idx = torch.from_numpy(spk)
    # --- oracle step
    opt = om.make_adam(ref)
    opt.zero_grad()
    mask = ref(feats, idx)[0]
    perm_ref = None
    if mode == "pit":
        assert _margin(ref, feats, X, Y, idx) > 1e-3
        perm_ref = om.pit_assign(mask.detach(), X, Y)[0]
        loss_ref, pred_ref = om.loss_pit(mask, X, Y)
    else:
        loss_ref, pred_ref = om.loss_label_ordered(mask, X, Y)
    loss_ref.backward()
    grads_ref = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    opt.step()
    # --- HIP step
    tr.spk.copy_(torch.from_numpy(spk.astype(np.int32)).to(dev))
    tr.features(torch.from_numpy(src.astype(np.float32)).to(dev), torch.from_numpy(gains.astype(np.float32)).to(dev))
    tr.forward()
    pred = torch.empty(B, K, tr.T * tr.F, device=dev)
    tr.attn(0, pred_out=pred)
    loss = tr.loss_and_grad()
    tr.backward()
    tr.optimizer_step()
    tr.check()
    l = float(loss[0].cpu())
    lr_ = float(loss_ref.detach())
    assert abs(l - lr_) / abs(lr_) < tol_loss, (l, lr_)
    if mode == "pit":
        assert torch.equal(tr.perm.cpu().long(), perm_ref)
    # masked magnitude: the prediction does not depend on the assignment
    rel = ((pred.cpu().view(pred_ref.shape) - pred_ref.detach()).norm() / pred_ref.detach().norm()).item()
    assert rel < tol_pred, rel
    errs = {}
    for name, gr in grads_ref.items():
        ours = net.view(name, net.grad).cpu()
        denom = gr.abs().max().item()
        errs[name] = (ours - gr).abs().max().item() / denom if denom > 0 else ours.abs().max().item()
    assert {"att.Linear_1.weight", "att.Linear_2.weight", "att.Linear_3.weight"} <= set(errs)
    bad = {k: v for k, v in errs.items() if v > tol_grad}
    assert not bad, (bad, errs)
    _assert_adam_params_close(net, ref, grads_ref, errs)


def test_align_graph_step_equals_eager_bitwise(dev):
    cell, L, B, K, N = "lstm", 2, 2, 2, 3000
    gen = synth.SyntheticMixtures(n_samples=N, k=K, seed=5)
    batches = []
    for _ in range(3):
        src, spk, u = gen.batch(B)
        batches.append((torch.from_numpy(src.astype(np.float32)).to(dev),
                        torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(dev),
                        torch.from_numpy(spk.astype(np.int32)).to(dev)))
    runs = []
    for graph in (False, True):
        net = engine.SepNet(cell=cell, num_layers=L, device=dev, seed=7, attention="align")
        tr = engine.SepTrainer(net, B, K, N, mode="label")
        init = {n: net.view(n).clone() for n in ("att.Linear_1.weight", "att.Linear_2.weight", "att.Linear_3.weight")}
        if graph:
            tr.capture()
        losses = []
        for b in batches:
            losses.append((tr.step_graph(*b) if graph else tr.step(*b)).clone())
        tr.check()
        for n, w0 in init.items():  # the attention weights train
            assert not torch.equal(net.view(n), w0), n
        runs.append((torch.stack(losses), net.grad.clone(), net.flat.clone(), tr.m.clone(), tr.v.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
