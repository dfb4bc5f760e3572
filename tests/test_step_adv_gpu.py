"""The adversarial term in the fused training step, SepTrainer(adversary=DiscNet): the step of
compat/drivers/main_run_sstune_dis.train_step(detach_fake=True) with a weight lambda on the adversarial term.

Reference (fp32 torch-CPU, computed once per case and shared): oracle.model.SepModel plus the reference
Discriminator written with torch.nn.functional.conv2d, weights those of the trainer's SepNet / DiscNet (the same
seeds on the CPU), torch.autograd.grad applied to
    L_dt = mean (D(Y) - 1)^2,  L_df = mean D(pred.detach())^2,  L_adv = mean (D(pred) - 1)^2,
    g_dis = d(L_dt + L_df)/d theta_D,  g_adv = d(lambda L_adv)/d theta_D,  gext = d(lambda L_adv)/d pred,
    separation gradients d(L_sep + lambda L_adv)/d theta_sep.
The separation gradient is linear in lambda: g(lambda) = g(0) + lambda g_ext, so one reference serves every
lambda.  Every comparison against the GPU is preceded by a precondition on the reference alone: for every
separation tensor max|g(lambda) - g(0)| >= 10 x (the gradient bar) x max|g(lambda)|, so that a step that drops
the term cannot pass."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import disc_ref as R
import small_ref as sr
from dl4ss_amd import engine, ops, synth
from oracle import model as om
from test_step_gpu import _assert_adam_params_close, _oracle_features

pytestmark = pytest.mark.gpu
F = 129
NET_SEED, DISC_SEED, BATCH_SEED = 3, 5, 3
LR = 2e-4


def _disc(P, x):
    """the reference Discriminator (main_run_sstune_dis.py:318-336) on maps x (n, T, F) -> scores (n, 1)"""
    h = x[:, None]
    for n in ("cnn", "cnn1", "cnn2"):
        h = torch.relu(Fn.conv2d(h, P[n + ".weight"], P[n + ".bias"], stride=2))
    return torch.sigmoid(Fn.linear(h.reshape(x.shape[0], -1), P["final.weight"], P["final.bias"]))


def _batch(B, K, N, seed=BATCH_SEED):
    src, spk, u = synth.SyntheticMixtures(n_samples=N, k=K, seed=seed).batch(B)
    return src, spk, synth.gains_for(u, K)


def _dev_batch(dev, b):
    src, spk, gains = b
    return (torch.from_numpy(src.astype(np.float32)).to(dev), torch.from_numpy(gains.astype(np.float32)).to(dev),
            torch.from_numpy(spk.astype(np.int32)).to(dev))


def _gate_margin(P, x):
    """The smallest |z| of the Discriminator's ReLU pre-activations on the maps x, in units of the fp32
    resolution of its own sum, 2^-24 (|x| (*) |w| + |b|), evaluated in fp64.  Two fp32 evaluations that order
    the sum differently agree on the sign of z -- the ReLU gate -- only where |z| exceeds a few of these units;
    a gate that differs changes conv gradients by whole elements, far beyond any rounding bar."""
    P = {k: v.detach().double() for k, v in P.items()}
    h, worst = x.detach().double()[:, None], float("inf")
    for n in ("cnn", "cnn1", "cnn2"):
        w, b = P[n + ".weight"], P[n + ".bias"]
        z = Fn.conv2d(h, w, b, stride=2)
        unit = R.U32 * (Fn.conv2d(h.abs(), w.abs(), None, stride=2) + b.abs().view(1, -1, 1, 1))
        worst = min(worst, float((z.abs() / unit).min()))
        h = torch.relu(z)
    return worst


@functools.lru_cache(maxsize=None)
def _reference(cell, mode, B, K, L, N, disc_seed=DISC_SEED, batch_seed=BATCH_SEED):
    """lambda = 1 quantities; unchanged once computed"""
    T = ops.n_frames(N)
    net = engine.SepNet(cell=cell, num_layers=L, device="cpu", seed=NET_SEED)
    disc = engine.DiscNet(T, F, device="cpu", seed=disc_seed)
    src, spk, gains = _batch(B, K, N, batch_seed)
    feats, X, Y = _oracle_features(src, gains, False)
    ref = om.SepModel(cell=cell, num_layers=L)
    ref.load_state_dict(net.state_dict())
    mask, _, _, _ = ref(feats, torch.from_numpy(spk))
    l_sep, pred = (om.loss_pit if mode == "pit" else om.loss_label_ordered)(mask, X, Y)
    P = {k: v.clone().requires_grad_(True) for k, v in disc.state_dict().items()}
    Pl = list(P.values())
    s_true, s_fd = _disc(P, Y.reshape(B * K, T, F)), _disc(P, pred.detach().reshape(B * K, T, F))
    l_dt, l_df = ((s_true - 1) ** 2).mean(), (s_fd ** 2).mean()
    g_dis = torch.autograd.grad(l_dt + l_df, Pl)
    pl = pred.detach().clone().requires_grad_(True)
    l_adv = ((_disc(P, pl.reshape(B * K, T, F)) - 1) ** 2).mean()
    *g_adv, gext = torch.autograd.grad(l_adv, Pl + [pl])
    names = [n for n, _ in ref.named_parameters()]
    params = [p for _, p in ref.named_parameters()]
    g0 = torch.autograd.grad(l_sep, params, retain_graph=True)
    g1 = torch.autograd.grad((gext * pred).sum(), params)
    return dict(l_sep=float(l_sep.detach()), scores=torch.cat([s_true, s_fd]).detach().view(-1),
                losses=[float(l_dt.detach()), float(l_df.detach()), float(l_adv.detach())], g_dis=dict(zip(P, g_dis)), g_adv=dict(zip(P, g_adv)),
                gext=gext, g0=dict(zip(names, g0)), g_ext=dict(zip(names, g1)), model=ref,
                gate_margin=_gate_margin(P, torch.cat([Y.reshape(B * K, T, F), pred.detach().reshape(B * K, T, F)])))


def _sep_grads(ref, lam):
    return {n: ref["g0"][n] + lam * ref["g_ext"][n] for n in ref["g0"]}


def _precondition(ref, lam, tol):
    """on the reference alone: the adversarial term moves every separation gradient by >= 10 tol of its max"""
    ratios = {}
    for n, g in _sep_grads(ref, lam).items():
        ratios[n] = float((lam * ref["g_ext"][n]).abs().max() / g.abs().max())
    print(f"precondition lambda={lam}: min ratio {min(ratios.values()):.3e} max {max(ratios.values()):.3e}")
    assert min(ratios.values()) >= 10 * tol, ratios
    return ratios


def _trainer(dev, cell, mode, B, K, L, N, lam, precision="fp32", disc_seed=DISC_SEED, **kw):
    net = engine.SepNet(cell=cell, num_layers=L, device=dev, seed=NET_SEED)
    disc = engine.DiscNet(ops.n_frames(N), F, device=dev, seed=disc_seed)
    tr = engine.SepTrainer(net, B, K, N, mode=mode, precision=precision, adversary=disc, adv_weight=lam, **kw)
    return net, disc, tr


def _grad_pass(tr, b):
    raw, gains, spk = b
    tr.spk.copy_(spk)
    tr.features(raw, gains)
    tr.forward()
    loss = tr.loss_and_grad()
    tr.backward()
    torch.cuda.synchronize()
    return loss


def _rel(a, ref):
    d = float(ref.abs().max())
    return float((a.detach().cpu().float() - ref).abs().max()) / d if d > 0 else float(a.abs().max())


def _sep_errs(net, grads_ref):
    return {n: _rel(net.view(n, net.grad), g) for n, g in grads_ref.items()}


# ------------------------------------------------------------------------------------------- 3. fp32 step
CASES32 = [("gru", "label", 2, 2), ("lstm", "pit", 2, 3)]
# (DiscNet seed, batch seed) of the fp32 comparison.  With (5, 3) the (lstm, pit) case has a conv1
# pre-activation of 9.9e-8 under inputs up to 56 -- 2.6 resolution units (_gate_margin) -- whose ReLU gate the
# kernel and torch-CPU take differently: one whole dy1 element in cnn.bias' gradient, 4.6e-3 of its largest.
# With (10, 7) the smallest pre-activation is 17 units in both cases.
SEEDS32 = (10, 7)


@pytest.mark.parametrize("lam", [1.0, 20.0])
@pytest.mark.parametrize("cell,mode,B,K", CASES32)
def test_adv_step_fp32_matches_reference(dev, cell, mode, B, K, lam):
    """L_sep 1e-4 relative and every separation gradient within 2e-3 of its largest element (_compare_step's
    bars); scores rtol 1e-5 / atol 1e-6, the three D losses 1e-5 relative, g_dis, g_adv and gext within 1e-4 of
    each tensor's largest element (test_disc_api_gpu.py's).  lambda = 1 is the reference's own step; there the
    term moves the separation gradients by only a few times the bar, so the precondition is asserted at
    lambda = 20 (linear in lambda), where dropping the term cannot pass.  Seeds: SEEDS32."""
    L, N = 2, 4000
    ref = _reference(cell, mode, B, K, L, N, *SEEDS32)
    _precondition(ref, 20.0, 2e-3)
    # and every ReLU gate of the reference is decided by a margin: the gradients compared are those of one
    # and the same piecewise-linear branch
    print(f"gate margin {ref['gate_margin']:.1f} units")
    assert ref["gate_margin"] >= 8.0
    net, disc, tr = _trainer(dev, cell, mode, B, K, L, N, lam, disc_seed=SEEDS32[0])
    loss = _grad_pass(tr, _dev_batch(dev, _batch(B, K, N, SEEDS32[1])))
    tr.check()
    l = float(loss[0])
    print(f"L_sep {l} ref {ref['l_sep']}")
    assert abs(l - ref["l_sep"]) <= 1e-4 * abs(ref["l_sep"])
    errs = _sep_errs(net, _sep_grads(ref, lam))
    print("separation gradients:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 2e-3, errs
    sc = tr.adv_scores.cpu()
    print("scores max err", float((sc - ref["scores"]).abs().max()))
    assert torch.allclose(sc, ref["scores"], rtol=1e-5, atol=1e-6)
    al = tr.adv_loss.cpu().tolist()
    print("adv_loss", al, "ref", ref["losses"])
    for a, r in zip(al, ref["losses"]):
        assert abs(a - r) <= 1e-5 * abs(r)
    ed = {k: _rel(disc.view(k, disc.grad_dis), g) for k, g in ref["g_dis"].items()}
    ea = {k: _rel(disc.view(k, disc.grad_adv), lam * g) for k, g in ref["g_adv"].items()}
    ex = _rel(tr.gext, lam * ref["gext"])
    print("g_dis", {k: f"{v:.2e}" for k, v in ed.items()})
    print("g_adv", {k: f"{v:.2e}" for k, v in ea.items()}, "gext", f"{ex:.2e}")
    assert max(ed.values()) <= 1e-4 and max(ea.values()) <= 1e-4 and ex <= 1e-4


# --------------------------------------------------------------------------------------------- 4. updates
def _adam_chain(theta, grads, steps):
    """torch.optim.Adam's updates in fp64 (small_ref.adam) from the fp32 theta over ``grads`` at the step
    counts ``steps``; returns the parameters and the bound on an fp32 kernel's deviation after the chain.
    Update u's own roundings stay within small_ref.adam's single-update bar dp_u; the moment errors it
    leaves re-enter each of the n - u later updates at most at full size (m decays by beta1, v by beta2), so
    each adds at most another dp_u: the total is within sum_u (n - u + 1) dp_u <= n sum_u dp_u."""
    p, m, v = theta.double(), torch.zeros_like(theta).double(), torch.zeros_like(theta).double()
    bound = torch.zeros_like(p)
    for g, s in zip(grads, steps):
        (p, dp), (m, _), (v, _) = sr.adam(p, g, m, v, LR, 0.9, 0.999, 1e-8, s)
        bound += dp
    return p, len(steps) * bound


@pytest.mark.parametrize("both", [True, False])
def test_adv_updates(dev, both):
    """Two training steps: the Discriminator's parameters against Adam(lr 2e-4) run on the CPU over the
    trainer's own g_dis, g_adv (checked against the reference above) -- four updates at D's step counts
    1, 2, 3, 4 in the order dis, adv, dis, adv, or two with disc_adv_update=False -- within the single-update
    bound of test_adam_topk_gpu.py carried over the chain (_adam_chain).  The separation parameters after the
    first step: the explanation rule of test_step_gpu._assert_adam_params_close."""
    cell, mode, B, K, L, N, lam = "gru", "label", 2, 2, 2, 4000, 1.0
    ref = _reference(cell, mode, B, K, L, N)
    net, disc, tr = _trainer(dev, cell, mode, B, K, L, N, lam, disc_adv_update=both)
    theta0 = disc.flat.detach().cpu().clone()
    grads = []
    for i in range(2):
        tr.step(*_dev_batch(dev, _batch(B, K, N, seed=BATCH_SEED + 10 * i)))
        tr.check()
        grads.append(disc.grad_dis.detach().cpu().clone())
        if both:
            grads.append(disc.grad_adv.detach().cpu().clone())
        if i == 0:
            # the separation net after its first update, against the reference model stepped by torch Adam
            grads_ref = _sep_grads(ref, lam)
            errs = _sep_errs(net, grads_ref)
            model = om.SepModel(cell=cell, num_layers=L)
            model.load_state_dict(ref["model"].state_dict())
            opt = om.make_adam(model)
            for n, p in model.named_parameters():
                p.grad = grads_ref[n].clone()
            opt.step()
            _assert_adam_params_close(net, model, grads_ref, errs)
    n = len(grads)
    assert tr.adv_step_count == n and tr.step_count == 2
    want, bound = _adam_chain(theta0, grads, range(1, n + 1))
    err = (disc.flat.detach().cpu().double() - want).abs()
    print(f"theta_D after {n} updates: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3g}")
    assert bool((err <= bound).all())
    moved = float((want - theta0.double()).abs().max())
    assert moved > 0.5 * LR  # the chain moved D by about lr per update: a skipped update is far outside the bound


def test_adv_refused_step_leaves_discriminator_untouched(dev):
    """A step whose status word is set beforehand (a timed-out hand-off): the guarded updates refuse theta_D,
    its moments and, after check(), its step count, like the separation net's."""
    cell, mode, B, K, L, N = "gru", "label", 2, 2, 2, 4000
    net, disc, tr = _trainer(dev, cell, mode, B, K, L, N, 1.0)
    b = _dev_batch(dev, _batch(B, K, N))
    tr.step(*b)
    tr.check()
    state = [t.detach().clone() for t in (disc.flat, tr.adv_m, tr.adv_v, net.flat, tr.m, tr.v)]
    counts = (tr.adv_step_count, tr.step_count)
    assert counts == (2, 1)
    tr.status[0] = 1
    loss = tr.step(*b)
    with pytest.raises(RuntimeError, match="refused"):
        tr.check()
    assert bool(torch.isnan(loss[0]))
    for before, now in zip(state, (disc.flat, tr.adv_m, tr.adv_v, net.flat, tr.m, tr.v)):
        assert torch.equal(before, now)
    assert (tr.adv_step_count, tr.step_count) == counts
    tr.step(*b)  # and the trainer continues
    tr.check()
    assert (tr.adv_step_count, tr.step_count) == (4, 2)
    assert not torch.equal(state[0], disc.flat)


# ------------------------------------------------------------------------------------- 5. graph vs eager
@pytest.mark.parametrize("precision,mode", [("fp32", "label"), ("bf16", "pit")])
def test_adv_graph_step_matches_eager(dev, precision, mode):
    """The procedure and bars of test_step_gpu.test_graph_step_matches_eager (save state, eager step, restore,
    graph step, over three batches; loss 1e-6 relative, gradients 1e-5 of max, parameters 1e-6 absolute up to
    lr on at most 1e-4 of the elements, and bitwise on the bf16 step), applied to the separation net and
    likewise to g_dis, g_adv, theta_D and adv_loss.  The capture runs at the default hardware-queue count."""
    B, K, N = 4, 2, 8000
    gen = synth.SyntheticMixtures(n_samples=N, k=K, seed=5)
    batches = []
    for _ in range(3):
        src, spk, u = gen.batch(B)
        batches.append(_dev_batch(dev, (src, spk, synth.gains_for(u, K))))
    net = engine.SepNet(cell="lstm", num_layers=2, device=dev, seed=7)
    disc = engine.DiscNet(ops.n_frames(N), F, device=dev, seed=DISC_SEED)
    tr = engine.SepTrainer(net, B, K, N, mode=mode, precision=precision, adversary=disc, adv_weight=20.0)
    tr.step(*batches[0])  # eager warm-up step before the capture
    live = lambda: (net.flat, tr.m, tr.v, disc.flat, tr.adv_m, tr.adv_v)  # noqa: E731
    outs = lambda: [t.detach().clone() for t in (net.grad, net.flat, disc.grad_dis, disc.grad_adv, disc.flat,  # noqa: E731
                                                  tr.adv_loss)]
    for b in batches:
        state, counts = [t.detach().clone() for t in live()], (tr.step_count, tr.adv_step_count)
        le = float(tr.step(*b)[0].item())
        eager = outs()
        for t, s in zip(live(), state):
            t.copy_(s)
        tr.step_count, tr.adv_step_count = counts
        lg = float(tr.step_graph(*b)[0].item())
        tr.check()
        graph = outs()
        if precision == "bf16":
            assert lg == le and all(torch.equal(a, c) for a, c in zip(graph, eager)), (lg, le)
        assert abs(lg - le) <= 1e-6 * abs(le), (lg, le)
        for i in (0, 2, 3):  # gradients
            assert float((graph[i] - eager[i]).abs().max()) <= 1e-5 * float(eager[i].abs().max()), i
        for i in (1, 4):  # parameters
            dp = (graph[i] - eager[i]).abs()
            assert float(dp.max()) <= 2 * LR and int((dp > 1e-6).sum()) <= max(1, dp.numel() // 10000), i
        assert float(((graph[5] - eager[5]).abs() / eager[5].abs()).max()) <= 1e-6
    assert tr.adv_step_count == 2 * tr.step_count


# ------------------------------------------------------------------------------------------ 6. bf16 paths
def _disc_bf16_errors(tr, disc, lam):
    """D's scores, g_dis, g_adv: (kernel error, emulation error) per tensor against the fp64 model fed the
    kernel's own maps and ReLU gates -- the emulation rounds to bf16 where the bf16 mode stores a value
    (disc_ref.run_model(rnd=bf16r)); the bound of the bf16 Discriminator tests is kernel <= 2 x emulation."""
    N = tr.B * tr.K
    x = tr._dmaps.detach().cpu().double()
    P = {k: v.cpu().double() for k, v in disc.state_dict().items()}
    gates = [R.from_cl(y.detach().cpu().float()) > 0 for y in tr._dy]
    tgt = torch.cat([torch.ones(N, 1), torch.zeros(N, 1)]).double()
    out = {}
    runs = {rnd: (R.run_model(x, P, gates, tgt, rnd=rnd), R.run_model(x[N:], P, [g[N:] for g in gates], 1.0, rnd=rnd))
            for rnd in (R.ident, R.bf16r)}
    (ref_all, ref_fake), (emu_all, emu_fake) = runs[R.ident], runs[R.bf16r]
    out["score"] = (R.rel_err(tr.adv_scores.cpu().view(-1, 1), ref_all["score"]),
                    R.rel_err(emu_all["score"], ref_all["score"]))
    for k in R.KEYS:  # run_model's loss is the mean over its 2 N maps: L_dt + L_df is twice that
        out["g_dis/" + k] = (R.rel_err(disc.view(k, disc.grad_dis).cpu(), 2 * ref_all["g/" + k]),
                             R.rel_err(2 * emu_all["g/" + k], 2 * ref_all["g/" + k]))
        out["g_adv/" + k] = (R.rel_err(disc.view(k, disc.grad_adv).cpu(), lam * ref_fake["g/" + k]),
                             R.rel_err(lam * emu_fake["g/" + k], lam * ref_fake["g/" + k]))
    out["gext"] = (R.rel_err(tr.gext.cpu().view(N, tr.T, tr.F), lam * ref_fake["dx"]),
                   R.rel_err(lam * emu_fake["dx"], lam * ref_fake["dx"]))
    return out


BF16_CASES = [("lstm", "pit", 4, "bf16"), ("gru", "label", 2, "bf16s")]


@functools.lru_cache(maxsize=None)
def _bf16_run(cell, mode, L, precision):
    """one GPU step of a bf16 case at lambda = 100, shared by the two tests below: the figures they assert"""
    B, K, N, lam = 4, 2, 8000, 100.0
    dev = torch.device("cuda:0")
    ref = _reference(cell, mode, B, K, L, N)
    _precondition(ref, lam, 5e-2)
    net, disc, tr = _trainer(dev, cell, mode, B, K, L, N, lam, precision=precision)
    loss = _grad_pass(tr, _dev_batch(dev, _batch(B, K, N)))
    tr.check()
    out = dict(l_sep=float(loss[0]), l_ref=ref["l_sep"], sep=_sep_errs(net, _sep_grads(ref, lam)),
               disc=_disc_bf16_errors(tr, disc, lam))
    print(f"{precision} L_sep {out['l_sep']} ref {out['l_ref']}")
    print("separation gradients:", {k: f"{v:.2e}" for k, v in out["sep"].items()})
    print("discriminator (kernel, emulation):", {k: (f"{a:.2e}", f"{b:.2e}") for k, (a, b) in out["disc"].items()})
    return out


@pytest.mark.parametrize("cell,mode,L,precision", BF16_CASES)
def test_adv_step_bf16_loss_and_discriminator(dev, cell, mode, L, precision):
    """lambda = 100 (the precondition at 10 x 5e-2 holds on the reference).  L_sep within 1e-2 relative
    (test_step_bilstm_bf16's bar); D's scores, g_dis and g_adv, in the bf16 activation mode, within twice the
    error of the bf16-rounding emulation fed the kernel's own maps and gates."""
    r = _bf16_run(cell, mode, L, precision)
    assert abs(r["l_sep"] - r["l_ref"]) <= 1e-2 * abs(r["l_ref"])
    bad = {k: v for k, v in r["disc"].items() if v[0] > 2 * v[1]}
    assert not bad, bad


@pytest.mark.parametrize("cell,mode,L,precision", [
    pytest.param(*BF16_CASES[0], marks=pytest.mark.xfail(
        strict=True, reason="a bf16 Discriminator supplying the dominant gradient: 6.1e-2 of max on the first "
                            "layer > the 5e-2 bar (the plain bf16 step at this shape: 1.3e-2); figures in the "
                            "docstring and DESIGN.md section 5")),
    pytest.param(*BF16_CASES[1], marks=pytest.mark.xfail(
        strict=True, reason="a bf16 Discriminator supplying the dominant gradient: 8.2e-2 of max on the first "
                            "layer, 5.7e-2 on the Linear > the 5e-2 bar (the plain bf16s step: 3.9e-3)"))])
def test_adv_step_bf16_separation_gradients(dev, cell, mode, L, precision):
    """Every separation gradient within 5e-2 of its tensor's largest element (test_step_bilstm_bf16's bar)
    against the fp32 reference at lambda = 100, where the adversarial term supplies at least half of every
    tensor's largest element.  The bar is missed in both cases and kept: strict xfails at the measured values.

    Measured on the MI355X, error / largest element per tensor:
      (lstm, pit, L = 4, bf16): weight_ih_l0 6.12e-2, weight_hh_l0 5.87e-2, bias_*_l0 5.84e-2, bias_*_l0_reverse
        5.12e-2 miss; weight_*_l0_reverse 4.6e-2 .. 4.7e-2, layer 1 3.2e-2 .. 4.5e-2, layers 2-3 2.8e-2 .. 4.0e-2,
        Linear 2.0e-2, emb 3.5e-2, adj 2.4e-2 meet it.  The plain bf16 step (no adversary) on the same batch
        against the same reference: 1.3e-2 at most (layer 0), 2.5e-3 on the Linear.
      (gru, label, L = 2, bf16s): weight_ih_l0 8.18e-2, weight_hh_l0 7.21e-2, bias_*_l0 5.9e-2 .. 6.7e-2, layer 0
        reverse 5.0e-2 .. 5.2e-2, weight_*_l1 5.3e-2, Linear 5.6e-2 .. 5.7e-2, emb 5.9e-2 miss; the rest
        4.1e-2 .. 4.8e-2.  The plain bf16s step: 3.9e-3 at most, 1.0e-3 on the Linear.
    The error enters at the top of the backward (the Linear's own gradient carries it), i.e. with gext: the
    Discriminator's input gradient through three bf16 activation / filter roundings, at lambda = 100 more than
    half of dL/dpred.  The Discriminator's own outputs stay within the bf16-rounding emulation (scores 2.2e-4 ..
    2.9e-4, its parameter gradients 2e-3 .. 8e-3 of max, kernel and emulation alike)."""
    r = _bf16_run(cell, mode, L, precision)
    assert max(r["sep"].values()) <= 5e-2, r["sep"]


# ------------------------------------------------------------------------------- 7. no adversary, no change
def test_no_adversary_is_bitwise_the_plain_trainer(dev):
    """adversary=None: three steps give the bits -- losses, gradients, parameters -- of a trainer constructed
    without the keyword at all (the bf16 step is bitwise reproducible, test_step_bitwise_reproducible)."""
    B, K, N = 4, 2, 8000
    batches = [_dev_batch(dev, _batch(B, K, N, seed=20 + i)) for i in range(3)]
    runs = []
    for kw in ({}, dict(adversary=None)):
        net = engine.SepNet(cell="lstm", num_layers=2, device=dev, seed=7)
        tr = engine.SepTrainer(net, B, K, N, mode="pit", precision="bf16", **kw)
        rec = []
        for b in batches:
            loss = tr.step(*b)
            tr.check()
            rec.append((loss.clone(), net.grad.clone(), net.flat.clone()))
        assert tr._mag.shape[0] == B + B * K and not hasattr(tr, "gext")
        runs.append(rec)
    for a, b in zip(*runs):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
