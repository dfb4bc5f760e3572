"""SepTrainer(clip_norm=..., adv_clip_norm=...) and ClassifierTrainer(clip_norm=...) in the training step:
inactive (bitwise the plain trainer), active (within clip_ref's bars, eager and graph-replayed), against the
oracle with torch's clip_grad_norm_, data parallel, with a NaN in the gradient, and with an adversary.

L = 2, B = 4 (the oracle and classifier cases 2), K = 2, N = 4000 (T = 32).  Every threshold comes from the
plain trainer's own first gradient, reduced in fp64 on the host: the suite holds no fixed norm.

The bf16 steps are bitwise reproducible (test_step_bitwise_reproducible), so two trainers can be compared run
against run.  The fp32 step is not (split-K float atomics in its backward GEMMs): there the plain trainer's
gradients are recorded and written over the other trainer's at the start of its optimizer_step(), so both
optimizers see the same bits and step() / step_graph() still run in full around them.
"""
import gc
import math
import socket

import numpy as np
import pytest
import torch

import clip_ref as cr
from dl4ss_amd import classifier, engine, infer, ops, synth
from oracle import model as om
from test_step_gpu import _oracle_features, _setup

pytestmark = pytest.mark.gpu

B, K, N, L = 4, 2, 4000, 2
HP = (2e-4, 0.9, 0.999, 1e-8)
CFGS = [("fp32", "label", "lstm"), ("bf16", "pit", "lstm"), ("bf16", "pit", "gru")]
INF = float("inf")


def _dev_batches(dev, n, batch=B, seed=5):
    gen = synth.SyntheticMixtures(n_samples=N, k=K, seed=seed)
    out = []
    for _ in range(n):
        src, spk, u = gen.batch(batch)
        out.append((torch.from_numpy(src.astype(np.float32)).to(dev),
                    torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(dev),
                    torch.from_numpy(spk.astype(np.int32)).to(dev)))
    return out


def _trainer(dev, cfg, batch=B, **kw):
    precision, mode, cell = cfg
    net = engine.SepNet(cell=cell, num_layers=L, adjust=cell == "lstm", device=dev, seed=7)
    return engine.SepTrainer(net, batch, K, N, mode=mode, precision=precision, **kw)


def _grad_pass(tr, b):
    raw, gains, spk = b
    tr.spk.copy_(spk)
    tr.features(raw, gains)
    tr.forward()
    loss = tr.loss_and_grad()
    tr.backward()
    torch.cuda.synchronize()
    return loss


def _host_norm(g):
    """the L2 norm of a device gradient, reduced in fp64 on the host"""
    return math.sqrt(float((g.detach().cpu().double() ** 2).sum()))


def _first_norm(dev, cfg, b, batch=B):
    tr = _trainer(dev, cfg, batch)
    _grad_pass(tr, b)
    tr.check()
    nrm = _host_norm(tr.net.grad)
    assert math.isfinite(nrm) and nrm > 0
    return nrm


def _wb(tr):
    """the bf16 weight copies the trainer's Adam keeps (bf16 steps)"""
    return [w.clone() for w in tr.wb_ih] + [tr.wb_lin.clone()] if tr.fast else []


def _run(dev, cfg, batches, graph, record=None, inject=None, **kw):
    """Steps over the batches (graph: the first eager, the rest replayed).  Every optimizer_step() is wrapped:
    inject -- a list of grad_ext tensors written over the gradient first; the state before (gradient, parameters,
    moments) and after (grad_norm) is recorded."""
    tr = _trainer(dev, cfg, **kw)
    net, rec = tr.net, []
    real = tr.optimizer_step

    def wrapped():
        tr.wait_allreduce()
        if inject is not None:
            net.grad_ext.copy_(inject[len(rec)])
        r = dict(gext=net.grad_ext.clone(), flat=net.flat.clone(), m=tr.m.clone(), v=tr.v.clone(), step=tr.step_count + 1)
        real()
        if tr.clip_norm is not None:
            r["gnorm"] = tr.grad_norm.clone()
        rec.append(r)

    tr.optimizer_step = wrapped
    losses = []
    for i, b in enumerate(batches):
        loss = tr.step_graph(*b) if (graph and i > 0) else tr.step(*b)
        losses.append(loss.clone())
    tr.check()
    torch.cuda.synchronize()
    tr.optimizer_step = real
    return dict(tr=tr, rec=rec, loss=losses, flat=net.flat.clone(), m=tr.m.clone(), v=tr.v.clone(), wb=_wb(tr))


def _assert_same_state(a, b):
    for k in ("flat", "m", "v"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert len(a["wb"]) == len(b["wb"])
    for i, (x, y) in enumerate(zip(a["wb"], b["wb"])):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), i
    assert a["tr"].step_count == b["tr"].step_count and a["tr"].status.tolist() == [0, 0] == b["tr"].status.tolist()


def _free(*runs):
    for r in runs:
        r.clear()
    gc.collect()
    torch.cuda.empty_cache()


# ---- inactive --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: "-".join(c))
def test_inactive_clip_is_bitwise_the_plain_trainer(dev, cfg):
    """clip_norm = 2 x the first norm, and inf: three steps, eager and graph, leave flat, m, v and the bf16
    weight copies bitwise those of a clip_norm=None trainer; grad_norm holds the norm and c == 1."""
    # batches on which the plain trainer's later gradients are no larger than its first (with seed 5 the second
    # batch's norm is twice the first's); checked here on the plain trainer alone, before any clipped step
    batches = _dev_batches(dev, 3, seed=8)
    nrm = _first_norm(dev, cfg, batches[0])
    plain = _run(dev, cfg, batches, False)
    assert not hasattr(plain["tr"], "grad_norm") and plain["tr"].skipped_nonfinite == 0
    inject = [r["gext"] for r in plain["rec"]] if cfg[0] == "fp32" else None
    norms = [_host_norm(r["gext"][4:]) for r in plain["rec"]]
    assert max(norms) < 1.5 * nrm, (norms, nrm)
    for graph in (False, True):
        for thr in (2.0 * nrm, INF):
            got = _run(dev, cfg, batches, graph, inject=inject, clip_norm=thr)
            _assert_same_state(got, plain)
            for r, want in zip(got["rec"], norms):
                gn = r["gnorm"].tolist()
                assert gn[1] == 1.0 and abs(gn[0] - want) <= 2 * cr.U * want, (gn, want)
            if cfg[0] != "fp32":  # the whole step, loss included
                assert all(torch.equal(x, y) for x, y in zip(got["loss"], plain["loss"]))
            assert got["tr"].skipped_nonfinite == 0
            _free(got)


# ---- active ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: "-".join(c))
def test_active_clip_within_bars_and_graph_equals_eager(dev, cfg):
    """clip_norm = 0.5 x the first norm.  From the trainer's own gradient and its state before each update:
    grad_norm within 2 u, the moments and parameters within clip_ref's bars (first and last step); the first
    step's v is c^2 of the plain trainer's; the graph-replayed steps equal the eager ones bitwise."""
    batches = _dev_batches(dev, 3)
    nrm = _first_norm(dev, cfg, batches[0])
    thr = 0.5 * nrm
    plain = _run(dev, cfg, batches[:1], False)
    inject = None
    if cfg[0] == "fp32":  # one recorded gradient per step for both clipped runs (see the module docstring)
        probe = _run(dev, cfg, batches, False, clip_norm=thr)
        inject = [r["gext"] for r in probe["rec"]]
        inject[0] = plain["rec"][0]["gext"]
        _free(probe)
    eager = _run(dev, cfg, batches, False, inject=inject, clip_norm=thr)
    tr = eager["tr"]
    after = [(r["flat"], r["m"], r["v"]) for r in eager["rec"][1:]] + [(eager["flat"], eager["m"], eager["v"])]
    cs = []
    for i, (r, (p2, m2, v2)) in enumerate(zip(eager["rec"], after)):
        g = r["gext"][4:].cpu()
        nrm_i, c, _ = cr.clip(g, thr)
        cs.append(c)
        print(f"{cfg} step {i + 1}: norm {nrm_i:.6g} c {c:.6g} gnorm {r['gnorm'].tolist()}")
        assert c < 1.0, (i, c)
        assert cr.gnorm_close(r["gnorm"].cpu(), nrm_i, c)
        if i not in (0, len(after) - 1):
            continue
        (pr, dp), (mr, dm), (vr, dv), _ = cr.adam_clipped(r["flat"].cpu(), g, r["m"].cpu(), r["v"].cpu(), *HP,
                                                          r["step"], thr)
        for name, x, ref, bar in (("p", p2, pr, dp), ("m", m2, mr, dm), ("v", v2, vr, dv)):
            err = (x.cpu().double() - ref).abs()
            worst = float((err / bar.clamp_min(1e-300)).max())
            print(f"  {name}: max err / bar = {worst:.3g}")
            assert bool((err <= bar).all()), (name, i, worst)
    assert abs(cs[0] - 0.5) < 1e-3
    # the first step's second moment against the plain trainer's (the same gradient bits): c^2
    v_plain, v_clip = plain["v"].cpu().double(), after[0][2].cpu().double()
    nz = v_plain > 0
    assert int(nz.sum()) > 0.5 * nz.numel()
    assert float((v_clip[nz] / v_plain[nz] - cs[0] ** 2).abs().max()) <= 16 * cr.U
    assert not torch.equal(after[0][1], plain["m"])
    # eager against graph
    graph = _run(dev, cfg, batches, True, inject=inject, clip_norm=thr)
    _assert_same_state(graph, eager)
    for a, b in zip(graph["rec"], eager["rec"]):
        assert torch.equal(a["gnorm"], b["gnorm"])
    assert tr.skipped_nonfinite == 0


# ---- oracle ------------------------------------------------------------------------------------------------------------
def test_clipped_step_matches_oracle_with_clip_grad_norm(dev):
    """fp32 'label', the oracle step of test_step_gpu._compare_step with torch.nn.utils.clip_grad_norm_ between
    backward() and step().  A first Adam step is scale-invariant in the parameters, so the first moments show the
    clip: per tensor, tr.m against exp_avg within (1 - beta1) c x 2e-3 of the tensor's largest reference
    gradient (that file's gradient tolerance) plus 2e-3 relative for c itself."""
    cell, Bo, mode = "lstm", 2, "label"
    net, tr0, src, spk, gains, ref = _setup(dev, cell, L, Bo, K, N, mode)
    raw = torch.from_numpy(src.astype(np.float32)).to(dev)
    g = torch.from_numpy(gains.astype(np.float32)).to(dev)
    sp = torch.from_numpy(spk.astype(np.int32)).to(dev)
    _grad_pass(tr0, (raw, g, sp))
    thr = 0.5 * _host_norm(net.grad)
    tr = engine.SepTrainer(net, Bo, K, N, mode=mode, clip_norm=thr)
    # oracle
    feats, X, Y = _oracle_features(src, gains, False)
    opt = om.make_adam(ref)
    opt.zero_grad()
    mask, _, _, _ = ref(feats, torch.from_numpy(spk))
    loss_ref, _ = om.loss_label_ordered(mask, X, Y)
    loss_ref.backward()
    grads_ref = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    total = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), thr))
    c = min(1.0, thr / (total + 1e-6))
    assert 0.45 < c < 0.55, c
    opt.step()
    # HIP
    loss = tr.step(raw, g, sp)
    tr.check()
    lr_ = float(loss_ref.detach())
    assert abs(float(loss[0]) - lr_) <= 1e-4 * abs(lr_)
    gn = tr.grad_norm.tolist()
    print(f"oracle norm {total:.6g} c {c:.6g}; grad_norm {gn}")
    assert abs(gn[0] - total) <= 2e-3 * total and abs(gn[1] - c) <= 2e-3 * c
    b1 = HP[1]
    worst = {}
    for name, p in ref.named_parameters():
        want = opt.state[p]["exp_avg"]
        ours = net.view(name, tr.m).cpu()
        bound = (1 - b1) * c * 2e-3 * float(grads_ref[name].abs().max()) + 2e-3 * float(want.abs().max())
        worst[name] = float((ours - want).abs().max()) / bound
        # and the clip shows: the unclipped moment (1 - beta1) g misses the bound by far
        assert float(((1 - b1) * grads_ref[name] - want).abs().max()) > 10 * bound, name
    print("m error / bound:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


# ---- data parallel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS[:2], ids=lambda c: "-".join(c))
@pytest.mark.parametrize("rel", [0.5, 2.0])
def test_dp_clip_on_the_summed_gradient_equals_world1_on_the_mean(dev, cfg, rel):
    """The tr.world = 2 pattern of test_dp_scaled_adam_on_summed_half_batches_equals_full_batch_step: the SUM
    of two half-batch gradients at world 2 with clip_norm against world 1 on the pre-halved sum with the same
    clip_norm -- bitwise (x 0.5 is exact, the sum of squares scales by 1/4, its root by 1/2)."""
    from dl4ss_amd import _lib

    b = _dev_batches(dev, 1)[0]

    def half(tr, lo, hi):
        t = _trainer(dev, cfg, hi - lo) if tr is None else tr
        _grad_pass(t, tuple(x[lo:hi].contiguous() for x in b))
        _lib.call("dl4ss_status_flag", _lib.ptr(t.status), _lib.ptr(t.net.dp_flag), _lib.stream_ptr())
        torch.cuda.synchronize()
        return t.net.grad_ext.clone()

    summed = half(None, 0, B // 2) + half(None, B // 2, B)
    assert float(summed[0]) == 0.0
    mean_norm = _host_norm(summed[4:] * 0.5)
    thr = rel * mean_norm
    out = []
    for world in (2, 1):
        tr = _trainer(dev, cfg, B // 2, clip_norm=thr)
        half(tr, 0, B // 2)  # a complete step state (bf16 copies, workspaces) before the update
        tr.net.grad_ext.copy_(summed if world == 2 else summed * 0.5)
        tr.world = world
        tr.optimizer_step()
        tr.check()
        torch.cuda.synchronize()
        assert tr.step_count == 1
        out.append(dict(tr=tr, flat=tr.net.flat.clone(), m=tr.m.clone(), v=tr.v.clone(), wb=_wb(tr),
                        gnorm=tr.grad_norm.clone()))
    _assert_same_state(out[0], out[1])
    assert torch.equal(out[0]["gnorm"], out[1]["gnorm"])
    nrm, c, _ = cr.clip(summed[4:].cpu(), thr, 0.5)
    assert (c < 1.0) == (rel < 1.0) and cr.gnorm_close(out[0]["gnorm"].cpu(), nrm, c)
    assert abs(nrm - mean_norm) <= 1e-12 * nrm


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def pg(dev):
    import torch.distributed as dist

    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", device_id=dev, init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0,
                            world_size=1)
    yield dist.group.WORLD
    dist.destroy_process_group()


@pytest.mark.parametrize("buckets", ["2", "0"])
def test_rccl_world1_clipped_step_bitwise_equal_to_single_gpu(dev, pg, buckets, monkeypatch):
    """World 1 over RCCL (the all-reduce is an identity), B = 4, bf16 'pit': the pg step with clip_norm is
    bitwise the pg=None step with the same clip_norm, two buckets and flat, eager then graph-replayed."""
    monkeypatch.setenv("DL4SS_DP_BUCKETS", buckets)
    cfg = CFGS[1]
    batches = _dev_batches(dev, 3)
    thr = 0.5 * _first_norm(dev, cfg, batches[0])
    runs = []
    for group in (None, pg):
        r = _run(dev, cfg, batches, True, clip_norm=thr, process_group=group)
        assert r["tr"].buckets == (group is not None and buckets != "0")
        runs.append(r)
    _assert_same_state(runs[0], runs[1])
    for a, b in zip(runs[0]["rec"], runs[1]["rec"]):
        assert torch.equal(a["gnorm"], b["gnorm"]) and torch.equal(a["gext"], b["gext"])
        assert float(a["gnorm"][1]) < 1.0
    assert all(torch.equal(x, y) for x, y in zip(runs[0]["loss"], runs[1]["loss"]))
    _free(*runs)


# ---- non-finite --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [None, INF], ids=["active", "inf"])
def test_nan_in_the_gradient_skips_the_step(dev, thr):
    """A NaN written into one element of net.grad between backward() and optimizer_step(): nothing moves, check()
    returns, step_count is rolled back, skipped_nonfinite == 1; the next clean step is bitwise the step of a
    trainer that never saw the NaN."""
    cfg = CFGS[1]
    batches = _dev_batches(dev, 2)
    if thr is None:
        thr = 0.5 * _first_norm(dev, cfg, batches[0])
    clean = _run(dev, cfg, batches, False, clip_norm=thr)
    tr = _trainer(dev, cfg, clip_norm=thr)
    tr.step(*batches[0])
    tr.check()
    before = dict(tr=tr, flat=tr.net.flat.clone(), m=tr.m.clone(), v=tr.v.clone(), wb=_wb(tr))
    _grad_pass(tr, batches[1])
    tr.net.grad[tr.net.grad.numel() // 2] = float("nan")
    tr.optimizer_step()
    torch.cuda.synchronize()
    assert tr.step_count == 2 and tr.status.tolist() == [0, 1] and math.isnan(float(tr.loss[0]))
    now = dict(tr=tr, flat=tr.net.flat.clone(), m=tr.m.clone(), v=tr.v.clone(), wb=_wb(tr))
    for k in ("flat", "m", "v"):
        assert torch.equal(now[k], before[k]), k
    assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(now["wb"], before["wb"]))
    tr.check()  # returns: a skipped step is not an error
    assert tr.step_count == 1 and tr.skipped_nonfinite == 1 and tr.status.tolist() == [0, 0]
    assert int(tr._nonfinite.item()) == 0
    loss = tr.step(*batches[1])
    tr.check()
    assert math.isfinite(float(loss[0])) and tr.step_count == 2 and tr.skipped_nonfinite == 1
    got = dict(tr=tr, flat=tr.net.flat.clone(), m=tr.m.clone(), v=tr.v.clone(), wb=_wb(tr))
    _assert_same_state(got, clean)


# ---- adversary ---------------------------------------------------------------------------------------------------------
def _adv_trainer(dev, **kw):
    net = engine.SepNet(cell="lstm", num_layers=L, device=dev, seed=7)
    disc = engine.DiscNet(ops.n_frames(N), 129, device=dev, seed=5)
    tr = engine.SepTrainer(net, B, K, N, mode="pit", precision="bf16", adversary=disc, adv_weight=20.0, **kw)
    return net, disc, tr


def _adv_state(net, disc, tr):
    return [t.clone() for t in (net.flat, tr.m, tr.v, disc.flat, tr.adv_m, tr.adv_v)]


def test_adversary_inactive_clips_are_bitwise_the_plain_adversarial_step(dev):
    """clip_norm and adv_clip_norm at twice the first norms (and inf): three bf16 steps bitwise the plain
    adversarial trainer's -- the separation net, the Discriminator and both Adam states."""
    batches = _dev_batches(dev, 3)
    net, disc, tr = _adv_trainer(dev)
    _grad_pass(tr, batches[0])
    n_sep, n_dis, n_adv = _host_norm(net.grad), _host_norm(disc.grad_dis), _host_norm(disc.grad_adv)
    runs = []
    for kw in ({}, dict(clip_norm=4 * n_sep, adv_clip_norm=4 * max(n_dis, n_adv)), dict(clip_norm=INF, adv_clip_norm=INF)):
        net, disc, tr = _adv_trainer(dev, **kw)
        losses = [tr.step(*b).clone() for b in batches]
        tr.check()
        assert tr.step_count == 3 and tr.adv_step_count == 6
        if kw:
            gn = tr.adv_grad_norm.cpu()
            assert gn[:, 1].tolist() == [1.0, 1.0] and bool((gn[:, 0] > 0).all()) and float(tr.grad_norm[1]) == 1.0
        runs.append((losses, _adv_state(net, disc, tr)))
    for losses, state in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(losses, runs[0][0]))
        for i, (a, b) in enumerate(zip(state, runs[0][1])):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i


def test_adv_clip_norm_clips_the_discriminator_update(dev):
    """adv_clip_norm = 0.5 x the norm of grad_dis, disc_adv_update=False (one Discriminator update per step):
    adv_grad_norm within 2 u, adv_m, adv_v and the Discriminator's parameters within clip_ref's bars from its
    own gradient; a NaN in grad_dis skips that update alone and check() accounts for it."""
    b = _dev_batches(dev, 1)[0]
    net, disc, tr = _adv_trainer(dev, disc_adv_update=False)
    _grad_pass(tr, b)
    thr = 0.5 * _host_norm(disc.grad_dis)
    net, disc, tr = _adv_trainer(dev, disc_adv_update=False, adv_clip_norm=thr)
    p0 = disc.flat.clone().cpu()
    lr = tr.adv_lr
    tr.step(*b)
    tr.check()
    g = disc.grad_dis.cpu()
    z = torch.zeros_like(p0)
    (pr, dp), (mr, dm), (vr, dv), (nrm, c, _) = cr.adam_clipped(p0, g, z, z, lr, *HP[1:], 1, thr)
    assert abs(c - 0.5) < 1e-3 and cr.gnorm_close(tr.adv_grad_norm[0].cpu(), nrm, c)
    assert tr.adv_grad_norm[1].tolist() == [0.0, 0.0]  # no second update
    for name, x, ref, bar in (("p", disc.flat, pr, dp), ("m", tr.adv_m, mr, dm), ("v", tr.adv_v, vr, dv)):
        err = (x.cpu().double() - ref).abs()
        worst = float((err / bar.clamp_min(1e-300)).max())
        print(f"discriminator {name}: max err / bar = {worst:.3g}")
        assert bool((err <= bar).all()), (name, worst)
    assert tr.adv_step_count == 1 and tr.step_count == 1 and not hasattr(tr, "grad_norm")
    # a NaN in the Discriminator's gradient: its update is skipped, the separation net's is applied
    state = _adv_state(net, disc, tr)
    _grad_pass(tr, b)
    disc.grad_dis[7] = float("nan")
    tr.optimizer_step()
    tr.check()
    assert tr.adv_step_count == 1 and tr.adv_skipped_nonfinite == 1 and tr.step_count == 2 and tr.skipped_nonfinite == 0
    now = _adv_state(net, disc, tr)
    assert all(torch.equal(a, b_) for a, b_ in zip(now[3:], state[3:]))
    assert not torch.equal(now[0], state[0])


# ---- the classifier ----------------------------------------------------------------------------------------------------
def _cls(dev, **kw):
    from test_classifier_train_gpu import LR, N_LAB, _batch

    H, Lc, Bc, Nc = 40, 2, 3, 3000  # the smallest net of test_classifier_train_gpu.py
    cnet = infer.ClassifierNet(hidden=H, num_layers=Lc, num_labels=N_LAB, device=dev, seed=3)
    tr = classifier.ClassifierTrainer(cnet, Bc, 2, Nc, precision="fp32", lr=LR, **kw)
    batch = tuple(torch.from_numpy(a).to(dev) for a in _batch(Bc, 2, Nc, 3))
    return cnet, tr, batch, LR


def test_classifier_trainer_clip(dev):
    """ClassifierTrainer(clip_norm=...) on the smallest net of test_classifier_train_gpu.py (its step repeats bit
    for bit): inactive bitwise the plain trainer over three steps, active within clip_ref's bars, a NaN skipped."""
    cnet, tr, batch, lr = _cls(dev)
    plain = []
    for _ in range(3):
        tr.step(*batch)
        plain.append((cnet.grad.clone(), cnet.flat.clone(), tr.m.clone(), tr.v.clone()))
    tr.check()
    nrm = _host_norm(plain[0][0])
    assert max(_host_norm(p[0]) for p in plain) < 1.9 * nrm
    for thr in (2 * nrm, INF):
        cnet2, tr2, _, _ = _cls(dev, clip_norm=thr)
        for want in plain:
            tr2.step(*batch)
            assert float(tr2.grad_norm[1]) == 1.0
            assert abs(float(tr2.grad_norm[0]) - _host_norm(want[0])) <= 2 * cr.U * _host_norm(want[0])
            for a, b in zip((cnet2.grad, cnet2.flat, tr2.m, tr2.v), want):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        tr2.check()
        assert tr2.step_count == 3 and tr2.skipped_nonfinite == 0
    # active
    thr = 0.5 * nrm
    cnet3, tr3, _, _ = _cls(dev, clip_norm=thr)
    p0 = cnet3.flat.clone().cpu()
    tr3.step(*batch)
    tr3.check()
    g = cnet3.grad.cpu()
    assert torch.equal(g, plain[0][0].cpu())
    z = torch.zeros_like(p0)
    (pr, dp), (mr, dm), (vr, dv), (n3, c, _) = cr.adam_clipped(p0, g, z, z, lr, *HP[1:], 1, thr)
    assert abs(c - 0.5) < 1e-3 and cr.gnorm_close(tr3.grad_norm.cpu(), n3, c)
    for name, x, ref, bar in (("p", cnet3.flat, pr, dp), ("m", tr3.m, mr, dm), ("v", tr3.v, vr, dv)):
        err = (x.cpu().double() - ref).abs()
        assert bool((err <= bar).all()), (name, float((err / bar.clamp_min(1e-300)).max()))
    assert not torch.equal(tr3.m, plain[0][2])
    # a NaN between backward() and optimizer_step()
    state = (cnet3.flat.clone(), tr3.m.clone(), tr3.v.clone())
    tr3.features(*batch[:2])
    tr3.forward()
    tr3.loss_and_grad(batch[2])
    tr3.backward()
    cnet3.grad[3] = float("nan")
    tr3.optimizer_step()
    torch.cuda.synchronize()
    assert tr3.step_count == 2 and math.isnan(float(tr3.loss[0]))
    tr3.check()
    assert tr3.step_count == 1 and tr3.skipped_nonfinite == 1 and tr3.status.tolist() == [0, 0]
    for a, b in zip((cnet3.flat, tr3.m, tr3.v), state):
        assert torch.equal(a, b)
    loss = tr3.step(*batch)
    tr3.check()
    assert math.isfinite(float(loss[0])) and tr3.step_count == 2
