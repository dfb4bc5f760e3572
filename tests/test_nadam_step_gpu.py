"""SepTrainer / ClassifierTrainer(optimizer="nadam", clipnorm=...) and compat.optim.Nadam in the training step.

L = 2, B = 4, K = 2, N = 4000 (T = 32), test_clip_step_gpu.py's shapes and helpers; the voiceprint and image-query
steps at their own tests' shape (B = 3, K = 2, N = 2048, H = 40).  Every reference is tests/nadam_ref.py applied to
the trainer's OWN gradient, parameters and moments read back before the update: what is checked is the plumbing,
the schedule advancing with the count and the clip, not the gradient (covered elsewhere).  As in
test_clip_step_gpu.py the fp32 step's gradients (float atomics) are recorded once and written over the other
run's at the start of its optimizer_step(), so that two runs can be compared bit for bit."""
import math

import pytest
import torch

import clip_ref as cr
import nadam_ref as nr
import test_imagequery_step_gpu as tiq
import test_voiceprint_step_gpu as tvp
from dl4ss_amd import _lib, ops
from dl4ss_amd.compat import optim as compat_optim
from test_clip_step_gpu import (B, CFGS, _assert_same_state, _cls, _dev_batches, _first_norm, _free, _grad_pass,
                                _host_norm, _trainer, _wb)

pytestmark = pytest.mark.gpu

HP = (2e-4, 0.9, 0.999, 1e-8)  # the trainers' defaults
IDS = lambda c: "-".join(c)


def _run(dev, cfg, batches, graph, inject=None, **kw):
    """test_clip_step_gpu._run, for any optimizer: steps over the batches (graph: the first eager, the rest
    replayed), the state before every update recorded and ``inject`` written over the gradient first."""
    tr = _trainer(dev, cfg, **kw)
    net, rec = tr.net, []
    real = tr.optimizer_step

    def wrapped():
        tr.wait_allreduce()
        if inject is not None:
            net.grad_ext.copy_(inject[len(rec)])
        r = dict(gext=net.grad_ext.clone(), flat=net.flat.clone(), m=tr.m.clone(), v=tr.v.clone(), step=tr.step_count + 1)
        real()
        if tr.opt.clip is not None:
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


def _after(run):
    return [(r["flat"], r["m"], r["v"]) for r in run["rec"][1:]] + [(run["flat"], run["m"], run["v"])]


def _within(got, refs, what):
    for name, x, (ref, bar) in zip("pmv", got, refs):
        err = (x.cpu().double() - ref).abs()
        worst = float((err / bar.clamp_min(1e-300)).max())
        print(f"  {what} {name}: max err / bar = {worst:.3g}")
        assert bool(torch.isfinite(x).all()) and bool((err <= bar).all()), (what, name, worst)


# ---- three steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS, ids=IDS)
def test_three_nadam_steps_follow_the_reference_and_graph_equals_eager(dev, cfg):
    batches = _dev_batches(dev, 3)
    eager = _run(dev, cfg, batches, False, optimizer="nadam")
    tr = eager["tr"]
    assert tr.step_count == 3 and tr.opt.kind == "nadam" and not hasattr(tr, "grad_norm")
    for i, (r, got) in enumerate(zip(eager["rec"], _after(eager))):
        assert r["step"] == i + 1
        refs = nr.nadam(r["flat"].cpu(), r["gext"][4:].cpu(), r["m"].cpu(), r["v"].cpu(), *HP, r["step"])
        _within(got, refs, f"{cfg} step {i + 1}")
        assert not torch.equal(got[0], r["flat"])
    # the schedule advanced: the third update evaluated at the first step's scalars misses the bars
    r, got = eager["rec"][2], _after(eager)[2]
    (p1, _), _, _ = nr.nadam(r["flat"].cpu(), r["gext"][4:].cpu(), r["m"].cpu(), r["v"].cpu(), *HP, 1)
    (_, dp), _, _ = nr.nadam(r["flat"].cpu(), r["gext"][4:].cpu(), r["m"].cpu(), r["v"].cpu(), *HP, 3)
    assert float(((got[0].cpu().double() - p1).abs() > dp).double().mean()) > 0.25
    # step_graph() is bitwise step()
    inject = [x["gext"] for x in eager["rec"]] if cfg[0] == "fp32" else None
    graph = _run(dev, cfg, batches, True, inject=inject, optimizer="nadam")
    if inject is not None:
        _free(eager)
        eager = _run(dev, cfg, batches, False, inject=inject, optimizer="nadam")
    _assert_same_state(graph, eager)
    if cfg[0] != "fp32":
        assert all(torch.equal(x, y) for x, y in zip(graph["loss"], eager["loss"]))
        # the bf16 copies are current after the update: the next forward equals one after a forced conversion
        tr = graph["tr"]
        assert tr._shadow_on and not tr._wb_stale()
        kept = _wb(tr)
        a = _grad_pass(tr, batches[0]).clone()
        tr._weights_to_bf16(force=True)
        torch.cuda.synchronize()
        assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(kept, _wb(tr)))
        assert torch.equal(a, _grad_pass(tr, batches[0]))
        tr.check()


@pytest.mark.parametrize("cfg", CFGS[:2], ids=IDS)
def test_default_optimizer_is_bitwise_the_adam_trainer(dev, cfg):
    batches = _dev_batches(dev, 3)
    plain = _run(dev, cfg, batches, False)
    assert plain["tr"].opt.kind == "adam" and plain["tr"].optimizer == "adam"
    inject = [r["gext"] for r in plain["rec"]] if cfg[0] == "fp32" else None
    named = _run(dev, cfg, batches, False, inject=inject, optimizer="adam", schedule_decay=0.5)
    _assert_same_state(named, plain)
    nadam = _run(dev, cfg, batches[:1], False, inject=inject, optimizer="nadam")
    assert not torch.equal(nadam["flat"], plain["rec"][1]["flat"])


# ---- clipnorm -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS, ids=IDS)
def test_clipnorm_inactive_is_bitwise_plain_nadam_and_active_is_within_bars(dev, cfg):
    batches = _dev_batches(dev, 3, seed=8)  # (later gradients no larger than 1.5 x the first: test_clip_step_gpu.py)
    nrm = _first_norm(dev, cfg, batches[0])
    plain = _run(dev, cfg, batches, False, optimizer="nadam")
    inject = [r["gext"] for r in plain["rec"]] if cfg[0] == "fp32" else None
    norms = [_host_norm(r["gext"][4:]) for r in plain["rec"]]
    assert max(norms) < 1.9 * nrm, (norms, nrm)
    for graph, thr in ((False, 2.0 * nrm), (True, float("inf"))):
        got = _run(dev, cfg, batches, graph, inject=inject, optimizer="nadam", clipnorm=thr)
        _assert_same_state(got, plain)
        for r, want in zip(got["rec"], norms):
            gn = r["gnorm"].tolist()
            assert gn[1] == 1.0 and abs(gn[0] - want) <= 2 * cr.U * want, (gn, want)
        assert got["tr"].skipped_nonfinite == 0
        _free(got)
    thr = 0.5 * min(norms)
    eager = _run(dev, cfg, batches, False, inject=inject, optimizer="nadam", clipnorm=thr)
    for i, (r, got) in enumerate(zip(eager["rec"], _after(eager))):
        g = r["gext"][4:].cpu()
        *refs, (nrm_i, c, _) = nr.nadam_clipped(r["flat"].cpu(), g, r["m"].cpu(), r["v"].cpu(), *HP, r["step"], thr)
        print(f"{cfg} step {i + 1}: norm {nrm_i:.6g} c {c:.6g} gnorm {r['gnorm'].tolist()}")
        assert (i > 0 or c <= 0.5 + 1e-3) and cr.gnorm_close(r["gnorm"].cpu(), nrm_i, c)
        _within(got, refs, f"clipped step {i + 1}")
    assert eager["tr"].step_count == 3 and eager["tr"].skipped_nonfinite == 0
    assert eager["tr"].grad_norm is eager["tr"].opt.grad_norm


def test_clipnorm_with_adam_goes_through_the_keras_rule(dev):
    """optimizer="adam" with clipnorm: Adam's update (clip_ref's bars; at half the norm the two rules' coefficients
    differ by the + 1e-6 alone, far inside them) with grad_norm holding Keras's coefficient, clip_norm unset."""
    cfg = CFGS[1]
    b = _dev_batches(dev, 1)
    thr = 0.5 * _first_norm(dev, cfg, b[0])
    run = _run(dev, cfg, b, False, clipnorm=thr)
    tr, r = run["tr"], run["rec"][0]
    g = r["gext"][4:].cpu()
    nrm, c, _ = nr.keras_clip(g, thr)
    assert abs(c - 0.5) < 1e-3 and cr.gnorm_close(r["gnorm"].cpu(), nrm, c)
    assert tr.opt.kind == "adam" and tr.clip_norm is None and tr.clipnorm == thr and tr.opt.clipnorm == thr
    (pr, dp), (mr, dm), (vr, dv), _ = cr.adam_clipped(r["flat"].cpu(), g, r["m"].cpu(), r["v"].cpu(), *HP, 1, thr)
    _within((run["flat"], run["m"], run["v"]), ((pr, dp), (mr, dm), (vr, dv)), "adam + clipnorm")


# ---- data parallel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS, ids=IDS)
def test_dp_nadam_on_summed_half_batches_equals_full_batch_step(dev, cfg):
    """test_step_gpu.py's data-parallel arithmetic for Nadam: the SUM of two half-batch gradients at world 2
    (gscale 1/2), with clipnorm active, against
      - world 1 on the pre-halved sum: bitwise (x 0.5 is exact);
      - the reference at gscale 0.5: within the bars;
      - the full-batch step at world 1, with that file's bounds: the mean gradient and the first moment within
        1e-5 (fp32) / 1e-3 (bf16) of the largest element; a first Nadam step moves a weight by
        (a1 + (1 - b1) a2) sign(g) whatever the gradient's scale, so two such steps differ by at most twice that
        (2.1 x allowed) and only where g is at rounding level;
    and a peer's flag refuses the update."""
    b = _dev_batches(dev, 1)[0]

    def half(tr, lo, hi):
        t = _trainer(dev, cfg, hi - lo) if tr is None else tr
        _grad_pass(t, tuple(x[lo:hi].contiguous() for x in b))
        _lib.call("dl4ss_status_flag", _lib.ptr(t.status), _lib.ptr(t.net.dp_flag), _lib.stream_ptr())
        torch.cuda.synchronize()
        return t.net.grad_ext.clone()

    summed = half(None, 0, B // 2) + half(None, B // 2, B)
    assert float(summed[0]) == 0.0
    thr = 0.5 * _host_norm(summed[4:] * 0.5)
    out = []
    for world in (2, 1):
        tr = _trainer(dev, cfg, B // 2, optimizer="nadam", clipnorm=thr)
        half(tr, 0, B // 2)
        p0 = tr.net.flat.clone().cpu()
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
    z = torch.zeros_like(p0)
    *refs, (nrm, c, _) = nr.nadam_clipped(p0, summed[4:].cpu(), z, z, *HP, 1, thr, gscale=0.5)
    assert abs(c - 0.5) < 1e-3 and cr.gnorm_close(out[0]["gnorm"].cpu(), nrm, c)
    _within((out[0]["flat"], out[0]["m"], out[0]["v"]), refs, f"{cfg} world 2")
    # the full-batch step at world 1
    trf = _trainer(dev, cfg, B, optimizer="nadam", clipnorm=thr)
    _grad_pass(trf, b)
    gf = trf.net.grad.clone()
    trf.optimizer_step()
    trf.check()
    torch.cuda.synchronize()
    tol = 1e-5 if cfg[0] == "fp32" else 1e-3
    mean = 0.5 * summed[4:]
    assert float((mean - gf).abs().max() / gf.abs().max()) < tol
    assert float((out[0]["m"] - trf.m).abs().max() / trf.m.abs().max()) < tol
    a1, a2, _ = nr.scalars(*HP[:3], 1)
    dpar = (out[0]["flat"] - trf.net.flat).abs()
    assert float(dpar.max()) <= 2.1 * (a1 + (1.0 - nr.f32(HP[1])) * a2)
    flip = dpar > 1e-6
    tiny = gf.abs() <= tol * gf.abs().max()
    assert bool(tiny[flip].all()), int((flip & ~tiny).sum())
    assert cr.gnorm_close(trf.grad_norm.cpu(), *nr.keras_clip(gf.cpu(), thr)[:2])
    # a peer's flag refuses the update (dp_flag), counted once
    tr = out[0]["tr"]
    tr.net.grad_ext.copy_(summed)
    tr.net.grad_ext[0] = 1.0
    tr.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(tr.net.flat, out[0]["flat"]) and torch.equal(tr.m, out[0]["m"]) and int(tr.status[1]) == 1
    with pytest.raises(RuntimeError, match="peer"):
        tr.check()
    assert tr.step_count == 1


# ---- the classifier -------------------------------------------------------------------------------------------------
def test_classifier_trainer_nadam_with_clipnorm(dev):
    cnet, tr, batch, lr = _cls(dev)
    tr.step(*batch)
    tr.check()
    nrm = _host_norm(cnet.grad)
    thr = 0.5 * nrm
    cnet2, tr2, _, _ = _cls(dev, optimizer="nadam", clipnorm=thr)
    state = []
    for step in (1, 2):
        p0, m0, v0 = cnet2.flat.clone().cpu(), tr2.m.clone().cpu(), tr2.v.clone().cpu()
        tr2.step(*batch)
        tr2.check()
        g = cnet2.grad.cpu()
        *refs, (n2, c, _) = nr.nadam_clipped(p0, g, m0, v0, lr, *HP[1:], step, thr)
        assert (c < 0.51 or step > 1) and cr.gnorm_close(tr2.grad_norm.cpu(), n2, c)
        _within((cnet2.flat, tr2.m, tr2.v), refs, f"classifier step {step}")
        state.append(cnet2.flat.clone())
    assert tr2.step_count == 2 and tr2.skipped_nonfinite == 0 and not torch.equal(state[0], state[1])
    # a NaN between backward() and optimizer_step(): counted and skipped as with clip_norm, no raise
    tr2.features(*batch[:2])
    tr2.forward()
    tr2.loss_and_grad(batch[2])
    tr2.backward()
    cnet2.grad[3] = float("nan")
    tr2.optimizer_step()
    torch.cuda.synchronize()
    assert tr2.step_count == 3 and math.isnan(float(tr2.loss[0])) and torch.equal(cnet2.flat, state[1])
    tr2.check()
    assert tr2.step_count == 2 and tr2.skipped_nonfinite == 1 and tr2.status.tolist() == [0, 0]


# ---- the joint norm -------------------------------------------------------------------------------------------------
def _query_step(dev, which, **kw):
    mod = tvp if which == "voiceprint" else tiq
    net, enc_net, memory, tr = mod._nets(dev, attention="dot", **kw)
    return mod, net, enc_net, memory, tr, mod._batch(dev)


def _snap(tr, memory):
    return dict(p=tr.net.flat.clone(), m=tr.m.clone(), v=tr.v.clone(), ep=tr.vp.net.flat.clone(),
                em=tr.vp.opt.m.clone(), ev=tr.vp.opt.v.clone(), mem=memory.mem.clone())


@pytest.mark.parametrize("which", ["voiceprint", "image_query"])
def test_joint_clipnorm_over_the_net_and_the_query_encoder(dev, which):
    mod, net, enc_net, memory, tr, batch = _query_step(dev, which, optimizer="nadam", clipnorm=1.0)
    mod._fwd_bwd(tr, *batch)
    torch.cuda.synchronize()
    joint0 = math.sqrt(_host_norm(net.grad) ** 2 + _host_norm(enc_net.grad) ** 2)
    assert _host_norm(enc_net.grad) > 1e-3 * joint0  # both gradients count
    thr = 0.5 * joint0
    mod, net, enc_net, memory, tr, batch = _query_step(dev, which, optimizer="nadam", clipnorm=thr)
    assert tr.opt.joint and tr.vp.opt.kind == "nadam"
    for step in (1, 2):  # the encoder steps with the net's count: its second update is at step 2 as well
        mod._fwd_bwd(tr, *batch)
        torch.cuda.synchronize()
        s = _snap(tr, memory)
        g, ge = net.grad.clone().cpu(), enc_net.grad.clone().cpu()
        tr.optimizer_step()
        tr.check()
        nrm, c, _ = nr.keras_clip([g, ge], thr)
        assert c < 0.51 or step > 1
        assert cr.gnorm_close(tr.grad_norm.cpu(), nrm, c) and cr.gnorm_close(tr.vp.opt.grad_norm.cpu(), nrm, c)
        assert torch.equal(tr.grad_norm.view(torch.int32), tr.vp.opt.grad_norm.view(torch.int32))
        *refs, _ = nr.nadam_clipped(s["p"].cpu(), g, s["m"].cpu(), s["v"].cpu(), *HP, step, thr, joint=[g, ge])
        _within((net.flat, tr.m, tr.v), refs, f"{which} net step {step}")
        *refs, _ = nr.nadam_clipped(s["ep"].cpu(), ge, s["em"].cpu(), s["ev"].cpu(), *HP, step, thr, joint=[g, ge])
        _within((enc_net.flat, tr.vp.opt.m, tr.vp.opt.v), refs, f"{which} encoder step {step}")
        assert tr.step_count == step and tr.vp.opt.step_count == 0
        assert not torch.equal(memory.mem, s["mem"])
    # a NaN in the encoder's gradient: no parameter, moment or memory row changes, the bit is set and stays
    mod._fwd_bwd(tr, *batch)
    enc_net.grad[3] = float("nan")
    s = _snap(tr, memory)
    tr.optimizer_step()
    torch.cuda.synchronize()
    after = _snap(tr, memory)
    for k in s:
        assert torch.equal(s[k].view(torch.int32), after[k].view(torch.int32)), k
    assert tr.status.tolist() == [ops.STATUS_NONFINITE_GRAD, 2] and int(tr.opt.nonfinite) == 1
    assert tr.step_count == 3 and math.isnan(float(tr.loss[0]))
    with pytest.raises(RuntimeError, match="non-finite gradient"):
        tr.check()
    assert tr.step_count == 2 and tr.skipped_nonfinite == 1 and tr.status.tolist() == [0, 0]
    assert int(tr.opt.nonfinite) == 0 and tr.vp.opt.step_count == 0
    tr.step(*batch[:3], **(dict(images=batch[3]) if which == "image_query" else {}))  # the following step trains
    tr.check()
    assert tr.step_count == 3 and not torch.equal(net.flat, s["p"]) and not torch.equal(enc_net.flat, s["ep"])
    assert not torch.equal(memory.mem, s["mem"])


# ---- the drivers' optimizer -----------------------------------------------------------------------------------------
def test_compat_nadam_on_three_parameters(dev):
    hp = (0.002, 0.9, 0.999, 1e-8)
    gen = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter(torch.randn(*s, generator=gen).to(dev)) for s in ((5,), (3, 7), (1027,))]
    unused = torch.nn.Parameter(torch.ones(4, device=dev))  # no gradient: skipped, and out of the norm
    grads = [[0.1 * torch.randn(*p.shape, generator=gen) for p in params] for _ in range(2)]
    thr = 0.5 * math.sqrt(sum(cr.sumsq(g) for g in grads[0]))
    opt = compat_optim.Nadam([{"params": params[:2] + [unused]}, {"params": params[2:]}], clipnorm=thr)
    for step, gs in enumerate(grads, 1):
        before = [(p.detach().clone().cpu(),) + tuple(opt.state[p][k].clone().cpu() if p in opt.state else
                                                      torch.zeros(p.shape) for k in "mv") for p in params]
        for p, g in zip(params, gs):
            p.grad = g.to(dev)
        opt.step()
        torch.cuda.synchronize()
        nrm, c, _ = nr.keras_clip(gs, thr)
        assert c < 1.0 and cr.gnorm_close(opt.grad_norm.cpu(), nrm, c)
        for p, g, (p0, m0, v0) in zip(params, gs, before):
            *refs, _ = nr.nadam_clipped(p0.reshape(-1), g.reshape(-1), m0.reshape(-1), v0.reshape(-1), *hp, step, thr,
                                        joint=gs)
            st = opt.state[p]
            _within((p.detach().reshape(-1), st["m"].reshape(-1), st["v"].reshape(-1)), refs,
                    f"compat step {step} {tuple(p.shape)}")
    assert opt.step_count == 2 and unused not in opt.state and torch.equal(unused.detach().cpu(), torch.ones(4))
    # a step whose global norm is not finite changes nothing; settle() takes it back out of the count
    kept = [p.detach().clone() for p in params]
    for p, g in zip(params, grads[0]):
        p.grad = g.to(dev)
    params[0].grad[1] = float("nan")
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(p.detach(), k) for p, k in zip(params, kept)) and opt.step_count == 3
    assert int(opt.nonfinite) == 3 and opt.settle() == 1
    assert (opt.step_count, opt.skipped_nonfinite, int(opt.nonfinite)) == (2, 1, 0) and opt.settle() == 0
    opt.zero_grad()
    assert all(p.grad is None for p in params)
