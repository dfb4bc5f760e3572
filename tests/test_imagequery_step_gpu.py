"""The training step with image queries (SepTrainer(image_query=..., memory=...)) and enrolment at inference.
B = 3, K = 2, N = 2048 (T = 17), a 2-layer H = 40 BiLSTM mask net without ADDJUST, six distinct speakers, one
28 x 28 glyph per source (tests/test_voiceprint_step_gpu.py's shapes)."""
import numpy as np
import pytest
import torch

import voiceprint_ref as vr
from dl4ss_amd import checkpoint, engine, infer, ops, synth
from dl4ss_amd.imagequery import ImageQueryEncoder, ImageQueryNet
from dl4ss_amd.voiceprint import SpeakerMemory, unit

pytestmark = pytest.mark.gpu
B, K, N, T, F, E = 3, 2, 2048, 17, 129, 50
IDS = [[3, 17], [42, 5], [99, 61]]
GLYPHS = synth.glyphs(101)


def _batch(dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(B, K, N, generator=g)
    gains = torch.rand(B, K, generator=g) * 0.5 + 0.75
    images = torch.from_numpy(GLYPHS.draw(np.array(IDS), np.random.default_rng(seed))).view(B, K, 28, 28)
    return raw.to(dev), gains.to(dev), torch.tensor(IDS, dtype=torch.int32, device=dev), images.to(dev)


def _unit_rows(n, seed):
    x = torch.randn(n, E, generator=torch.Generator().manual_seed(seed)).double()
    return (x / x.norm(dim=1, keepdim=True)).float()


def _inet(dev):
    """Conv biases away from zero (the default initialisation's zero biases leave the flat background dead)."""
    inet = ImageQueryNet(device=dev, seed=3)
    g = torch.Generator().manual_seed(8)
    for i in (1, 2, 3):
        b = inet.view(f"img.conv{i}.bias")
        b.copy_(torch.empty(b.shape).uniform_(-0.1, 0.1, generator=g))
    return inet


def _nets(dev, attention="align", refresh="reference", **kw):
    net = engine.SepNet(cell="lstm", num_layers=2, hidden=40, adjust=False, device=dev, seed=7, attention=attention)
    inet = _inet(dev)
    memory = SpeakerMemory(101, E, device=dev)
    memory.mem[17] = _unit_rows(1, 11)[0].to(dev)  # a touched row
    memory.mem[50] = _unit_rows(1, 12)[0].to(dev)  # an untouched one
    tr = engine.SepTrainer(net, B, K, N, image_query=inet, memory=memory, memory_refresh=refresh, **kw)
    return net, inet, memory, tr


def _fwd_bwd(tr, raw, gains, spk, images):
    """step() without the optimizer"""
    tr.set_images(images)
    tr.spk.copy_(spk)
    tr.features(raw, gains, None)
    tr.forward()
    loss = tr.loss_and_grad()
    tr.backward()
    return loss


@pytest.mark.parametrize("attention", ["align", "dot"])
def test_step_equals_plain_step_on_the_same_queries(dev, attention):
    """The image step's loss, dq and mask-net gradients against a plain trainer whose embedding rows hold the
    step's queries: bitwise on 'align' (unsplit GEMMs), within test_voiceprint_step_gpu.py's fp32 bounds on 'dot'
    (split-K float atomics: loss 1e-6 relative, gradients 1e-5 of the largest element)."""
    raw, gains, spk, images = _batch(dev)
    net, inet, memory, tr = _nets(dev, attention)
    loss = _fwd_bwd(tr, raw, gains, spk, images).clone()
    tr.check()
    q = tr.q.clone()
    assert q.isfinite().all() and ((q.norm(dim=-1) - 1).abs() < 1e-5).all()
    net2 = engine.SepNet(cell="lstm", num_layers=2, hidden=40, adjust=False, device=dev, seed=7, attention=attention)
    assert torch.equal(net2.flat, net.flat)
    net2.view("emb.layer.weight")[spk.view(-1).long()] = q.view(B * K, E)
    tr2 = engine.SepTrainer(net2, B, K, N)
    tr2.spk.copy_(spk)
    tr2.features(raw, gains, None)
    tr2.forward()
    loss2 = tr2.loss_and_grad()
    tr2.backward()
    tr2.check()
    assert torch.equal(tr2.q, q)
    emb = net.offsets["emb.layer.weight"]
    keep = torch.ones_like(net.grad, dtype=torch.bool)
    keep[emb[0]:emb[0] + 101 * E] = False
    assert (net.grad[~keep] == 0).all()  # emb.layer.weight gets no gradient from an image step
    if attention == "align":
        assert torch.equal(loss, loss2) and torch.equal(tr.dq, tr2.dq)
        assert torch.equal(net.grad[keep], net2.grad[keep])
    else:
        assert abs(float(loss[0]) - float(loss2[0])) <= 1e-6 * abs(float(loss2[0]))
        assert float((tr.dq - tr2.dq).abs().max()) <= 1e-5 * float(tr2.dq.abs().max())
        assert float((net.grad[keep] - net2.grad[keep]).abs().max()) <= 1e-5 * float(net2.grad[keep].abs().max())


def test_queries_follow_the_reference_memory_arithmetic(dev):
    """q, u and dv against voiceprint_ref's fp64 memory arithmetic on the encoder's own vectors, within its bars."""
    raw, gains, spk, images = _batch(dev)
    net, inet, memory, tr = _nets(dev)
    before = memory.mem.clone()
    _fwd_bwd(tr, raw, gains, spk, images)
    tr.check()
    r = vr.memory(tr.vp_enc.vec.cpu(), spk.view(-1).cpu(), before.cpu(), dq=tr.dq.view(B * K, E).cpu())
    assert ((tr.q.view(B * K, E).double().cpu() - r["q"]).abs() <= r["bar_q"]).all()
    assert ((tr.vp.u.double().cpu() - r["u"]).abs() <= r["bar_u"]).all()
    assert ((tr.vp.dv.double().cpu() - r["dv"]).abs() <= r["bar_dv"]).all()


def test_encoder_gradients_are_the_encoder_backward(dev):
    raw, gains, spk, images = _batch(dev)
    net, inet, memory, tr = _nets(dev)
    _fwd_bwd(tr, raw, gains, spk, images)
    g1 = inet.grad.clone()
    assert g1.isfinite().all() and float(g1.abs().max()) > 0
    for name in ("img.conv1.weight", "img.conv2.bias", "img.dense.weight"):
        assert float(inet.grad_view(name).abs().max()) > 0, name
    enc = ImageQueryEncoder(inet, B * K)
    v = enc.forward(images.view(B * K, 28, 28))
    q, u = ops.spk_memory_fwd(v, spk.view(-1), memory.mem)
    assert torch.equal(q.view(B, K, E), tr.q)
    dv = ops.spk_memory_bwd(tr.dq.view(B * K, E), v, u, spk.view(-1), memory.mem)
    inet.grad.fill_(float("nan"))
    enc.backward(dv)
    assert torch.equal(inet.grad, g1)


@pytest.mark.parametrize("refresh", ["reference", "reuse"])
def test_memory_refresh(dev, refresh):
    raw, gains, spk, images = _batch(dev)
    net, inet, memory, tr = _nets(dev, refresh=refresh)
    before, w0 = memory.mem.clone(), inet.flat.clone()
    tr.step(raw, gains, spk, images=images)
    tr.check()
    assert not torch.equal(inet.flat, w0)  # the encoder trained
    ids = spk.view(-1).long()
    enc = ImageQueryEncoder(inet, B * K)
    if refresh == "reuse":
        want = tr.q.view(B * K, E)
        r = vr.memory(tr.vp_enc.vec.cpu(), spk.view(-1).cpu(), before.cpu())  # the step's own forward
        assert ((want.double().cpu() - r["q"]).abs() <= r["bar_q"]).all()
    else:  # by hand with the updated weights, from the memory as the step found it
        want, _ = ops.spk_memory_fwd(enc.forward(images.view(B * K, 28, 28)), spk.view(-1), before)
        assert not torch.equal(want, tr.q.view(B * K, E))
        # ... and that is voiceprint_ref's memory arithmetic on the re-encoded vectors
        r = vr.memory(enc.vec.cpu(), spk.view(-1).cpu(), before.cpu())
        assert ((want.double().cpu() - r["q"]).abs() <= r["bar_q"]).all()
    assert torch.equal(memory.mem[ids], want)
    rest = torch.ones(101, dtype=torch.bool, device=dev)
    rest[ids] = False
    assert torch.equal(memory.mem[rest], before[rest]) and float(memory.mem[50].abs().max()) > 0

    # a refused update stores nothing: a non-finite loss, injected by the input
    mem1, w1, nw1, n1 = memory.mem.clone(), inet.flat.clone(), net.flat.clone(), tr.step_count
    m1, v1 = tr.vp_opt.m.clone(), tr.vp_opt.v.clone()
    bad = raw.clone()
    bad[1, 0, 100] = float("nan")
    loss = tr.step(bad, gains, spk, images=images)
    assert torch.isnan(loss[0]) and torch.equal(memory.mem, mem1) and torch.equal(inet.flat, w1)
    assert torch.equal(net.flat, nw1) and torch.equal(tr.vp_opt.m, m1) and torch.equal(tr.vp_opt.v, v1)
    with pytest.raises(RuntimeError, match="non-finite loss"):
        tr.check()
    assert tr.step_count == n1 and tr.status.tolist() == [0, 0]
    # ... and the trainer goes on from there
    loss = tr.step(raw, gains, spk, images=images)
    tr.check()
    assert loss.isfinite().all() and tr.step_count == n1 + 1 and not torch.equal(inet.flat, w1)


def test_three_steps_repeat_bitwise(dev):
    out = []
    for _ in range(2):
        net, inet, memory, tr = _nets(dev)
        losses = []
        for s in range(3):
            raw, gains, spk, images = _batch(dev, seed=s + 1)
            losses.append(tr.step(raw, gains, spk, images=images).clone())
        tr.check()
        out.append((torch.stack(losses), net.flat.clone(), inet.flat.clone(), memory.mem.clone()))
    for a, b in zip(*out):
        assert a.isfinite().all() and torch.equal(a, b)


def test_graph_capture_and_missing_images_are_refused(dev):
    raw, gains, spk, images = _batch(dev)
    _, _, _, tr = _nets(dev)
    with pytest.raises(NotImplementedError):
        tr.step_graph(raw, gains, spk)
    with pytest.raises(NotImplementedError):
        tr.capture()
    with pytest.raises(ValueError, match="images="):
        tr.step(raw, gains, spk)
    net = engine.SepNet(cell="lstm", num_layers=2, hidden=40, adjust=False, device=dev, seed=7)
    with pytest.raises(ValueError, match="image_query="):
        engine.SepTrainer(net, B, K, N).step(raw, gains, spk, images=images)


@pytest.mark.parametrize("attention", ["dot", "align"])
def test_enrolment_from_images(dev, attention):
    """enrol(images) returns unit rows equal to voiceprint.unit(encoder forward); run() with them equals
    run_memory() on a memory that holds those rows."""
    net = engine.SepNet(cell="lstm", num_layers=2, hidden=40, adjust=False, device=dev, seed=7, attention=attention)
    inet = _inet(dev)
    ex = infer.EnrolledExtractor(net, inet, B, T, K)
    images = _batch(dev, seed=5)[3].view(B * K, 28, 28)
    u = ex.enrol(images)
    assert u.shape == (B * K, E) and ((u.norm(dim=1) - 1).abs() < 1e-5).all()
    enc = ImageQueryEncoder(inet, B * K)
    assert torch.equal(u, unit(enc.forward(images)))
    v = enc.vec.double()
    assert (u.double() - v / v.norm(dim=1, keepdim=True)).abs().max() < 1e-6
    g = torch.Generator().manual_seed(5)
    mix = ops.stft(torch.randn(B, N, generator=g).to(dev), complex_out=False)[1]
    masks = ex.run(mix, u.view(B, K, E)).clone()
    assert masks.isfinite().all() and float(masks.min()) >= 0 and float(masks.max()) <= 1
    memory = SpeakerMemory(101, E, device=dev)
    ids = torch.tensor(IDS, dtype=torch.int32, device=dev)
    ops.spk_memory_store(u, ids.view(-1), memory.mem)
    m2 = ex.run_memory(mix, memory, ids)
    assert float((m2 - masks).abs().max()) < 1e-5  # (the stored rows are re-normalised: test_voiceprint_step_gpu's bound)
    none = ex.queries_of(memory, torch.full((B, K), -1, dtype=torch.int32, device=dev))
    assert (none == 0).all()


def test_checkpoint_round_trip(dev, tmp_path):
    raw, gains, spk, images = _batch(dev)
    net, inet, memory, tr = _nets(dev)
    tr.step(raw, gains, spk, images=images)
    tr.check()
    p = str(tmp_path / "iq.pt")
    checkpoint.save_image_query(p, inet, memory)
    inet2, memory2 = ImageQueryNet(device=dev, seed=9), SpeakerMemory(101, E, device=dev)
    checkpoint.load_image_query(p, inet2, memory2)
    assert torch.equal(inet2.flat, inet.flat) and torch.equal(memory2.mem, memory.mem)
