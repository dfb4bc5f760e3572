"""The training step with voiceprint queries (SepTrainer(voiceprint=..., memory=...)) and enrolment at inference.
B = 3, K = 2, N = 2048 (T = 17), a 2-layer H = 40 BiLSTM mask net without ADDJUST, six distinct speakers."""
import numpy as np
import pytest
import torch

from dl4ss_amd import engine, infer, ops
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintEncoder, VoiceprintNet

pytestmark = pytest.mark.gpu
B, K, N, T, F, E = 3, 2, 2048, 17, 129, 50
IDS = [[3, 17], [42, 5], [99, 61]]


def _batch(dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(B, K, N, generator=g)
    gains = torch.rand(B, K, generator=g) * 0.5 + 0.75
    return raw.to(dev), gains.to(dev), torch.tensor(IDS, dtype=torch.int32, device=dev)


def _unit_rows(n, seed):
    x = torch.randn(n, E, generator=torch.Generator().manual_seed(seed)).double()
    return (x / x.norm(dim=1, keepdim=True)).float()


def _nets(dev, attention="align", refresh="reference", **kw):
    net = engine.SepNet(cell="lstm", num_layers=2, hidden=40, adjust=False, device=dev, seed=7, attention=attention)
    vnet = VoiceprintNet(device=dev, seed=3)
    memory = SpeakerMemory(101, E, device=dev)
    memory.mem[17] = _unit_rows(1, 11)[0].to(dev)  # a touched row
    memory.mem[50] = _unit_rows(1, 12)[0].to(dev)  # an untouched one
    tr = engine.SepTrainer(net, B, K, N, voiceprint=vnet, memory=memory, memory_refresh=refresh, **kw)
    return net, vnet, memory, tr


def _fwd_bwd(tr, raw, gains, spk, lengths=None):
    """step() without the optimizer"""
    tr.spk.copy_(spk)
    tr.features(raw, gains, lengths)
    tr.forward()
    loss = tr.loss_and_grad()
    tr.backward()
    return loss


@pytest.mark.parametrize("attention", ["align", "dot"])
def test_step_equals_plain_step_on_the_same_queries(dev, attention):
    """The voiceprint step's loss, dq and mask-net gradients against a plain trainer whose embedding rows hold
    the step's queries: bitwise on 'align' (unsplit GEMMs), within test_step_gpu.py's fp32 bounds on 'dot'
    (split-K float atomics: loss 1e-6 relative, gradients 1e-5 of the largest element)."""
    raw, gains, spk = _batch(dev)
    net, vnet, memory, tr = _nets(dev, attention)
    loss = _fwd_bwd(tr, raw, gains, spk).clone()
    tr.check()
    q = tr.q.clone()
    assert q.isfinite().all() and ((q.norm(dim=-1) - 1).abs() < 1e-5).all()
    net2 = engine.SepNet(cell="lstm", num_layers=2, hidden=40, adjust=False, device=dev, seed=7, attention=attention)
    assert torch.equal(net2.flat, net.flat)
    net2.view("emb.layer.weight")[spk.view(-1).long()] = q.view(B * K, E)
    tr2 = engine.SepTrainer(net2, B, K, N)
    loss2 = _fwd_bwd(tr2, raw, gains, spk)
    tr2.check()
    assert torch.equal(tr2.q, q)
    emb = net.offsets["emb.layer.weight"]
    keep = torch.ones_like(net.grad, dtype=torch.bool)
    keep[emb[0]:emb[0] + 101 * E] = False
    assert (net.grad[~keep] == 0).all()  # emb.layer.weight gets no gradient from a voiceprint step
    if attention == "align":
        assert torch.equal(loss, loss2) and torch.equal(tr.dq, tr2.dq)
        assert torch.equal(net.grad[keep], net2.grad[keep])
    else:
        assert abs(float(loss[0]) - float(loss2[0])) <= 1e-6 * abs(float(loss2[0]))
        assert float((tr.dq - tr2.dq).abs().max()) <= 1e-5 * float(tr2.dq.abs().max())
        assert float((net.grad[keep] - net2.grad[keep]).abs().max()) <= 1e-5 * float(net2.grad[keep].abs().max())


def test_encoder_gradients_are_the_encoder_backward(dev):
    raw, gains, spk = _batch(dev)
    net, vnet, memory, tr = _nets(dev)
    _fwd_bwd(tr, raw, gains, spk)
    g1 = vnet.grad.clone()
    assert g1.isfinite().all() and float(g1.abs().max()) > 0
    enc = VoiceprintEncoder(vnet, B * K, T)
    v = enc.forward(tr.mag_src.view(B * K, T, F))
    q, u = ops.spk_memory_fwd(v, spk.view(-1), memory.mem)
    assert torch.equal(q.view(B, K, E), tr.q)
    dv = ops.spk_memory_bwd(tr.dq.view(B * K, E), v, u, spk.view(-1), memory.mem)
    vnet.grad.fill_(float("nan"))
    enc.backward(dv)
    assert torch.equal(vnet.grad, g1)


@pytest.mark.parametrize("refresh", ["reference", "reuse"])
def test_memory_refresh(dev, refresh):
    raw, gains, spk = _batch(dev)
    net, vnet, memory, tr = _nets(dev, refresh=refresh)
    before, w0 = memory.mem.clone(), vnet.flat.clone()
    tr.step(raw, gains, spk)
    tr.check()
    assert not torch.equal(vnet.flat, w0)  # the encoder trained
    ids = spk.view(-1).long()
    if refresh == "reuse":
        want = tr.q.view(B * K, E)
    else:  # by hand with the updated weights, from the memory as the step found it
        enc = VoiceprintEncoder(vnet, B * K, T)
        want, _ = ops.spk_memory_fwd(enc.forward(tr.mag_src.view(B * K, T, F)), spk.view(-1), before)
        assert not torch.equal(want, tr.q.view(B * K, E))
    assert torch.equal(memory.mem[ids], want)
    rest = torch.ones(101, dtype=torch.bool, device=dev)
    rest[ids] = False
    assert torch.equal(memory.mem[rest], before[rest]) and float(memory.mem[50].abs().max()) > 0

    # a refused update stores nothing: the status word as a timed-out hand-off leaves it
    mem1, w1, n1 = memory.mem.clone(), vnet.flat.clone(), tr.step_count
    tr.status[0] = 1
    loss = tr.step(raw, gains, spk)
    assert torch.isnan(loss[0]) and torch.equal(memory.mem, mem1) and torch.equal(vnet.flat, w1)
    with pytest.raises(RuntimeError, match="timed out"):
        tr.check()
    assert tr.step_count == n1 and tr.status.tolist() == [0, 0]


def test_variable_lengths(dev):
    raw, gains, spk = _batch(dev)
    net, vnet, memory, tr = _nets(dev)
    lengths = torch.full((B, K), N, dtype=torch.int32)
    lengths[0, 1] = 600  # id 17, whose row is stored: frames 0 .. 5 reach samples < 600
    lengths[2, 0] = 0    # id 99, no stored row
    lengths[1, 1] = 0    # id 5: give it a stored row
    memory.mem[5] = _unit_rows(1, 13)[0].to(dev)
    stored = memory.mem.clone()
    _fwd_bwd(tr, raw, gains, spk, lengths.to(dev))
    tr.check()
    assert tr.vp_enc.len.tolist() == [17, 6, 17, 0, 0, 17]
    q = tr.q.view(B * K, E)
    assert (q[4] == 0).all()  # nothing enrolled, nothing stored
    row = stored[5].double()
    assert ((q[3].double().cpu() - (row / row.norm()).cpu()).abs().max()) < 1e-6  # the stored row re-normalised
    assert tr.loss.isfinite().all() and vnet.grad.isfinite().all() and net.grad.isfinite().all()
    # the same through step(lengths=)
    tr.step(raw, gains, spk, lengths.to(dev))
    tr.check()
    assert tr.vp_enc.len.tolist() == [17, 6, 17, 0, 0, 17] and memory.mem.isfinite().all()


def test_three_steps_repeat_bitwise(dev):
    out = []
    for _ in range(2):
        net, vnet, memory, tr = _nets(dev)
        losses = []
        for s in range(3):
            losses.append(tr.step(*_batch(dev, seed=s + 1)).clone())
        tr.check()
        out.append((torch.stack(losses), net.flat.clone(), vnet.flat.clone(), memory.mem.clone()))
    for a, b in zip(*out):
        assert a.isfinite().all() and torch.equal(a, b)


def test_graph_capture_is_refused(dev):
    raw, gains, spk = _batch(dev)
    _, _, _, tr = _nets(dev)
    with pytest.raises(NotImplementedError):
        tr.step_graph(raw, gains, spk)
    with pytest.raises(NotImplementedError):
        tr.capture()


@pytest.mark.parametrize("attention", ["dot", "align"])
def test_enrolment_of_an_unseen_speaker(dev, attention):
    """An unseen speaker enrolled from a clean excerpt: the masks equal sigmoid(V . u) ('dot') or
    sigmoid(tanh(V W1^T + u W2^T) . w3) ('align') formed with torch in fp64 from
    MaskNetForward's V, within 1e-4 (the bound of tests/test_recursive_gpu.py for its fp32 masks)."""
    net = engine.SepNet(cell="lstm", num_layers=2, hidden=40, adjust=False, device=dev, seed=7, attention=attention)
    vnet = VoiceprintNet(device=dev, seed=3)
    ex = infer.EnrolledExtractor(net, vnet, B, T, K)
    g = torch.Generator().manual_seed(5)
    clean = torch.randn(B * K, 4000, generator=g)
    clean[1, 1400:] = 0  # a shorter excerpt: frames 0 .. 11 reach samples < 1400, the silent ones are masked
    feats_c = ops.stft(clean.to(dev), complex_out=False)[1]  # (B K, 32, F)
    u = ex.enrol(feats_c)
    assert u.shape == (B * K, E) and ((u.norm(dim=1) - 1).abs() < 1e-5).all()
    enc = ex._enc[(B * K, 32)]
    assert enc.len.tolist()[1] == 12 and enc.len.tolist()[0] == 32
    v = enc.vec.double()
    assert (u.double() - v / v.norm(dim=1, keepdim=True)).abs().max() < 1e-6
    mix = ops.stft(torch.randn(B, N, generator=g).to(dev), complex_out=False)[1]
    masks = ex.run(mix, u.view(B, K, E)).clone()
    V = ex.V.view(B, T * F, E).double()
    if attention == "dot":
        want = torch.einsum("bre,bke->bkr", V, u.view(B, K, E).double())
    else:
        w1, w2, w3 = (net.view(f"att.Linear_{i}.weight").double() for i in (1, 2, 3))
        pre = (V @ w1.T)[:, None] + (u.view(B, K, E).double() @ w2.T)[:, :, None]  # (B, K, R, A)
        want = torch.tanh(pre) @ w3.view(-1)
    want = torch.sigmoid(want).view(B, K, T, F)
    err = float((masks.double() - want).abs().max())
    print("enrolment masks: max abs err", err)
    assert err < 1e-4
    # the seen-speaker path: stored rows, re-normalised, as queries
    memory = SpeakerMemory(101, E, device=dev)
    ids = torch.tensor(IDS, dtype=torch.int32, device=dev)
    ops.spk_memory_store(u, ids.view(-1), memory.mem)
    m2 = ex.run_memory(mix, memory, ids)
    assert float((m2 - masks).abs().max()) < 1e-5
    none = ex.queries_of(memory, torch.full((B, K), -1, dtype=torch.int32, device=dev))
    assert (none == 0).all()
