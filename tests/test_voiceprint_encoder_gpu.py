"""``VoiceprintEncoder`` on the GPU against the contract in fp64: per-utterance ``nn.LSTM`` over each utterance's
valid prefix plus the mean over its own frames (tests/voiceprint_ref.encoder_ref).  n = 5, T = 9, F = 23, zero
tails behind 9, 4, 0, 1, 8 frames and a silent frame inside the last utterance: lengths 9, 4, 0, 1, 7, the full
length (no shift at all, what nearly every training utterance is) among them.  The voiceprint within 2e-5 absolute,
every gradient within 1e-4 of its largest element (the bounds of tests/test_kernels_gpu.py for one layer)."""
import pytest
import torch

import voiceprint_ref as ref
from dl4ss_amd import autograd as ag, library  # noqa: F401  (library registers the ops)
from dl4ss_amd.voiceprint import VoiceprintEncoder, VoiceprintNet

pytestmark = pytest.mark.gpu
N, T, F = 5, 9, 23


def _feats(interior=True):
    x = ref.inputs(51, N, T, F)
    for b, L in enumerate(ref.LENS):
        x[b, L:] = 0
    if interior:
        x[4, 3] = 0  # utterance 4: 7 valid frames around a silent one
    return x


@pytest.mark.parametrize("hidden,layers", [(25, 2), (25, 1), (40, 2)])
def test_encoder_matches_per_utterance_lstm(dev, hidden, layers):
    vnet = VoiceprintNet(input_fre=F, emb=2 * hidden, num_layers=layers, device=dev, seed=hidden + layers)
    enc = VoiceprintEncoder(vnet, N, T)
    x = _feats()
    xc, lens, _ = ref.compact(x, ref.frame_mask(x))
    assert lens.tolist() == [9, 4, 0, 1, 7]
    dvec = ref.inputs(52, N, 2 * hidden)
    want, grads = ref.encoder_ref(xc, lens, vnet.state_dict(), F, hidden, layers, dvec)

    vec = enc.forward(x.to(dev)).clone()
    vnet.grad.fill_(float("nan"))  # backward writes every element, no zeroing pass
    enc.backward(dvec.to(dev))
    enc.check()
    assert torch.equal(enc.len.cpu(), lens)
    err = (vec.cpu().double() - want).abs().max().item()
    print(f"H={hidden} L={layers}: voiceprint max abs err {err:.3e}")
    assert err < 2e-5, err
    assert (vec[2] == 0).all()  # len 0: the zero vector
    assert not vnet.grad.isnan().any()
    for name, _ in vnet.specs:
        g, w = vnet.grad_view(name).cpu().double(), grads[name]
        rel = ((g - w).abs().max() / w.abs().max()).item()
        print(f"  {name}: {rel:.3e} of the largest element")
        assert rel < 1e-4, (name, rel)

    # a repeated pass gives the same bits (unsplit GEMMs, fixed-order sums)
    g1 = vnet.grad.clone()
    vec2 = enc.forward(x.to(dev)).clone()
    enc.backward(dvec.to(dev))
    assert torch.equal(vec2, vec) and torch.equal(vnet.grad, g1)


def test_backward_repeats_bitwise_over_many_row_blocks(dev):
    """n T = 64 * 17 = 1088 rows: the bias gradient's column sum runs over 17 blocks of 64 rows (ops.colsum would add
    5 row blocks atomically, in the order they arrive).  Five passes give the same bits, and the bias gradient is
    the fixed-order sum of the dG the pass left behind."""
    n, t = 64, 17
    vnet = VoiceprintNet(input_fre=F, emb=50, device=dev, seed=6)
    enc = VoiceprintEncoder(vnet, n, t)
    x = ref.inputs(54, n, t, F)
    for b in range(n):
        x[b, t - b % 5:] = 0  # lengths 17, 16, 15, 14, 13, ...
    x, dvec = x.to(dev), ref.inputs(55, n, 50).to(dev)
    runs = []
    for _ in range(5):
        vec = enc.forward(x).clone()
        vnet.grad.fill_(float("nan"))
        enc.backward(dvec)
        runs.append((vec, vnet.grad.clone()))
    enc.check()
    assert runs[0][1].isfinite().all()
    for vec, g in runs[1:]:
        assert torch.equal(vec, runs[0][0]) and torch.equal(g, runs[0][1])
    # layer 0 was the last to run: enc.G still holds its dG in the recurrence's frame
    want = ref.colsum_f32(enc.G.view(n * t, -1).cpu())
    assert torch.equal(vnet.cat_view("bias_ih", 0, vnet.grad).cpu(), want)


def test_caller_lengths_equal_zero_tails(dev):
    """lengths= on features without silent frames gives what the rule gives on the same features zero-tailed"""
    vnet = VoiceprintNet(input_fre=F, emb=50, device=dev, seed=4)
    enc = VoiceprintEncoder(vnet, N, T)
    full = ref.inputs(51, N, T, F)
    lens = torch.tensor(ref.LENS, dtype=torch.int32)
    a = enc.forward(full.to(dev), lengths=lens.to(dev)).clone()
    b = enc.forward(_feats(interior=False).to(dev)).clone()
    assert torch.equal(a, b)
    # the 'gt' rule on log features: frames whose every bin is <= thr are silent
    c = enc.forward(_feats(interior=False).abs().clamp_min(1e-3).log().to(dev), rule="gt", thr=-5.0)
    assert enc.len.tolist() == ref.LENS and c.isfinite().all()


def test_autograd_function_and_memory_op(dev):
    vnet = VoiceprintNet(input_fre=F, emb=50, device=dev, seed=5)
    x = _feats().to(dev)
    ids = torch.tensor([2, 5, 2, -1, 0], dtype=torch.int32, device=dev)
    mem = torch.zeros(7, 50, device=dev)
    flat = vnet.flat.requires_grad_(True)
    vec = ag.voiceprint(x, vnet, flat=flat)
    q = torch.ops.dl4ss.spk_memory(vec, ids, mem)
    dq = ref.inputs(53, N, 50).to(dev)
    (q * dq).sum().backward()
    # the same through the raw calls
    enc = VoiceprintEncoder(vnet, N, T)
    from dl4ss_amd import ops

    v2 = enc.forward(x)
    q2, u2 = ops.spk_memory_fwd(v2, ids, mem)
    dv2 = ops.spk_memory_bwd(dq, v2, u2, ids, mem)
    enc.backward(dv2)
    assert torch.equal(q.detach(), q2) and torch.equal(flat.grad, vnet.grad)
    flat.requires_grad_(False)


def test_spk_memory_opcheck(dev):
    v, ids, mem, dq = ref.memory_case()
    v = v.to(dev).requires_grad_(True)
    ids, mem, dq = ids.to(dev), mem.to(dev), dq.to(dev)
    torch.library.opcheck(torch.ops.dl4ss.spk_memory.default, (v, ids, mem),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    torch.library.opcheck(torch.ops.dl4ss.spk_memory_bwd.default, (dq, v.detach(), ids, mem),
                          test_utils=("test_schema", "test_faketensor"))
