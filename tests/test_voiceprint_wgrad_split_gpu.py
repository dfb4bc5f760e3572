"""VoiceprintEncoder(wgrad_split=...) and the voiceprint step under SepTrainer(splitk_reduce="fixed"): the six
weight-gradient GEMMs split over K = n T with the fixed-order reduce.  They still repeat bit for bit, everything
else of the encoder is bitwise the unsplit encoder's, and every weight gradient -- split or not -- is within the
worst-case bound of an fp32 sum of K exact products in any order, K 2^-24 sum|a||b| per element, of the fp64
product of the operands the encoder itself handed to the GEMM (tests/test_gemm_fixed_cpu.py restates the split
order in numpy and checks that inputs of this kind stay inside that bound)."""
import pytest
import torch

from dl4ss_amd import engine, ops
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintEncoder, VoiceprintNet

pytestmark = pytest.mark.gpu
NU, T, F, HV, E = 8, 160, 129, 25, 50
LENS = [160, 0, 37, 160, 1, 96, 129, 64]


def _encoder_case(dev):
    g = torch.Generator().manual_seed(21)
    x = torch.rand(NU, T, F, generator=g) + 0.05
    dvec = torch.randn(NU, E, generator=g)
    return x.to(dev), dvec.to(dev), torch.tensor(LENS, dtype=torch.int32, device=dev)


def _backward_recorded(monkeypatch, enc, dvec):
    """enc.backward(dvec) with the operands of its weight-gradient GEMMs (the transA calls) copied as they go in"""
    calls, real = [], ops.gemm

    def gemm(A, B, **kw):
        out = real(A, B, **kw)
        if kw.get("transA"):
            calls.append((A.clone(), B.clone(), out.clone(), kw.get("reduce", "atomic")))
        return out

    with monkeypatch.context() as m:
        m.setattr(ops, "gemm", gemm)
        enc.backward(dvec)
    return calls


def _assert_inside_bound(calls, what):
    assert len(calls) == 6  # per layer: dW_hh of both directions, dW_ih
    for A, B, out, _ in calls:
        Kk = A.shape[0]
        ref = A.double().T @ B.double()
        bound = Kk * 2.0 ** -24 * (A.double().abs().T @ B.double().abs())
        err = (out.double() - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{what} {tuple(out.shape)} K={Kk}: max err / bound = {worst:.3e}")
        assert bool((err <= bound).all()), (what, tuple(out.shape), worst)


def test_encoder_split_weight_gradients(dev, monkeypatch):
    x, dvec, lens = _encoder_case(dev)
    vnet = VoiceprintNet(device=dev, seed=3)
    assert (vnet.H, vnet.L, vnet.F) == (HV, 2, F)
    nT = NU * T
    for M, N in ((4 * HV, HV), (8 * HV, F), (8 * HV, 2 * HV)):
        assert ops.auto_splitk(M, N, nT) > 1  # "auto" really splits every weight gradient
    one = VoiceprintEncoder(vnet, NU, T)
    enc = VoiceprintEncoder(vnet, NU, T, wgrad_split="auto")
    assert one.wgrad_ws is None and enc.wgrad_ws.numel() * 4 >= ops.gemm_fixed_ws_bytes(8 * HV, F, nT, "auto") > 0

    v1 = one.forward(x, lengths=lens).clone()
    vnet.grad.fill_(float("nan"))
    calls1 = _backward_recorded(monkeypatch, one, dvec)
    one.check()
    g1, dx1 = vnet.grad.clone(), one.dX.clone()
    assert all(c[3] == "atomic" for c in calls1)

    v2 = enc.forward(x, lengths=lens).clone()
    assert enc.len.tolist() == LENS and torch.equal(v2, v1)  # the forward is the unsplit encoder's
    vnet.grad.fill_(float("nan"))
    calls2 = _backward_recorded(monkeypatch, enc, dvec)
    enc.check()
    g2 = vnet.grad.clone()
    assert all(c[3] == "fixed" for c in calls2)
    assert g2.isfinite().all() and torch.equal(enc.dX, dx1)
    for _ in range(2):  # three backward passes, the same bits
        vnet.grad.fill_(float("nan"))
        enc.backward(dvec)
        assert torch.equal(vnet.grad, g2)

    # the GEMMs got the same operands; each result is inside the any-order bound, split or not
    for (A1, B1, _, _), (A2, B2, _, _) in zip(calls1, calls2):
        assert torch.equal(A1, A2) and torch.equal(B1, B2)
    _assert_inside_bound(calls1, "unsplit")
    _assert_inside_bound(calls2, "split")
    split_differs = False
    for name, _ in vnet.specs:
        a, b = vnet.view(name, g1), vnet.view(name, g2)
        if "bias" in name:
            assert torch.equal(a, b), name  # vp_colsum either way
        else:
            split_differs |= not torch.equal(a, b)
    assert split_differs  # another summation order: not the unsplit bits

    # an explicit factor: the same k-ranges as "auto" when it asks for auto's factor
    s = ops.auto_splitk(4 * HV, HV, nT)
    assert ops.auto_splitk(8 * HV, F, nT) == s == ops.auto_splitk(8 * HV, 2 * HV, nT)
    enc3 = VoiceprintEncoder(vnet, NU, T, wgrad_split=s)
    enc3.forward(x, lengths=lens)
    vnet.grad.fill_(float("nan"))
    enc3.backward(dvec)
    assert torch.equal(vnet.grad, g2)


# ---- the voiceprint step: B K T = 2064 encoder rows, B T = 1032 mask-net rows
B, K, N = 8, 2, 16384
TS = ops.n_frames(N)
IDS = [[3, 17], [42, 5], [99, 61], [0, 100], [8, 77], [23, 50], [64, 12], [31, 90]]


def _batch(dev, seed):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(B, K, N, generator=g)
    gains = torch.rand(B, K, generator=g) * 0.5 + 0.75
    return raw.to(dev), gains.to(dev), torch.tensor(IDS, dtype=torch.int32, device=dev)


def _nets(dev, reduce):
    net = engine.SepNet(cell="lstm", num_layers=2, hidden=40, adjust=False, device=dev, seed=7, attention="dot")
    vnet = VoiceprintNet(device=dev, seed=3)
    memory = SpeakerMemory(101, E, device=dev)
    x = torch.randn(E, generator=torch.Generator().manual_seed(11)).double()
    memory.mem[17] = (x / x.norm()).float().to(dev)  # a touched row
    tr = engine.SepTrainer(net, B, K, N, voiceprint=vnet, memory=memory, splitk_reduce=reduce)
    return net, vnet, memory, tr


def test_step_three_steps_repeat_bitwise(dev):
    """everything tests/test_voiceprint_step_gpu.py::test_three_steps_repeat_bitwise compares, on 'dot' (which
    that test cannot take: the default step's atomics), plus both flat gradients -- no element masked out"""
    assert ops.auto_splitk(8 * HV, F, B * K * TS) > 1 and ops.auto_splitk(320, F, B * TS) > 1
    out = []
    for _ in range(2):
        net, vnet, memory, tr = _nets(dev, "fixed")
        assert tr.vp_enc.wgrad_split == "auto"
        losses = []
        for s in range(3):
            losses.append(tr.step(*_batch(dev, seed=s + 1)).clone())
        tr.check()
        out.append((torch.stack(losses), net.flat.clone(), vnet.flat.clone(), memory.mem.clone(), net.grad.clone(),
                    vnet.grad.clone()))
    for a, b in zip(*out):
        assert a.isfinite().all() and torch.equal(a, b)


def test_step_memory_rows_agree_with_the_atomic_step(dev):
    """one step of the "fixed" and of the default trainer on the same data: the rows the refresh wrote (re-encoded
    with the updated encoder) within the tolerance tests/test_voiceprint_step_gpu.py uses on 'dot', 1e-5 of the
    largest element; the loss within its 1e-6 relative"""
    rows = []
    for reduce in ("fixed", "atomic"):
        net, vnet, memory, tr = _nets(dev, reduce)
        before = memory.mem.clone()
        loss = float(tr.step(*_batch(dev, seed=1))[0].item())
        tr.check()
        ids = torch.tensor(IDS, device=dev).view(-1).long()
        assert not torch.equal(memory.mem[ids], before[ids])
        rows.append((loss, memory.mem[ids].clone(), vnet.grad.clone()))
    (lf, mf, gf), (la, ma, ga) = rows
    dm, dg = float((mf - ma).abs().max()), float((gf - ga).abs().max())
    print(f"loss {lf} vs {la}; memory rows max diff {dm:.3e} of {float(ma.abs().max()):.3e}; "
          f"encoder grad max diff {dg:.3e} of {float(ga.abs().max()):.3e}")
    assert abs(lf - la) <= 1e-6 * abs(la)
    assert dg <= 1e-5 * float(ga.abs().max())
    assert dm <= 1e-5 * float(ma.abs().max())
