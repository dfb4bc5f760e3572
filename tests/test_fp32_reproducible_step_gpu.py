"""SepTrainer(splitk_reduce="fixed"): the fp32 step with every backward GEMM split through fixed-order slabs
(ops.gemm(reduce="fixed")) and fixed-order bias column sums repeats bit for bit -- every element of the gradient,
eager or replayed -- and agrees with the default ("atomic") step within the fp32 bounds tests/test_step_gpu.py
uses between two orders of the same sums (test_graph_step_matches_eager: loss 1e-6 relative, gradients 1e-5 of
the largest element).  B = 8, N = 16384 (T = 129, B T = 1032 rows), a 2-layer H = 40 net: the smallest shape at
which auto_splitk splits every weight gradient."""
import functools

import numpy as np
import pytest
import torch

from dl4ss_amd import engine, ops, synth

pytestmark = pytest.mark.gpu
B, K, N, H, L = 8, 2, 16384, 40, 2
T = ops.n_frames(N)
CASES = [("lstm", "dot", "label"), ("lstm", "dot", "pit"), ("gru", "dot", "pit"), ("lstm", "align", "label")]
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _batches():
    gen = synth.SyntheticMixtures(n_samples=N, k=K, seed=5)
    out = []
    for _ in range(3):
        src, spk, u = gen.batch(B)
        out.append((torch.from_numpy(src.astype(np.float32)).to(DEV),
                    torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(DEV),
                    torch.from_numpy(spk.astype(np.int32)).to(DEV)))
    return out


def _trainer(cell, attention, mode, reduce):
    net = engine.SepNet(cell=cell, num_layers=L, hidden=H, adjust=(cell == "lstm" and attention == "dot"),
                        device=DEV, seed=7, attention=attention)
    return net, engine.SepTrainer(net, B, K, N, mode=mode, splitk_reduce=reduce)


def _three_steps(cell, attention, mode, reduce):
    net, tr = _trainer(cell, attention, mode, reduce)
    losses, grads = [], []
    for b in _batches():
        losses.append(tr.step(*b).clone())
        grads.append(net.grad.clone())
    tr.check()
    return torch.stack(losses), torch.stack(grads), net.flat.clone(), tr.m.clone(), tr.v.clone()


@functools.lru_cache(maxsize=None)
def _fixed_run(cell, attention, mode):
    """the reference run of a case, computed once and left unchanged"""
    return _three_steps(cell, attention, mode, "fixed")


def test_the_shape_splits_every_weight_gradient():
    """a shape change must not turn these tests into unsplit ones"""
    BT = B * T
    for ngate in (4, 3):
        NGH = ngate * H
        for M, Nn in ((2 * NGH, 129), (2 * NGH, 2 * H), (NGH, H)):  # dW_ih of layer 0 and above, dW_hh
            assert ops.auto_splitk(M, Nn, BT) > 1, (M, Nn, BT)
            assert ops.gemm_fixed_ws_bytes(M, Nn, BT, "auto") > 0
    assert ops.auto_splitk(129 * 50, 2 * H, BT) > 1  # dW_lin


@pytest.mark.parametrize("cell,attention,mode", CASES)
def test_three_steps_repeat_bitwise(dev, cell, attention, mode):
    """two trainers from the same seed, three steps each: losses, the whole flat gradient of every step (biases
    included, every element), parameters and both moments"""
    a = _fixed_run(cell, attention, mode)
    b = _three_steps(cell, attention, mode, "fixed")
    for x, y, what in zip(a, b, ("loss", "grad", "params", "m", "v")):
        assert x.isfinite().all(), what
        assert torch.equal(x, y), what
    assert float(a[1].abs().max()) > 0


@pytest.mark.parametrize("cell,attention,mode", CASES)
def test_graph_replay_equals_eager(dev, cell, attention, mode):
    net, tr = _trainer(cell, attention, mode, "fixed")
    batches = _batches()
    tr.step(*batches[0])  # eager warm-up before the capture
    for b in batches[1:]:
        state = (net.flat.clone(), tr.m.clone(), tr.v.clone(), tr.step_count)
        le = tr.step(*b).clone()
        ge, pe, me, ve = net.grad.clone(), net.flat.clone(), tr.m.clone(), tr.v.clone()
        net.flat.copy_(state[0]); tr.m.copy_(state[1]); tr.v.copy_(state[2]); tr.step_count = state[3]
        lg = tr.step_graph(*b).clone()
        tr.check()
        assert le.isfinite().all() and torch.equal(lg, le)
        assert torch.equal(net.grad, ge) and torch.equal(net.flat, pe)
        assert torch.equal(tr.m, me) and torch.equal(tr.v, ve)


@pytest.mark.parametrize("cell,attention,mode", CASES)
def test_agrees_with_the_atomic_step(dev, cell, attention, mode):
    """the first step (same parameters, same data) of a default trainer -- on 'align' that is the unsplit step --
    within the fp32 bounds of tests/test_step_gpu.py::test_graph_step_matches_eager"""
    lf, gf = _fixed_run(cell, attention, mode)[:2]
    net, tr = _trainer(cell, attention, mode, "atomic")
    la = float(tr.step(*_batches()[0])[0].item())
    tr.check()
    ga = net.grad
    dl, dg = abs(float(lf[0, 0]) - la), float((gf[0] - ga).abs().max())
    print(f"{cell} {attention} {mode}: loss diff {dl:.3e} of {abs(la):.3e}, grad diff {dg:.3e} of "
          f"{float(ga.abs().max()):.3e}")
    assert dl <= 1e-6 * abs(la)
    assert dg <= 1e-5 * float(ga.abs().max())
