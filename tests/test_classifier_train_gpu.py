"""One training step of the speaker classifier (dl4ss_amd.classifier.ClassifierTrainer) against the CPU
oracle: oracle.recursive.Classifier + torch MultiLabelSoftMarginLoss on its sigmoid output
(test_multi_labels_speech.py:263,397,437) + torch Adam.  Bounds are test_step_gpu.py's: fp32 loss 1e-4,
every gradient within 2e-3 of its largest element, the Adam-updated parameters with that file's sign-flip
allowance; bf16 loss 1e-2, gradients 5e-2."""
import numpy as np
import pytest
import torch

from dl4ss_amd import _lib, classifier, infer, synth
from oracle import dsp, recursive

pytestmark = pytest.mark.gpu

LR = 2e-4  # test_step_gpu.py's, so its Adam allowance applies as written
N_LAB = 11


def _batch(B, K, N, seed):
    gen = synth.SyntheticMixtures(n_samples=N, k=K, seed=seed)
    src, spk, u = gen.batch(B)
    gains = synth.gains_for(u, K)
    y = np.zeros((B, N_LAB), np.float32)
    for b in range(B):
        y[b, np.asarray(spk[b]) % N_LAB] = 1.0
    return src.astype(np.float32), gains.astype(np.float32), y


def _oracle_feats(src, gains):
    B, K, N = src.shape
    feats = []
    for b in range(B):
        _, m = dsp.mix_sources([dsp.normalise_source(src[b, k], N) for k in range(K)], gains[b])
        feats.append(np.abs(dsp.stft_tf(m)))
    return torch.from_numpy(np.array(feats, np.float32))


def _setup(dev, H, L, B, N, precision, seed=3):
    cnet = infer.ClassifierNet(hidden=H, num_layers=L, num_labels=N_LAB, device=dev, seed=seed)
    tr = classifier.ClassifierTrainer(cnet, B, 2, N, precision=precision, lr=LR)
    src, gains, y = _batch(B, 2, N, seed)
    return cnet, tr, src, gains, y


def _assert_adam_params_close(net, ref, grads_ref, errs, lr=LR, eps=1e-8):
    """test_step_gpu.py's allowance: after a first Adam step (~lr * sign(g) per weight) a disagreeing
    weight must be explained by its tensor's measured gradient error -- a sign flip (|g| <= err) or a
    step change within 4 lr err eps / (|g| + eps)^2 -- and be rare."""
    for name, p in ref.named_parameters():
        ours = net.view(name).cpu()
        diff = (ours - p.detach()).abs()
        assert diff.max().item() <= 2.1 * lr, name
        moved = diff > 1e-6
        if moved.any():
            gr = grads_ref[name]
            err_abs = errs[name] * max(gr.abs().max().item(), 1e-30)
            ga = gr.abs()
            ok = (ga <= err_abs) | (diff <= 4 * lr * err_abs * eps / (ga + eps) ** 2)
            assert bool(ok[moved].all()), (name, int(moved.sum()), gr[moved & ~ok][:8])
            assert moved.float().mean().item() < 1e-2, name


@pytest.mark.parametrize("H,L,B,N,precision", [(600, 3, 2, 3000, "fp32"), (600, 3, 2, 3000, "bf16"),
                                               (40, 2, 3, 3000, "fp32")])
def test_classifier_step_matches_oracle(dev, H, L, B, N, precision):
    cnet, tr, src, gains, y = _setup(dev, H, L, B, N, precision)
    assert B * tr.T <= 256  # dl4ss_colsum's atomic-free path: the step repeats bit for bit
    ref = recursive.Classifier(hidden=H, num_layers=L, num_labels=N_LAB)
    ref.load_state_dict({k: v.cpu() for k, v in cnet.state_dict().items()})
    opt = torch.optim.Adam(ref.parameters(), lr=LR)
    opt.zero_grad()
    prob_ref = ref(_oracle_feats(src, gains))
    loss_ref = torch.nn.MultiLabelSoftMarginLoss()(prob_ref, torch.from_numpy(y))
    loss_ref.backward()
    grads_ref = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    opt.step()
    # HIP step, from a saved state so that it can be repeated
    state = (cnet.flat.clone(), tr.m.clone(), tr.v.clone())
    raw, g, yd = (torch.from_numpy(a).to(dev) for a in (src, gains, y))
    loss = tr.step(raw, g, yd)
    tr.check()
    tol_loss, tol_grad = (1e-4, 2e-3) if precision == "fp32" else (1e-2, 5e-2)
    lv = float(loss[0].cpu())
    assert abs(lv - float(loss_ref)) / abs(float(loss_ref)) < tol_loss, (lv, float(loss_ref))
    perr = (tr.prob.cpu() - prob_ref.detach()).abs().max().item()
    assert perr < tol_loss, perr  # probabilities lie in (0, 1): the loss tolerance, absolute
    errs = {}
    for name, gr in grads_ref.items():
        ours = cnet.grad_view(name).cpu()
        denom = gr.abs().max().item()
        errs[name] = (ours - gr).abs().max().item() / denom if denom > 0 else ours.abs().max().item()
    print(f"classifier step H={H} L={L} {precision}: loss {lv:.6f} (oracle {float(loss_ref):.6f}) "
          f"max grad err {max(errs.values()):.3e}")
    bad = {k: v for k, v in errs.items() if v > tol_grad}
    assert not bad, (bad, errs)
    if precision == "fp32":
        _assert_adam_params_close(cnet, ref, grads_ref, errs)
    # the same step from the same state on the same batch: bit for bit
    after = (cnet.flat.clone(), cnet.grad.clone(), tr.m.clone(), tr.v.clone(), loss.clone())
    cnet.flat.copy_(state[0]); tr.m.copy_(state[1]); tr.v.copy_(state[2])  # noqa: E702
    tr.step_count = 0
    loss2 = tr.step(raw, g, yd)
    tr.check()
    again = (cnet.flat, cnet.grad, tr.m, tr.v, loss2)
    for a, b in zip(after, again):
        assert torch.equal(a, b)


def test_compat_classifier_autograd_matches_trainer(dev):
    """myNet.MIX_SPEECH_classifier(hidden=600, num_layers=3) through torch autograd (the large-hidden
    BPTT behind dl4ss::birnn_layer_bwd) gives the trainer's gradients: same kernels, the GEMM calls may
    differ (1e-6 of each tensor's largest element)."""
    from dl4ss_amd.compat import myNet

    H, L, B, N = 600, 3, 2, 3000
    cnet, tr, src, gains, y = _setup(dev, H, L, B, N, "fp32")
    raw, g, yd = (torch.from_numpy(a).to(dev) for a in (src, gains, y))
    tr.features(raw, g)
    tr.forward()
    tr.loss_and_grad(yd)
    tr.backward()
    tr.check()
    mod = myNet.MIX_SPEECH_classifier(cnet.F, tr.T, N_LAB, hidden=H, num_layers=L, precision="fp32").to(dev)
    mod.load_state_dict(cnet.state_dict())
    prob = mod(tr.feats.clone())
    loss = torch.nn.MultiLabelSoftMarginLoss()(prob, yd)
    loss.backward()
    assert abs(float(loss) - float(tr.loss[0])) / float(tr.loss[0]) < 1e-5
    for name, p in mod.named_parameters():
        ours, theirs = cnet.grad_view(name), p.grad
        e = ((ours - theirs).abs().max() / theirs.abs().max()).item()
        assert e < 1e-6, (name, e)


def test_classifier_timed_out_step_is_refused(dev):
    """A hand-off timeout (forced with a tiny spin limit) never reaches the weights: the guarded Adam
    leaves parameters and moments unchanged, check() raises once, and the next step is normal."""
    cnet, tr, src, gains, y = _setup(dev, 600, 3, 2, 3000, "bf16")
    raw, g, yd = (torch.from_numpy(a).to(dev) for a in (src, gains, y))
    tr.step(raw, g, yd)
    tr.check()
    before = (cnet.flat.clone(), tr.m.clone(), tr.v.clone())
    lib = _lib.lib()
    lib.dl4ss_debug_set_spin_limit(1)  # every poll gives up at once
    try:
        loss = tr.step(raw, g, yd)
        torch.cuda.synchronize()
    finally:
        lib.dl4ss_debug_set_spin_limit(0)
    assert int(tr.status[0].item()) != 0 and int(tr.status[1].item()) == 1
    assert torch.isnan(loss[0]).item()
    assert torch.equal(cnet.flat, before[0]) and torch.equal(tr.m, before[1]) and torch.equal(tr.v, before[2])
    n_before = tr.step_count
    with pytest.raises(RuntimeError, match="timed out"):
        tr.check()
    assert tr.status.tolist() == [0, 0] and tr.step_count == n_before - 1
    loss = tr.step(raw, g, yd)
    tr.check()
    assert np.isfinite(float(loss[0].item()))
    assert not torch.equal(cnet.flat, before[0])
