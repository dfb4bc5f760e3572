"""The HIP classifier training step on the reference-pinned fixture (tests/golden/ref_cls_train.npz: the
reference's own MIX_SPEECH_classifier, loss, backward and Adam step at H = 16, 3 layers) at the fp32 bounds
of test_classifier_train_gpu.py: loss 1e-4, every gradient within 2e-3 of its largest element, the updated
parameters within the first Adam step's reach."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from dl4ss_amd import classifier, infer

pytestmark = pytest.mark.gpu

FIX = os.path.join(ROOT, "tests", "golden", "ref_cls_train.npz")


def test_hip_step_on_reference_fixture(dev):
    z = np.load(FIX)
    H, L, n_lab, F, B, T = (int(z[f"meta/{k}"]) for k in ("hidden", "layers", "n_lab", "F", "B", "T"))
    lr = float(z["meta/lr"])
    cnet = infer.ClassifierNet(input_fre=F, hidden=H, num_layers=L, num_labels=n_lab, device=dev)
    cnet.load_state_dict({k[len("weight/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("weight/")})
    tr = classifier.ClassifierTrainer(cnet, B, 2, 128 * (T - 1), precision="fp32", lr=lr)
    assert tr.T == T
    loss = tr.step(feats=torch.from_numpy(z["in/mix_feas"]).to(dev), y_map=torch.from_numpy(z["in/y_map"]).to(dev))
    tr.check()
    lv, lref = float(loss[0].cpu()), float(z["out/loss"])
    assert abs(lv - lref) / abs(lref) < 1e-4, (lv, lref)
    assert np.abs(tr.prob.cpu().numpy() - z["out/prob"]).max() < 1e-4
    errs = {}
    for name, _ in cnet.specs:
        g = z[f"grad/{name}"]
        errs[name] = float(np.abs(cnet.grad_view(name).cpu().numpy() - g).max() / np.abs(g).max())
    bad = {k: v for k, v in errs.items() if v > 2e-3}
    assert not bad, (bad, errs)
    _assert_adam_params_close(cnet, z, errs, lr)


def _assert_adam_params_close(cnet, z, errs, lr, eps=1e-8):
    """test_step_gpu.py's allowance against the reference's own updated parameters.  A first Adam step
    moves each weight by lr g / (|g| + eps) ~ lr sign(g), so "within 2 lr" alone would pass a skipped or a
    reversed step: every weight must also have MOVED as the reference's did (the step taken is within 10 %
    of lr of the reference's step for all but the explained ones), and a weight that disagrees by more
    than 1e-6 (a tenth of the step at this lr) must be explained by its tensor's measured gradient error
    -- a sign flip (|g| <= err) or a step change within 4 lr err eps / (|g| + eps)^2 -- and be rare."""
    for name, _ in cnet.specs:
        ours = cnet.view(name).cpu().numpy().astype(np.float64)
        ref, w0, gr = (z[f"{k}/{name}"].astype(np.float64) for k in ("param", "weight", "grad"))
        diff = np.abs(ours - ref)
        assert diff.max() <= 2.1 * lr, name
        moved = diff > 1e-6
        if moved.any():
            err_abs = errs[name] * max(np.abs(gr).max(), 1e-30)
            ga = np.abs(gr)
            ok = (ga <= err_abs) | (diff <= 4 * lr * err_abs * eps / (ga + eps) ** 2)
            assert bool(ok[moved].all()), (name, int(moved.sum()), gr[moved & ~ok][:8])
            assert moved.mean() < 1e-2, name
        # the step was taken, and in the reference's direction: where the reference moved a weight by a
        # full step, ours moved it the same way
        full = np.abs(ref - w0) > 0.5 * lr
        assert full.any(), name
        same = np.sign(ours - w0) == np.sign(ref - w0)
        assert same[full & ~moved].all() and (full & ~moved).mean() > 0.9 * full.mean(), name
