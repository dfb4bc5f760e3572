"""Pins tests/golden/ref_dis.npz (the reference's own Discriminator and loss lines, run by
tests/golden/make_ref_dis_fixture.py on torch-CPU fp32) with a torch-CPU restatement written here: three
stride-2 3x3 'valid' convolutions + ReLU, the (c, h, w) flatten, Linear + sigmoid, the MSE against 1 / 0 --
in fp64, on the inputs and weights regenerated from the fixture's seeded recipe."""
import os

import numpy as np
import torch
import torch.nn.functional as Fn

import disc_ref as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_dis.npz")


def _restatement(W, spec):
    bs, topk, T, F = spec.shape
    h = spec.reshape(bs * topk, 1, T, F)
    for name in ("cnn", "cnn1", "cnn2"):
        h = torch.relu(Fn.conv2d(h, W[f"{name}.weight"], W[f"{name}.bias"], stride=2))
    return torch.sigmoid(h.reshape(bs * topk, -1) @ W["final.weight"].T + W["final.bias"])


def test_fixture_is_data_only_and_small():
    assert os.path.getsize(FIXTURE) < 400 * 1024
    fx = np.load(FIXTURE, allow_pickle=False)
    assert all(fx[k].dtype.kind in "fiU" for k in fx.files)
    assert not any(k.startswith(("weight/", "in/")) for k in fx.files)  # inputs and weights are regenerated
    assert tuple(fx["meta/shape"]) == R.FIXTURE_SHAPE and int(fx["meta/seed"]) == R.FIXTURE_SEED


def test_restatement_matches_the_reference_fixture():
    fx = np.load(FIXTURE, allow_pickle=False)
    Wn, y_true, pred = R.fixture_recipe()
    W = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in Wn.items()}
    assert W["final.weight"].shape == (1, 36480)  # the reference's constant
    p = torch.from_numpy(pred).double().requires_grad_(True)
    st, sf = _restatement(W, torch.from_numpy(y_true).double()), _restatement(W, p)
    l_true, l_false = ((st - 1) ** 2).mean(), (sf ** 2).mean()
    l_adv = ((sf - 1) ** 2).mean()
    g = torch.autograd.grad(l_true + l_false, [W[k] for k in R.KEYS] + [p], retain_graph=True)
    grads = {k: v.numpy() for k, v in zip(list(R.KEYS) + ["dis_dpred"], g)}
    grads["adv_dpred"] = torch.autograd.grad(l_adv, p)[0].numpy()
    bad = R.check_against_fixture(fx, {"true": st.detach().numpy(), "false": sf.detach().numpy()},
                                  {"dis_true": l_true, "dis_false": l_false, "dis": l_true + l_false, "adv": l_adv},
                                  grads)
    assert not bad, bad
