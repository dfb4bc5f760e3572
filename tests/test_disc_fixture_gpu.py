"""The HIP Discriminator (``myNet.Discriminator``, fp32) against tests/golden/ref_dis.npz -- the reference's own
class and loss lines (main_run_sstune_dis.py:318-336,615-616,622-624,642) at its own map size (313, 129),
Linear(36480, 1): scores at rtol 1e-5 / atol 1e-6, losses at 1e-5, every gradient within 1e-4 of its largest
stored element."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import disc_ref as R
from dl4ss_amd import compat

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_dis.npz")


def test_module_matches_the_reference_fixture(dev):
    compat.install()
    import myNet

    fx = np.load(FIXTURE, allow_pickle=False)
    W, y_true, pred = R.fixture_recipe()
    d = myNet.Discriminator(precision="fp32")          # the defaults: (313, 129), Linear(36480, 1)
    d.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    d.to(dev)
    p = torch.from_numpy(pred).to(dev).requires_grad_(True)
    mse = nn.MSELoss()
    score_true = d(torch.from_numpy(y_true).to(dev))   # dis.py:615-616
    score_false = d(p)
    ones, zeros = torch.ones_like(score_true), torch.zeros_like(score_true)
    l_true, l_false = mse(score_true, ones), mse(score_false, zeros)   # :622-624
    l_adv = mse(score_false, ones)                                      # :642
    params = dict(d.named_parameters())
    g = torch.autograd.grad(l_true + l_false, list(params.values()) + [p], retain_graph=True)
    grads = {k: v.cpu().numpy() for k, v in zip(list(params) + ["dis_dpred"], g)}
    grads["adv_dpred"] = torch.autograd.grad(l_adv, p)[0].cpu().numpy()
    bad = R.check_against_fixture(fx, {"true": score_true.detach().cpu().numpy(),
                                       "false": score_false.detach().cpu().numpy()},
                                  {"dis_true": l_true, "dis_false": l_false, "dis": l_true + l_false, "adv": l_adv},
                                  grads)
    assert not bad, bad
