"""Golden fixture of the reference's own ATTENTION class in 'align' mode (run where the reference
tree is available: ``python tests/golden/make_ref_align_fixture.py``; ``$DL4SS_REFERENCE``).

Like ``make_ref_fixtures.py`` (whose helpers it uses) this reads the py2 driver as text, translates it
in memory with ``lib2to3``, takes the ``ATTENTION`` class definition out by AST and runs
``ATTENTION(50, 'align')`` (TDAA_beta/main_run_sstune_EvalVer.py:199-242) on torch-CPU fp32, with
torch autograd for the gradients.  Nothing of the reference is written into the repository: only
data goes into ``tests/golden/ref_align.npz``:

    V (B,T,F,E) = tanh(randn), q (B,E), W1 / W2 / w3 (the class's own nn.Linear initial weights),
    dmask (B,T,F), mask (B,T,F), and dV, dq, dW1, dW2, dw3 of sum(mask * dmask)

at (B, T, F) = (2, 5, 37), E = 50.
"""
import os

import numpy as np
import torch

import make_ref_fixtures as mr

HERE = os.path.dirname(os.path.abspath(__file__))


def main(B=2, T=5, F=37, E=50, seed=21):
    ns = mr.base_namespace(mr.make_config())
    exec(mr.module_defs(mr.EVALVER, ["ATTENTION"]), ns)
    torch.manual_seed(seed)
    with mr.cpu_cuda():
        att = ns["ATTENTION"](E, 'align')
        V = torch.tanh(torch.randn(B, T, F, E)).requires_grad_(True)
        q = torch.randn(B, E).requires_grad_(True)
        dmask = torch.randn(B, T, F)
        mask = att(V, q)
        (mask * dmask).sum().backward()
    out = dict(V=V, q=q, dmask=dmask, mask=mask, W1=att.Linear_1.weight, W2=att.Linear_2.weight,
               w3=att.Linear_3.weight, dV=V.grad, dq=q.grad, dW1=att.Linear_1.weight.grad,
               dW2=att.Linear_2.weight.grad, dw3=att.Linear_3.weight.grad)
    path = os.path.join(HERE, "ref_align.npz")
    np.savez_compressed(path, **{k: v.detach().numpy().astype(np.float32) for k, v in out.items()})
    print(path, {k: tuple(v.shape) for k, v in out.items()})


if __name__ == "__main__":
    main()
