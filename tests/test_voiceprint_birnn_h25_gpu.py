"""Precondition of the voiceprint encoder: the generic fp32 recurrence at H = 25.  Its plan is J = 20, NG = 2, so
the second unit group holds 5 of 20 units -- a group that is not full, which no other test of the small plan runs
(H = 300 and 40 fill theirs).  The existing ``dl4ss::birnn_layer``, full length, against fp64 ``torch.nn.LSTM``:
forward within 2e-5 absolute, every gradient within 1e-4 of its largest element (the bounds of
tests/test_kernels_gpu.py).  B = 5 runs batch chunks of 1, B = 64 of 2."""
import pytest
import torch

from dl4ss_amd import library  # noqa: F401  (registers the ops)
from dl4ss_amd import ops

pytestmark = pytest.mark.gpu
H, D = 25, 23


def test_plan_has_a_partial_group():
    for B, bc in ((5, 1), (64, 2), (96, 2)):
        p = ops.birnn_plan("lstm", B, H, precision="fp32", max_wg=240)
        assert p is not None and (p["J"], p["NG"], p["BC"]) == (20, 2, bc), p
        assert p["NG"] * p["J"] > H  # the last group is not full


@pytest.mark.parametrize("B,T", [(5, 9), (64, 3)])
def test_birnn_layer_h25_matches_fp64(dev, B, T):
    torch.manual_seed(100 * B + T)
    rnn = torch.nn.LSTM(D, H, 1, batch_first=True, bidirectional=True).double()
    x = torch.randn(B, T, D, dtype=torch.float64, requires_grad=True)
    ref, _ = rnn(x)
    gout = torch.randn(B, T, 2 * H, dtype=torch.float64)
    (ref * gout).sum().backward()
    cat = lambda k: torch.cat([getattr(rnn, f"{k}_l0"), getattr(rnn, f"{k}_l0_reverse")])  # noqa: E731
    p = [cat(k).detach().float().contiguous().to(dev).requires_grad_(True)
         for k in ("weight_ih", "bias_ih", "weight_hh", "bias_hh")]
    xd = x.detach().float().to(dev).requires_grad_(True)
    out = torch.ops.dl4ss.birnn_layer(xd, *p, "lstm", H, "fp32")[0]
    err = (out.detach().cpu().double() - ref.detach()).abs().max().item()
    print(f"H=25 B={B} T={T}: forward max abs err {err:.3e}")
    assert err < 2e-5, err
    (out * gout.float().to(dev)).sum().backward()
    want = [torch.cat([getattr(rnn, f"{k}_l0").grad, getattr(rnn, f"{k}_l0_reverse").grad])
            for k in ("weight_ih", "bias_ih", "weight_hh", "bias_hh")]
    for name, g, w in zip(("dx", "dw_ih", "db_ih", "dw_hh", "db_hh"), [xd.grad] + [t.grad for t in p],
                          [x.grad] + want):
        rel = ((g.cpu().double() - w).abs().max() / w.abs().max()).item()
        print(f"  {name}: {rel:.3e} of the largest element")
        assert rel < 1e-4, (name, rel)
