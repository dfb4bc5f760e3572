"""dl4ss_te_assemble: the evaluation mixture in the reference's summation order (predict.py:134-158), bitwise
against the same fp32 adds done by torch on the CPU."""
import numpy as np
import pytest
import torch

from dl4ss_amd import targeteval

pytestmark = pytest.mark.gpu
S = 3


def cpu_assemble(srcs, lengths, bgd, spk_num):
    mix = srcs[:, 0] + srcs[:, 1]
    noise = srcs[:, 1].clone()
    for k in range(2, spk_num):
        mix = mix + srcs[:, k]
        noise = noise + srcs[:, k]
    if bgd is not None:
        mix = mix + bgd
        noise = noise + bgd
    N = srcs.shape[2]
    mix_len = torch.full((srcs.shape[0],), N, dtype=torch.int32) if lengths is None else \
        lengths[:, :spk_num].max(1).values.to(torch.int32)
    return mix, noise, srcs[:, 0].clone(), mix_len


@pytest.mark.parametrize("with_bgd", (False, True))
@pytest.mark.parametrize("spk_num", (2, 3))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("N", (1, 130, 4000))
def test_bitwise(dev, N, B, spk_num, with_bgd):
    g = torch.Generator().manual_seed(100 * N + 10 * B + spk_num)
    # values of mixed magnitude, so that the order of the adds shows in the last bit
    srcs = torch.randn(B, S, N, generator=g) * torch.tensor([1.0, 37.0, 1e-3]).view(1, S, 1)
    lengths = torch.randint(0, N + 1, (B, S), generator=g, dtype=torch.int32)
    lengths[0, 0], lengths[-1, 1] = N, 0  # lengths that include 0 and N
    lengths[0, 2] = N  # beyond spk_num = 2 it must not count
    for b in range(B):
        for k in range(S):
            srcs[b, k, lengths[b, k]:] = 0
    bgd = torch.randn(N, generator=g) * 5 if with_bgd else None
    want = cpu_assemble(srcs, lengths, bgd, spk_num)
    got = targeteval.assemble(srcs.to(dev), lengths.to(dev), None if bgd is None else bgd.to(dev), spk_num)
    for w, x, name in zip(want, got, ("mix", "noise", "target", "mix_len")):
        assert torch.equal(w, x.cpu()), name
    no_len = targeteval.assemble(srcs.to(dev), None, None, spk_num)
    assert torch.equal(no_len[3].cpu(), torch.full((B,), N, dtype=torch.int32))
    assert torch.equal(no_len[0].cpu(), cpu_assemble(srcs, None, None, spk_num)[0])


def test_order_matters_on_these_inputs():
    """The inputs above tell the reference's order from another one (so the bitwise test can fail)."""
    g = torch.Generator().manual_seed(100 * 4000 + 10 * 3 + 3)
    srcs = torch.randn(3, S, 4000, generator=g) * torch.tensor([1.0, 37.0, 1e-3]).view(1, S, 1)
    a = (srcs[:, 0] + srcs[:, 1]) + srcs[:, 2]
    b = srcs[:, 0] + (srcs[:, 1] + srcs[:, 2])
    assert not torch.equal(a, b)


def test_refusals(dev):
    s = torch.zeros(2, 3, 64, device=dev)
    with pytest.raises(RuntimeError):
        targeteval.assemble(s, None, None, 4)  # spk_num > S
    with pytest.raises(RuntimeError):
        targeteval.assemble(s, None, None, 1)
    with pytest.raises(RuntimeError):
        targeteval.assemble(s, None, torch.zeros(63, device=dev), 2)
    out = (s.view(-1)[64:192].view(2, 64), torch.empty(2, 64, device=dev), torch.empty(2, 64, device=dev), None)
    with pytest.raises(RuntimeError):
        targeteval.assemble(s, None, None, 2, out=out)  # an output inside the input
