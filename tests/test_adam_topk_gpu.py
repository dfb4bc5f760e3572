"""dl4ss_adam / dl4ss_adam_guarded_dp_scaled against the fp64 update at step > 1 with non-zero moments (the
bias corrections, sqrtf(v) / bc2s + eps, gscale, the n % 4 tail and the second grid-stride pass), and
dl4ss_top_k_mask / dl4ss_classifier_select at their documented limits.  References and bars: small_ref.py."""
import numpy as np
import pytest
import torch

import small_ref as sr
from dl4ss_amd import _lib

pytestmark = pytest.mark.gpu

P = _lib.ptr
HP = (2e-4, 0.9, 0.999, 1e-8)


def _run_adam(dev, scaled, p, g, m, v, step, gscale):
    pd, gd, md, vd = (t.to(dev).clone() for t in (p, g, m, v))
    if scaled:
        _lib.call("dl4ss_adam_guarded_dp_scaled", P(pd), P(gd), P(md), P(vd), p.numel(), *HP, step, None, None, gscale,
                  None, _lib.stream_ptr())
    else:
        assert gscale == 1.0
        _lib.call("dl4ss_adam", P(pd), P(gd), P(md), P(vd), p.numel(), *HP, step, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(gd.cpu(), g)
    return pd.cpu(), md.cpu(), vd.cpu()


def _check_adam(p, g, got, step, gscale, m, v, what):
    (pr, dp), (mr, dm), (vr, dv) = sr.adam(p, g, m, v, *HP, step, gscale)
    for name, x, ref, b in (("p", got[0], pr, dp), ("m", got[1], mr, dm), ("v", got[2], vr, dv)):
        err = (x.double() - ref).abs()
        worst = float((err / b.clamp_min(1e-300)).max())
        print(f"{what} {name}: max err / bar = {worst:.3g}")
        assert bool(torch.isfinite(x).all())
        assert bool((err <= b).all()), (what, name, worst)
    # g = m = v = 0: the parameter keeps its bits
    assert torch.equal(got[0][::7].view(torch.int32), p[::7].view(torch.int32))
    assert float(got[1][::7].abs().max()) == 0.0 and float(got[2][::7].abs().max()) == 0.0


@pytest.mark.parametrize("step", [1, 7, 1000])
@pytest.mark.parametrize("n", sr.ADAM_N)
def test_adam_matches_fp64_update(dev, n, step):
    """n = 1, 3 (tail only), 4 (one quad), 5, 1027 (quads and a tail of 3); steps 1, 7 and 1000 (bias
    corrections 0.1 / 0.001, 0.52 / 0.007, 1 / 0.63); gscale 1 and 0.5; both entry points."""
    p, g, m, v = sr.adam_case(n, step)
    got = _run_adam(dev, False, p, g, m, v, step, 1.0)
    _check_adam(p, g, got, step, 1.0, m, v, "dl4ss_adam")
    got1 = _run_adam(dev, True, p, g, m, v, step, 1.0)
    for a, b in zip(got, got1):  # gscale 1 is bitwise the unscaled step
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    got2 = _run_adam(dev, True, p, g, m, v, step, 0.5)
    _check_adam(p, g, got2, step, 0.5, m, v, "dl4ss_adam_guarded_dp_scaled 0.5")


def test_adam_second_grid_stride_pass(dev):
    """n = 8192 * 1024 + 5: the 8192-block grid covers 8192 * 1024 elements per pass; the last quad and the
    one-element tail belong to the second pass."""
    n, step = sr.ADAM_N_LARGE, 7
    p, g, m, v = sr.adam_case(n, step)
    got = _run_adam(dev, True, p, g, m, v, step, 0.5)
    _check_adam(p, g, got, step, 0.5, m, v, "second pass")
    moved = g != 0
    assert bool((got[0][moved] != p[moved])[-4:].all())  # the second pass ran
    got = _run_adam(dev, False, p, g, m, v, step, 1.0)
    _check_adam(p, g, got, step, 1.0, m, v, "second pass dl4ss_adam")


def _probs(B, N, seed):
    g = np.random.default_rng(seed)
    p = g.random((B, N), dtype=np.float32)
    if N >= 8:  # ties: a value repeated at scattered ids, among the largest and around alpha
        p[:, N // 3] = p[:, 5] = p[:, N - 1] = np.float32(0.999)
        p[:, 7] = p[:, N // 2] = np.float32(0.5)
    return p


@pytest.mark.parametrize("N", [1, 8192])
@pytest.mark.parametrize("alpha", [0.5, 0.997])
def test_top_k_mask_limits(dev, N, alpha):
    """N = 1 and the documented limit N = 8192 with top_k = 64, B = 2 (two probability rows and their
    selection flags in LDS: 64 KB of dynamic shared memory); alpha 0.997 leaves fewer than top_k above it."""
    B, top_k = 2, 64
    prob = _probs(B, N, N + 1)
    pd = torch.from_numpy(prob).to(dev)
    mask = torch.full((B, N), float("nan"), device=dev)
    idx = torch.full((B, top_k), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=dev)
    _lib.call("dl4ss_top_k_mask", P(pd), B, N, alpha, top_k, P(mask), P(idx), P(cnt), _lib.stream_ptr())
    torch.cuda.synchronize()
    rm, ri, rc = sr.top_k_mask(prob, alpha, top_k)
    assert np.array_equal(cnt.cpu().numpy(), rc), (cnt.cpu().numpy(), rc)
    assert np.array_equal(mask.cpu().numpy(), rm)
    assert np.array_equal(idx.cpu().numpy(), ri)
    if N == 8192 and alpha == 0.5:
        assert rc.tolist() == [64, 64]
    if N == 8192 and alpha > 0.9:
        assert 0 < rc.max() < 64
    # idx / count NULL
    m2 = torch.full((B, N), float("nan"), device=dev)
    _lib.call("dl4ss_top_k_mask", P(pd), B, N, alpha, top_k, P(m2), None, None, _lib.stream_ptr())
    assert torch.equal(m2, mask)


@pytest.mark.parametrize("N", [1, 8192])
def test_classifier_select_limits(dev, N):
    """prob = sigmoid(logits): expf within 1 ulp (2 u), 1 + e (u), the division (u), 4 u relative; the order and
    the choice are checked on the probabilities the kernel itself wrote (a stable descending sort)."""
    B, top_k, alpha = 2, 64, 0.5
    g = np.random.default_rng(N)
    logits = (g.standard_normal((B, N)) * 3).astype(np.float32)
    if N >= 8:
        logits[:, 5] = logits[:, N // 3] = logits[:, N - 1] = np.float32(9.0)  # ties at the top
    top = sr.sort_desc(1 / (1 + np.exp(-logits[0].astype(np.float64))))
    prev = np.full((3, B), -1, np.int32)
    prev[0, 0] = top[0]                      # row 0: the two best already extracted
    prev[1, 0] = top[1] if N > 1 else -1
    ld, pv = torch.from_numpy(logits).to(dev), torch.from_numpy(prev).to(dev)
    prob = torch.full((B, N), float("nan"), device=dev)
    si = torch.full((B, top_k), -7, dtype=torch.int32, device=dev)
    ch = torch.full((B,), -7, dtype=torch.int32, device=dev)
    _lib.call("dl4ss_classifier_select", P(ld), B, N, alpha, top_k, P(pv), 3, P(prob), P(si), P(ch),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    pr = prob.cpu().numpy()
    ref = 1 / (1 + np.exp(-logits.astype(np.float64)))
    assert np.all(np.abs(pr - ref) <= 4 * sr.U * ref), float(np.max(np.abs(pr - ref) / ref)) / sr.U
    rsi, rch = sr.classifier_select(pr, alpha, top_k, prev)
    assert np.array_equal(si.cpu().numpy(), rsi)
    assert np.array_equal(ch.cpu().numpy(), rch), (ch.cpu().numpy(), rch)
    if N > 1:
        assert int(rch[0]) == int(rsi[0, 2]) and int(rch[1]) == int(rsi[1, 0])
