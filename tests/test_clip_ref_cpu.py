"""tests/clip_ref.py checked without a GPU.

1. It is right: clip + adam_clipped equal torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam in fp64,
   on several tensors viewed from one flat buffer (the trainers' layout), with the clip active, inactive,
   max_norm = inf, and on a SUM gradient with gscale 0.5.
2. Its bars can fail: an fp32 numpy emulation of the kernels (fp64 sum, one fp32 factor, fp32 Adam) passes them,
   the same emulation with the LAST element left out of the sum misses them.
"""
import numpy as np
import pytest
import torch

import clip_ref as cr
import small_ref as sr

D64 = torch.float64
HP = (2e-4, 0.9, 0.999, 1e-8)
MISS = 4
N = 1027
SHAPES = [(10, 30), (700,), (3, 9)]  # 300 + 700 + 27 = N


def _close(a, b, tol):
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max()) / scale


def _norm(g, gscale=1.0):
    return cr.clip(g, float("inf"), gscale)[0]


@pytest.mark.parametrize("rel,gscale", [(0.5, 1.0), (2.0, 1.0), (float("inf"), 1.0), (0.5, 0.5), (2.0, 0.5)])
def test_clip_ref_matches_torch(rel, gscale):
    """Three steps.  torch works in fp64 throughout; the reference rounds the factor f and the bias corrections
    to fp32 as the kernels do (2^-24 each): 1e-6 relative covers them."""
    lr, b1, b2, eps = (cr.f32(x) for x in HP)
    p0, _, _, _ = sr.adam_case(N, 1)
    flat = p0.double().clone()
    gflat = torch.zeros(N, dtype=D64)
    params, off = [], 0
    for shp in SHAPES:
        n = int(np.prod(shp))
        q = torch.nn.Parameter(flat[off:off + n].view(shp))
        q.grad = gflat[off:off + n].view(shp)
        assert q.data_ptr() == flat[off:].data_ptr()
        params.append(q)
        off += n
    assert off == N
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps)
    pr, m, v = p0.double(), torch.zeros(N, dtype=D64), torch.zeros(N, dtype=D64)
    for step in (1, 2, 3):
        g = sr.inputs(200 + step, N, scale=0.1)  # the SUM gradient (fp32); the mean is g * gscale
        max_norm = cr.f32(rel * _norm(g, gscale))
        gflat.copy_(g.double() * gscale)
        total = torch.nn.utils.clip_grad_norm_(params, max_norm)
        nrm, c, f = cr.clip(g, max_norm, gscale)
        assert abs(float(total) - nrm) <= 1e-12 * nrm
        assert (c < 1.0) == (rel < 1.0)
        if rel >= 1.0:
            assert c == 1.0 and f == gscale
        else:
            assert abs(c - rel) < 1e-4  # the 1e-6 in the denominator and max_norm's rounding
        _close(gflat, g.double() * f, 1e-12)
        opt.step()
        (pr, _), (m, _), (v, _), (n2, c2, f32_) = cr.adam_clipped(pr, g, m, v, *HP, step, max_norm, gscale)
        assert (n2, c2) == (nrm, c) and f32_ == cr.f32(f)
        _close(pr, flat, 1e-6)
        _close(m, torch.cat([opt.state[q]["exp_avg"].reshape(-1) for q in params]), 1e-6)
        _close(v, torch.cat([opt.state[q]["exp_avg_sq"].reshape(-1) for q in params]), 1e-6)


def _emulate(p, g, m, v, step, max_norm, gscale, drop_last=False):
    """The kernels in numpy: the squares summed in fp64 (all of them, or all but the last), nrm, c, f in fp64,
    f rounded to fp32 once, then the fp32 Adam at gscale = f.  Returns p', m', v' (fp64 tensors) and gnorm."""
    f = np.float32
    gd = g.numpy().astype(np.float64)
    S = float(np.sum((gd[:-1] if drop_last else gd) ** 2))
    nrm = float(f(gscale)) * np.sqrt(S)
    c = min(1.0, float(f(max_norm)) / (nrm + 1e-6))
    fac = f(float(f(gscale)) * c)
    lr, b1, b2, eps = (f(x) for x in HP)
    pn, gn, mn, vn = (t.numpy().astype(f) for t in (p, g, m, v))
    bc1 = f(1.0 - float(b1) ** step)
    bc2s = f(np.sqrt(1.0 - float(b2) ** step))
    gs = gn * fac
    m2 = mn + (f(1) - b1) * (gs - mn)
    v2 = b2 * vn + (f(1) - b2) * gs * gs
    p2 = pn - (lr / bc1) * (m2 / (np.sqrt(v2) / bc2s + eps))
    assert p2.dtype == m2.dtype == v2.dtype == np.float32
    return [torch.from_numpy(x.astype(np.float64)) for x in (p2, m2, v2)], (f(nrm), f(c))


@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_bars_pass_faithful_and_fail_dropped_element(step, gscale):
    p, g, m, v = sr.adam_case(N, step)
    assert float(g[-1]) != 0.0
    max_norm = cr.f32(0.5 * _norm(g, gscale))
    (pr, dp), (mr, dm), (vr, dv), (nrm, c, _) = cr.adam_clipped(p, g, m, v, *HP, step, max_norm, gscale)
    assert c < 1.0
    (p2, m2, v2), gn = _emulate(p, g, m, v, step, max_norm, gscale)
    assert cr.gnorm_close(gn, nrm, c)
    assert bool(((p2 - pr).abs() <= dp).all()) and bool(((m2 - mr).abs() <= dm).all())
    assert bool(((v2 - vr).abs() <= dv).all())
    assert bool((p2[::7] == p.double()[::7]).all())  # g = m = v = 0: p does not move
    # the last element left out of the sum: a smaller norm, a larger coefficient, every moved element off
    (pb, mb, vb), gb = _emulate(p, g, m, v, step, max_norm, gscale, drop_last=True)
    assert not cr.gnorm_close(gb, nrm, c)
    assert abs(float(gb[0]) - nrm) > MISS * cr.GNORM_U * cr.U * nrm
    moved = g != 0
    assert bool(((mb - mr).abs()[moved] > MISS * dm[moved]).all())
    if step == 1:  # later v' is 0.999 v + 0.001 gs^2: a 1e-3 change of the small term is below 5 u v'
        assert bool(((vb - vr).abs()[moved] > MISS * dv[moved]).all())
    # (p shows nothing: one update is ~1e-4 of |p|, and a change of 1e-3 of it is below the u |p'| of p's bar;
    # the moments are what tells a wrong factor)


def test_inactive_factor_is_bitwise_gscale():
    """c == 1 (a threshold above the norm, or inf): f rounds to the fp32 gscale itself."""
    g = sr.inputs(3, N, scale=0.1)
    for gscale in (1.0, 0.5, 1.0 / 3.0):
        for max_norm in (2.0 * _norm(g, gscale), float("inf")):
            _, c, f = cr.clip(g, max_norm, gscale)
            assert c == 1.0 and np.float32(f) == np.float32(gscale)
