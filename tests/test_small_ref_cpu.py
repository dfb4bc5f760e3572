"""The references of tests/small_ref.py, checked without a GPU.

1. They are right: the query / ADDJUST, dot-attention and column-sum restatements equal fp64 torch.autograd on
   the composed expression q = emb[idx] + cat(mean_t h, emb[idx]) @ W_adj^T (rows with id -1 zero), and the Adam
   restatement equals torch.optim.Adam in fp64 over three steps.
2. Their bars can fail: on the inputs the GPU tests use, a sequential fp32 numpy emulation of each sum passes
   the a-priori bar, and the same emulation with ONE term left out (the last term of the last chunk, the last
   row) misses it at every output that term belongs to.
"""
import numpy as np
import pytest
import torch

import small_ref as sr

D64 = torch.float64
# a left-out term must miss the bar by this factor (term / bar ~ 1 / (n^2 u): 12 at the longest sum, n = 1001)
MISS = 4


def _close(a, b, tol=1e-12):
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max()) / scale


# ---- 1. the references against autograd ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,T,D,W,kind", [(3, 2, 11, 600, 50, "mixed"), (5, 3, 4, 63, 64, "mixed"),
                                            (70, 1, 3, 130, 70, "far")])
def test_query_refs_match_autograd(B, K, T, D, W, kind):
    c = sr.query_case(B, K, T, D, W, kind)
    idx = c["idx"]
    h = c["h"].double().requires_grad_(True)
    emb = c["emb"].double().requires_grad_(True)
    wadj = c["wadj"].double().requires_grad_(True)
    valid = (idx >= 0)[..., None].double()
    e = emb[idx.clamp_min(0)]
    cat = torch.cat([h.mean(1)[:, None, :].expand(B, K, D), e], -1)
    q = (e + cat @ wadj.T) * valid
    mean32 = h.detach().mean(1).float()  # the kernel's fp32 mean, as the reference receives it
    # forward from the fp32 mean: compare on the expression evaluated with that mean
    cat32 = torch.cat([mean32.double()[:, None, :].expand(B, K, D), e.detach()], -1)
    _close(sr.query_fwd(mean32, idx, c["emb"], c["wadj"]).val, (e.detach() + cat32 @ wadj.detach().T) * valid)
    _close(sr.time_mean(c["h"]).val, h.detach().mean(1))
    # the plain gather
    _close(sr.query_fwd(None, idx, c["emb"], None).val, e.detach() * valid)
    dq = c["dq"].double()
    (q * dq).sum().backward()
    r = sr.query_bwd(c["dq"], idx, c["emb"], c["wadj"], h.detach().mean(1), T, sr.N_LABELS)
    _close(r["dh"].val, h.grad[:, 0, :])          # the gradient of every step t of h[b] (dh_bcast)
    _close(r["demb"].val, emb.grad)
    _close(r["dwadj"].val, wadj.grad)
    # beta 1: the prefilled gradients are added
    r1 = sr.query_bwd(c["dq"], idx, c["emb"], c["wadj"], h.detach().mean(1), T, sr.N_LABELS, c["old_emb"],
                      c["old_wadj"])
    _close(r1["demb"].val, emb.grad + c["old_emb"].double())
    _close(r1["dwadj"].val, wadj.grad + c["old_wadj"].double())
    # without ADDJUST: the scatter of dq alone
    emb2 = c["emb"].double().requires_grad_(True)
    ((emb2[idx.clamp_min(0)] * valid) * dq).sum().backward()
    _close(sr.query_bwd(c["dq"], idx, c["emb"], None, None, T, sr.N_LABELS)["demb"].val, emb2.grad)
    # a -1 row: zero query, and no term anywhere
    assert (idx < 0).any() or B * K < 5
    qf = sr.query_fwd(mean32, idx, c["emb"], c["wadj"])
    assert float(qf.val[idx < 0].abs().max() if (idx < 0).any() else 0.0) == 0.0


@pytest.mark.parametrize("act", [0, 1])
def test_attn_dot_refs_match_autograd(act):
    c = sr.dot_case(3, 257)
    V = c["V"].double().requires_grad_(True)
    q = c["q"][:, :50].double().requires_grad_(True)
    lg = (V * q[:, None, :]).sum(-1)
    mask = torch.sigmoid(lg) if act == 0 else 10 * torch.tanh(lg)
    ref, _ = sr.attn_dot_fwd(c["V"], c["q"][:, :50], act)
    _close(ref, mask.detach())
    (mask * c["dmask"].double()).sum().backward()
    dV, _, dq, _ = sr.attn_dot_bwd(c["V"], c["q"][:, :50], mask.detach(), c["dmask"], act, c["dV_old"])
    _close(dV, V.grad + c["dV_old"].double())
    _close(dq.val, q.grad)


def test_colsum_ref_matches_autograd():
    A = sr.inputs(3, 257, 65).double().requires_grad_(True)
    w = sr.inputs(4, 65).double()
    (A.sum(0) * w).sum().backward()  # d/dA is w broadcast; the sum itself is what the bias gradient is
    old = sr.inputs(5, 65)
    s = sr.colsum(A.detach().float(), old)
    _close(s.val, A.detach().sum(0) + old.double())
    _close(sr.colsum(A.detach().float().bfloat16()).val, A.detach().float().bfloat16().double().sum(0))
    assert s.n == 258


def test_adam_ref_matches_torch_optim():
    """Three steps of torch.optim.Adam in fp64.  torch forms the bias corrections in double; the reference
    rounds them to fp32 as the launcher does: 1e-6 relative covers that rounding (2^-24 each)."""
    lr, b1, b2, eps = (float(np.float32(x)) for x in (2e-4, 0.9, 0.999, 1e-8))
    p0, _, _, _ = sr.adam_case(1027, 1)
    p = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    pr, m, v = p0.double(), torch.zeros(1027, dtype=D64), torch.zeros(1027, dtype=D64)
    for step in (1, 2, 3):
        g = sr.inputs(100 + step, 1027, scale=0.1).double()
        p.grad = g.clone()
        opt.step()
        (pr, _), (m, _), (v, _) = sr.adam(pr, g, m, v, lr, b1, b2, eps, step)
        _close(pr, p.detach(), 1e-6)
        st = opt.state[p]
        _close(m, st["exp_avg"], 1e-12)
        _close(v, st["exp_avg_sq"], 1e-12)
    # gscale scales the gradient
    (a, _), _, _ = sr.adam(p0, g.float(), m.float(), v.float(), lr, b1, b2, eps, 7, 0.5)
    (b, _), _, _ = sr.adam(p0, (g.float() * 0.5), m.float(), v.float(), lr, b1, b2, eps, 7, 1.0)
    _close(a, b)


def test_topk_refs():
    prob = np.array([[0.2, 0.9, 0.9, 0.1, 0.6]], np.float32)
    mask, idx, count = sr.top_k_mask(prob, 0.5, 2)
    assert mask.tolist() == [[0, 1, 1, 0, 0]] and idx.tolist() == [[1, 2]] and count.tolist() == [2]
    mask, idx, count = sr.top_k_mask(prob, 0.5, 4)
    assert mask.tolist() == [[0, 1, 1, 0, 1]] and idx.tolist() == [[1, 2, 4, -1]] and count.tolist() == [3]
    si, ch = sr.classifier_select(prob, 0.5, 3, np.array([[1]], np.int32))
    assert si.tolist() == [[1, 2, 4]] and ch.tolist() == [2]
    assert sr.classifier_select(prob, 0.95, 3, None)[1].tolist() == [-1]


# ---- 2. the bars pass a faithful fp32 emulation and fail one with a term left out --------------------------------
def _passes_and_fails(s, owns_last=None):
    """s: a Sum.  owns_last: mask of the outputs the last term belongs to (default: all)."""
    b = sr.bar(s)
    ok = (sr.seq_f32(s) - s.val).abs()
    assert bool((ok <= b).all()), float((ok / b.clamp_min(1e-300)).max())
    bad = (sr.seq_f32(s, drop_last=True) - s.val).abs()
    sel = torch.ones_like(bad, dtype=torch.bool) if owns_last is None else owns_last.expand_as(bad)
    assert bool(sel.any())
    assert bool((s.terms[..., -1].abs()[sel] > 0).all())
    assert bool((bad[sel] > MISS * b[sel]).all()), float((bad[sel] / b[sel]).min())


@pytest.mark.parametrize("B,T,D", sr.MEAN_SHAPES)
def test_bar_time_mean(B, T, D):
    if T == 1:  # a one-term sum is exact; leaving the term out leaves nothing
        s = sr.time_mean(sr.query_case(B, 1, T, D, 4)["h"])
        assert float((sr.seq_f32(s) - s.val).abs().max()) == 0.0
        return
    _passes_and_fails(sr.time_mean(sr.query_case(B, 1, T, D, 4)["h"]))


@pytest.mark.parametrize("B,K,T,D,W", sr.QFWD_SHAPES)
def test_bar_query_fwd(B, K, T, D, W):
    c = sr.query_case(B, K, T, D, W)
    s = sr.query_fwd(c["mean"], c["idx"], c["emb"], c["wadj"])
    _passes_and_fails(s, (c["idx"] >= 0)[..., None])


@pytest.mark.parametrize("B,K,D,W,kind", sr.QBWD_SHAPES)
def test_bar_query_bwd(B, K, D, W, kind):
    c = sr.query_case(B, K, 5, D, W, kind)
    idx = c["idx"]
    assert int(idx.view(-1)[-1]) >= 0  # the last row is valid: its terms are the ones left out
    r = sr.query_bwd(c["dq"], idx, c["emb"], c["wadj"], c["mean"], 5, sr.N_LABELS, c["old_emb"], c["old_wadj"])
    _passes_and_fails(r["dh"], (idx[:, -1] >= 0)[:, None])
    _passes_and_fails(r["dwadj"])
    last = torch.arange(sr.N_LABELS) == int(idx.view(-1)[-1])
    _passes_and_fails(r["demb"], last[:, None])
    if kind == "far":
        assert int(idx.view(-1)[2]) == int(idx.view(-1)[66]) and int((idx == idx.view(-1)[2]).sum()) == 2


@pytest.mark.parametrize("M,N,lda", sr.COLSUM_SHAPES[1:])
def test_bar_colsum(M, N, lda):
    _passes_and_fails(sr.colsum(sr.inputs(M, M, N), sr.inputs(M + 1, N)))


@pytest.mark.parametrize("M,N", [(300, 513), (257, 520), (300, 129), (70, 65)])
def test_bar_colsum_bf16(M, N):
    _passes_and_fails(sr.colsum(sr.inputs(M, M, N).bfloat16(), sr.inputs(M + 1, N)))


@pytest.mark.parametrize("Bq,R", sr.DOT_SHAPES)
@pytest.mark.parametrize("act", [0, 1])
def test_bar_attn_dot(Bq, R, act):
    c = sr.dot_case(Bq, R)
    q = c["q"][:, :50]
    lg = sr.attn_dot_logits(c["V"], q)
    f = (lambda x: torch.sigmoid(x)) if act == 0 else (lambda x: 10 * torch.tanh(x))
    ref, b = sr.attn_dot_fwd(c["V"], q, act)
    assert bool(((f(sr.seq_f32(lg)) - ref).abs() <= b).all())
    assert bool(((f(sr.seq_f32(lg, drop_last=True)) - ref).abs() > MISS * b).all())
    if R == 1:
        return  # dq is a one-term sum
    _, _, dq, dq_bar = sr.attn_dot_bwd(c["V"], q, ref.float(), c["dmask"], act)
    assert bool(((sr.seq_f32(dq) - dq.val).abs() <= dq_bar).all())
    assert bool(((sr.seq_f32(dq, drop_last=True) - dq.val).abs() > MISS * dq_bar).all())


def _adam_f32(p, g, m, v, lr, b1, b2, eps, step, gscale, bc2_off=False):
    f = np.float32
    p, g, m, v = (t.numpy().astype(f) for t in (p, g, m, v))
    lr, b1, b2, eps, gscale = f(lr), f(b1), f(b2), f(eps), f(gscale)
    bc1 = f(1.0 - float(b1) ** step)
    bc2s = f(1.0) if bc2_off else f(np.sqrt(1.0 - float(b2) ** step))
    gs = g * gscale
    m2 = m + (f(1) - b1) * (gs - m)
    v2 = b2 * v + (f(1) - b2) * gs * gs
    p2 = p - (lr / bc1) * (m2 / (np.sqrt(v2) / bc2s + eps))
    return [torch.from_numpy(x.astype(np.float64)) for x in (p2, m2, v2)]


@pytest.mark.parametrize("step", [1, 7, 1000])
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_bar_adam(step, gscale):
    """An fp32 numpy Adam passes the counted bars; one that drops the second-moment bias correction, or that
    forgets gscale in the second moment, misses them."""
    hp = (2e-4, 0.9, 0.999, 1e-8)
    p, g, m, v = sr.adam_case(1027, step)
    (pr, dp), (mr, dm), (vr, dv) = sr.adam(p, g, m, v, *hp, step, gscale)
    p2, m2, v2 = _adam_f32(p, g, m, v, *hp, step, gscale)
    assert bool(((p2 - pr).abs() <= dp).all()) and bool(((m2 - mr).abs() <= dm).all())
    assert bool(((v2 - vr).abs() <= dv).all())
    assert bool((p2[::7] == p.double()[::7]).all())  # g = m = v = 0: p does not move
    pb, _, _ = _adam_f32(p, g, m, v, *hp, step, gscale, bc2_off=True)
    moved = g != 0
    assert bool(((pb - pr).abs()[moved] > MISS * dp[moved]).all())
    if gscale != 1.0:
        _, mb, vb = _adam_f32(p, g, m, v, *hp, step, 1.0)
        assert bool(((vb - vr).abs()[moved] > MISS * dv[moved]).all())
        assert bool(((mb - mr).abs()[moved] > MISS * dm[moved]).all())
