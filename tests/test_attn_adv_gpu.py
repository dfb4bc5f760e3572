"""The adversarial form of the magnitude GRAD pass (dl4ss_mask_attn_loss_adv, dl4ss_mask_attn_loss_adv_bf16v)
and the adversarial step's loss-head kernel (dl4ss_disc_adv_heads) against fp64.

GRAD pass: the three kernel forms -- attn_kernel's ADV form (fp32 V, fp32 dPre), attn_q4_kernel's on bf16 V and on
fp32 V with bf16 dPre -- for K = 1..3 on the shapes of test_attn_gpu.py (ragged 256-row tiles, a V buffer that
is no multiple of 16 B, dPre rows that do not start 16-B aligned).  The reference is the fp64 gradient of
    s1 sum (pred - Y_perm)^2 + s2 sum (sum_k m - 1)^2 + sum gext pred,   pred = m |X|, m = sigmoid(V . q)
at V (times 1 - V^2: dPre) and at q.  Two cases: s1 = s2 = 0 (only the new term: a kernel that ignores gext
returns zeros), and the trainer's s1, s2 with a gext that carries at least half of max|dPre| (asserted on the
reference).  Bars, those of test_attn_gpu.py: dq 1e-4 of its largest element, bf16 dPre 2^-8 max|dPre| + 1e-12,
fp32 dPre 1e-4 of its largest element; the loss partials are bitwise those of the call without gext through the
old entry point (same kernel form); two calls give the same bits."""
import numpy as np
import pytest
import torch

from dl4ss_amd import _lib

pytestmark = pytest.mark.gpu
E = 50
P = _lib.ptr
FORMS = ["fp32", "bf16v", "fp32v_bf16dpre"]


def _ref(Vf, q, X, Y, perm, s1, s2, gext):
    """fp64 by autograd: dPre = dL/dV (1 - V^2), dq."""
    V = Vf.double().cpu().clone().requires_grad_(True)
    q = q.double().cpu().clone().requires_grad_(True)
    X, Y, gext = X.double().cpu(), Y.double().cpu(), gext.double().cpu()
    B = V.shape[0]
    m = torch.sigmoid(torch.einsum("bre,bke->bkr", V, q))
    pred = m * X[:, None, :]
    yp = torch.stack([Y[b, perm[b]] for b in range(B)])
    L = s1 * ((pred - yp) ** 2).sum() + s2 * ((m.sum(1) - 1.0) ** 2).sum() + (gext * pred).sum()
    dV, dq = torch.autograd.grad(L, (V, q))
    return dV * (1 - V.detach() ** 2), dq


def _call(dev, form, adv, B, K, T, F, ldpb, Vd, q, X, Y, perm, s1, s2, gext):
    """One GRAD pass; adv False: the old entry point of the same kernel form (no gext).
    Returns (part_loss, dq, dPre as fp32 (B, R, E), the raw bf16 dPre buffer or None)."""
    R = T * F
    nblk = _lib.query("dl4ss_attn_nblk", T, F)
    part_loss = torch.full((B, nblk, K * K + 1), float("nan"), device=dev)
    part_dq = torch.empty(B, nblk, K, E, device=dev)
    bf = form != "fp32"
    dpre = None if bf else torch.full((B, R, E), float("nan"), device=dev)
    dpreb = torch.full((B * T, ldpb), float("nan"), device=dev).to(torch.bfloat16) if bf else None
    st = _lib.stream_ptr()
    tail = (P(dpre), P(dpreb), ldpb if bf else 0, P(part_loss), P(part_dq), None, None, st)
    head = (B, K, T, F, E, P(Vd), P(q), P(X), R, P(Y), K * R, R, P(perm), s1, s2)
    if adv:
        fn = "dl4ss_mask_attn_loss_adv_bf16v" if form == "bf16v" else "dl4ss_mask_attn_loss_adv"
        _lib.call(fn, *head, P(gext), *tail)
    else:
        fn = "dl4ss_mask_attn_loss_bf16v" if form == "bf16v" else "dl4ss_mask_attn_loss_ex"
        _lib.call(fn, 1, 0, *head, *tail)
    dq = torch.empty(B, K, E, device=dev)
    loss = torch.empty(3, device=dev)
    _lib.call("dl4ss_loss_finalize", P(part_loss), B, K, nblk, P(perm), s1, s2, P(loss), P(part_dq), E, P(dq), st)
    torch.cuda.synchronize()
    got = dpreb[:, :F * E].float().view(B, T, F, E).reshape(B, R, E) if bf else dpre
    return part_loss, dq, got, dpreb


@pytest.mark.parametrize("case", ["only_gext", "trainer_scales"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("B,T,F,ld_pad", [(3, 7, 129, 6), (2, 33, 129, 2), (1, 5, 37, 0)])
def test_attn_adv_matches_fp64(dev, B, T, F, ld_pad, K, form, case):
    g = torch.Generator(device="cpu").manual_seed(7 * K + T)
    R = T * F
    Vf = torch.tanh(torch.randn(B, R, E, generator=g))
    if form == "bf16v":
        Vf = Vf.to(torch.bfloat16).float()
    q = 0.3 * torch.randn(B, K, E, generator=g)
    X = torch.rand(B, R, generator=g)
    Y = torch.rand(B, K, R, generator=g)
    perm = torch.stack([torch.randperm(K, generator=g) for _ in range(B)])
    if case == "only_gext":
        s1 = s2 = 0.0
        gext = torch.randn(B, K, R, generator=g)
    else:
        s1, s2 = 1.0 / (B * K * R), 0.5 / (B * R)
        gext = 8.0 * s1 * torch.randn(B, K, R, generator=g)
    dpre_ref, dq_ref = _ref(Vf, q, X, Y, perm, s1, s2, gext)
    if case == "trainer_scales":  # the new term's share of max|dPre|, on the reference alone
        only, _ = _ref(Vf, q, X, Y, perm, 0.0, 0.0, gext)
        share = float(only.abs().max() / dpre_ref.abs().max())
        print(f"gext share of max|dPre|: {share:.3f}")
        assert share >= 0.5, share
    Vd = (Vf.to(torch.bfloat16) if form == "bf16v" else Vf).to(dev)
    dv = [t.to(dev) for t in (q, X, Y, perm.to(torch.int32), gext)]
    ldpb = F * E + ld_pad
    args = (dev, form, True, B, K, T, F, ldpb, Vd, dv[0], dv[1], dv[2], dv[3], s1, s2, dv[4])
    pl, dq, dpre, raw = _call(*args)
    e_dq = float((dq.double().cpu() - dq_ref).abs().max()) / float(dq_ref.abs().max())
    e_dp = float((dpre.double().cpu() - dpre_ref).abs().max())
    dmax = float(dpre_ref.abs().max())
    print(f"{form} K={K} {case}: dq {e_dq:.3e} of max, dPre {e_dp / dmax:.3e} of max")
    assert not torch.isnan(dpre).any() and not torch.isnan(dq).any()
    assert e_dq <= 1e-4
    assert e_dp <= (2 ** -8 * dmax + 1e-12 if form != "fp32" else 1e-4 * dmax)
    if raw is not None and ld_pad:  # the row padding beyond F * E is never written
        assert torch.isnan(raw[:, F * E:].float()).all()
    # the loss partials: bitwise those of the same kernel form without gext
    pl0, _, _, _ = _call(*args[:2], False, *args[3:])
    assert torch.equal(pl.view(torch.int32), pl0.view(torch.int32))
    # two calls: the same bits
    pl2, dq2, dpre2, _ = _call(*args)
    assert torch.equal(pl2.view(torch.int32), pl.view(torch.int32))
    assert torch.equal(dq2.view(torch.int32), dq.view(torch.int32))
    assert torch.equal(dpre2.view(torch.int32), dpre.view(torch.int32))


def test_attn_adv_rejects_missing_gext_and_crm_shapes(dev):
    p = P(torch.zeros(64, device=dev))
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_mask_attn_loss_adv", 1, 1, 1, 1, E, p, p, p, 1, p, 1, 1, None, 1.0, 1.0, None, p, None, 0, p, p,
                  None, None, _lib.stream_ptr())
    with pytest.raises(RuntimeError):  # K = 4
        _lib.call("dl4ss_mask_attn_loss_adv", 1, 4, 1, 1, E, p, p, p, 1, p, 1, 1, None, 1.0, 1.0, p, p, None, 0, p, p,
                  None, None, _lib.stream_ptr())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ loss heads
def _scores(N):
    """2 N scores [true; fake] with the limits: exactly 0 and 1, and one ulp from each"""
    one_m = np.nextafter(np.float32(1), np.float32(0))
    tiny = np.nextafter(np.float32(0), np.float32(1))
    if N == 1:
        return np.array([one_m, 1.0], np.float32)
    r = np.random.default_rng(N).random(2 * N).astype(np.float32)
    r[:4] = [0.0, 1.0, one_m, tiny]
    r[N:N + 4] = [1.0, 0.0, tiny, one_m]
    return r


@pytest.mark.parametrize("lam", [1.0, 20.0])
@pytest.mark.parametrize("N", [1, 4, 6])
def test_adv_heads_match_fp64(dev, N, lam):
    s = _scores(N)
    sd = torch.from_numpy(s).to(dev)
    loss = torch.full((3,), float("nan"), device=dev)
    ds_dis = torch.full((2 * N,), float("nan"), device=dev)
    ds_adv = torch.full((N,), float("nan"), device=dev)
    outs = []
    for _ in range(2):
        _lib.call("dl4ss_disc_adv_heads", P(sd), N, lam, P(loss), P(ds_dis), P(ds_adv), _lib.stream_ptr())
        torch.cuda.synchronize()
        outs.append((loss.cpu().numpy().copy(), ds_dis.cpu().numpy().copy(), ds_adv.cpu().numpy().copy()))
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    s64 = s.astype(np.float64)
    st, sf = s64[:N], s64[N:]
    ref_loss = np.array([((st - 1) ** 2).mean(), (sf ** 2).mean(), ((sf - 1) ** 2).mean()])
    ref_dis = np.concatenate([2 * (st - 1) / N, 2 * sf / N])
    ref_adv = lam * 2 * (sf - 1) / N
    got_loss, got_dis, got_adv = outs[0]
    print(f"N={N} lambda={lam}: losses {got_loss} ref {ref_loss}")
    assert np.all(np.abs(got_loss - ref_loss) <= 1e-6 * np.abs(ref_loss))
    for got, ref in ((got_dis, ref_dis), (got_adv, ref_adv)):
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= 4 * ulp), (got, ref)
