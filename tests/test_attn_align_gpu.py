"""The ATTENTION 'align' kernels (dl4ss_amd/csrc/attn_align.hip) against an fp64 torch restatement
of the reference's additive attention (TDAA_beta/main_run_sstune_EvalVer.py:228-239;
Cocktail/software/DL4SS_Keras/extend_layers.py:50-64):

    mask = sigmoid(Linear_3(tanh(Linear_1(V) + Linear_2(q))))        (no biases, E = A = 50)

with the separation loss of the 'dot' kernel (EvalVer.py:641,659-666: MSE + 0.5 sum-to-one) and its
gradients by torch autograd in fp64.  Covered: the fused step kernel (COST / GRAD passes + finalize)
for K = 1..3 over full, ragged and multi-block tilings; PIT through its COST pass; bitwise
reproducibility; untouched neighbouring memory; the module-level forward / backward.

Tolerances are the fp32 attention tests': masks rtol 1e-5 / atol 1e-6, loss 1e-5 relative, dq / dW1 /
dW2 / dw3 within 1e-4 of the tensor's largest element, dPre (dV) within 1e-5 of its largest."""
import ctypes
import functools
import itertools

import pytest
import torch

from dl4ss_amd import _lib

pytestmark = pytest.mark.gpu
E = 50
SHAPES = [(3, 7, 129), (2, 33, 129), (1, 5, 37)]


def ref_masks(V, q, W1, W2, w3):
    """fp64 (or any dtype): V (B,R,E), q (B,K,E) -> masks (B,K,R)."""
    U = V @ W1.t()                                  # Linear_1 on the mixture embedding
    p = q @ W2.t()                                  # Linear_2 on the query
    s = torch.tanh(U[:, None] + p[:, :, None])      # (B,K,R,A)
    return torch.sigmoid(s @ w3.reshape(-1))        # Linear_3 -> one logit, sigmoid


def ref_fused(V, q, W1, W2, w3, X, Y, perm, s1, s2):
    """fp64 masks, loss, dPre = dL/dV (1 - V^2), dq, dW1, dW2, dw3 for a given permutation."""
    V, q, W1, W2, w3, X, Y = (t.detach().double().cpu().clone() for t in (V, q, W1, W2, w3, X, Y))
    leaves = [V, q, W1, W2, w3]
    for t in leaves:
        t.requires_grad_(True)
    m = ref_masks(V, q, W1, W2, w3)
    B = V.shape[0]
    yp = torch.stack([Y[b, perm[b]] for b in range(B)])
    loss = s1 * ((m * X[:, None] - yp) ** 2).sum() + s2 * ((m.sum(1) - 1.0) ** 2).sum()
    dV, dq, dW1, dW2, dw3 = torch.autograd.grad(loss, leaves)
    return dict(m=m.detach(), loss=loss.detach(), dpre=dV * (1 - V.detach() ** 2), dq=dq, dW1=dW1, dW2=dW2, dw3=dw3)


@functools.lru_cache(maxsize=None)
def case(K, B, T, F, seed=0):
    """Inputs (CPU fp32) and the fp64 reference of one parametrisation, computed once."""
    g = torch.Generator(device="cpu").manual_seed(13 * K + T + 1000 * seed)
    R = T * F
    k = 1.0 / E ** 0.5
    V = torch.tanh(torch.randn(B, R, E, generator=g))
    q = torch.randn(B, K, E, generator=g)
    W1 = torch.empty(E, E).uniform_(-k, k, generator=g)
    W2 = torch.empty(E, E).uniform_(-k, k, generator=g)
    w3 = torch.empty(1, E).uniform_(-k, k, generator=g)
    X = torch.rand(B, R, generator=g)
    Y = torch.rand(B, K, R, generator=g)
    perm = torch.stack([torch.randperm(K, generator=g) for _ in range(B)])
    s1, s2 = 1.0 / (B * K * R), 0.5 / (B * R)
    ref = ref_fused(V, q, W1, W2, w3, X, Y, perm, s1, s2)
    return dict(V=V, q=q, W1=W1, W2=W2, w3=w3, X=X, Y=Y, perm=perm, s1=s1, s2=s2, ref=ref)


GUARD = 64


def guarded(n, dev, dtype=torch.float32):
    """(whole, body): n elements followed by GUARD elements, all NaN (int: -1) before the call."""
    whole = torch.full((n + GUARD,), float("nan") if dtype.is_floating_point else -1, device=dev, dtype=dtype)
    return whole, whole[:n]


def run_fused(dev, c, K, B, T, F, passes=(0, 1), perm=None, in_place=False):
    """COST and / or GRAD + finalize on guarded buffers; returns every output and its whole buffer."""
    R = T * F
    V, q, W1, W2, w3, X, Y = (c[n].to(dev) for n in ("V", "q", "W1", "W2", "w3", "X", "Y"))
    perm = (c["perm"] if perm is None else perm).to(torch.int32).to(dev)
    nblk = _lib.query("dl4ss_attn_align_nblk", R)
    npart = _lib.query("dl4ss_attn_align_part_floats", B, K, nblk)
    o = {"nblk": nblk}
    for name, n in (("part_loss", B * nblk * (K * K + 1)), ("part", npart), ("dpre", B * R * E), ("mask", B * K * R),
                    ("pred", B * K * R), ("loss", 3), ("dq", B * K * E), ("dW1", E * E), ("dW2", E * E), ("dw3", E)):
        o[name + "_whole"], o[name] = guarded(n, dev)
    dpre = V if in_place else o["dpre"]
    st = _lib.stream_ptr()
    for pass_ in passes:
        _lib.call("dl4ss_mask_attn_align_loss", pass_, B, K, T, F, E, _lib.ptr(V), _lib.ptr(q), _lib.ptr(W1),
                  _lib.ptr(W2), _lib.ptr(w3), _lib.ptr(X), R, _lib.ptr(Y), K * R, R, _lib.ptr(perm), c["s1"], c["s2"],
                  _lib.ptr(dpre) if pass_ else None, _lib.ptr(o["part_loss"]), _lib.ptr(o["part"]) if pass_ else None,
                  npart, _lib.ptr(o["mask"]) if pass_ == 0 else None, _lib.ptr(o["pred"]) if pass_ == 0 else None, st)
    if 1 in passes:
        _lib.call("dl4ss_loss_finalize", _lib.ptr(o["part_loss"]), B, K, nblk, _lib.ptr(perm), c["s1"], c["s2"],
                  _lib.ptr(o["loss"]), None, E, None, st)
        _lib.call("dl4ss_attn_align_finalize", _lib.ptr(o["part"]), npart, B, K, T, F, _lib.ptr(q), _lib.ptr(W2),
                  _lib.ptr(o["dq"]), _lib.ptr(o["dW1"]), _lib.ptr(o["dW2"]), _lib.ptr(o["dw3"]), st)
    torch.cuda.synchronize()
    if in_place:
        o["dpre"] = V
    return o


def rel_max(got, ref):
    return float((got.double().cpu().reshape(ref.shape) - ref).abs().max()) / float(ref.abs().max())


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("B,T,F", SHAPES)
def test_align_fused_matches_fp64(dev, K, B, T, F):
    c = case(K, B, T, F)
    ref = c["ref"]
    o = run_fused(dev, c, K, B, T, F)
    R = T * F
    errs = {n: rel_max(o[n], ref[n]) for n in ("dq", "dW1", "dW2", "dw3")}
    errs["dpre"] = rel_max(o["dpre"], ref["dpre"])
    errs["loss"] = abs(float(o["loss"][0]) - float(ref["loss"])) / abs(float(ref["loss"]))
    errs["mask"] = float((o["mask"].double().cpu().view(B, K, R) - ref["m"]).abs().max())
    print("align fused", (K, B, T, F), errs)
    assert torch.allclose(o["mask"].double().cpu().view(B, K, R), ref["m"], rtol=1e-5, atol=1e-6)
    pred_ref = ref["m"] * c["X"].double()[:, None]
    assert torch.allclose(o["pred"].double().cpu().view(B, K, R), pred_ref, rtol=1e-5, atol=1e-6)
    assert errs["loss"] <= 1e-5
    for n in ("dq", "dW1", "dW2", "dw3"):
        assert errs[n] <= 1e-4, (n, errs)
    assert errs["dpre"] <= 1e-5, errs


def test_align_fused_in_place_over_v(dev):
    """dPre written over V itself (the training step's use) is bitwise the out-of-place result."""
    K, B, T, F = 2, 2, 33, 129
    c = case(K, B, T, F)
    a = run_fused(dev, c, K, B, T, F, passes=(1,))
    b = run_fused(dev, c, K, B, T, F, passes=(1,), in_place=True)
    assert torch.equal(a["dpre"].view(-1), b["dpre"].view(-1))
    for n in ("dq", "dW1", "dW2", "dw3", "loss"):
        assert torch.equal(a[n], b[n]), n


def pit_case(K, B, T, F, seed=0):
    """Targets built from the fp64 reference's own masks under a known non-identity permutation per
    utterance: Y[b, j] = m_ref[b, pi_b^-1(j)] X[b] (1 + 0.01 noise), so channel k's target is pi_b(k)."""
    c = dict(case(K, B, T, F, seed))
    g = torch.Generator(device="cpu").manual_seed(5 * K + B)
    perms = [p for p in itertools.permutations(range(K)) if p != tuple(range(K))]
    pi = torch.tensor([perms[b % len(perms)] for b in range(B)])
    m = c["ref"]["m"]
    X = c["X"].double()
    Y = torch.empty_like(m)
    for b in range(B):
        for k in range(K):
            Y[b, pi[b, k]] = m[b, k] * X[b] * (1 + 0.01 * torch.randn(m.shape[-1], generator=g, dtype=torch.float64))
    c["Y"] = Y.float()
    # the condition on the inputs, in fp64: the best permutation's cost is below 0.1 x the second best
    pred = m * X[:, None]
    C = ((pred[:, :, None] - c["Y"].double()[:, None]) ** 2).sum(-1)
    allp = list(itertools.permutations(range(K)))
    costs = torch.stack([sum(C[:, k, p[k]] for k in range(K)) for p in allp], 1)
    srt, idx = costs.sort(1)
    assert bool((srt[:, 0] < 0.1 * srt[:, 1]).all()), srt
    assert all(allp[int(idx[b, 0])] == tuple(pi[b].tolist()) for b in range(B))
    return c, pi


# (the K = 3 seed is the first whose three queries give masks distinct enough for the 0.1 margin, chosen
# on the fp64 reference alone: two similar masks make the second-best permutation cheap)
@pytest.mark.parametrize("K,B,T,F,seed", [(2, 3, 7, 129, 0), (3, 3, 7, 129, 3), (2, 2, 33, 129, 0)])
def test_align_pit_selects_known_permutation(dev, K, B, T, F, seed):
    c, pi = pit_case(K, B, T, F, seed)  # (asserts the margin before any GPU call)
    o = run_fused(dev, c, K, B, T, F, passes=(0,))
    perm = torch.full((B, K), -1, dtype=torch.int32, device=dev)
    _lib.call("dl4ss_pit_select", _lib.ptr(o["part_loss"]), B, K, o["nblk"], _lib.ptr(perm), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(perm.cpu().long(), pi)


def test_align_grad_bitwise_reproducible_and_isolated(dev):
    """Two GRAD launches agree bit for bit; every output is fully written (no NaN left of the NaN
    fill) and the guard region behind each buffer is untouched."""
    K, B, T, F = 3, 2, 33, 129
    c = case(K, B, T, F)
    a = run_fused(dev, c, K, B, T, F)
    b = run_fused(dev, c, K, B, T, F)
    for n in ("dpre", "dq", "dW1", "dW2", "dw3", "loss", "part", "part_loss", "mask", "pred"):
        assert torch.equal(a[n], b[n]), n
        assert not torch.isnan(a[n]).any(), n
        assert torch.isnan(a[n + "_whole"][a[n].numel():]).all(), n
    # the COST pass alone writes neither dPre nor the gradient partials
    o = run_fused(dev, c, K, B, T, F, passes=(0,))
    assert torch.isnan(o["dpre_whole"]).all() and torch.isnan(o["part_whole"]).all()
    assert not torch.isnan(o["part_loss"]).any() and torch.isnan(o["part_loss_whole"][o["part_loss"].numel():]).all()


def test_align_rejects_bad_arguments(dev):
    c = case(1, 1, 5, 37)
    V, q, W1, W2, w3 = (c[n].to(dev) for n in ("V", "q", "W1", "W2", "w3"))
    m = torch.empty(1, 185, device=dev)
    with pytest.raises(RuntimeError):  # E != 50
        _lib.call("dl4ss_attn_align_fwd", _lib.ptr(V), _lib.ptr(q), E, _lib.ptr(W1), _lib.ptr(W2), _lib.ptr(w3), 1, 185,
                  48, _lib.ptr(m), 185, _lib.stream_ptr())
    with pytest.raises(RuntimeError):  # NULL weights
        _lib.call("dl4ss_attn_align_fwd", _lib.ptr(V), _lib.ptr(q), E, None, _lib.ptr(W2), _lib.ptr(w3), 1, 185, E,
                  _lib.ptr(m), 185, _lib.stream_ptr())
    with pytest.raises(RuntimeError):  # mask stride below R
        _lib.call("dl4ss_attn_align_fwd", _lib.ptr(V), _lib.ptr(q), E, _lib.ptr(W1), _lib.ptr(W2), _lib.ptr(w3), 1, 185,
                  E, _lib.ptr(m), 100, _lib.stream_ptr())


# ------------------------------------------------------------------ module-level forward / backward
@functools.lru_cache(maxsize=None)
def mod_case(Bq, R):
    g = torch.Generator(device="cpu").manual_seed(Bq + R)
    k = 1.0 / E ** 0.5
    V = torch.tanh(torch.randn(Bq, R, E, generator=g))
    q = torch.randn(Bq, E, generator=g)
    W1, W2 = (torch.empty(E, E).uniform_(-k, k, generator=g) for _ in range(2))
    w3 = torch.empty(1, E).uniform_(-k, k, generator=g)
    dmask = torch.randn(Bq, R, generator=g)
    leaves = [t.double().clone().requires_grad_(True) for t in (V, q, W1, W2, w3)]
    m = ref_masks(leaves[0], leaves[1][:, None], *leaves[2:])[:, 0]
    grads = torch.autograd.grad(m, leaves, dmask.double())
    return dict(V=V, q=q, W1=W1, W2=W2, w3=w3, dmask=dmask, m=m.detach(),
                ref=dict(zip(("dV", "dq", "dW1", "dW2", "dw3"), grads)))


def mod_bwd(dev, c, Bq, R, dV):
    t = {n: c[n].to(dev) for n in ("V", "q", "W1", "W2", "w3", "dmask")}
    npart = _lib.query("dl4ss_attn_align_part_floats", Bq, 1, _lib.query("dl4ss_attn_align_nblk", R))
    part = torch.empty(npart, device=dev)
    out = dict(dq=torch.empty(Bq, E, device=dev), dW1=torch.empty(E, E, device=dev), dW2=torch.empty(E, E, device=dev),
               dw3=torch.empty(1, E, device=dev))
    _lib.call("dl4ss_attn_align_bwd", _lib.ptr(t["V"]), _lib.ptr(t["q"]), E, _lib.ptr(t["W1"]), _lib.ptr(t["W2"]),
              _lib.ptr(t["w3"]), _lib.ptr(t["dmask"]), Bq, R, E, _lib.ptr(dV), _lib.ptr(part), npart, _lib.ptr(out["dq"]),
              _lib.ptr(out["dW1"]), _lib.ptr(out["dW2"]), _lib.ptr(out["dw3"]), _lib.stream_ptr())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("Bq,R", [(4, 129 * 9), (1, 185)])
def test_align_module_kernels_match_fp64(dev, Bq, R):
    c = mod_case(Bq, R)
    t = {n: c[n].to(dev) for n in ("V", "q", "W1", "W2", "w3")}
    mask = torch.empty(Bq, R, device=dev)
    _lib.call("dl4ss_attn_align_fwd", _lib.ptr(t["V"]), _lib.ptr(t["q"]), E, _lib.ptr(t["W1"]), _lib.ptr(t["W2"]),
              _lib.ptr(t["w3"]), Bq, R, E, _lib.ptr(mask), R, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.allclose(mask.double().cpu(), c["m"], rtol=1e-5, atol=1e-6)
    dV = torch.zeros(Bq, R, E, device=dev)
    out = mod_bwd(dev, c, Bq, R, dV)
    errs = {n: rel_max(out[n], c["ref"][n]) for n in out}
    errs["dV"] = rel_max(dV, c["ref"]["dV"])
    print("align module", (Bq, R), errs)
    for n in ("dq", "dW1", "dW2", "dw3"):
        assert errs[n] <= 1e-4, (n, errs)
    assert errs["dV"] <= 1e-5, errs
    # dV accumulates: a second call onto the same buffer doubles it, bit for bit
    first = dV.clone()
    out2 = mod_bwd(dev, c, Bq, R, dV)
    assert torch.equal(dV, 2 * first)
    # dV = NULL is accepted and leaves the other gradients as they were
    out3 = mod_bwd(dev, c, Bq, R, None)
    for n in out:
        assert torch.equal(out[n], out2[n]) and torch.equal(out[n], out3[n]), n


def test_align_fwd_mask_stride_shares_v(dev):
    """K = 2 queries over one V with a mask row stride of K R: bitwise two stride-R calls."""
    K, B, T, F = 2, 3, 7, 129
    R = T * F
    c = case(K, B, T, F)
    V, q, W1, W2, w3 = (c[n].to(dev) for n in ("V", "q", "W1", "W2", "w3"))
    st = _lib.stream_ptr()
    whole, _ = guarded(B * K * R, dev)
    mask = whole[:B * K * R].view(B, K, R)
    for k in range(K):
        _lib.call("dl4ss_attn_align_fwd", _lib.ptr(V), ctypes.c_void_p(q.data_ptr() + 4 * k * E), K * E, _lib.ptr(W1),
                  _lib.ptr(W2), _lib.ptr(w3), B, R, E, ctypes.c_void_p(mask.data_ptr() + 4 * k * R), K * R, st)
    singles = []
    for k in range(K):
        qk = q[:, k].contiguous()
        mk = torch.empty(B, R, device=dev)
        _lib.call("dl4ss_attn_align_fwd", _lib.ptr(V), _lib.ptr(qk), E, _lib.ptr(W1), _lib.ptr(W2), _lib.ptr(w3), B, R,
                  E, _lib.ptr(mk), R, st)
        singles.append(mk)
    torch.cuda.synchronize()
    assert torch.equal(mask, torch.stack(singles, 1))
    assert torch.isnan(whole[B * K * R:]).all()
    assert torch.allclose(mask.double().cpu(), c["ref"]["m"], rtol=1e-5, atol=1e-6)


def test_align_module_kernels_match_reference_class(dev):
    """tests/golden/ref_align.npz: inputs, weights, mask and autograd gradients of the reference's own
    ATTENTION(50, 'align') class on torch-CPU fp32 (tests/golden/make_ref_align_fixture.py)."""
    import os

    import numpy as np

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_align.npz"))
    B, T, F, _ = z["V"].shape
    R = T * F
    c = {n: torch.from_numpy(z[n]) for n in z.files}
    c["V"], c["dmask"] = c["V"].reshape(B, R, E), c["dmask"].reshape(B, R)
    t = {n: c[n].to(dev) for n in ("V", "q", "W1", "W2", "w3")}
    mask = torch.empty(B, R, device=dev)
    _lib.call("dl4ss_attn_align_fwd", _lib.ptr(t["V"]), _lib.ptr(t["q"]), E, _lib.ptr(t["W1"]), _lib.ptr(t["W2"]),
              _lib.ptr(t["w3"]), B, R, E, _lib.ptr(mask), R, _lib.stream_ptr())
    dV = torch.zeros(B, R, E, device=dev)
    out = mod_bwd(dev, c, B, R, dV)
    assert torch.allclose(mask.cpu(), c["mask"].reshape(B, R), rtol=1e-5, atol=1e-6)
    for n in ("dq", "dW1", "dW2", "dw3"):
        assert rel_max(out[n], c[n].double()) <= 1e-4, n
    assert rel_max(dV, c["dV"].double()) <= 1e-5
