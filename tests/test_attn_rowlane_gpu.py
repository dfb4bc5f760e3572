"""The row-per-lane kernel of the fused mask attention + loss (attn_kernel: one lane per (b, t, f) row) at kernel
level, in the forms no other kernel-level test reaches: the plain (non-adversarial) kernel on fp32 V with fp32 dPre,
on bf16 V with fp32 dPre, cRM at K = 3 with bf16 dPre (the one bf16-dPre form not routed to the quad kernel), and
the fall-back from the quad kernel for a V that is not 16-B aligned (its word-per-lane bf16 dPre copy-out), plain and
adversarial.

Reference: the fp64 restatements of tests/test_attn_gpu.py (magnitude and cRM); the adversarial gradient from the
fp64 one of tests/test_attn_adv_gpu.py.  Shapes, those of test_attn_gpu.py: (3, 7, 129) a ragged last tile,
utterance bases and (ld_pad 6) dPre rows not 16-B aligned; (2, 33, 129) five blocks per utterance, three frames per
tile; (1, 5, 37) less than one tile.  Bars, the existing ones for the same quantities: magnitude masks (rtol 1e-5,
atol 1e-6) and every loss 1e-5 relative, dq 1e-4 of its largest element, bf16 dPre 2^-8 max|dPre| + 1e-12 with the
NaN-prefilled row padding untouched, fp32 dPre 1e-4 of its largest element.

The cRM masks take test_attn_gpu.py's bar for cRM masks, rtol 1e-4 / atol 1e-5, not the magnitude masks' one: the
kernel evaluates M = -10 log((10 - Mc) / (10 + Mc)) in fp32 "as the reference" does, and the roundings of 10 - Mc,
10 + Mc and their quotient (2^-24 each, of values near 1 where M is small) alone leave an absolute error of
10 * 3 * 2^-24 = 1.8e-6 in M before tanhf's and logf's own, above atol 1e-6.

The COST pass is asked for pred_out as well as mask_out.  Magnitude: pred = mask |X| at the masks' bar, as
test_attn_align_bf16_gpu.py checks it.  cRM: P = M (x) X, each component a sum of two products, so the masks' bar
propagates as (atol + rtol |M_re|) |x_.| + (atol + rtol |M_im|) |x_.| per component, plus atol once for the two
fp32 products' own roundings (2^-24 |M| |X| < 2e-6)."""
import functools

import pytest
import torch

from dl4ss_amd import _lib
from test_attn_adv_gpu import _ref as _ref_adv
from test_attn_gpu import _ref, _ref_crm

pytestmark = pytest.mark.gpu
E = 50
P = _lib.ptr
SHAPES = [(3, 7, 129, 6), (2, 33, 129, 2), (1, 5, 37, 0)]


@functools.lru_cache(maxsize=None)
def _case(crm, K, B, T, F, vtype, adv=False):
    """Fixed-seed inputs (on the host) and their fp64 reference, computed once; V holds bf16 values for vtype bf16."""
    g = torch.Generator(device="cpu").manual_seed(13 * K + T + 5 * crm)
    R = T * F
    QW = 2 * E if crm else E
    V = torch.tanh(torch.randn(B, R, E, generator=g))
    c = {"V": V.to(torch.bfloat16).float() if vtype == "bf16" else V,
         "q": (0.05 if crm else 0.3) * torch.randn(B, K, QW, generator=g),
         "X": torch.rand(B, R, 2, generator=g) if crm else torch.rand(B, R, generator=g),
         "Y": torch.rand(B, K, R, 2, generator=g) if crm else torch.rand(B, K, R, generator=g),
         "perm": torch.stack([torch.randperm(K, generator=g) for _ in range(B)]),
         "s1": 1.0 / (B * K * R), "s2": 0.0 if crm else 0.5 / (B * R), "gext": None}
    if crm:
        ref = _ref_crm(c["V"], c["q"], c["X"], c["Y"], c["perm"], c["s1"])
    else:
        ref = _ref(c["V"], c["q"], c["X"], c["Y"], c["perm"], c["s1"], c["s2"])
    c["m"], c["loss"], c["dpre"], c["dq"] = ref
    if adv:  # the second gradient at the prediction: dPre and dq from the adversarial reference
        c["gext"] = 8.0 * c["s1"] * torch.randn(B, K, R, generator=g)
        c["dpre"], c["dq"] = _ref_adv(c["V"], c["q"], c["X"], c["Y"], c["perm"], c["s1"], c["s2"], c["gext"])
    return c


def _device_v(dev, c, vtype, misalign):
    """V on the device; misalign: a view that starts 4 bytes past a 16-B boundary of a larger buffer."""
    V = c["V"].to(torch.bfloat16) if vtype == "bf16" else c["V"]
    if not misalign:
        return V.to(dev)
    off = 4 // V.element_size()
    buf = torch.zeros(V.numel() + 16, dtype=V.dtype, device=dev)
    view = buf[off:off + V.numel()].view(V.shape)
    view.copy_(V)
    assert view.data_ptr() % 16 == 4
    return view


def _run_and_check(dev, crm, K, B, T, F, ld_pad, vtype, dpre, adv=False, misalign=False):
    """COST then GRAD (with gext: through the adversarial entry point), the finalize, and every bar.
    dpre "fp32": dPre given, no dPre_bf16; "bf16": dPre_bf16 given to both passes, as the steps do."""
    c = _case(crm, K, B, T, F, vtype, adv)
    R, QW = T * F, (2 * E if crm else E)
    Vd = _device_v(dev, c, vtype, misalign)
    q, X, Y = (c[n].to(dev) for n in ("q", "X", "Y"))
    perm = c["perm"].to(torch.int32).to(dev)
    gext = c["gext"].to(dev) if adv else None
    nblk = _lib.query("dl4ss_attn_nblk", T, F)
    part_loss = torch.full((B, nblk, K * K + 1), float("nan"), device=dev)
    part_dq = torch.full((B, nblk, K, QW), float("nan"), device=dev)
    mask = torch.full((B, K, R, 2) if crm else (B, K, R), float("nan"), device=dev)
    pred = torch.full_like(mask, float("nan"))
    ldpb = F * E + ld_pad
    bf = dpre == "bf16"
    dpre32 = None if bf else torch.full((B, R, E), float("nan"), device=dev)
    dpreb = torch.full((B * T, ldpb), float("nan"), device=dev).to(torch.bfloat16) if bf else None
    st = _lib.stream_ptr()
    sfx = "_bf16v" if vtype == "bf16" else ""
    head = (B, K, T, F, E, P(Vd), P(q), P(X), R, P(Y), K * R, R, P(perm), c["s1"], c["s2"])
    _lib.call("dl4ss_mask_attn_loss" + (sfx or "_ex"), 0, crm, *head, None, P(dpreb), ldpb if bf else 0, P(part_loss),
              None, P(mask), P(pred), st)
    tail = (P(dpre32), P(dpreb), ldpb if bf else 0, P(part_loss), P(part_dq), None, None, st)
    if adv:
        _lib.call("dl4ss_mask_attn_loss_adv" + sfx, *head, P(gext), *tail)
    else:
        _lib.call("dl4ss_mask_attn_loss" + (sfx or "_ex"), 1, crm, *head, *tail)
    loss = torch.full((3,), float("nan"), device=dev)
    dq = torch.full((B, K, QW), float("nan"), device=dev)
    _lib.call("dl4ss_loss_finalize", P(part_loss), B, K, nblk, P(perm), c["s1"], c["s2"], P(loss), P(part_dq), QW,
              P(dq), st)
    torch.cuda.synchronize()
    got = dpreb[:, :F * E].float().view(B, T, F, E).reshape(B, R, E) if bf else dpre32
    got = got.double().cpu()
    dmax = float(c["dpre"].abs().max())
    m_rtol, m_atol = (1e-4, 1e-5) if crm else (1e-5, 1e-6)
    e_m = float(((mask.double().cpu() - c["m"]).abs() / (m_atol + m_rtol * c["m"].abs())).max())
    e_loss = abs(float(loss[0]) - float(c["loss"])) / abs(float(c["loss"]))
    e_dq = float((dq.double().cpu() - c["dq"]).abs().max()) / float(c["dq"].abs().max())
    e_dp = float((got - c["dpre"]).abs().max())
    print(f"crm={crm} K={K} {(B, T, F, ld_pad)} V {vtype} dPre {dpre} adv={adv} misalign={misalign}: mask "
          f"{e_m:.3f} of its bar, loss {e_loss:.3e}, dq {e_dq:.3e} of max, dPre {e_dp / dmax:.3e} of max")
    assert torch.allclose(mask.double().cpu(), c["m"], rtol=m_rtol, atol=m_atol)
    Xd, M, pr = c["X"].double(), c["m"], pred.double().cpu()
    if crm:
        xr, xi = Xd[..., 0][:, None], Xd[..., 1][:, None]
        p_ref = torch.stack([M[..., 0] * xr - M[..., 1] * xi, M[..., 0] * xi + M[..., 1] * xr], -1)
        br, bi = m_atol + m_rtol * M[..., 0].abs(), m_atol + m_rtol * M[..., 1].abs()
        bound = torch.stack([br * xr.abs() + bi * xi.abs(), br * xi.abs() + bi * xr.abs()], -1) + m_atol
        assert bool(((pr - p_ref).abs() <= bound).all()), float(((pr - p_ref).abs() / bound).max())
    else:
        assert torch.allclose(pr, M * Xd[:, None, :], rtol=m_rtol, atol=m_atol)
    assert e_loss <= 1e-5
    assert not torch.isnan(dq).any() and e_dq <= 1e-4
    assert not torch.isnan(got).any()
    assert e_dp <= (2 ** -8 * dmax + 1e-12 if bf else 1e-4 * dmax)
    if bf and ld_pad:  # the row padding beyond F * E is never written
        assert torch.isnan(dpreb[:, F * E:].float()).all()


@pytest.mark.parametrize("crm", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("B,T,F,ld_pad", SHAPES)
def test_rowlane_fp32v_fp32_dpre_matches_fp64(dev, B, T, F, ld_pad, K, crm):
    """fp32 V with fp32 dPre, COST and GRAD: magnitude under a random permutation, and cRM."""
    _run_and_check(dev, crm, K, B, T, F, ld_pad, "fp32", "fp32")


@pytest.mark.parametrize("crm", [0, 1])
@pytest.mark.parametrize("B,T,F,ld_pad", SHAPES)
def test_rowlane_bf16v_fp32_dpre_matches_fp64(dev, B, T, F, ld_pad, crm):
    """bf16 V with fp32 dPre in the GRAD pass (dPre given, no dPre_bf16), K = 2."""
    _run_and_check(dev, crm, 2, B, T, F, ld_pad, "bf16", "fp32")


@pytest.mark.parametrize("vtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,F,ld_pad", SHAPES)
def test_rowlane_crm_k3_bf16_dpre_matches_fp64(dev, B, T, F, ld_pad, vtype):
    """cRM at K = 3 with bf16 dPre: the bf16-dPre form that stays on the row-per-lane kernel."""
    _run_and_check(dev, 1, 3, B, T, F, ld_pad, vtype, "bf16")


@pytest.mark.parametrize("adv", [False, True])
@pytest.mark.parametrize("vtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,F,ld_pad", SHAPES)
def test_rowlane_unaligned_v_bf16_dpre_matches_fp64(dev, B, T, F, ld_pad, vtype, adv):
    """A V that starts 4 bytes past a 16-B boundary, bf16 dPre, magnitude K = 2: the quad kernel's loads need
    16-B alignment, so the launch falls back to the row-per-lane kernel and its bf16 dPre branch."""
    _run_and_check(dev, 0, 2, B, T, F, ld_pad, vtype, "bf16", adv=adv, misalign=True)
