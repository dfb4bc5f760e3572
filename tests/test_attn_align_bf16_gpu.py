"""The bf16 step's forms of the ATTENTION 'align' kernel (dl4ss_mask_attn_align_loss_ex, include/dl4ss_align.h):
V read as bf16, dPre written as bf16 rows at the GEMMs' pitch, against the fp64 restatement of
tests/test_attn_align_gpu.py evaluated ON THE bf16 VALUES OF V upcast to fp64 -- V's rounding is an input, not an
error.  The arithmetic is the fp32 kernel's, so masks, loss, dq, dW1, dW2, dw3 keep that test's tolerances (masks
rtol 1e-5 / atol 1e-6, loss 1e-5 relative, the four gradients 1e-4 of the tensor's largest element), and every dPre
element is within 2^-8 |ref| + 1e-6 max|ref|: one bf16 rounding (half a unit in the last of 8 significant bits, at
most 2^-8 |x|) on top of the fp32 kernel's measured error (4.7e-7 of the largest element).

Shapes (E = 50, K = 1, 2, 3): (2, 3, 129) one full tile plus a ragged one, utterance bases not 16-B aligned;
(3, 9, 129) more rows than one block's four tiles; (1, 1, 7) a tile of 7 rows; (2, 4, 129) aligned bases."""
import functools

import pytest
import torch

from dl4ss_amd import _lib
from test_attn_align_gpu import E, case, ref_fused, rel_max

pytestmark = pytest.mark.gpu
SHAPES = [(2, 3, 129), (3, 9, 129), (1, 1, 7), (2, 4, 129)]
SENT = 0x7A5B  # the bf16 dPre buffer's prefill (a finite bf16 no result equals by chance in every element)
ENTRY = "dl4ss_mask_attn_align_loss_ex"


def pad8(n):
    return (n + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def bcase(K, B, T, F, order):
    """test_attn_align_gpu.case with V rounded to bf16 and the fp64 reference on those values, computed once.
    order "label": the identity (perm NULL); "perm": a non-identity permutation in every utterance where K > 1."""
    c = dict(case(K, B, T, F))
    c["Vb"] = c["V"].to(torch.bfloat16)
    c["V"] = c["Vb"].float()
    c["perm"] = torch.stack([torch.arange(K) if order == "label" else (torch.arange(K) + 1 + b % max(K - 1, 1)) % K
                             for b in range(B)])
    c["order"] = order
    c["ref"] = ref_fused(c["V"], c["q"], c["W1"], c["W2"], c["w3"], c["X"], c["Y"], c["perm"], c["s1"], c["s2"])
    return c


def run(dev, c, K, B, T, F, vform, ld=None, passes=(0, 1), **over):
    """COST and / or GRAD + the two finalizes through the new entry point; every output NaN- / sentinel-filled
    before.  vform "bf16": V_bf16; "fp32": the same values as fp32 V.  Returns the outputs and, per pass, a copy of
    the bf16 dPre buffer taken right after it."""
    R = T * F
    ld = pad8(F * E) if ld is None else ld
    q, W1, W2, w3, X, Y = (c[n].to(dev) for n in ("q", "W1", "W2", "w3", "X", "Y"))
    V = c["Vb"].to(dev) if vform == "bf16" else c["V"].to(dev)
    perm = None if c["order"] == "label" else c["perm"].to(torch.int32).to(dev)
    nblk = _lib.query("dl4ss_attn_align_nblk", R)
    npart = _lib.query("dl4ss_attn_align_part_floats", B, K, nblk)
    o = {"nblk": nblk, "ld": ld}
    for name, n in (("part_loss", B * nblk * (K * K + 1)), ("part", npart), ("mask", B * K * R), ("pred", B * K * R),
                    ("loss", 3), ("dq", B * K * E), ("dW1", E * E), ("dW2", E * E), ("dw3", E)):
        o[name] = torch.full((n,), float("nan"), device=dev)
    o["dpre_bits"] = torch.full((B * T, ld), SENT, device=dev, dtype=torch.int16)
    st = _lib.stream_ptr()
    for pass_ in passes:
        kw = dict(pass_=pass_, B=B, K=K, T=T, F=F, E=E, V=_lib.ptr(V) if vform == "fp32" else None,
                  V_bf16=_lib.ptr(V) if vform == "bf16" else None, q=_lib.ptr(q), W1=_lib.ptr(W1), W2=_lib.ptr(W2),
                  w3=_lib.ptr(w3), X=_lib.ptr(X), x_bstride=R, Y=_lib.ptr(Y), y_bstride=K * R, y_kstride=R,
                  perm=_lib.ptr(perm), s1=c["s1"], s2=c["s2"], dPre=None, dPre_bf16=_lib.ptr(o["dpre_bits"]),
                  dpre_bf16_ld=ld, part_loss=_lib.ptr(o["part_loss"]), part=_lib.ptr(o["part"]) if pass_ else None,
                  part_floats=npart, mask_out=_lib.ptr(o["mask"]) if pass_ == 0 else None,
                  pred_out=_lib.ptr(o["pred"]) if pass_ == 0 else None, stream=st)
        kw.update(over)
        _lib.call(ENTRY, **kw)
        o[f"dpre_bits_after{pass_}"] = o["dpre_bits"].clone()
        o[f"part_loss_after{pass_}"] = o["part_loss"].clone()
    if 1 in passes:
        _lib.call("dl4ss_loss_finalize", _lib.ptr(o["part_loss"]), B, K, nblk, _lib.ptr(perm), c["s1"], c["s2"],
                  _lib.ptr(o["loss"]), None, E, None, st)
        _lib.call("dl4ss_attn_align_finalize", _lib.ptr(o["part"]), npart, B, K, T, F, _lib.ptr(q), _lib.ptr(W2),
                  _lib.ptr(o["dq"]), _lib.ptr(o["dW1"]), _lib.ptr(o["dW2"]), _lib.ptr(o["dw3"]), st)
    torch.cuda.synchronize()
    return o


def dpre_values(o, B, T, F):
    """the written columns of the bf16 dPre matrix as (B, T*F, E) fp64, and its padding columns' bits"""
    bits = o["dpre_bits"].view(B, T, o["ld"])
    vals = bits[:, :, :F * E].contiguous().view(torch.bfloat16).double().cpu().view(B, T * F, E)
    return vals, bits[:, :, F * E:]


def check_against_fp64(o, c, K, B, T, F, tag):
    ref, R = c["ref"], T * F
    errs = {n: rel_max(o[n], ref[n]) for n in ("dq", "dW1", "dW2", "dw3")}
    errs["loss"] = abs(float(o["loss"][0]) - float(ref["loss"])) / abs(float(ref["loss"]))
    errs["mask"] = float((o["mask"].double().cpu().view(B, K, R) - ref["m"]).abs().max())
    got, pad = dpre_values(o, B, T, F)
    bound = 2.0 ** -8 * ref["dpre"].abs() + 1e-6 * ref["dpre"].abs().max()
    errs["dpre_over_bound"] = float(((got - ref["dpre"]).abs() / bound).max())
    print("align bf16", tag, (K, B, T, F), c["order"], errs)
    assert torch.allclose(o["mask"].double().cpu().view(B, K, R), ref["m"], rtol=1e-5, atol=1e-6)
    assert torch.allclose(o["pred"].double().cpu().view(B, K, R), ref["m"] * c["X"].double()[:, None], rtol=1e-5,
                          atol=1e-6)
    assert errs["loss"] <= 1e-5, errs
    for n in ("dq", "dW1", "dW2", "dw3"):
        assert errs[n] <= 1e-4, (n, errs)
    assert bool(((got - ref["dpre"]).abs() <= bound).all()), errs
    # the pitch: the padding columns keep the prefill, and the COST pass wrote nothing at all
    assert bool((pad == SENT).all())
    assert bool((o["dpre_bits_after0"] == SENT).all())


@pytest.mark.parametrize("vform", ["bf16", "fp32"])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("B,T,F", SHAPES)
def test_align_bf16_forms_match_fp64(dev, B, T, F, K, vform):
    """COST + GRAD with bf16 dPre, V as bf16 and as fp32, in label order and under a non-identity perm."""
    for order in ("label", "perm"):
        c = bcase(K, B, T, F, order)
        if order == "perm" and K > 1:
            assert not any(torch.equal(p, torch.arange(K)) for p in c["perm"])
        check_against_fp64(run(dev, c, K, B, T, F, vform), c, K, B, T, F, vform)


@pytest.mark.parametrize("vform", ["bf16", "fp32"])
@pytest.mark.parametrize("B,T,F", [(2, 3, 129), (1, 1, 7)])
def test_align_bf16_dpre_pitch_with_unaligned_rows(dev, B, T, F, vform):
    """ld = F E + 10: even, but rows start 16-B aligned only every fourth frame (the head / tail words of the
    copy-out); the ten padding columns of every row keep the prefill."""
    K = 2
    c = bcase(K, B, T, F, "perm")
    o = run(dev, c, K, B, T, F, vform, ld=F * E + 10)
    check_against_fp64(o, c, K, B, T, F, vform + " ld+10")
    # the values do not depend on the pitch
    a, _ = dpre_values(o, B, T, F)
    b, _ = dpre_values(run(dev, c, K, B, T, F, vform), B, T, F)
    assert torch.equal(a, b)


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("B,T,F", SHAPES)
def test_align_cost_partials_equal_on_bf16_and_fp32_v(dev, B, T, F, K):
    """The COST pass's part_loss is the same, bit for bit, whether V arrives as bf16 or as the same values in fp32,
    through the new entry point or the fp32 one: dl4ss_pit_select cannot differ between a bf16 step and a check run.
    The GRAD pass's partials, masks and gradients agree in the same way."""
    c = bcase(K, B, T, F, "perm")
    a, b = run(dev, c, K, B, T, F, "bf16"), run(dev, c, K, B, T, F, "fp32")
    assert not torch.isnan(a["part_loss_after0"]).any()
    assert torch.equal(a["part_loss_after0"], b["part_loss_after0"])
    for n in ("part_loss", "part", "mask", "pred", "loss", "dq", "dW1", "dW2", "dw3", "dpre_bits"):
        assert torch.equal(a[n], b[n]), n
    R = T * F
    old = torch.full_like(a["part_loss"], float("nan"))
    t = {n: c[n].to(dev) for n in ("V", "q", "W1", "W2", "w3", "X", "Y")}  # (held until the launch has run)
    _lib.call("dl4ss_mask_attn_align_loss", 0, B, K, T, F, E, _lib.ptr(t["V"]), _lib.ptr(t["q"]), _lib.ptr(t["W1"]),
              _lib.ptr(t["W2"]), _lib.ptr(t["w3"]), _lib.ptr(t["X"]), R, _lib.ptr(t["Y"]), K * R, R, None, c["s1"],
              c["s2"], None, _lib.ptr(old), None, 0, None, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(old, a["part_loss_after0"])
    perm = [torch.full((B, K), -1, dtype=torch.int32, device=dev) for _ in range(2)]
    for p, o in zip(perm, (a, b)):
        _lib.call("dl4ss_pit_select", _lib.ptr(o["part_loss_after0"]), B, K, o["nblk"], _lib.ptr(p), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(perm[0], perm[1]) and int(perm[0].min()) >= 0


@pytest.mark.parametrize("vform", ["bf16", "fp32"])
def test_align_bf16_forms_bitwise_reproducible(dev, vform):
    """Two launches on the same inputs agree bit for bit in every output, and every output is fully written."""
    K, B, T, F = 3, 3, 9, 129
    c = bcase(K, B, T, F, "perm")
    a, b = run(dev, c, K, B, T, F, vform), run(dev, c, K, B, T, F, vform)
    for n in ("dpre_bits", "part", "part_loss", "part_loss_after0", "mask", "pred", "loss", "dq", "dW1", "dW2", "dw3"):
        assert torch.equal(a[n], b[n]), n
        if n != "dpre_bits":
            assert not torch.isnan(a[n]).any(), n
    assert bool((a["dpre_bits"][:, :F * E] != SENT).all())


def test_align_ex_fp32_v_fp32_dpre_is_the_fp32_entry(dev):
    """fp32 V with fp32 dPre through the new entry point is the existing kernel: bitwise dl4ss_mask_attn_align_loss,
    also in place over V."""
    K, B, T, F = 2, 2, 3, 129
    c = bcase(K, B, T, F, "perm")
    R = T * F
    nblk = _lib.query("dl4ss_attn_align_nblk", R)
    npart = _lib.query("dl4ss_attn_align_part_floats", B, K, nblk)
    t = {n: c[n].to(dev) for n in ("q", "W1", "W2", "w3", "X", "Y")}
    perm = c["perm"].to(torch.int32).to(dev)
    out = []
    for new in (False, True):
        V = c["V"].to(dev)
        pl, part = torch.full((B * nblk * (K * K + 1),), float("nan"), device=dev), torch.zeros(npart, device=dev)
        common = dict(pass_=1, B=B, K=K, T=T, F=F, E=E, V=_lib.ptr(V), q=_lib.ptr(t["q"]), W1=_lib.ptr(t["W1"]),
                      W2=_lib.ptr(t["W2"]), w3=_lib.ptr(t["w3"]), X=_lib.ptr(t["X"]), x_bstride=R, Y=_lib.ptr(t["Y"]),
                      y_bstride=K * R, y_kstride=R, perm=_lib.ptr(perm), s1=c["s1"], s2=c["s2"], dPre=_lib.ptr(V),
                      part_loss=_lib.ptr(pl), part=_lib.ptr(part), part_floats=npart, mask_out=None, pred_out=None,
                      stream=_lib.stream_ptr())
        if new:
            _lib.call(ENTRY, V_bf16=None, dPre_bf16=None, dpre_bf16_ld=0, **common)
        else:
            _lib.call("dl4ss_mask_attn_align_loss", **common)
        torch.cuda.synchronize()
        out.append((V, pl, part[:B * nblk * (2 * E * E + K * E + E)]))
    for x, y in zip(*out):
        assert torch.equal(x, y)




def test_align_ex_refuses_bad_arguments_and_writes_nothing(dev):
    """Every refused combination returns hipErrorInvalidValue before any launch: no output changes."""
    K, B, T, F = 2, 1, 1, 7
    c = bcase(K, B, T, F, "perm")
    R = T * F
    Vf, Vb = c["V"].to(dev), c["Vb"].to(dev)
    t = {n: c[n].to(dev) for n in ("q", "W1", "W2", "w3", "X", "Y")}
    nblk = _lib.query("dl4ss_attn_align_nblk", R)
    npart = _lib.query("dl4ss_attn_align_part_floats", B, K, nblk)
    bufs = {n: torch.full((k,), float("nan"), device=dev)
            for n, k in (("part_loss", B * nblk * (K * K + 1)), ("part", npart), ("mask", B * K * R),
                         ("pred", B * K * R), ("dpre", B * R * E))}
    bits = torch.full((B * T, pad8(F * E) + 8), SENT, device=dev, dtype=torch.int16)
    ptr = _lib.ptr
    bad = [  # (what, the passes it is refused in, the arguments that differ from a good call)
        ("both V pointers", (0, 1), dict(V=ptr(Vf))),
        ("neither V pointer", (0, 1), dict(V_bf16=None)),
        ("ld < F E", (0, 1), dict(dpre_bf16_ld=F * E - 2)),
        ("ld odd", (0, 1), dict(dpre_bf16_ld=F * E + 1)),
        ("E != 50", (0, 1), dict(E=48)),
        ("K = 0", (0, 1), dict(K=0)),
        ("K = 4", (0, 1), dict(K=4)),
        ("pass = 2", (2,), {}),
        ("V_bf16 not 4-B aligned", (0, 1), dict(V_bf16=_lib.ctypes.c_void_p(Vb.data_ptr() + 2))),
        ("dPre_bf16 not 4-B aligned", (0, 1), dict(dPre_bf16=_lib.ctypes.c_void_p(bits.data_ptr() + 2))),
        ("both dPre pointers", (1,), dict(dPre=ptr(bufs["dpre"]))),
        ("neither dPre pointer", (1,), dict(dPre_bf16=None)),
        ("bf16 V with fp32 dPre", (1,), dict(dPre=ptr(bufs["dpre"]), dPre_bf16=None)),
        ("part too small", (1,), dict(part_floats=npart - 1)),
        ("no part", (1,), dict(part=None)),
    ]
    fn = getattr(_lib.lib(), ENTRY)
    for what, passes, over in bad:
        for pass_ in passes:
            kw = dict(pass_=pass_, B=B, K=K, T=T, F=F, E=E, V=None, V_bf16=ptr(Vb), q=ptr(t["q"]), W1=ptr(t["W1"]),
                      W2=ptr(t["W2"]), w3=ptr(t["w3"]), X=ptr(t["X"]), x_bstride=R, Y=ptr(t["Y"]), y_bstride=K * R,
                      y_kstride=R, perm=None, s1=c["s1"], s2=c["s2"], dPre=None, dPre_bf16=ptr(bits),
                      dpre_bf16_ld=bits.stride(0), part_loss=ptr(bufs["part_loss"]), part=ptr(bufs["part"]),
                      part_floats=npart, mask_out=ptr(bufs["mask"]), pred_out=ptr(bufs["pred"]),
                      stream=_lib.stream_ptr())
            kw.update(over)
            assert fn(*_lib.bind(ENTRY, (), kw)) == 1, (what, pass_)  # hipErrorInvalidValue
    with pytest.raises(RuntimeError, match=ENTRY):  # and through _lib.call: raised, with the entry point's name
        _lib.call(ENTRY, **dict(kw, part=None))
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b).all()) for b in bufs.values())
    assert bool((bits == SENT).all())
    assert torch.equal(Vf.cpu(), c["V"]) and torch.equal(Vb.cpu(), c["Vb"])
