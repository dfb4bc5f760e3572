"""Keras 1's LSTM cell in the generic fp32 recurrence kernels (DL4SS_RNN_HARD_GATES, ``ops.HARD_GATES``): forward and
BPTT through ``ops.birnn_fwd`` / ``ops.birnn_bwd`` against the fp64 restatement of tests/keras_cell_ref.py.

The inputs (keras_cell_ref.case: G ~ N(0, 9)) make every gate saturate at both ends -- asserted on the fp64
reference -- so hs(z) = 0.2 z + 0.5 without the clip would fail.  Forward (out, act, cs, hprev) within 2e-5 absolute;
the device's saturation pattern equals the fp64 one except at gates within 1e-4 of a kink, at most 0.1 % of them; the
fp64 gradients are then taken with the device's pattern and dG must match within 1e-4 of its largest element (the
bounds of the logistic tests of the same kernels, tests/test_kernels_gpu.py, tests/test_voiceprint_birnn_h25_gpu.py).

Shapes (B, T, H), the smallest that reach each path: (5, 9, 25) the small plan whose second unit group is partial, at
batch chunks of 1; (64, 3, 25) chunks of 2; (3, 1, 40), (4, 2, 40) the T = 1 / 2 edges; (9, 4, 300) and (32, 3, 300)
the H = 300 plan (whose logistic form runs compile-time-sliced kernels, the hard form the runtime-bounds ones) at
narrow and wide chunks; (1, 5, 600) the large-H plan and (32, 2, 600) its sub-batch split (no plan at B = 32).
"""
import pytest
import torch

import keras_cell_ref as K
from dl4ss_amd import _lib, ops

pytestmark = pytest.mark.gpu

SHAPES = [(5, 9, 25), (64, 3, 25), (3, 1, 40), (4, 2, 40), (9, 4, 300), (32, 3, 300), (1, 5, 600), (32, 2, 600)]
TOL_FWD, TOL_GRAD = 2e-5, 1e-4


class Layer:
    """Device buffers of one layer for (B, T, H) and the two calls."""

    def __init__(self, dev, B, T, H, c, cell="lstm"):
        self.B, self.T, self.H, self.cell = B, T, H, cell
        ng = 4 if cell == "lstm" else 3
        self.G = c["G"][..., :ng * H].contiguous().to(dev)
        self.w_hh = c["w_hh"][:, :ng * H].contiguous().to(dev)
        self.b_hh = c["b_hh"][:, :ng * H].contiguous().to(dev)
        self.wsn = _lib.query("dl4ss_birnn_workspace_bytes", ops.CELLS[cell], B, H)
        assert self.wsn > 0
        self.ws = torch.empty((self.wsn + 7) // 8, dtype=torch.int64, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.dev, self.ng = dev, ng

    def forward(self, flags, precision="fp32", **extra):
        B, T, H, dev = self.B, self.T, self.H, self.dev
        r = dict(out=torch.full((B, T, 2 * H), 7.0, device=dev), hprev=torch.empty(B, T, 2 * H, device=dev),
                 act=torch.empty(B, T, 2, 4 * H, device=dev), cs=torch.empty(B, T, 2, H, device=dev))
        ops.birnn_fwd(self.cell, B, T, H, G=self.G, w_hh=self.w_hh, b_hh=self.b_hh, ws=self.ws, ws_bytes=self.wsn,
                      status=self.status, precision=precision, flags=flags,
                      cs=r["cs"] if self.cell == "lstm" else None,
                      **{k: v for k, v in r.items() if k != "cs"}, **extra)
        torch.cuda.synchronize()
        assert int(self.status.item()) == 0
        return r

    def backward(self, fw, flags, dOut=None, dOut_bcast=None):
        B, T, H = self.B, self.T, self.H
        dG = torch.zeros(B, T, 2, 4 * H, device=self.dev)
        ops.birnn_bwd("lstm", B, T, H, w_hh=self.w_hh, act=fw["act"], cs=fw["cs"], hprev=fw["hprev"], dOut=dOut,
                      dOut_bcast=dOut_bcast, dG=dG, ws=self.ws, ws_bytes=self.wsn, status=self.status, flags=flags)
        torch.cuda.synchronize()
        assert int(self.status.item()) == 0
        return dG


_REF = {}


def _ref(B, T, H):
    """The case and its fp64 forward, computed once per shape and left unchanged."""
    if (B, T, H) not in _REF:
        c = K.case(B, T, H)
        _REF[(B, T, H)] = (c, K.forward(c["G"], c["w_hh"], c["b_hh"]))
    return _REF[(B, T, H)]


@pytest.mark.parametrize("B,T,H", SHAPES)
def test_hard_cell_matches_fp64(dev, B, T, H):
    c, ref = _ref(B, T, H)
    K.assert_saturates(ref["act"])
    L = Layer(dev, B, T, H, c)
    fw = L.forward(ops.HARD_GATES)
    for name in ("out", "act", "cs", "hprev"):
        err = (fw[name].cpu().double() - ref[name]).abs().max().item()
        print(f"hard cell B={B} T={T} H={H}: {name} max abs err {err:.3e}")
        assert err < TOL_FWD, (name, err)
    act = fw["act"].cpu()
    i, f, o = K.gate_blocks(act)
    assert all(float(g.min()) >= 0.0 and float(g.max()) <= 1.0 for g in (i, f, o))  # act holds the clipped values
    pattern, share = K.check_pattern(act, ref)
    print(f"  saturation flags that differ from fp64 (all within {K.KINK} of a kink): {share:.2e} of the gates")
    for what, kw in (("dOut", dict(dOut=c["dOut"])),
                     ("dOut + dOut_bcast", dict(dOut=c["dOut"], dOut_bcast=c["dOut_bcast"]))):
        want = K.backward(ref, c["w_hh"], pattern=pattern, **kw)["dG"]
        dG = L.backward(fw, ops.HARD_GATES, **{k: v.to(dev) for k, v in kw.items()})
        rel = ((dG.cpu().double() - want).abs().max() / want.abs().max()).item()
        print(f"  dG ({what}): {rel:.3e} of the largest element")
        assert rel < TOL_GRAD, (what, rel)
        # where the device's gate sits on the clip, its pre-activation gradient is exactly zero
        gi, gf, go = K.gate_blocks(dG.cpu())
        pi, pf, po = K.gate_blocks(pattern)
        assert all(bool((g[~p] == 0).all()) for g, p in ((gi, pi), (gf, pf), (go, po)))


def test_layer_gradients_through_the_op(dev):
    """dl4ss::keras_lstm_layer under autograd at (5, 9, 25): dx, dW_ih, db_ih, dW_hh, db_hh against fp64 with the
    device's saturation pattern."""
    from dl4ss_amd import library  # noqa: F401 (registers the ops)

    B, T, H, D = 5, 9, 25, 23
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, T, D, generator=g)
    w_ih = torch.randn(8 * H, D, generator=g) * (3.0 / D ** 0.5)  # G of standard deviation ~3: the gates saturate
    b_ih = torch.randn(8 * H, generator=g) * 0.1
    c = K.case(B, T, H)
    w_hh, b_hh = c["w_hh"].reshape(8 * H, H), c["b_hh"].reshape(8 * H)
    Gd = (x.double().view(B * T, D) @ w_ih.double().T + b_ih.double()).view(B, T, 2, 4 * H)
    ref = K.forward(Gd, c["w_hh"], c["b_hh"])
    K.assert_saturates(ref["act"])
    p = [t.clone().to(dev).requires_grad_(True) for t in (x, w_ih, b_ih, w_hh, b_hh)]
    out, _, act, _ = torch.ops.dl4ss.keras_lstm_layer(*p, H)
    assert (out.detach().cpu().double() - ref["out"]).abs().max().item() < TOL_FWD
    pattern, _ = K.check_pattern(act.cpu(), ref)
    (out * c["dOut"].to(dev)).sum().backward()
    r = K.backward(ref, c["w_hh"], dOut=c["dOut"], pattern=pattern)
    dx, dw_ih, db_ih = K.layer_grads(x, w_ih, r["dG"])
    want = (dx, dw_ih, db_ih, r["dw_hh"].reshape(8 * H, H), r["db_hh"].reshape(8 * H))
    for name, t, w in zip(("dx", "dw_ih", "db_ih", "dw_hh", "db_hh"), p, want):
        rel = ((t.grad.cpu().double() - w).abs().max() / w.abs().max()).item()
        print(f"keras_lstm_layer {name}: {rel:.3e} of the largest element")
        assert rel < TOL_GRAD, (name, rel)
    from dl4ss_amd.library import birnn
    assert torch.equal(birnn(*[t.detach() for t in p], cell="lstm", H=H, gates="hard"), out.detach())
    # the autograd Function with its optional ninth argument: the same forward bits, the same gradients (up to the
    # order of the weight-gradient GEMMs' split-K atomics: 1e-5 of the largest element, tests/test_step_gpu.py's bound)
    from dl4ss_amd import autograd as ag
    q = [t.detach().clone().requires_grad_(True) for t in p]
    out2 = ag.BiRNNLayerFn.apply(*q, "lstm", H, "fp32", "hard")
    assert torch.equal(out2.detach(), out.detach())
    (out2 * c["dOut"].to(dev)).sum().backward()
    for a, b in zip(p, q):
        assert ((a.grad - b.grad).abs().max() / a.grad.abs().max()).item() < 1e-5


def test_flag_changes_the_result_and_leaks_no_state(dev):
    """Hard and logistic outputs of the same inputs differ by more than 1e-2 somewhere; the logistic call after a
    flagged one on the same workspace equals the one before it bit for bit."""
    B, T, H = 5, 9, 25
    c, _ = _ref(B, T, H)
    L = Layer(dev, B, T, H, c)
    before = L.forward(0)
    hard = L.forward(ops.HARD_GATES)
    after = L.forward(0)
    assert (hard["out"] - before["out"]).abs().max().item() > 1e-2
    for k in before:
        assert torch.equal(before[k], after[k]), k
    dout = c["dOut"].to(dev)
    d0 = L.backward(before, 0, dOut=dout)
    L.backward(hard, ops.HARD_GATES, dOut=dout)
    assert torch.equal(d0, L.backward(after, 0, dOut=dout))


def test_refusals_leave_out_untouched(dev):
    """GRU + flag, precision 1 + flag, flag + out_bf16: hipErrorInvalidValue before any launch."""
    B, T, H = 4, 2, 40
    c, _ = _ref(B, T, H)
    for cell, precision, extra in (("gru", "fp32", {}), ("lstm", "bf16", {}),
                                   ("lstm", "fp32", dict(out_bf16=torch.zeros(B * T, ops.pad8(2 * H), device=dev,
                                                                              dtype=torch.bfloat16)))):
        L = Layer(dev, B, T, H, c, cell)
        out = torch.full((B, T, 2 * H), 7.0, device=dev)
        with pytest.raises(RuntimeError, match=r"hipError 1 "):
            ops.birnn_fwd(cell, B, T, H, G=L.G, w_hh=L.w_hh, b_hh=L.b_hh, ws=L.ws, ws_bytes=L.wsn, status=L.status,
                          precision=precision, flags=ops.HARD_GATES, out=out,
                          hprev=torch.empty(B, T, 2 * H, device=dev), act=torch.empty(B, T, 2, 4 * H, device=dev),
                          cs=torch.empty(B, T, 2, H, device=dev) if cell == "lstm" else None, **extra)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), (cell, precision)
    # the BPTT: GRU, precision 1, a bf16 dG and dOut slabs
    L = Layer(dev, B, T, H, c)
    fw = L.forward(ops.HARD_GATES)
    dout = c["dOut"].to(dev)
    for cell, precision, flags, extra in (("gru", "fp32", 0, {}), ("lstm", "bf16", 0, {}),
                                          ("lstm", "fp32", ops.DOUT_SLABS(2), {}),
                                          ("lstm", "fp32", 0, dict(dG_bf16=torch.zeros(B, T, 2, 4 * H, device=dev,
                                                                                       dtype=torch.bfloat16)))):
        dG = torch.full((B, T, 2, 4 * H), 7.0, device=dev)
        with pytest.raises(RuntimeError, match=r"hipError 1 "):
            ops.birnn_bwd(cell, B, T, H, w_hh=L.w_hh, act=fw["act"], cs=fw["cs"], hprev=fw["hprev"], dOut=dout, dG=dG,
                          dGh=torch.empty_like(dG) if cell == "gru" else None, ws=L.ws, ws_bytes=L.wsn,
                          status=L.status, precision=precision, flags=ops.HARD_GATES | flags, **extra)
        torch.cuda.synchronize()
        assert bool((dG == 7.0).all()), (cell, precision, flags)
