"""Classifier head kernels (cls_head.hip) against fp64 torch: Linear + sigmoid, then
nn.MultiLabelSoftMarginLoss applied -- as the reference does (test_multi_labels_speech.py:263,397,437)
-- to the sigmoid output, and its autograd.  fp32 conventions of test_attn_align_gpu.py: z / p at rtol
1e-5, atol 1e-6; loss 1e-5 relative; dW / db / dOut_bcast within 1e-4 of each tensor's largest element."""
import pytest
import torch

from dl4ss_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -12345.0


def _guarded(n, dev):
    """n writable floats with GUARD sentinel floats behind them"""
    buf = torch.full((n + GUARD,), SENTINEL, device=dev)
    return buf, buf[:n]


def _run(dev, m, W, b, y, T):
    B, D = m.shape
    C = W.shape[0]
    md, Wd, bd, yd = (t.float().to(dev).contiguous() for t in (m, W, b, y))
    bufs = {k: _guarded(n, dev) for k, n in dict(z=B * C, p=B * C, loss=1, dz=B * C, dW=C * D, db=C, dmb=B * D).items()}
    v = {k: x[1] for k, x in bufs.items()}
    _lib.call("dl4ss_cls_head_fwd", _lib.ptr(md), _lib.ptr(Wd), _lib.ptr(bd), B, D, C, _lib.ptr(v["z"]),
              _lib.ptr(v["p"]), _lib.stream_ptr())
    _lib.call("dl4ss_cls_head_loss_bwd", _lib.ptr(v["p"]), _lib.ptr(yd), _lib.ptr(md), _lib.ptr(Wd), B, D, C, T,
              _lib.ptr(v["loss"]), _lib.ptr(v["dz"]), _lib.ptr(v["dW"]), _lib.ptr(v["db"]), _lib.ptr(v["dmb"]),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert bool((buf[view.numel():] == SENTINEL).all()), f"guard behind {k} overwritten"
    return {k: x.clone() for k, x in v.items()}


@pytest.mark.parametrize("B,D,C", [(1, 40, 5), (3, 1200, 101), (32, 1200, 101), (2, 1280, 7)])
def test_cls_head_matches_fp64(dev, B, D, C):
    T = 7
    g = torch.Generator().manual_seed(B * 1000 + D + C)
    m = (torch.randn(B, D, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    W = (torch.randn(C, D, generator=g, dtype=torch.float64) / D ** 0.5).requires_grad_(True)
    b = (torch.randn(C, generator=g, dtype=torch.float64) * 0.1).requires_grad_(True)
    y = (torch.rand(B, C, generator=g) < 0.1).double()
    y[:, 0] = 1.0
    # the reference numerics in fp64, with the time mean in front: out (B, T, D) with mean_t out = m
    z = m @ W.T + b
    p = torch.sigmoid(z)
    loss = torch.nn.MultiLabelSoftMarginLoss()(p, y)
    loss.backward()
    r = _run(dev, m.detach(), W.detach(), b.detach(), y, T)
    z_o, p_o = r["z"].cpu().double().view(B, C), r["p"].cpu().double().view(B, C)
    assert torch.allclose(z_o, z.detach(), rtol=1e-5, atol=1e-6), (z_o - z.detach()).abs().max()
    assert torch.allclose(p_o, p.detach(), rtol=1e-5, atol=1e-6), (p_o - p.detach()).abs().max()
    lv = float(r["loss"].cpu())
    assert abs(lv - float(loss)) / abs(float(loss)) < 1e-5, (lv, float(loss))

    def close(ours, ref, what):
        e = (ours.cpu().double().view_as(ref) - ref).abs().max() / ref.abs().max()
        assert e < 1e-4, (what, float(e))

    close(r["dW"], W.grad, "dW")
    close(r["db"], b.grad, "db")
    close(r["dmb"], m.grad / T, "dOut_bcast")  # d(out)[b, t, :] = dm[b, :] / T
    # repeated launches agree bit for bit (fixed-order sums, no atomics)
    r2 = _run(dev, m.detach(), W.detach(), b.detach(), y, T)
    for k in r:
        assert torch.equal(r[k], r2[k]), k


def test_cls_head_refuses_bad_arguments(dev):
    B, D, C, T = 2, 16, 3, 4
    t = torch.zeros(B * D + C * D, device=dev)
    pt, st = _lib.ptr(t), _lib.stream_ptr()
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_cls_head_fwd", None, pt, pt, B, D, C, pt, pt, st)
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_cls_head_fwd", pt, pt, pt, 0, D, C, pt, pt, st)
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_cls_head_fwd", pt, pt, pt, B, D, -1, pt, pt, st)
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_cls_head_loss_bwd", pt, pt, pt, pt, B, D, C, 0, pt, pt, pt, pt, pt, st)
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_cls_head_loss_bwd", pt, None, pt, pt, B, D, C, T, pt, pt, pt, pt, pt, st)
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_cls_head_loss_bwd", pt, pt, pt, pt, B, D, C, T, pt, pt, pt, pt, None, st)
    torch.cuda.synchronize()
