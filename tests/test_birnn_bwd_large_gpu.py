"""Large-hidden BPTT (320 < H <= 640, dl4ss_birnn_bwd_ex): the recurrence backward of the H = 600
speaker classifier (test_multi_labels_speech.py:240-246,444), against fp64 autograd through an explicit
recurrence -- the structure of test_kernels_gpu.py::test_birnn_bwd_dG_per_step.

Bounds.  precision 0 (exact fp32 VALU): |h - ref| < 1e-5 and dG, b_hh gradient within 1e-4 of the largest
reference element (the H = 300 bounds; the sums are twice as long, so up to 4e-4 would still be a rounding effect -- it was not
needed).  precision 1 (bf16 MFMA matvec): 3e-3 on h, 2e-3 on dG against the fp64 recurrence with the same
operand rounding, as at H = 300.  Every figure is printed before it is asserted (pytest -s).
Measured on an MI355X over every case below: precision 0 h <= 2.3e-7, dG <= 2.4e-7, db_hh <= 1.7e-7;
precision 1 h <= 2.7e-4, dG <= 3.8e-4, db_hh <= 1.7e-4."""
import pytest
import torch

from dl4ss_amd import _lib

pytestmark = pytest.mark.gpu

TOL = {0: (1e-5, 1e-4), 1: (3e-3, 2e-3)}  # precision -> (abs on h, of max|ref| on dG / db_hh)


def _bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


class _Bf16MatVec(torch.autograd.Function):
    """gh = bf16(h) bf16(W)^T with fp64 accumulate; backward dh = bf16(dgh) bf16(W): the operand
    rounding of the kernels' bf16 MFMA recurrence (precision 1)."""

    @staticmethod
    def forward(ctx, h, w):
        wb = _bf16(w)
        ctx.save_for_backward(wb)
        return _bf16(h) @ wb.T

    @staticmethod
    def backward(ctx, g):
        (wb,) = ctx.saved_tensors
        return _bf16(g) @ wb, None


def _manual_birnn(cell, G, whh, bhh, H, bf16=False):
    """Explicit bidirectional recurrence on input projections G (B,T,2,NGH) (fp64, autograd)."""
    B, T = G.shape[:2]
    outs = [[None] * T, [None] * T]
    for d in range(2):
        h = torch.zeros(B, H, dtype=G.dtype)
        c = torch.zeros(B, H, dtype=G.dtype)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            gh = (_Bf16MatVec.apply(h, whh[d]) if bf16 else h @ whh[d].T) + bhh[d]
            gx = G[:, t, d]
            if cell == "lstm":
                i, f, g, o = (gx + gh).chunk(4, 1)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
            else:
                xr, xz, xn = gx.chunk(3, 1)
                hr, hz, hn = gh.chunk(3, 1)
                r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
                n = torch.tanh(xn + r * hn)
                h = (1 - z) * n + z * h
            outs[d][t] = h
    return torch.cat([torch.stack(outs[0], 1), torch.stack(outs[1], 1)], dim=2)


def _bwd_ex(cellid, prec, B, T, H, dout, bcast, whd, act, cs, hp, dG, dGh, wsb, ws, st):
    _lib.call("dl4ss_birnn_bwd_ex", cellid, prec, B, T, H, _lib.ptr(dout), _lib.ptr(bcast), _lib.ptr(whd),
              _lib.ptr(act), _lib.ptr(cs), _lib.ptr(hp), _lib.ptr(dG), _lib.ptr(dGh), None, None, None, None,
              _lib.ptr(wsb), ws, _lib.ptr(st), _lib.stream_ptr())


def _case(dev, cell, prec, B, T, H, top_layer=False):
    """Forward + BPTT on the device and in fp64; checks h, dG per step and direction, the b_hh gradient,
    status and bitwise repeatability.  top_layer: dOut NULL, dOut_bcast = g / T, i.e. the loss
    (mean_t out * g).sum()."""
    ng = 4 if cell == "lstm" else 3
    NGH = ng * H
    gen = torch.Generator().manual_seed(B * 31 + T + H)
    G = torch.randn(B, T, 2, NGH, generator=gen, dtype=torch.float64) * 0.5
    whh = torch.randn(2, NGH, H, generator=gen, dtype=torch.float64) / H ** 0.5
    bhh = torch.randn(2, NGH, generator=gen, dtype=torch.float64) * 0.1
    Gl = G.clone().requires_grad_(True)
    bl = bhh.clone().requires_grad_(True)
    out = _manual_birnn(cell, Gl, whh, bl, H, bf16=prec == 1)
    if top_layer:
        g = torch.randn(B, 2 * H, generator=gen, dtype=torch.float64)
        (out.mean(1) * g).sum().backward()
        gd, bcd = None, (g / T).float().to(dev).contiguous()
    else:
        gout = torch.randn(out.shape, generator=gen, dtype=torch.float64)
        (out * gout).sum().backward()
        gd, bcd = gout.float().to(dev).contiguous(), None
    tol_h, tol_g = TOL[prec]
    cellid = 0 if cell == "lstm" else 1
    Gd, whd, bhd = (t.float().to(dev).contiguous() for t in (G, whh, bhh))
    o = torch.empty(B, T, 2 * H, device=dev)
    hp = torch.empty_like(o)
    act = torch.empty(B, T, 2, 4 * H, device=dev)
    cs = torch.empty(B, T, 2, H, device=dev)
    ws = _lib.query("dl4ss_birnn_workspace_bytes", cellid, B, H)
    assert ws > 0
    wsb = torch.empty((ws + 7) // 8, dtype=torch.int64, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("dl4ss_birnn_fwd", cellid, prec, B, T, H, _lib.ptr(Gd), _lib.ptr(whd), _lib.ptr(bhd), _lib.ptr(o),
              _lib.ptr(hp), _lib.ptr(act), _lib.ptr(cs), _lib.ptr(wsb), ws, _lib.ptr(st), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    err_h = (o.cpu().double() - out.detach()).abs().max().item()
    res = []
    for _ in range(2):
        dG = torch.zeros(B * T, 2 * NGH, device=dev)
        dGh = torch.zeros_like(dG)
        _bwd_ex(cellid, prec, B, T, H, gd, bcd, whd, act, cs, hp, dG, dGh, wsb, ws, st)
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        res.append((dG, dGh))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])  # bit for bit
    dG, dGh = res[0]
    ours = dG.cpu().double().view(B, T, 2, NGH)
    ref = Gl.grad
    errs = [[(ours[:, t, d] - ref[:, t, d]).abs().max().item() for t in range(T)] for d in range(2)]
    scale = ref.abs().max().item()
    err_g = max(max(e) for e in errs) / scale
    dgh = (dGh if cell == "gru" else dG).cpu().double().view(B, T, 2, NGH).sum((0, 1))
    err_b = ((dgh - bl.grad).abs().max() / bl.grad.abs().max()).item()
    print(f"birnn_bwd_large {cell} prec={prec} B={B} T={T} H={H} top={top_layer}: "
          f"h {err_h:.3e} dG {err_g:.3e} db_hh {err_b:.3e}")
    assert err_h < tol_h, err_h
    assert err_g < tol_g, (err_g, errs, scale)
    assert err_b < tol_g, err_b


# batch chunks BC that the plans give under the 240-workgroup budget of a full (256-CU) part.  bf16
# (J = 20, 30 workgroups per group) B = 1, 5, 9, 32 -> 1, 2, 4, 8 for both cells, (5, .) and (9, .) with a
# ragged last chunk.  fp32: LSTM J = 12, 50 workgroups per group: B = 1, 3, 5, 9 -> 1, 2, 4, 8; GRU
# J = 17, 36 per group (three chunks fit, so B = 3 still plans chunks of 1): 1, 1, 2, 4; B = 32 has no plan
# and runs as two sub-batches of 16 at chunks of 8 (both cells).
CHUNKS = {(1, "lstm"): {1: 1, 5: 2, 9: 4, 32: 8}, (1, "gru"): {1: 1, 5: 2, 9: 4, 32: 8},
          (0, "lstm"): {1: 1, 3: 2, 5: 4, 9: 8, 16: 8}, (0, "gru"): {1: 1, 3: 1, 5: 2, 9: 4, 16: 8}}


def _plan(cell, B, H, prec, max_wg=0):
    import ctypes

    info = (ctypes.c_int * 5)()
    rc = _lib.lib().dl4ss_birnn_plan_info(0 if cell == "lstm" else 1, B, H, prec, max_wg, info)
    return rc, list(info)


def _check_chunks(dev, cell, prec, B):
    if torch.cuda.get_device_properties(dev).multi_processor_count != 256:
        return
    if prec == 0 and B == 32:
        assert _plan(cell, 32, 600, 0)[0] != 0  # no plan: the two-sub-batch path
        B = 16
    rc, info = _plan(cell, B, 600, prec)
    assert rc == 0 and info[0] == CHUNKS[(prec, cell)][B], (info, cell, prec, B)


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("B,T", [(1, 5), (5, 2), (9, 7), (32, 1), (32, 7)])
def test_bwd_large_bf16(dev, cell, B, T):
    _check_chunks(dev, cell, 1, B)
    _case(dev, cell, 1, B, T, 600)


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("B,T", [(1, 5), (3, 2), (5, 7), (9, 3), (32, 4)])
def test_bwd_large_fp32(dev, cell, B, T):
    _check_chunks(dev, cell, 0, B)
    _case(dev, cell, 0, B, T, 600)


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("H", [640, 321])
def test_bwd_large_edges(dev, cell, H, prec):
    """HMAX_L itself, and a ragged last unit group just above HMAX."""
    _case(dev, cell, prec, 4, 6, H)


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_bwd_large_top_layer_null_dout(dev, cell, prec):
    """dOut NULL with dOut_bcast: the classifier's top layer, d/dG of (mean_t out * g).sum()."""
    _case(dev, cell, prec, 5, 3, 600, top_layer=True)


def test_bwd_large_refusals(dev):
    """The plain entry point keeps refusing H > 320; the _ex entry refuses H > 640, the bf16 extras at
    large H and a missing dOut without dOut_bcast -- all before any launch."""
    B, T = 1, 2
    for H in (600, 641):
        NGH = 4 * H
        z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
        dout, whd, act, cs, hp = z(B, T, 2 * H), z(2, NGH, H), z(B, T, 2, 4 * H), z(B, T, 2, H), z(B, T, 2 * H)
        dG = z(B * T, 2 * NGH)
        wsb = torch.zeros(1 << 20, dtype=torch.int64, device=dev)
        ws = wsb.numel() * 8
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError):
            _lib.call("dl4ss_birnn_bwd", 0, 1, B, T, H, _lib.ptr(dout), None, _lib.ptr(whd), _lib.ptr(act),
                      _lib.ptr(cs), _lib.ptr(hp), _lib.ptr(dG), _lib.ptr(dG), _lib.ptr(wsb), ws, _lib.ptr(st),
                      _lib.stream_ptr())
        if H == 641:
            with pytest.raises(RuntimeError):
                _bwd_ex(0, 1, B, T, H, dout, None, whd, act, cs, hp, dG, dG, wsb, ws, st)
            continue
        with pytest.raises(RuntimeError):  # neither dOut nor dOut_bcast
            _bwd_ex(0, 1, B, T, H, None, None, whd, act, cs, hp, dG, dG, wsb, ws, st)
        with pytest.raises(RuntimeError):  # bf16 copies are the packed kernels' (H <= 320)
            _lib.call("dl4ss_birnn_bwd_ex", 0, 1, B, T, H, _lib.ptr(dout), None, _lib.ptr(whd), _lib.ptr(act),
                      _lib.ptr(cs), _lib.ptr(hp), _lib.ptr(dG), _lib.ptr(dG), _lib.ptr(wsb), None, None, None,
                      _lib.ptr(wsb), ws, _lib.ptr(st), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert int(st.item()) == 0
