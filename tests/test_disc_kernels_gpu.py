"""The Discriminator kernels (disc.hip) through the C ABI against fp64 ``torch.nn.functional.conv2d`` and its
autograd on torch CPU.

Per layer, with operands exact in the tested precision (bf16: bf16-rounded activations and filter banks), a
sum of K products must satisfy the a-priori bound |err| <= 2 K 2^-24 (|x| (*) |w| + |b|) elementwise (K = 9 or
576 forward, taps x 64 for dX, N Hout Wout for dW / db; the factor 2 is slack for the MFMA's fused chains); a
bf16 output adds one rounding 2^-8 |ref|.  The backward tests take the saved Y (the fp64 forward, rounded) as
an input, so the gate is the same on both sides.  Every output has a sentinel guard region behind it, dX is
pre-filled with the sentinel and must be overwritten everywhere, with exact zeros where no window reaches.
Two calls agree bit for bit.  The whole-module test runs the fp64 model with the kernel's own gates."""
import ctypes

import pytest
import torch
import torch.nn.functional as Fn

import disc_ref as R
from dl4ss_amd import _lib, autograd as ag

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -12345.0
PRECS = ["fp32", "bf16"]
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
PREC = {"fp32": 0, "bf16": 1}


def _rnd(prec):
    return R.bf16r if prec == "bf16" else (lambda t: t.float().double())


def _u_out(prec):
    return 2.0 ** -8 if prec == "bf16" else 0.0


class Out:
    """an output buffer of ``shape`` pre-filled with the sentinel, GUARD sentinel elements behind it"""

    def __init__(self, shape, dev, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=dev)
        self.sent = float(torch.tensor(SENTINEL, dtype=dtype))
        self.view = self.buf[:n].view(shape)

    def check(self, name):
        assert bool((self.buf[self.n:] == self.sent).all()), f"guard behind {name} overwritten"
        assert not bool((self.buf[:self.n] == self.sent).any()), f"{name}: elements left unwritten"
        return self.view.clone()


def _dev_act(t_nchw, prec, dev):
    return R.to_cl(t_nchw).to(DT[prec]).to(dev)


def _ws(N, T, F, dev):
    n = _lib.query("dl4ss_disc_ws_bytes", N, T, F)
    assert n > 0
    return torch.empty((n + 3) // 4, device=dev), n


def _within(got, ref, bound, what):
    d = (got.double().cpu() - ref).abs()
    over = d - bound
    assert bool((over <= 0).all()), (what, float(over.max()), float(d.max()), float(bound.max()))


def _layer_data(N, Hin, Win, cin, prec, seed):
    """X (N, cin, Hin, Win), w, b, the saved Y and a dY, each exact in the precision's storage type"""
    g = torch.Generator().manual_seed(seed)
    rnd = _rnd(prec)
    rx = rnd if cin == 64 else (lambda t: t.float().double())  # conv1 reads the fp32 map and fp32 filters
    X = rx(torch.randn(N, cin, Hin, Win, generator=g, dtype=torch.float64).clamp_min(0) +
           (0.1 * torch.rand(N, cin, Hin, Win, generator=g, dtype=torch.float64) if cin == 1 else 0))
    k = (9 * cin) ** -0.5
    w = rx((torch.rand(64, cin, 3, 3, generator=g, dtype=torch.float64) * 2 - 1) * k)
    b = ((torch.rand(64, generator=g, dtype=torch.float64) * 2 - 1) * k).float().double()
    z = Fn.conv2d(X, w, b, stride=2)
    Y = rnd(z.clamp_min(0))
    dY = rnd(torch.randn(z.shape, generator=g, dtype=torch.float64) * 0.1)
    return X, w, b, z, Y, dY


def _taps(n):
    """number of window taps that reach input index i: even indices taps {0, 2}, odd ones tap {1}"""
    return torch.tensor([2.0 if i % 2 == 0 else 1.0 for i in range(n)], dtype=torch.float64)


def _uncovered(Hin, Win):
    """mask of the input positions no window covers (the last row / column of an even extent)"""
    m = torch.zeros(Hin, Win, dtype=torch.bool)
    if 2 * (R.out_dim(Hin) - 1) + 2 < Hin - 1:
        m[-1, :] = True
    if 2 * (R.out_dim(Win) - 1) + 2 < Win - 1:
        m[:, -1] = True
    return m


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_conv1_fwd(dev, shape, prec):
    N, T, F = shape
    X, w, b, z, _, _ = _layer_data(N, T, F, 1, prec, 11)
    ref = z.clamp_min(0)
    y = Out((N, R.out_dim(T), R.out_dim(F), 64), dev, DT[prec])
    xd, wd, bd = X[:, 0].float().to(dev).contiguous(), w.float().to(dev), b.float().to(dev)
    outs = []
    for _ in range(2):
        _lib.call("dl4ss_disc_conv1_fwd", PREC[prec], _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), N, T, F,
                  _lib.ptr(y.view), _lib.stream_ptr())
        torch.cuda.synchronize()
        outs.append(y.check("y1"))
    assert torch.equal(outs[0], outs[1])
    _within(R.from_cl(outs[0].cpu()), ref, R.fwd_bound(X, w, b, 9, _u_out(prec), ref), "y1")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_conv64_fwd(dev, shape, prec):
    N, T, F = shape
    hw = R.dims(T, F)
    for layer in (0, 1):  # conv2 on conv1's output size, conv3 on conv2's
        Hin, Win = hw[2 * layer], hw[2 * layer + 1]
        X, w, b, z, _, _ = _layer_data(N, Hin, Win, 64, prec, 23 + layer)
        ref = z.clamp_min(0)
        y = Out((N, R.out_dim(Hin), R.out_dim(Win), 64), dev, DT[prec])
        xd, wd, bd = _dev_act(X, prec, dev), w.float().to(dev), b.float().to(dev)
        outs = []
        for _ in range(2):
            _lib.call("dl4ss_disc_conv64_fwd", PREC[prec], _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), N, Hin, Win,
                      _lib.ptr(y.view), _lib.stream_ptr())
            torch.cuda.synchronize()
            outs.append(y.check(f"y{layer + 2}"))
        assert torch.equal(outs[0], outs[1])
        _within(R.from_cl(outs[0].cpu()), ref, R.fwd_bound(X, w, b, 576, _u_out(prec), ref), f"y{layer + 2}")


# ----------------------------------------------------------------------------------------------- backward
def _bwd_refs(X, w, Y, dY):
    G = dY * (Y > 0)
    dX, dW, db = R.conv_bwd(X, w, G)
    aX, aW, ab = R.conv_bwd(X.abs(), w.abs(), G.abs())
    return (dX, dW, db), (aX, aW, ab)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_conv64_bwd(dev, shape, prec):
    N, T, F = shape
    hw = R.dims(T, F)
    ws, wsn = _ws(N, T, F, dev)
    for layer in (0, 1):
        Hin, Win = hw[2 * layer], hw[2 * layer + 1]
        X, w, b, z, Y, dY = _layer_data(N, Hin, Win, 64, prec, 41 + layer)
        (dX, dW, db), (aX, aW, ab) = _bwd_refs(X, w, Y, dY)
        xd, yd, dyd, wd = _dev_act(X, prec, dev), _dev_act(Y, prec, dev), _dev_act(dY, prec, dev), w.float().to(dev)
        runs = []
        for need_dx in (True, True, False):
            o = dict(dw=Out((64, 64, 3, 3), dev), db=Out((64,), dev))
            if need_dx:
                o["dx"] = Out((N, Hin, Win, 64), dev, DT[prec])
            _lib.call("dl4ss_disc_conv64_bwd", PREC[prec], _lib.ptr(xd), _lib.ptr(yd), _lib.ptr(dyd), _lib.ptr(wd), N,
                      Hin, Win, _lib.ptr(o["dx"].view) if need_dx else None, _lib.ptr(o["dw"].view),
                      _lib.ptr(o["db"].view), _lib.ptr(ws), wsn, _lib.stream_ptr())
            torch.cuda.synchronize()
            runs.append({k: v.check(k) for k, v in o.items()})
        for k in runs[0]:
            assert torch.equal(runs[0][k], runs[1][k]), k      # two calls, bit for bit
        for k in runs[2]:
            assert torch.equal(runs[0][k], runs[2][k]), k      # dx = NULL changes nothing else
        K = N * R.out_dim(Hin) * R.out_dim(Win)
        _within(runs[0]["dw"], dW, 2 * K * R.U32 * aW, "dw")
        _within(runs[0]["db"], db, 2 * K * R.U32 * ab, "db")
        Kx = 64 * _taps(Hin)[:, None] * _taps(Win)[None, :]
        got = R.from_cl(runs[0]["dx"].cpu())
        _within(got, dX, 2 * Kx * R.U32 * aX + _u_out(prec) * dX.abs(), "dx")
        unc = _uncovered(Hin, Win)
        assert bool((got[:, :, unc] == 0).all())               # exact zeros where no window reaches


# (1, 15, 141): 71 half-resolution columns, two tiles of the input-gradient kernel along W (and its left halo)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", R.SHAPES + [(1, 15, 141)])
def test_conv1_bwd(dev, shape, prec):
    N, T, F = shape
    ws, wsn = _ws(N, T, F, dev)
    X, w, b, z, Y, dY = _layer_data(N, T, F, 1, prec, 61)
    (dX, dW, db), (aX, aW, ab) = _bwd_refs(X, w, Y, dY)
    xd, yd, dyd, wd = X[:, 0].float().to(dev).contiguous(), _dev_act(Y, prec, dev), _dev_act(dY, prec, dev), \
        w.float().to(dev)
    runs = []
    for need_dx in (True, True, False):
        o = dict(dw=Out((64, 1, 3, 3), dev), db=Out((64,), dev))
        if need_dx:
            o["dx"] = Out((N, T, F), dev)
        _lib.call("dl4ss_disc_conv1_bwd", PREC[prec], _lib.ptr(xd), _lib.ptr(yd), _lib.ptr(dyd), _lib.ptr(wd), N, T, F,
                  _lib.ptr(o["dx"].view) if need_dx else None, _lib.ptr(o["dw"].view), _lib.ptr(o["db"].view),
                  _lib.ptr(ws), wsn, _lib.stream_ptr())
        torch.cuda.synchronize()
        runs.append({k: v.check(k) for k, v in o.items()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    for k in runs[2]:
        assert torch.equal(runs[0][k], runs[2][k]), k
    K = N * R.out_dim(T) * R.out_dim(F)
    _within(runs[0]["dw"], dW, 2 * K * R.U32 * aW, "dw")
    _within(runs[0]["db"], db, 2 * K * R.U32 * ab, "db")
    Kx = 64 * _taps(T)[:, None] * _taps(F)[None, :]
    got = runs[0]["dx"].cpu()
    _within(got, dX[:, 0], 2 * Kx * R.U32 * aX[:, 0], "dx")
    assert bool((got[:, _uncovered(T, F)] == 0).all())


# --------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_head(dev, shape, prec, fused):
    N, T, F = shape
    hw = R.dims(T, F)
    H3, W3 = hw[4], hw[5]
    L = 64 * H3 * W3
    g = torch.Generator().manual_seed(77)
    y3 = _rnd(prec)(torch.randn(N, 64, H3, W3, generator=g, dtype=torch.float64).clamp_min(0))
    wf = ((torch.rand(1, L, generator=g, dtype=torch.float64) * 2 - 1) * L ** -0.5 * 4).float().double()
    bf = torch.tensor([0.05], dtype=torch.float64).float().double()
    target = 1.0
    yd, wd, bd = _dev_act(y3, prec, dev), wf.float().to(dev), bf.float().to(dev)
    runs = []
    for _ in range(2):
        o = dict(z=Out((N,), dev), score=Out((N, 1), dev), dz=Out((N,), dev), dwf=Out((1, L), dev), dbf=Out((1,), dev),
                 dy3=Out((N, H3, W3, 64), dev, DT[prec]))
        if fused:
            o["loss"] = Out((1,), dev)
        _lib.call("dl4ss_disc_head_fwd", PREC[prec], _lib.ptr(yd), _lib.ptr(wd), _lib.ptr(bd), N, H3, W3,
                  _lib.ptr(o["z"].view), _lib.ptr(o["score"].view), _lib.stream_ptr())
        torch.cuda.synchronize()
        s_dev = o["score"].view.clone()
        ds = None if fused else (2.0 * (s_dev - target) / N).contiguous()
        _lib.call("dl4ss_disc_head_bwd", PREC[prec], _lib.ptr(yd), _lib.ptr(wd), _lib.ptr(s_dev),
                  _lib.ptr(ds) if ds is not None else None, target, N, H3, W3,
                  _lib.ptr(o["loss"].view) if fused else None, _lib.ptr(o["dz"].view), _lib.ptr(o["dwf"].view),
                  _lib.ptr(o["dbf"].view), _lib.ptr(o["dy3"].view), _lib.stream_ptr())
        torch.cuda.synchronize()
        runs.append({k: v.check(k) for k, v in o.items()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    r = {k: v.cpu().double() for k, v in runs[0].items()}
    feat = y3.reshape(N, L)
    z = feat @ wf.T + bf
    zb = 2 * L * R.U32 * (feat.abs() @ wf.abs().T + bf.abs())
    _within(r["z"].view(N, 1), z, zb, "z")
    s = torch.sigmoid(z)
    assert torch.allclose(r["score"], s, rtol=1e-5, atol=1e-6), (r["score"] - s).abs().max()
    if fused:
        loss = ((s - target) ** 2).mean()
        assert abs(float(r["loss"]) - float(loss)) <= 1e-5 * float(loss)
    dz = 2.0 * (s - target) / N * s * (1 - s)
    assert R.rel_err(r["dz"].view(N, 1), dz) < 1e-5
    # the remaining sums take the kernel's own dz as their (exact) operand
    dzk = r["dz"].view(N, 1)
    _within(r["dwf"], dzk.T @ feat, 2 * N * R.U32 * (dzk.abs().T @ feat.abs()), "dwf")
    _within(r["dbf"], dzk.sum().view(1), 2 * N * R.U32 * dzk.abs().sum().view(1), "dbf")
    dy3 = (dzk @ wf).reshape(N, 64, H3, W3)
    _within(R.from_cl(r["dy3"]), dy3, (2 * R.U32 + _u_out(prec)) * dy3.abs(), "dy3")


# ------------------------------------------------------------------------------------------------- limits
def test_too_small_sizes_are_refused(dev):
    t = torch.zeros(1 << 16, device=dev)
    p, st = _lib.ptr(t), _lib.stream_ptr()
    assert _lib.query("dl4ss_disc_dims", 14, 15, (ctypes.c_int * 6)()) == -1
    assert _lib.query("dl4ss_disc_ws_bytes", 1, 15, 14) == -1
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_disc_conv1_fwd", 0, p, p, p, 1, 2, 15, p, st)
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_disc_conv64_fwd", 0, p, p, p, 1, 7, 2, p, st)
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_disc_conv64_fwd", 1, p, p, p, 0, 7, 7, p, st)
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_disc_conv64_bwd", 0, p, p, p, p, 1, 2, 7, None, p, p, p, 1 << 18, st)
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_disc_conv64_bwd", 0, p, p, p, p, 1, 7, 7, None, p, p, p, 64, st)  # workspace too small
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_disc_conv1_bwd", 0, p, p, p, p, 1, 15, 2, None, p, p, p, 1 << 18, st)
    with pytest.raises(RuntimeError):
        _lib.call("dl4ss_disc_head_fwd", 0, p, p, p, 1, 0, 1, p, p, st)
    with pytest.raises(RuntimeError):
        ag.disc_dims(14, 129)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- whole module
GRADS = ["g/" + k for k in R.KEYS] + ["dx"]


def _run_module(dev, x, P, prec, target):
    args = [P[k].float().to(dev) for k in R.KEYS]
    xd = x.float().to(dev)
    score, y1, y2, y3 = ag.disc_fwd_impl(xd, *args, prec)
    out = ag.disc_bwd_impl(None, xd, args[0], args[2], args[4], args[6], score, y1, y2, y3, prec, True, target=target)
    torch.cuda.synchronize()
    r = {"score": score.cpu().double(), "loss": out[9].cpu().double(), "dx": out[0].cpu().double()}
    for i, y in enumerate((y1, y2, y3)):
        r[f"y{i + 1}"] = R.from_cl(y.cpu().double())
    for k, v in zip(("cnn.weight", "cnn.bias", "cnn1.weight", "cnn1.bias", "cnn2.weight", "cnn2.bias", "final.weight",
                     "final.bias"), out[1:9]):
        r["g/" + k] = v.cpu().double().view(P[k].shape)
    return r


@pytest.mark.parametrize("target", [1.0, 0.0])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_whole_module(dev, shape, prec, target):
    """fp32: score at rtol 1e-5 / atol 1e-6, every gradient within 1e-4 of its tensor's largest element.
    bf16: per tensor, the kernel's error against the (kernel-gated) fp64 model is at most twice that of a
    torch-CPU emulation rounding to bf16 at the same points."""
    N, T, F = shape
    for seed in (0, 1):
        P, x = R.make_params(T, F, seed), R.make_input(N, T, F, seed)
        k = _run_module(dev, x, P, prec, target)
        gates = [k[f"y{i}"] > 0 for i in (1, 2, 3)]
        ref = R.run_model(x, P, gates, target)
        # gates: the share that differs from the fp64 sign, and each differing |z_ref| within its forward bound
        bounds = R.module_fwd_bounds(x, P, [ref["y1"], ref["y2"]], prec == "bf16")
        flips = tot = 0
        for l in range(3):
            diff = gates[l] != (ref[f"z{l + 1}"] > 0)
            flips += int(diff.sum())
            tot += diff.numel()
            assert bool((ref[f"z{l + 1}"].abs()[diff] <= bounds[l][diff]).all()), f"layer {l + 1}: a gate flipped " \
                "where |z_ref| is beyond the forward bound"
        share = flips / tot
        print(f"disc module {shape} {prec} target {target} seed {seed}: gate flips {flips}/{tot}")
        assert share <= (0.01 if prec == "bf16" else 0.001), share
        if prec == "fp32":
            assert torch.allclose(k["score"], ref["score"], rtol=1e-5, atol=1e-6)
            assert abs(float(k["loss"]) - float(ref["loss"])) <= 1e-5 * max(float(ref["loss"]), 1e-6)
            for name in GRADS:
                e = R.rel_err(k[name], ref[name])
                print(f"  {name}: {e:.3e}")
                assert e <= 1e-4, (name, e)
        else:
            emu = R.run_model(x, P, gates, target, rnd=R.bf16r)
            for name in ["y1", "y2", "y3", "score"] + GRADS:
                ek, ee = R.rel_err(k[name], ref[name]), R.rel_err(emu[name], ref[name])
                print(f"  {name}: kernel {ek:.3e} emulation {ee:.3e}")
                assert ek <= 2 * ee, (name, ek, ee)
