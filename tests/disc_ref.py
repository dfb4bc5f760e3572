"""fp64 torch-CPU restatement of the Discriminator (TDAA_beta/main_run_sstune_dis.py:318-336 and its loss
lines :622-624,642) shared by the test_disc_* files: seeded parameters, the model run layer by layer with
given ReLU gates and optional storage roundings (the bf16 emulation), and the a-priori error bounds."""
import torch
import torch.nn.functional as Fn

U32 = 2.0 ** -24   # unit roundoff of fp32
U16 = 2.0 ** -9    # unit roundoff of bf16 (8 significand bits, round to nearest)
KEYS = ("cnn.weight", "cnn.bias", "cnn1.weight", "cnn1.bias", "cnn2.weight", "cnn2.bias", "final.weight",
        "final.bias")
# (N, T, F): minimum size; even extents (uncovered last row / column); mixed parity; conv2 M = 315 (more than
# one ragged 128-row tile); the real F
SHAPES = [(1, 15, 15), (2, 16, 18), (3, 23, 33), (5, 31, 41), (2, 31, 129)]


def out_dim(n):
    return (n - 3) // 2 + 1


def dims(T, F):
    hw = []
    for _ in range(3):
        T, F = out_dim(T), out_dim(F)
        hw += [T, F]
    return hw


def bf16r(t):
    """round to bf16 (nearest even), kept in fp64"""
    return t.float().bfloat16().double()


def ident(t):
    return t


def make_params(T, F, seed):
    """torch's default init scale (uniform +-1/sqrt(fan_in)), fp32 values held in fp64"""
    g = torch.Generator().manual_seed(seed)
    hw = dims(T, F)
    feat = 64 * hw[4] * hw[5]
    shapes = {"cnn.weight": (64, 1, 3, 3), "cnn.bias": (64,), "cnn1.weight": (64, 64, 3, 3), "cnn1.bias": (64,),
              "cnn2.weight": (64, 64, 3, 3), "cnn2.bias": (64,), "final.weight": (1, feat), "final.bias": (1,)}
    fan = {"cnn": 9, "cnn1": 576, "cnn2": 576, "final": feat}
    P = {}
    for k in KEYS:
        b = fan[k.split(".")[0]] ** -0.5
        P[k] = ((torch.rand(shapes[k], generator=g, dtype=torch.float64) * 2 - 1) * b).float().double()
    return P


def make_input(N, T, F, seed):
    """magnitude-like maps: |normal|, fp32 values in fp64"""
    g = torch.Generator().manual_seed(seed + 7919)
    return torch.randn(N, T, F, generator=g, dtype=torch.float64).abs().float().double()


def to_cl(t):
    """(N, C, H, W) -> channels-last (N, H, W, C) contiguous"""
    return t.permute(0, 2, 3, 1).contiguous()


def from_cl(t):
    """channels-last (N, H, W, C) -> (N, C, H, W)"""
    return t.permute(0, 3, 1, 2).contiguous()


def conv_bwd(X, w, G):
    """(dX, dW, db) of conv2d(X, w, b, stride 2) for the output gradient G, by autograd in fp64"""
    X = X.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    b = torch.zeros(w.shape[0], dtype=X.dtype, requires_grad=True)
    Fn.conv2d(X, w, b, stride=2).backward(G)
    return X.grad, w.grad, b.grad


def run_model(x, P, gates, target, rnd=ident):
    """The network in fp64 with the ReLU gates given (list of three (N, 64, H, W) bool; None: the model's own
    sign) and ``rnd`` applied wherever the bf16 mode stores a value: y1..y3, the 64 -> 64 filter banks, the
    activation gradients dy3, dy2, dy1.  Returns z1..z3 (pre-activation), y1..y3, score, loss, the eight
    parameter gradients (``g/<key>``) and the input gradient ``dx`` of loss = mean (score - target)^2."""
    N = x.shape[0]
    ws = [P["cnn.weight"], rnd(P["cnn1.weight"]), rnd(P["cnn2.weight"])]
    bs = [P["cnn.bias"], P["cnn1.bias"], P["cnn2.bias"]]
    r = {}
    X = [x[:, None]]
    G = []
    for l in range(3):
        z = Fn.conv2d(X[l], ws[l], bs[l], stride=2)
        gate = (z > 0) if gates is None else gates[l]
        G.append(gate)
        X.append(rnd(z * gate))
        r[f"z{l + 1}"], r[f"y{l + 1}"] = z, X[l + 1]
    feat = X[3].reshape(N, -1)
    wf, bf = P["final.weight"], P["final.bias"]
    s = torch.sigmoid(feat @ wf.T + bf)
    r["score"], r["loss"] = s, ((s - target) ** 2).mean()
    dz = 2.0 * (s - target) / N * s * (1 - s)
    r["g/final.weight"], r["g/final.bias"] = dz.T @ feat, dz.sum().view(1)
    dy = rnd((dz @ wf).reshape(X[3].shape))
    for l in (2, 1, 0):
        dX, dW, db = conv_bwd(X[l], ws[l], dy * G[l])
        name = ("cnn", "cnn1", "cnn2")[l]
        r[f"g/{name}.weight"], r[f"g/{name}.bias"] = dW, db
        dy = rnd(dX) if l > 0 else dX
    r["dx"] = dy[:, 0]
    return r


def fwd_bound(X, w, b, K, u_out=0.0, ref=None):
    """|computed - exact| <= 2 K 2^-24 (|x| (*) |w| + |b|) for a sum of K products accumulated in fp32 (the
    factor 2 covers the MFMA's fused chains), plus one output rounding u_out |ref|."""
    bd = 2 * K * U32 * (Fn.conv2d(X.abs(), w.abs(), None, stride=2) + b.abs().view(1, -1, 1, 1))
    return bd + (u_out * ref.abs() if ref is not None else 0.0)


def module_fwd_bounds(x, P, ys, bf16):
    """A-priori bound on |z_l(kernel) - z_l(fp64 model)| of the whole network, layer by layer: the incoming
    activation error carried through |w|, plus this layer's own summation error (and, in bf16, the relative
    2^-9 of the rounded filter bank); the stored activation adds its own rounding.  ys: the fp64 y1, y2."""
    e_in = torch.zeros_like(x[:, None])
    X = x[:, None]
    out = []
    for l, name in enumerate(("cnn", "cnn1", "cnn2")):
        w, b = P[f"{name}.weight"], P[f"{name}.bias"]
        K = 9 if l == 0 else 576
        rw = U16 if (bf16 and l > 0) else 0.0
        own = (2 * K * U32 + rw) * (Fn.conv2d(X.abs(), w.abs(), None, stride=2) + b.abs().view(1, -1, 1, 1))
        e = Fn.conv2d(e_in, w.abs(), None, stride=2) + own
        out.append(e)
        if l < 2:
            X = ys[l]
            e_in = e + (U16 * X.abs() if bf16 else 0.0)
    return out


def rel_err(a, ref):
    """largest difference in units of the reference tensor's largest element"""
    return float((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


# ---------------------------------------------------------------- the reference-generated fixture's recipe
FIXTURE_SEED = 2024
FIXTURE_SHAPE = (1, 2, 313, 129)  # (bs, topk, len, fre): the reference's own map size, Linear(36480, 1)
SAMPLE = 512


def fixture_recipe(seed=FIXTURE_SEED):
    """Inputs and weights of tests/golden/ref_dis.npz, regenerated from the seed (not stored): the eight
    parameters at torch's default init scale, the true maps and the predicted maps, all fp32 numpy."""
    import numpy as np

    r = np.random.Generator(np.random.PCG64(seed))
    shapes = {"cnn.weight": (64, 1, 3, 3), "cnn.bias": (64,), "cnn1.weight": (64, 64, 3, 3), "cnn1.bias": (64,),
              "cnn2.weight": (64, 64, 3, 3), "cnn2.bias": (64,), "final.weight": (1, 36480), "final.bias": (1,)}
    fan = {"cnn": 9, "cnn1": 576, "cnn2": 576, "final": 36480}
    W = {k: (r.uniform(-1.0, 1.0, size=shapes[k]) * fan[k.split(".")[0]] ** -0.5).astype(np.float32) for k in KEYS}
    y_true = np.abs(r.normal(0.0, 1.0, size=FIXTURE_SHAPE)).astype(np.float32)
    pred = (y_true * r.uniform(0.0, 1.0, size=FIXTURE_SHAPE) + 0.1 * np.abs(r.normal(size=FIXTURE_SHAPE))).astype(
        np.float32)
    return W, y_true, pred


def sample_index(name, numel):
    """the seeded SAMPLE-element subset of a gradient the fixture stores (all of it when smaller)"""
    import zlib

    import numpy as np

    if numel <= SAMPLE:
        return np.arange(numel)
    r = np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))
    return np.sort(r.choice(numel, size=SAMPLE, replace=False))


def check_against_fixture(fx, scores, losses, grads, score_tol=(1e-5, 1e-6), grad_tol=1e-4):
    """scores {true, false}, losses {dis_true, dis_false, adv}, grads {name: tensor} against ref_dis.npz: the
    scores at (rtol, atol); each loss at 1e-5 relative; each gradient's stored sample within grad_tol of the
    largest stored element (never above the tensor's largest), and its sum / L2 norm within what that
    elementwise bound allows (numel resp. sqrt(numel) times it)."""
    import numpy as np

    bad = []
    for k, v in scores.items():
        ref = fx[f"score/{k}"].astype(np.float64)
        if not np.allclose(np.asarray(v, np.float64).reshape(ref.shape), ref, rtol=score_tol[0], atol=score_tol[1]):
            bad.append((f"score/{k}", float(np.abs(np.asarray(v).reshape(ref.shape) - ref).max())))
    for k, v in losses.items():
        ref = float(fx[f"loss/{k}"])
        v = v.detach() if hasattr(v, "detach") else v
        if abs(float(v) - ref) > 1e-5 * abs(ref):
            bad.append((f"loss/{k}", float(v), ref))
    for k, g in grads.items():
        g = np.asarray(g, np.float64).reshape(-1)
        smp = fx[f"grad/{k}/sample"].astype(np.float64)
        unit = grad_tol * float(np.abs(smp).max())  # the largest stored element: at most the tensor's
        e = np.abs(g[sample_index(k, g.size)] - smp).max()
        if e > unit:
            bad.append((f"grad/{k}/sample", float(e), unit))
        if abs(g.sum() - float(fx[f"grad/{k}/sum"])) > unit * g.size:
            bad.append((f"grad/{k}/sum", float(g.sum()), float(fx[f"grad/{k}/sum"])))
        if abs(np.linalg.norm(g) - float(fx[f"grad/{k}/norm"])) > unit * g.size ** 0.5:
            bad.append((f"grad/{k}/norm", float(np.linalg.norm(g)), float(fx[f"grad/{k}/norm"])))
    return bad
