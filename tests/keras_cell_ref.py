"""fp64 torch-CPU restatement of one bidirectional layer of Keras 1's LSTM cell (DL4SS_RNN_HARD_GATES), written from
the cell's formulae -- shared by test_keras_cell_api_cpu.py and the test_keras_cell_* GPU files.

With z = G[:, t] + h W_hh^T + b_hh (this project's gate order i, f, g, o; both directions from a zero state, the
reverse one walking t = T-1 .. 0):

    i, f, o = hs(z),  hs(z) = min(max(0.2 z + 0.5, 0), 1)        g = tanh(z_g)
    c = f c + i g                                                 h = o tanh(c)

The gradients are a hand-written BPTT that takes the saturation pattern -- for every i, f, o value whether it lies
strictly inside (0, 1), where hs' = 0.2, or on the clip, where hs' = 0 -- as an INPUT.  hs has kinks at z = +-2.5: a
pre-activation that fp32 and fp64 place on opposite sides of one flips a derivative between 0 and 0.2, and the flip
travels through the whole BPTT.  A test therefore compares the patterns first (they may differ only where the fp64
|z| is within KINK of 2.5, and only at a share CAP of the gates) and then takes the fp64 gradients with the pattern
of the code under test.  ``HardLSTMLayer`` is the same pair as a torch.autograd.Function, for restatements composed
with autograd.
"""
import torch

KINK = 1e-4   # a gate whose fp64 | |z| - 2.5 | is below this may saturate differently in fp32
CAP = 1e-3    # at most this share of the i, f, o gates may do so
SLOPE, SHIFT, EDGE = 0.2, 0.5, 2.5


def hs(z):
    """Theano's hard_sigmoid: slope 0.2, shift 0.5, clip to [0, 1]."""
    return (SLOPE * z + SHIFT).clamp(0.0, 1.0)


def inside(act):
    """(.., 4H) bool: True where an i / f / o activation lies strictly inside (0, 1) (hs' = 0.2); the g block
    (columns [2H, 3H)) is True throughout and unused."""
    m = (act > 0) & (act < 1)
    H = act.shape[-1] // 4
    m[..., 2 * H:3 * H] = True
    return m


def forward(G, w_hh, b_hh):
    """G (B, T, 2, 4H), w_hh (2, 4H, H), b_hh (2, 4H), any float dtype -> fp64 dict: out (B, T, 2H) [fwd | reverse],
    hprev (B, T, 2H) (h before step t in its direction), act (B, T, 2, 4H) the gate activations (i, f, o clipped),
    z (B, T, 2, 4H) the gate pre-activations, cs (B, T, 2, H) the cell states."""
    G, w_hh, b_hh = G.double(), w_hh.double(), b_hh.double()
    B, T, _, GH = G.shape
    H = GH // 4
    out, hprev = torch.zeros(B, T, 2 * H, dtype=torch.float64), torch.zeros(B, T, 2 * H, dtype=torch.float64)
    act, z = torch.zeros(B, T, 2, GH, dtype=torch.float64), torch.zeros(B, T, 2, GH, dtype=torch.float64)
    cs = torch.zeros(B, T, 2, H, dtype=torch.float64)
    for d in range(2):
        h = torch.zeros(B, H, dtype=torch.float64)
        c = torch.zeros(B, H, dtype=torch.float64)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            zt = G[:, t, d] + h @ w_hh[d].T + b_hh[d]
            zi, zf, zg, zo = zt.chunk(4, -1)
            i, f, g, o = hs(zi), hs(zf), torch.tanh(zg), hs(zo)
            hprev[:, t, d * H:(d + 1) * H] = h
            c = f * c + i * g
            h = o * torch.tanh(c)
            z[:, t, d], act[:, t, d], cs[:, t, d] = zt, torch.cat([i, f, g, o], -1), c
            out[:, t, d * H:(d + 1) * H] = h
    return dict(out=out, hprev=hprev, act=act, z=z, cs=cs)


def backward(fw, w_hh, dOut=None, dOut_bcast=None, pattern=None):
    """BPTT of ``forward``'s result ``fw``: dOut (B, T, 2H) and / or dOut_bcast (B, 2H) (added at every t) -> fp64
    dict: dG (B, T, 2, 4H) (the gradient of G, and of W_hh h + b_hh), dw_hh (2, 4H, H), db_hh (2, 4H).  ``pattern``
    (B, T, 2, 4H) bool as ``inside`` gives it: where hs' = 0.2; default: the reference's own."""
    w_hh = w_hh.double()
    act, cs, hprev = fw["act"], fw["cs"], fw["hprev"]
    B, T, _, GH = act.shape
    H = GH // 4
    pattern = inside(act) if pattern is None else pattern
    dh_in = torch.zeros(B, T, 2 * H, dtype=torch.float64)
    if dOut is not None:
        dh_in = dh_in + dOut.double()
    if dOut_bcast is not None:
        dh_in = dh_in + dOut_bcast.double()[:, None, :]
    dG = torch.zeros(B, T, 2, GH, dtype=torch.float64)
    for d in range(2):
        dh_rec = torch.zeros(B, H, dtype=torch.float64)
        dc_next = torch.zeros(B, H, dtype=torch.float64)
        order = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))
        for k in range(T - 1, -1, -1):
            t = order[k]
            i, f, g, o = act[:, t, d].chunk(4, -1)
            pi, pf, _, po = (SLOPE * p.double() for p in pattern[:, t, d].chunk(4, -1))
            c = cs[:, t, d]
            c_prev = cs[:, order[k - 1], d] if k > 0 else torch.zeros_like(c)
            tc = torch.tanh(c)
            dh = dh_in[:, t, d * H:(d + 1) * H] + dh_rec
            dc = dc_next + dh * o * (1 - tc * tc)
            dz = torch.cat([dc * g * pi, dc * c_prev * pf, dc * i * (1 - g * g), dh * tc * po], -1)
            dc_next = dc * f
            dh_rec = dz @ w_hh[d]
            dG[:, t, d] = dz
    hp = hprev.view(B, T, 2, H)
    dw_hh = torch.einsum("btdg,btdh->dgh", dG, hp)
    return dict(dG=dG, dw_hh=dw_hh, db_hh=dG.sum((0, 1)))


def layer_grads(x, w_ih, dG):
    """The input projection's share, G = x W_ih^T + b_ih with x (B, T, D), w_ih (2 * 4H, D) [fwd; reverse]:
    (dx (B, T, D), dw_ih (8H, D), db_ih (8H))."""
    B, T, D = x.shape
    d2 = dG.reshape(B * T, -1)
    return (d2 @ w_ih.double()).view(B, T, D), d2.T @ x.double().reshape(B * T, D), d2.sum(0)


class HardLSTMLayer(torch.autograd.Function):
    """out (B, T, 2H) = the layer over G (B, T, 2, 4H) with w_hh (2, 4H, H), b_hh (2, 4H), in fp64; the backward is
    ``backward`` above with ``pattern`` (a bool tensor as ``inside`` gives it, or None for the reference's own)."""

    @staticmethod
    def forward(ctx, G, w_hh, b_hh, pattern=None):
        fw = forward(G.detach(), w_hh.detach(), b_hh.detach())
        ctx.fw, ctx.w_hh, ctx.pattern = fw, w_hh.detach(), pattern
        return fw["out"].clone()

    @staticmethod
    def backward(ctx, dout):
        r = backward(ctx.fw, ctx.w_hh, dOut=dout, pattern=ctx.pattern)
        return r["dG"], r["dw_hh"], r["db_hh"], None


def near_kink(z):
    """(.., 4H) bool: the i / f / o pre-activations whose | |z| - 2.5 | < KINK (the g block False)."""
    m = (z.abs() - EDGE).abs() < KINK
    H = z.shape[-1] // 4
    m[..., 2 * H:3 * H] = False
    return m


def gate_blocks(t):
    """The i, f and o blocks of a (.., 4H) tensor."""
    i, f, _, o = t.chunk(4, -1)
    return i, f, o


def saturation_shares(act):
    """{gate: (share at exactly 0, share at exactly 1, share strictly inside)} of the i, f, o activations."""
    return {n: ((a == 0).double().mean().item(), (a == 1).double().mean().item(),
                ((a > 0) & (a < 1)).double().mean().item()) for n, a in zip("ifo", gate_blocks(act))}


def assert_saturates(act):
    """The inputs make the cell saturate: each of i, f, o has >= 10 % of its values at exactly 0, >= 10 % at exactly
    1 and >= 20 % strictly inside (a test that never left the linear region would pass with hs(z) = 0.2 z + 0.5)."""
    for n, (lo, hi, mid) in saturation_shares(act).items():
        assert lo >= 0.10 and hi >= 0.10 and mid >= 0.20, (n, lo, hi, mid)


def check_pattern(dev_act, fw):
    """The device's saturation pattern against the fp64 one: equal except at gates within KINK of a kink, and those
    exceptions at most CAP of the gates.  Returns (the device's pattern, the share of exceptions)."""
    pd, pr = inside(dev_act.double()), inside(fw["act"])
    diff = pd != pr
    assert not (diff & ~near_kink(fw["z"])).any(), "a saturation flag differs away from every kink"
    share = diff.double().sum().item() / (0.75 * diff.numel())
    assert share <= CAP, share
    return pd, share


def case(B, T, H, seed=None, std=3.0):
    """The kernel tests' inputs from a fixed seed: G ~ N(0, std^2) so that the gates saturate, W_hh ~ U(+-1/sqrt(H)),
    b_hh ~ 0.1 N(0, 1), dOut and dOut_bcast ~ N(0, 1); fp32 CPU tensors."""
    g = torch.Generator().manual_seed(1000 * B + 10 * T + H if seed is None else seed)
    k = H ** -0.5
    return dict(G=torch.randn(B, T, 2, 4 * H, generator=g) * std,
                w_hh=(torch.rand(2, 4 * H, H, generator=g) * 2 - 1) * k,
                b_hh=torch.randn(2, 4 * H, generator=g) * 0.1,
                dOut=torch.randn(B, T, 2 * H, generator=g), dOut_bcast=torch.randn(B, 2 * H, generator=g))
