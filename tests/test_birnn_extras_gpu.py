"""The bf16 by-products of the packed recurrence (precision 1, H = 300), the operands every GEMM of the bf16 step
reads, checked against the fp32 outputs of the SAME call rather than against another run of themselves:
out_bf16 / hprev_bf16 / h_mean / the out = NULL form of the forward, dG_bf16 / dGh_bf16 (also with
DL4SS_RNN_DGH_PAD8), the fused db_ih / db_hh and DL4SS_RNN_DEFER_BIAS with dl4ss_birnn_bias_reduce[_ex] of the
BPTT.  A bf16 copy must be the round-to-nearest-even of the fp32 value, bit for bit (torch's .bfloat16() is that
rounding); a sum is held to its a-priori bound (small_ref.py); pad columns and guard regions keep a sentinel."""
import ctypes

import pytest
import torch

import small_ref as sr
from dl4ss_amd import _lib

pytestmark = pytest.mark.gpu

H = 300
CELLS = {"lstm": 0, "gru": 1}
DGH_PAD8, DEFER_BIAS = 0x200, 0x400
P = _lib.ptr
SENT = 7.0       # exact in bf16
GUARD = 64       # elements behind a buffer that must keep the sentinel
# (B, T, max_wg): batch chunks of 1 (B = 3), 4 (B = 32; T = 1 and 3: the edges of the BPTT's two-step prefetch)
# and 8 (B = 33: a partial last chunk; B = 29 under a 120-workgroup budget)
SHAPES = [(3, 5, 0), (32, 1, 0), (32, 3, 0), (33, 4, 0), (29, 3, 120)]


def p8(n):
    return (n + 7) // 8 * 8


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


class _Budget:
    """dl4ss_debug_set_rnn_max_wg for the duration of a test, restored in any case"""

    def __init__(self, max_wg):
        self.max_wg = max_wg

    def __enter__(self):
        if self.max_wg:
            _lib.lib().dl4ss_debug_set_rnn_max_wg(self.max_wg)

    def __exit__(self, *exc):
        if self.max_wg:
            _lib.lib().dl4ss_debug_set_rnn_max_wg(0)


def _plan(cell, B):
    info = (ctypes.c_int * 5)()
    _lib.call("dl4ss_birnn_plan_info", CELLS[cell], B, H, 1, 0, info)
    return list(info)


def test_plans_cover_batch_chunks_1_4_8():
    seen = set()
    for B, _, wg in SHAPES:
        with _Budget(wg):
            seen.add(_plan("lstm", B)[0])
            assert _plan("gru", B)[0] == _plan("lstm", B)[0]
    assert {1, 4, 8} <= seen, seen


class _Layer:
    def __init__(self, dev, cell, B, T, seed):
        g = torch.Generator().manual_seed(seed)
        self.dev, self.cell, self.cid, self.B, self.T = dev, cell, CELLS[cell], B, T
        self.NGH = (4 if cell == "lstm" else 3) * H
        NGH = self.NGH
        self.G = (torch.randn(B, T, 2, NGH, generator=g) * 0.5).to(dev)
        self.whh = (torch.randn(2, NGH, H, generator=g) / H ** 0.5).to(dev)
        self.bhh = (torch.randn(2, NGH, generator=g) * 0.1).to(dev)
        self.dout = torch.randn(B, T, 2 * H, generator=g).to(dev)
        self.dout2 = torch.randn(B, T, 2 * H, generator=g).to(dev)
        self.bcast = torch.randn(B, 2 * H, generator=g).to(dev)
        self.dbi0 = torch.randn(2, NGH, generator=g)
        self.dbh0 = torch.randn(2, NGH, generator=g)
        self.wsn = _lib.query("dl4ss_birnn_workspace_bytes", self.cid, B, H)
        assert self.wsn > 0
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)

    def ws(self):
        return torch.zeros((self.wsn + 7) // 8, dtype=torch.int64, device=self.dev)

    def f32(self, *shape):
        return torch.full(shape, float("nan"), device=self.dev)

    def b16(self, n):
        return torch.full((n + GUARD,), SENT, device=self.dev, dtype=torch.bfloat16)

    def done(self):
        torch.cuda.synchronize()
        assert int(self.status.item()) == 0

    def forward(self, out=True, hprev=True, mean=None, entry="dl4ss_birnn_fwd_ex"):
        B, T = self.B, self.T
        r = dict(out=self.f32(B, T, 2 * H) if out else None, hprev=self.f32(B, T, 2 * H) if hprev else None,
                 act=self.f32(B, T, 2, 4 * H), cs=self.f32(B, T, 2, H) if self.cell == "lstm" else None,
                 outb=self.b16(B * T * p8(2 * H)), hprevb=self.b16(B * T * 2 * p8(H)),
                 mean=self.f32(B, 2 * H) if mean else None, ws=self.ws())
        args = [self.cid, 1, B, T, H, P(self.G), P(self.whh), P(self.bhh), P(r["out"]), P(r["hprev"]), P(r["act"]),
                P(r["cs"]), P(r["outb"]), P(r["hprevb"])]
        if entry == "dl4ss_birnn_fwd_mean":
            args.append(P(r["mean"]))
        _lib.call(entry, *args, P(r["ws"]), self.wsn, P(self.status), _lib.stream_ptr())
        self.done()
        return r

    def backward(self, fwd, flags=0, f32=True, dout=None, dbi=None, dbh=None, ws=None):
        B, T, NGH, gru = self.B, self.T, self.NGH, self.cell == "gru"
        ghb = p8(NGH) if flags & DGH_PAD8 else NGH
        r = dict(dG=self.f32(B * T, 2 * NGH) if f32 else None, dGh=self.f32(B * T, 2 * NGH) if f32 and gru else None,
                 dGb=self.b16(B * T * 2 * NGH), dGhb=self.b16(B * T * 2 * ghb) if gru else None,
                 dbi=(self.dbi0 if dbi is None else dbi).to(self.dev).clone(),
                 dbh=(self.dbh0 if dbh is None else dbh).to(self.dev).clone(), ws=self.ws() if ws is None else ws)
        _lib.call("dl4ss_birnn_bwd_ex", self.cid, 1 | flags, B, T, H, P(self.dout if dout is None else dout),
                  P(self.bcast), P(self.whh), P(fwd["act"]), P(fwd["cs"]), P(fwd["hprev"]), P(r["dG"]), P(r["dGh"]),
                  P(r["dGb"]), P(r["dGhb"]), P(r["dbi"]), P(r["dbh"]), P(r["ws"]), self.wsn, P(self.status),
                  _lib.stream_ptr())
        self.done()
        return r


def _guard_ok(buf, n):
    return bool((buf[n:].float() == SENT).all())


# ---- forward: dl4ss_birnn_fwd_ex -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("B,T,wg", SHAPES)
def test_fwd_bf16_copies(dev, cell, B, T, wg):
    with _Budget(wg):
        L = _Layer(dev, cell, B, T, 100 * B + T)
        r = L.forward()
        hp8 = p8(H)
        outb = r["outb"][:B * T * 2 * H].view(B * T, 2 * H)
        assert _same(outb, r["out"].view(B * T, 2 * H).bfloat16())
        assert _guard_ok(r["outb"], B * T * 2 * H)
        hb = r["hprevb"][:B * T * 2 * hp8].view(B * T, 2, hp8)
        assert _same(hb[:, :, :H], r["hprev"].view(B * T, 2, H).bfloat16())
        assert bool((hb[:, :, H:].float() == SENT).all()), "pad columns 300..303 / 604..607 are not written"
        assert _guard_ok(r["hprevb"], B * T * 2 * hp8)
        # hprev is the output shifted by one step, zero at each direction's first step
        o = r["out"].view(B, T, 2, H)
        shifted = torch.zeros_like(o)
        shifted[:, 1:, 0] = o[:, :-1, 0]
        shifted[:, :-1, 1] = o[:, 1:, 1]
        assert _same(r["hprev"].view(B, T, 2, H), shifted)
        if cell == "lstm":  # hprev NULL: the bf16 copy is still written
            r2 = L.forward(hprev=False)
            hb2 = r2["hprevb"][:B * T * 2 * hp8].view(B * T, 2, hp8)
            assert _same(r2["out"], r["out"])
            assert _same(hb2[:, :, :H], shifted.view(B * T, 2, H).bfloat16())
            assert bool((hb2[:, :, H:].float() == SENT).all()) and _guard_ok(r2["hprevb"], B * T * 2 * hp8)


# ---- forward: h_mean and the out = NULL form -------------------------------------------------------------------
def _check_mean(mean, out, T):
    """h_mean against the fp64 mean over t of the fp32 out of the same call: T terms summed in step order and
    one division: (T + 2) u S / T (n = T; c = 2: the division and the second-order unit)."""
    s = sr.time_mean(out.cpu())
    assert s.n == T and s.c == 2
    err = (mean.cpu().double() - s.val).abs()
    b = sr.bar(s)
    print(f"h_mean: max err / bar = {float((err / b.clamp_min(1e-300)).max()):.3g}")
    assert bool((err <= b).all())


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("T", [1, 2, 5, 17])
def test_fwd_mean(dev, cell, T):
    B = 3
    L = _Layer(dev, cell, B, T, 7 + T)
    r = L.forward(mean=True, entry="dl4ss_birnn_fwd_mean")
    _check_mean(r["mean"], r["out"], T)
    assert _same(r["outb"][:B * T * 2 * H].view(B, T, 2 * H), r["out"].bfloat16())
    r2 = L.forward(out=False, mean=True, entry="dl4ss_birnn_fwd_mean")  # out NULL
    assert _same(r2["outb"], r["outb"]) and _same(r2["mean"], r["mean"]) and _same(r2["hprevb"], r["hprevb"])


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("T", [1, 2, 5, 17])
def test_fwd_xw_mean(dev, cell, T):
    """dl4ss_birnn_fwd_xw_ex (the fused input projection, Kin = 129 at a row stride of 136)."""
    B, K = 3, 129
    L = _Layer(dev, cell, B, T, 11 + T)
    g = torch.Generator().manual_seed(T)
    x = torch.zeros(B * T, p8(K), dtype=torch.bfloat16)
    x[:, :K] = torch.randn(B * T, K, generator=g).bfloat16()
    wih = torch.zeros(2 * L.NGH, p8(K), dtype=torch.bfloat16)
    wih[:, :K] = (torch.randn(2 * L.NGH, K, generator=g) * 0.1).bfloat16()
    bih = (torch.randn(2, L.NGH, generator=g) * 0.1).to(dev)
    x, wih = x.to(dev), wih.to(dev)
    assert _lib.query("dl4ss_birnn_fwd_xw_supported", L.cid, B, T, H, K) == 1

    def run(out):
        r = dict(out=L.f32(B, T, 2 * H) if out else None, hprev=L.f32(B, T, 2 * H), act=L.f32(B, T, 2, 4 * H),
                 cs=L.f32(B, T, 2, H) if cell == "lstm" else None, outb=L.b16(B * T * 2 * H),
                 hprevb=L.b16(B * T * 2 * p8(H)), mean=L.f32(B, 2 * H), ws=L.ws())
        _lib.call("dl4ss_birnn_fwd_xw_ex", L.cid, B, T, H, P(x), K, p8(K), P(wih), p8(K), P(bih), P(L.whh), P(L.bhh),
                  P(r["out"]), P(r["hprev"]), P(r["act"]), P(r["cs"]), P(r["outb"]), P(r["hprevb"]), P(r["mean"]),
                  P(r["ws"]), L.wsn, P(L.status), _lib.stream_ptr(), 0)
        L.done()
        return r

    r = run(True)
    _check_mean(r["mean"], r["out"], T)
    assert _same(r["outb"][:B * T * 2 * H].view(B, T, 2 * H), r["out"].bfloat16())
    assert _same(r["hprevb"][:B * T * 2 * p8(H)].view(B * T, 2, p8(H))[:, :, :H],
                 r["hprev"].view(B * T, 2, H).bfloat16())
    r2 = run(False)
    assert _same(r2["outb"], r["outb"]) and _same(r2["mean"], r["mean"]) and _same(r2["hprevb"], r["hprevb"])


# ---- backward: dl4ss_birnn_bwd_ex ----------------------------------------------------------------------------------
def _check_bias(db, prefill, dG, B, T, what):
    """db = prefill + sum_{(b, t)} dG: each cell sums its T steps, the reduce then the B rows and the prefill --
    B T + 1 terms in all; the issue's count (B T + B + 4) u S is kept (it allows a rounding per row partial
    more than the B T + 1 + c of the plain chain)."""
    NGH2 = dG.shape[1]
    t = torch.cat([prefill.double().view(1, NGH2), dG.cpu().double()], 0)  # (1 + B T, 2 NGH)
    ref, S = t.sum(0), t.abs().sum(0)
    b = (B * T + B + 4) * sr.U * S
    err = (db.cpu().double().view(-1) - ref).abs()
    print(f"{what}: max err / bar = {float((err / b).max()):.3g}")
    assert bool((err <= b).all()), what


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("B,T,wg", SHAPES)
def test_bwd_bf16_copies_and_bias(dev, cell, B, T, wg):
    with _Budget(wg):
        L = _Layer(dev, cell, B, T, 31 * B + T)
        NGH, gru = L.NGH, cell == "gru"
        n = B * T * 2 * NGH
        f = L.forward()
        a = L.backward(f)
        assert bool(torch.isfinite(a["dG"]).all())
        assert _same(a["dGb"][:n].view(B * T, 2 * NGH), a["dG"].bfloat16()) and _guard_ok(a["dGb"], n)
        if gru:
            assert _same(a["dGhb"][:n].view(B * T, 2 * NGH), a["dGh"].bfloat16()) and _guard_ok(a["dGhb"], n)
        # the fused bias gradients, from the prefilled buffers
        _check_bias(a["dbi"], L.dbi0, a["dG"], B, T, "db_ih")
        _check_bias(a["dbh"], L.dbh0, a["dGh"] if gru else a["dG"], B, T, "db_hh")
        # fp32 outputs NULL: the bf16 ones and the bias sums keep their bits
        b = L.backward(f, f32=False)
        assert _same(b["dGb"], a["dGb"]) and _same(b["dbi"], a["dbi"]) and _same(b["dbh"], a["dbh"])
        if gru:
            assert _same(b["dGhb"], a["dGhb"])
            # DL4SS_RNN_DGH_PAD8: each direction's 900 columns at a stride of 904, pads untouched
            c = L.backward(f, flags=DGH_PAD8, f32=False)
            gp = p8(NGH)
            assert gp == 904
            padded = c["dGhb"][:B * T * 2 * gp].view(B * T, 2, gp)
            assert _same(padded[:, :, :NGH], a["dGhb"][:n].view(B * T, 2, NGH))
            assert bool((padded[:, :, NGH:].float() == SENT).all()), "the four pad columns are not written"
            assert _guard_ok(c["dGhb"], B * T * 2 * gp)
            assert _same(c["dGb"], a["dGb"]) and _same(c["dbi"], a["dbi"]) and _same(c["dbh"], a["dbh"])


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("B,T,wg", SHAPES)
def test_bwd_deferred_bias(dev, cell, B, T, wg):
    with _Budget(wg):
        L = _Layer(dev, cell, B, T, 17 * B + T)
        f = L.forward()
        VP = ctypes.c_void_p
        one = lambda t: (VP * 1)(t.data_ptr())
        a = L.backward(f)                                   # undeferred, into the prefill
        d = L.backward(f, flags=DEFER_BIAS)
        assert _same(d["dbi"], L.dbi0.to(dev)) and _same(d["dbh"], L.dbh0.to(dev)), "the BPTT leaves db untouched"
        assert _same(d["dGb"], a["dGb"])
        _lib.call("dl4ss_birnn_bias_reduce", L.cid, B, H, 1, one(d["ws"]), one(d["dbi"]), one(d["dbh"]),
                  _lib.stream_ptr())
        torch.cuda.synchronize()
        assert _same(d["dbi"], a["dbi"]) and _same(d["dbh"], a["dbh"])
        # beta 0 over NaN: the undeferred call into zeros
        z = L.backward(f, dbi=torch.zeros(2, L.NGH), dbh=torch.zeros(2, L.NGH))
        ni, nh = L.f32(2, L.NGH), L.f32(2, L.NGH)
        _lib.call("dl4ss_birnn_bias_reduce_ex", L.cid, B, H, 1, one(d["ws"]), one(ni), one(nh), 0.0, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ni).all()) and torch.equal(ni, z["dbi"]) and torch.equal(nh, z["dbh"])
        # two launches with different dOut on two workspaces, one n = 2 reduce: each its own result
        a2 = L.backward(f, dout=L.dout2)
        assert not _same(a2["dbi"], a["dbi"])
        d1 = L.backward(f, flags=DEFER_BIAS)
        d2 = L.backward(f, flags=DEFER_BIAS, dout=L.dout2)
        two = lambda x, y: (VP * 2)(x.data_ptr(), y.data_ptr())
        _lib.call("dl4ss_birnn_bias_reduce", L.cid, B, H, 2, two(d1["ws"], d2["ws"]), two(d1["dbi"], d2["dbi"]),
                  two(d1["dbh"], d2["dbh"]), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert _same(d1["dbi"], a["dbi"]) and _same(d1["dbh"], a["dbh"])
        assert _same(d2["dbi"], a2["dbi"]) and _same(d2["dbh"], a2["dbh"])
