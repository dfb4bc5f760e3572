"""Kernel-level tests of the step's small kernels against the fp64 references of tests/small_ref.py:
csrc/small.hip (time mean, speaker queries and their backward, fp32 column sums), the bf16 column sums of
csrc/convert.hip and csrc/modules.hip (tanh backward, mask split, ATTENTION 'dot').  Every bar is the a-priori
bound derived in small_ref.py, bitwise equality, or (attn_dot_fwd's device exponential) the 1e-5 of max the
project already uses for that kernel.  The C ABI is called with explicit pointers."""
import ctypes

import pytest
import torch

import small_ref as sr
from dl4ss_amd import _lib

pytestmark = pytest.mark.gpu

NAN = float("nan")
P = _lib.ptr


def _st():
    return _lib.stream_ptr()


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _within(got, s, what=""):
    """got (device fp32) against a Sum, printed before it is asserted"""
    err = (got.detach().cpu().double() - s.val).abs()
    b = sr.bar(s)
    worst = float((err / b.clamp_min(1e-300)).max())
    print(f"{what}: max err / bar = {worst:.3g}")
    assert bool(torch.isfinite(got).all()), what
    assert bool((err <= b).all()), (what, worst)


def _within_bar(got, ref, b, what=""):
    err = (got.detach().cpu().double() - ref).abs()
    worst = float((err / b.clamp_min(1e-300)).max())
    print(f"{what}: max err / bar = {worst:.3g}")
    assert bool(torch.isfinite(got).all()), what
    assert bool((err <= b).all()), (what, worst)


# ---- dl4ss_time_mean and the mean inside dl4ss_query_fwd ------------------------------------------------------
@pytest.mark.parametrize("B,T,D", sr.MEAN_SHAPES)
def test_time_mean(dev, B, T, D):
    """T = 1; T < 16 phases; T = 17 (one phase with two steps); T = 83 (the 4-way unrolled loop and its tail);
    D = 63 / 65 / 130 / 600 (partial 64-column blocks)."""
    W, K = 5, 1
    c = sr.query_case(B, K, T, D, W)
    h = c["h"].to(dev)
    ref = sr.time_mean(c["h"])
    out = torch.full((B, D), NAN, device=dev)
    _lib.call("dl4ss_time_mean", P(h), B, T, D, P(out), _st())
    _within(out, ref, "time_mean")
    # the same kernel inside dl4ss_query_fwd (h given): mean_out bitwise, q from it
    idx = c["idx"].to(torch.int32).to(dev)
    emb, wadj = c["emb"].to(dev), c["wadj"].to(dev)
    q = torch.full((B, K, W), NAN, device=dev)
    mo = torch.full((B, D), NAN, device=dev)
    _lib.call("dl4ss_query_fwd", P(h), B, T, D, P(idx), P(emb), P(wadj), K, W, P(q), P(mo), _st())
    assert _same(mo, out)
    _within(q, sr.query_fwd(mo.cpu(), c["idx"], c["emb"], c["wadj"]), "query_fwd after mean")


# ---- dl4ss_query_fwd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,T,D,W", sr.QFWD_SHAPES)
def test_query_fwd(dev, B, K, T, D, W):
    """K = 4 / 5 / 9 (one full grid.z group, a group of one, three groups), W = 64 / 70 (more than one lane
    pass over the embedding part), D = 63 / 130 (D % 64 != 0); ids with a repeat within a row, the last label
    and -1.  A -1 row is an exactly zero query with and without w_adj."""
    c = sr.query_case(B, K, T, D, W)
    idx64 = c["idx"]
    assert (idx64 == sr.N_LABELS - 1).any() and (idx64 < 0).any() and int(idx64[0, 0]) == int(idx64[0, 1])
    idx = idx64.to(torch.int32).to(dev)
    h, emb, wadj = c["h"].to(dev), c["emb"].to(dev), c["wadj"].to(dev)
    none = (idx64 < 0).to(dev)
    # the gather as EmbeddingGatherFn calls it: w_adj NULL, mean_out NULL; bit for bit the embedding rows
    q0 = torch.full((B, K, W), NAN, device=dev)
    _lib.call("dl4ss_query_fwd", P(emb), B, 1, 1, P(idx), P(emb), None, K, W, P(q0), None, _st())
    want = torch.where(none[..., None], torch.zeros((), device=dev), emb[idx.long().clamp_min(0)])
    assert _same(q0, want.contiguous())
    assert float(q0[none].abs().max()) == 0.0
    # h given
    q1 = torch.full((B, K, W), NAN, device=dev)
    mo = torch.full((B, D), NAN, device=dev)
    _lib.call("dl4ss_query_fwd", P(h), B, T, D, P(idx), P(emb), P(wadj), K, W, P(q1), P(mo), _st())
    _within(mo, sr.time_mean(c["h"]), "mean_out")
    ref = sr.query_fwd(mo.cpu(), idx64, c["emb"], c["wadj"])
    _within(q1, ref, "query_fwd (h given)")
    # h NULL: mean_out is read
    q2 = torch.full((B, K, W), NAN, device=dev)
    mo2 = mo.clone()
    _lib.call("dl4ss_query_fwd", None, B, T, D, P(idx), P(emb), P(wadj), K, W, P(q2), P(mo2), _st())
    assert _same(q2, q1) and _same(mo2, mo)
    assert float(q1[none].abs().max()) == 0.0, "a -1 row must be a zero query with w_adj"


# ---- dl4ss_query_bwd / _ex ---------------------------------------------------------------------------------------
def _qbwd(dev, name, c, B, K, T, D, W, demb, dwadj, dh, wadj=True, ex=None):
    idx = c["idx"].to(torch.int32).to(dev)
    dq = c["dq"].to(dev)
    emb, wa, mean = c["emb"].to(dev), c["wadj"].to(dev), c["mean"].to(dev)
    args = [P(dq), B, T, D, P(idx), P(emb) if wadj else None, P(wa) if wadj else None, P(mean) if wadj else None, K, W,
            P(demb), P(dwadj), P(dh)]
    if ex is not None:
        args += [sr.N_LABELS, ex]
    _lib.call(name, *args, _st())
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,K,D,W,kind", sr.QBWD_SHAPES)
def test_query_bwd(dev, B, K, D, W, kind):
    """B = 33: a partial last QCH = 32 chunk of dW_adj's sum over b (and 66 rows: a partial third chunk of its
    sum over b k); 70 rows: two 64-row ballots of query_bwd_emb with one speaker at rows 2 and 66; W = 64 / 70:
    full / partial chunks of the sums over o and a second lane pass; D = 63 / 130; one batch of a single speaker;
    -1 rows contribute nothing."""
    T = 5
    c = sr.query_case(B, K, T, D, W, kind)
    L = sr.N_LABELS
    if kind == "far":
        f = c["idx"].view(-1)
        assert int(f[2]) == int(f[66]) and int((f == f[2]).sum()) == 2 and (f < 0).any()
    new = lambda: (c["old_emb"].to(dev).clone(), c["old_wadj"].to(dev).clone(), torch.full((B, D), NAN, device=dev))
    # beta 1: adds into prefilled gradients
    demb, dwadj, dh = new()
    _qbwd(dev, "dl4ss_query_bwd", c, B, K, T, D, W, demb, dwadj, dh)
    r = sr.query_bwd(c["dq"], c["idx"], c["emb"], c["wadj"], c["mean"], T, L, c["old_emb"], c["old_wadj"])
    _within(dh, r["dh"], "dh_bcast")
    _within(demb, r["demb"], "d_emb")
    _within(dwadj, r["dwadj"], "d_wadj")
    # a second call, and _ex with beta 1: the same bits
    for name, ex in (("dl4ss_query_bwd", None), ("dl4ss_query_bwd_ex", 1.0)):
        e2, w2, h2 = new()
        _qbwd(dev, name, c, B, K, T, D, W, e2, w2, h2, ex=ex)
        assert _same(e2, demb) and _same(w2, dwadj) and _same(h2, dh), name
    # beta 0 over NaN-filled gradients: every element written or zeroed, nothing read
    e0 = torch.full((L, W), NAN, device=dev)
    w0 = torch.full((W, D + W), NAN, device=dev)
    h0 = torch.full((B, D), NAN, device=dev)
    _qbwd(dev, "dl4ss_query_bwd_ex", c, B, K, T, D, W, e0, w0, h0, ex=0.0)
    r0 = sr.query_bwd(c["dq"], c["idx"], c["emb"], c["wadj"], c["mean"], T, L)
    _within(e0, r0["demb"], "d_emb beta 0")
    _within(w0, r0["dwadj"], "d_wadj beta 0")
    assert _same(h0, dh)
    owned = torch.zeros(L, dtype=torch.bool)
    owned[c["idx"][c["idx"] >= 0]] = True
    assert float(e0.cpu()[~owned].abs().max() if (~owned).any() else 0.0) == 0.0
    # NULL forms: each part's bits do not depend on which others are asked for
    e3, w3, _ = new()
    _qbwd(dev, "dl4ss_query_bwd", c, B, K, T, D, W, e3, w3, None)
    assert _same(e3, demb) and _same(w3, dwadj)
    e4, _, h4 = new()
    _qbwd(dev, "dl4ss_query_bwd", c, B, K, T, D, W, e4, None, h4)
    assert _same(e4, demb) and _same(h4, dh)
    # d_emb only, w_adj NULL: the scatter EmbeddingGatherFn's backward runs
    e5, _, _ = new()
    _qbwd(dev, "dl4ss_query_bwd", c, B, K, 1, 1, W, e5, None, None, wadj=False)
    _within(e5, sr.query_bwd(c["dq"], c["idx"], c["emb"], None, None, 1, L, c["old_emb"])["demb"], "d_emb gather")


# ---- column sums ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,lda", sr.COLSUM_SHAPES)
def test_colsum_f32(dev, M, N, lda):
    """M = 255 / 257 / 1000: a short block, one row past a 256-row block, four blocks; N = 63 / 65 / 130; a
    padded leading dimension whose NaN padding must not be read into any sum; out is added to."""
    A = torch.full((M, lda), NAN)
    A[:, :N] = sr.inputs(M, M, N)
    old = sr.inputs(M + 1, N)
    out = torch.full((N + 3,), 7.0, device=dev)
    out[:N] = old.to(dev)
    Ad = A.to(dev)
    _lib.call("dl4ss_colsum", P(Ad), lda, M, N, P(out), _st())
    _within(out[:N], sr.colsum(A[:, :N], old), "colsum")
    assert bool((out[N:] == 7.0).all())


def _bf16_case(dev, M, N, lda, off):
    flat = torch.full((M * lda + 16,), NAN, dtype=torch.bfloat16)
    A = flat[off:off + M * lda].view(M, lda)
    A[:, :N] = sr.inputs(M, M, N).bfloat16()
    fd = flat.to(dev)
    return A[:, :N].clone(), fd, fd.data_ptr() + 2 * off


@pytest.mark.parametrize("M,N,lda,off", [s + (0,) for s in sr.COLSUM_BF16_VEC] + sr.COLSUM_BF16_SCALAR)
def test_colsum_bf16(dev, M, N, lda, off):
    """The 16-B vector path (lda % 8 == 0, aligned base: N = 513 and 520 end in a partly / fully used last
    8-column group of a second 512-column block, N = 8 is one group) and the scalar path (lda = 129; lda = 66
    from a base one element off 16-B alignment).  The padding columns hold NaN, `part` is NaN-filled."""
    vec = lda % 8 == 0 and off == 0
    assert vec == ((M, N, lda) in sr.COLSUM_BF16_VEC)
    A, keep, ap = _bf16_case(dev, M, N, lda, off)
    ap = ctypes.c_void_p(ap)
    old = sr.inputs(M + 1, N)
    ref = sr.colsum(A, old)
    # the atomic form
    out = old.to(dev).clone()
    _lib.call("dl4ss_colsum_bf16", ap, lda, M, N, P(out), _st())
    _within(out, ref, "colsum_bf16")
    # the deterministic forms
    pb = _lib.query("dl4ss_colsum_bf16_part_bytes", M, N)
    assert pb == (M + 255) // 256 * N * 4

    def det(name, o, *beta):
        part = torch.full((pb // 4 + 8,), NAN, device=dev)
        _lib.call(name, ap, lda, M, N, P(o), P(part), pb, *beta, _st())
        torch.cuda.synchronize()
        assert bool(torch.isnan(part[pb // 4:]).all())
        return o

    o1 = det("dl4ss_colsum_bf16_det", old.to(dev).clone())
    _within(o1, ref, "colsum_bf16_det")
    assert _same(det("dl4ss_colsum_bf16_det", old.to(dev).clone()), o1)
    assert _same(det("dl4ss_colsum_bf16_det_ex", old.to(dev).clone(), 1.0), o1)
    z = det("dl4ss_colsum_bf16_det", torch.zeros(N, device=dev))
    b0 = det("dl4ss_colsum_bf16_det_ex", torch.full((N,), NAN, device=dev), 0.0)
    assert bool(torch.isfinite(b0).all()) and torch.equal(b0, z)
    _within(b0, sr.colsum(A), "colsum_bf16_det_ex beta 0")
    # M = 0: an empty sum
    e0 = torch.full((N,), NAN, device=dev)
    _lib.call("dl4ss_colsum_bf16_det_ex", ap, lda, 0, N, P(e0), None, 0, 0.0, _st())
    assert float(e0.abs().max()) == 0.0
    e1 = old.to(dev).clone()
    _lib.call("dl4ss_colsum_bf16_det_ex", ap, lda, 0, N, P(e1), None, 0, 1.0, _st())
    assert _same(e1, old.to(dev))
    del keep


# ---- dl4ss_tanh_bwd, dl4ss_mask_split -------------------------------------------------------------------------------
ELEMWISE_N = [1, 3, 4, 5, 1027, 16384 * 1024 + 5]  # the last: the second grid-stride pass (16384 blocks x 1024)


@pytest.mark.parametrize("n", ELEMWISE_N)
def test_tanh_bwd(dev, n):
    g = torch.Generator().manual_seed(n % 9973)
    v = torch.tanh(torch.randn(n, generator=g))
    dv = torch.randn(n, generator=g)
    out = torch.full((n + 4,), 7.0, device=dev)
    vd, dvd = v.to(dev), dv.to(dev)
    _lib.call("dl4ss_tanh_bwd", P(vd), P(dvd), P(out), n, _st())
    ref, b = sr.tanh_bwd(v, dv)
    _within_bar(out[:n], ref, b, "tanh_bwd")
    assert bool((out[n:] == 7.0).all())


@pytest.mark.parametrize("n", ELEMWISE_N)
def test_mask_split(dev, n):
    """pred = m x and resid = (1 - m) x are single fp32 operations: bit for bit torch's.  Either output NULL;
    the scalar path from pointers one element off 16-B alignment."""
    g = torch.Generator().manual_seed(n % 9973 + 1)
    m = torch.rand(n + 1, generator=g)
    x = torch.randn(n + 1, generator=g)
    md, xd = m.to(dev), x.to(dev)
    for off in ((0, 1) if n < 10 ** 6 else (0,)):
        mm, xx = m[off:off + n], x[off:off + n]
        want_p, want_r = (mm * xx).to(dev), ((1.0 - mm) * xx).to(dev)
        for use_p, use_r in ((True, True), (True, False), (False, True)):
            pred = torch.full((n + 5,), 7.0, device=dev)
            res = torch.full((n + 5,), 7.0, device=dev)
            pv, rv = pred[off:off + n], res[off:off + n]
            _lib.call("dl4ss_mask_split", P(md[off:off + n]), P(xd[off:off + n]), n, P(pv) if use_p else None,
                      P(rv) if use_r else None, _st())
            assert _same(pv, want_p if use_p else torch.full_like(pv, 7.0)), (off, use_p, use_r)
            assert _same(rv, want_r if use_r else torch.full_like(rv, 7.0)), (off, use_p, use_r)
            assert bool((pred[off + n:] == 7.0).all()) and bool((res[off + n:] == 7.0).all())
            assert bool((pred[:off] == 7.0).all()) and bool((res[:off] == 7.0).all())
            if n > 10 ** 6:
                break


# ---- ATTENTION 'dot' ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("Bq,R", sr.DOT_SHAPES)
def test_attn_dot(dev, Bq, R, act):
    """R = 1 / 255 / 256 / 257 / 903: one row, one row short of a 256-row block, exactly one, one past it,
    four blocks with a ragged last one.  Both activations; q_stride 50 and 100 (the cRM halves)."""
    E = 50
    c = sr.dot_case(Bq, R)
    V = c["V"].clone()
    if R >= 255:  # logits of exactly +-20: rows 0-9 / 10-19 of every utterance
        V[:, :20, :] = 0.0
        V[:, :10, 0] = 20.0 / c["q"][:, None, 0]
        V[:, 10:20, 0] = -20.0 / c["q"][:, None, 0]
    Vd, q2 = V.to(dev), c["q"].to(dev)
    nblk = _lib.query("dl4ss_attn_dot_nblk", R)
    assert nblk == (R + 255) // 256
    first = None
    for half in (0, 1):
        qh = c["q"][:, half * E:(half + 1) * E].contiguous()
        ref, b = sr.attn_dot_fwd(V, qh, act)
        mask = torch.full((Bq, R), NAN, device=dev)
        qptr = ctypes.c_void_p(q2.data_ptr() + 4 * E * half)
        _lib.call("dl4ss_attn_dot_fwd", P(Vd), qptr, 2 * E, Bq, R, E, act, P(mask), _st())
        _within_bar(mask, ref, b, f"attn_dot_fwd half {half}")
        if half == 0:  # the contiguous query: the same bits; the strided output: gaps untouched
            qc = qh.to(dev)
            m2 = torch.full((Bq, R), NAN, device=dev)
            _lib.call("dl4ss_attn_dot_fwd", P(Vd), P(qc), E, Bq, R, E, act, P(m2), _st())
            assert _same(m2, mask)
            ms = 2 * R + 3
            m3 = torch.full((Bq, ms), 7.0, device=dev)
            _lib.call("dl4ss_attn_dot_fwd_ex", P(Vd), P(qc), E, Bq, R, E, act, P(m3), ms, _st())
            assert _same(m3[:, :R].contiguous(), mask) and bool((m3[:, R:] == 7.0).all())
            first = (qh, qc, mask)
    # backward, from the mask the forward saved
    qh, qc, mask = first
    dmask = c["dmask"].to(dev)
    dV_old = c["dV_old"]
    dV, dV_bar, dq, dq_bar = sr.attn_dot_bwd(V, qh, mask.cpu(), c["dmask"], act, dV_old)

    def bwd(dv):
        part = torch.full((Bq * nblk * E,), NAN, device=dev)
        o = torch.full((Bq, E), NAN, device=dev)
        _lib.call("dl4ss_attn_dot_bwd", P(Vd), P(qc), E, P(mask), P(dmask), Bq, R, E, act, P(dv), P(part), P(o), _st())
        torch.cuda.synchronize()
        return o

    dvd = dV_old.to(dev).clone()
    o1 = bwd(dvd)
    _within_bar(dvd, dV, dV_bar, "attn_dot dV")
    _within_bar(o1, dq.val, dq_bar, "attn_dot dq")
    assert _same(bwd(None), o1)                    # dV NULL
    assert _same(bwd(dV_old.to(dev).clone()), o1)  # twice the same bits
    if R >= 255:
        sat = mask.cpu()[:, :20]
        if act == 0:
            assert bool((sat[:, :10] == 1.0).all()) and bool((sat[:, 10:] < 3e-9).all())
            # a mask of exactly 1: no gradient, dV keeps its prefilled bits
            assert _same(dvd[:, :10].contiguous(), dV_old[:, :10].to(dev).contiguous())
        else:
            assert bool((sat[:, :10] == 10.0).all()) and bool((sat[:, 10:] == -10.0).all())
            assert _same(dvd[:, :20].contiguous(), dV_old[:, :20].to(dev).contiguous())
