"""Fixed-order split-K of the fp32 GEMM (dl4ss_gemm_fixed, ops.gemm(reduce="fixed")): slab z is the unsplit
kernel on k-range z and the combine adds the slabs in the order z = 0..S-1, so the result is pinned bitwise
against plain unsplit ops.gemm calls over the same k-ranges, summed in order with torch on the device."""
import pytest
import torch

from dl4ss_amd import _lib, ops

pytestmark = pytest.mark.gpu

# M, N, K, splitk
SHAPES = [(128, 128, 64, 4),     # exact tiles; 16-B combine path
          (130, 257, 129, 3),    # ragged tiles; K tail; last slab short
          (200, 129, 1004, 7),   # N % 4 != 0: scalar combine path
          (100, 25, 1000, 31),   # the voiceprint dW_hh shape; effective S below the request
          (64, 72, 40, 4),       # kps rounds to 16, S = 3
          (5, 3, 2, 4)]          # S collapses to 1
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
SENTINEL = -7.25


def _slabs(K, splitk):
    kps = int(_lib.query("dl4ss_gemm_fixed_kps", K, splitk))
    return kps, -(-K // kps)


def _operands(dev, ta, tb, M, N, K, seed):
    """A as a column slice of a wider matrix (ld > cols, as G2[:, d*NGH:(d+1)*NGH] is), B plain, a bias."""
    g = torch.Generator().manual_seed(seed)
    ra, ca = (K, M) if ta else (M, K)
    wide = torch.randn(ra, ca + 13, generator=g).to(dev)
    A = wide[:, 5:5 + ca]
    B = (torch.randn(N, K, generator=g) if tb else torch.randn(K, N, generator=g)).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    C0 = torch.randn(M, N, generator=g).to(dev)
    return A, B, bias, C0


def _kslice(X, trans_is_k_rows, k0, k1):
    """rows k0..k1 of an operand stored with k along its rows, else the columns"""
    return X[k0:k1] if trans_is_k_rows else X[:, k0:k1]


def _in_order(A, B, ta, tb, K, splitk, bias):
    """((p0 + p1) + p2) ... + bias from unsplit ops.gemm calls over dl4ss_gemm_fixed_kps's k-ranges"""
    kps, S = _slabs(K, splitk)
    acc = None
    for z in range(S):
        k0, k1 = z * kps, min(K, (z + 1) * kps)
        p = ops.gemm(_kslice(A, ta, k0, k1), _kslice(B, not tb, k0, k1), transA=ta, transB=tb)
        acc = p if acc is None else acc + p
    return acc + bias if bias is not None else acc


def _out_views(dev, M, N, C0, pad):
    """out as a row slice of a taller matrix (as whh_g[d*NGH:(d+1)*NGH] is), and as a view with ldc = N + pad
    with sentinels in the padding; both hold C0"""
    tall = torch.full((M + 9, N), SENTINEL, device=dev)
    rows = tall[4:4 + M]
    rows.copy_(C0)
    wide = torch.full((M, N + pad), SENTINEL, device=dev)
    cols = wide[:, :N]
    cols.copy_(C0)
    return (tall, rows), (wide, cols)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("M,N,K,splitk", SHAPES)
def test_structure_bitwise_and_fp64(dev, ta, tb, M, N, K, splitk):
    A, B, bias, C0 = _operands(dev, ta, tb, M, N, K, seed=M * 7 + N)
    opA, opB = (A.double().T if ta else A.double()), (B.double().T if tb else B.double())
    prod = opA @ opB + bias.double()
    want0 = _in_order(A, B, ta, tb, K, splitk, bias)
    ws = torch.empty(max(ops.gemm_fixed_ws_bytes(M, N, K, splitk), 1), device=dev, dtype=torch.uint8)
    for beta in (0.0, 1.0, 0.5):
        (tall, rows), (wide, cols) = _out_views(dev, M, N, C0, pad=4)
        for out in (rows, cols):
            ops.gemm(A, B, transA=ta, transB=tb, bias=bias, beta=beta, out=out, splitk=splitk, reduce="fixed", ws=ws)
        assert torch.equal(rows, cols)
        assert (tall[:4] == SENTINEL).all() and (tall[4 + M:] == SENTINEL).all() and (wide[:, N:] == SENTINEL).all()
        if beta == 0.0:
            assert torch.equal(rows, want0)
        elif beta == 1.0:
            assert torch.equal(rows, C0 + want0)
        ref = prod + beta * C0.double()
        err = float((rows.double() - ref).abs().max() / ref.abs().max())
        print(f"beta {beta}: max|err| / max|ref| = {err:.3e}")
        assert err < 1e-5, err


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_vector_and_scalar_combine_give_the_same_bits(dev, ta, tb):
    """N % 4 == 0: ldc = N + 4 takes the 16-B path, ldc = N + 3 the scalar one"""
    M, N, K, splitk = 128, 128, 64, 4
    A, B, bias, C0 = _operands(dev, ta, tb, M, N, K, seed=3)
    outs = []
    for pad in (4, 3):
        _, (wide, cols) = _out_views(dev, M, N, C0, pad)
        ops.gemm(A, B, transA=ta, transB=tb, bias=bias, beta=0.5, out=cols, splitk=splitk, reduce="fixed")
        assert (wide[:, N:] == SENTINEL).all()
        outs.append(cols.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("M,N,K,splitk", [(5, 3, 2, 4), (64, 72, 40, 1), (130, 257, 16, 8)])
def test_one_slab_is_the_unsplit_launch(dev, M, N, K, splitk):
    assert _slabs(K, splitk)[1] == 1 and ops.gemm_fixed_ws_bytes(M, N, K, splitk) == 0
    A, B, bias, C0 = _operands(dev, False, True, M, N, K, seed=5)
    A = A * 0.1
    for kw in (dict(), dict(epilogue=ops.EPI_TANH), dict(beta=0.5)):
        a, b = C0.clone(), C0.clone()
        ops.gemm(A, B, transB=True, bias=bias, out=a, splitk=1, **kw)
        ops.gemm(A, B, transB=True, bias=bias, out=b, splitk=splitk, reduce="fixed", **kw)
        assert torch.equal(a, b)
    # bf16 operands are no concern of the fixed split, but one slab passes them through
    a = ops.gemm(A, B, transB=True, precision="bf16")
    assert torch.equal(a, ops.gemm(A, B, transB=True, precision="bf16", splitk=splitk, reduce="fixed"))


def test_five_runs_repeat_bitwise(dev):
    M, N, K, splitk = 100, 25, 1000, 31
    assert 1 < _slabs(K, splitk)[1] < splitk
    A, B, _, C0 = _operands(dev, True, False, M, N, K, seed=9)
    runs = []
    for _ in range(5):
        out = C0.clone()
        ops.gemm(A, B, transA=True, out=out, beta=1.0, splitk=splitk, reduce="fixed")
        runs.append(out)
    assert all(torch.equal(runs[0], r) for r in runs[1:])


@pytest.mark.parametrize("M,N,K,splitk,pad", [(128, 128, 64, 4, 4), (200, 129, 1004, 7, 2)])
def test_beta_zero_does_not_read_out(dev, M, N, K, splitk, pad):
    A, B, bias, _ = _operands(dev, True, False, M, N, K, seed=11)
    wide = torch.full((M, N + pad), SENTINEL, device=dev)
    out = wide[:, :N]
    out.fill_(float("nan"))
    ops.gemm(A, B, transA=True, bias=bias, out=out, splitk=splitk, reduce="fixed")
    assert out.isfinite().all() and (wide[:, N:] == SENTINEL).all()
    assert torch.equal(out, _in_order(A, B, True, False, K, splitk, bias))


def test_auto_splits_whatever_beta_is(dev):
    """splitk="auto" with reduce="fixed": auto_splitk's factor for any beta, out neither zeroed nor beta forced"""
    M, N, K = 100, 25, 2048
    s = ops.auto_splitk(M, N, K)
    assert s > 1
    A, B, _, C0 = _operands(dev, True, False, M, N, K, seed=13)
    for beta in (0.0, 0.5):
        a, b = C0.clone(), C0.clone()
        ops.gemm(A, B, transA=True, out=a, beta=beta, splitk="auto", reduce="fixed")
        ops.gemm(A, B, transA=True, out=b, beta=beta, splitk=s, reduce="fixed")
        assert torch.equal(a, b)
    ref = A.double().T @ B.double() + 0.5 * C0.double()
    assert float((a.double() - ref).abs().max() / ref.abs().max()) < 1e-5


def test_refusals(dev):
    M, N, K, splitk = 130, 257, 129, 3
    A, B, bias, C0 = _operands(dev, False, False, M, N, K, seed=1)
    nb = ops.gemm_fixed_ws_bytes(M, N, K, splitk)
    assert nb == 3 * M * N * 4
    out = C0.clone()
    with pytest.raises(RuntimeError, match="workspace"):
        ops.gemm(A, B, out=out, splitk=splitk, reduce="fixed", ws=torch.empty(nb - 4, device=dev, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="workspace"):
        ops.gemm(A, B, out=out, splitk=splitk, reduce="fixed", ws=torch.empty(nb // 4 - 1, device=dev))
    with pytest.raises(RuntimeError, match="fp32 only"):
        ops.gemm(A, B, out=out, splitk=splitk, reduce="fixed", precision="bf16")
    with pytest.raises(RuntimeError, match="epilogue"):
        ops.gemm(A, B, out=out, splitk=splitk, reduce="fixed", epilogue=ops.EPI_TANH)
    with pytest.raises(ValueError):
        ops.gemm(A, B, out=out, splitk=splitk, reduce="tree")
    # the C entry point refuses the same on its own
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    args = lambda epi, prec, w, wb: (0, 0, M, N, K, _lib.ptr(A, True), A.stride(0), _lib.ptr(B), B.stride(0),
                                     _lib.ptr(out), out.stride(0), None, epi, 0.0, prec, splitk, w, wb,
                                     _lib.stream_ptr())
    for bad in (args(0, 0, _lib.ptr(ws), nb - 1), args(0, 0, None, 0), args(0, 1, _lib.ptr(ws), nb),
                args(1, 0, _lib.ptr(ws), nb)):
        with pytest.raises(RuntimeError, match="dl4ss_gemm_fixed failed"):
            _lib.call("dl4ss_gemm_fixed", *bad)
    assert torch.equal(out, C0)  # nothing was launched
    _lib.call("dl4ss_gemm_fixed", *args(0, 0, _lib.ptr(ws), nb))
    assert torch.equal(out, _in_order(A, B, False, False, K, splitk, None))


def test_implicit_workspace_is_not_grown_inside_a_capture(dev):
    """The per-stream workspace is sized by eager calls; a capture that would have to grow it is refused, one that
    fits replays to the eager bits."""
    M, N, K, splitk = 100, 25, 1000, 31
    A, B, _, _ = _operands(dev, True, False, M, N, K, seed=15)
    out = torch.empty(M, N, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="before graph capture"):
        with torch.cuda.graph(g, stream=side):  # this stream has no workspace yet
            out.zero_()
            ops.gemm(A, B, transA=True, out=out, splitk=splitk, reduce="fixed")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # an eager call on the stream sizes it
        want = ops.gemm(A, B, transA=True, splitk=splitk, reduce="fixed").clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ops.gemm(A, B, transA=True, out=out, splitk=splitk, reduce="fixed")
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
