"""The voiceprint kernels (csrc/voiceprint.hip) on the GPU against tests/voiceprint_ref.py: compaction and shift
bitwise against torch indexing; the masked mean and the speaker memory within the a-priori bars of their fp32
arithmetic.  n = 5, T = 9, F = 23; memory M = 7, E = 50."""
import pytest
import torch

import voiceprint_ref as ref
from dl4ss_amd import ops

pytestmark = pytest.mark.gpu
IDS, LENS, memory_case = ref.IDS, ref.LENS, ref.memory_case
N, T, F = 5, 9, 23


def _feats(lens, seed=1, t=T):
    x = ref.inputs(seed, len(lens), t, F)
    for b, L in enumerate(lens):
        x[b, L:] = 0
    return x


def _i32(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


def _compact_case(dev, x, rule="nonzero", thr=None, lengths=None):
    mask = ref.frame_mask(x, rule, thr, lengths)
    xc_r, len_r, idx_r = ref.compact(x, mask)
    xc, ln, idx = ops.vp_compact(x.to(dev), rule, thr, None if lengths is None else lengths.to(dev))
    assert torch.equal(xc.cpu(), xc_r) and torch.equal(ln.cpu(), len_r) and torch.equal(idx.cpu(), idx_r)
    return xc_r, len_r


def test_compact_prefix_lengths(dev):
    xc, ln = _compact_case(dev, _feats(LENS))
    assert ln.tolist() == LENS


def test_compact_interior_masked_frame(dev):
    x = _feats([9, 4, 0, 1, 8])
    x[0, 3] = 0  # a silent frame inside utterance 0
    x[4, 0] = 0
    xc, ln = _compact_case(dev, x)
    assert ln.tolist() == [8, 4, 0, 1, 7] and torch.equal(xc[0, 3], x[0, 4])


def test_compact_gt_rule(dev):
    x = _feats(LENS, seed=2)  # clamped normals: both signs; a frame is valid when any bin > thr
    x[1, 2] = -x[1, 2].abs()  # no bin above 0.5: masked by 'gt', kept by 'nonzero'
    xc, ln = _compact_case(dev, x, "gt", 0.5)
    assert ln.tolist() == [9, 3, 0, 1, 8]
    _compact_case(dev, x, "nonzero")


def test_compact_caller_lengths(dev):
    x = ref.inputs(3, N, T, F)  # no zero frame: the rule would keep everything
    lengths = torch.tensor([3, 9, 0, 12, -2], dtype=torch.int32)  # clamped to [0, T]
    xc, ln = _compact_case(dev, x, lengths=lengths)
    assert ln.tolist() == [3, 9, 0, 9, 0]


def test_compact_single_frame(dev):
    x = _feats([1, 0, 1], t=1)
    _, ln = _compact_case(dev, x)
    assert ln.tolist() == [1, 0, 1]


@pytest.mark.parametrize("direction", [+1, -1])
@pytest.mark.parametrize("other", [0, 1, 2])
@pytest.mark.parametrize("t", [T, 1])
def test_shift_bitwise(dev, direction, other, t):
    lens = torch.tensor([min(L, t) for L in LENS], dtype=torch.int32)
    src = ref.inputs(5, N, t, 14)
    dst0 = ref.inputs(6, N, t, 14)
    for c0, c1 in ((7, 14), (0, 7), (3, 9), (0, 14), (5, 5)):
        want = ref.shift(src, lens, c0, c1, direction, other, dst0)
        dst = dst0.to(dev)
        ops.vp_shift(src.to(dev), dst, lens.to(dev), c0, c1, direction, other)
        assert torch.equal(dst.cpu(), want), (c0, c1)


def test_shift_round_trip(dev):
    lens = _i32(LENS, dev)
    x = _feats(LENS).to(dev)[:, :, :14].contiguous()
    a, b = torch.empty_like(x), torch.empty_like(x)
    ops.vp_shift(x, a, lens, 7, 14, +1, other=2)
    ops.vp_shift(a, b, lens, 7, 14, -1, other=1)
    assert torch.equal(b, x)


def test_masked_mean_fwd_bwd(dev):
    H = 25
    lens = torch.tensor(LENS, dtype=torch.int32)
    out = ref.inputs(7, N, T, 2 * H)
    val, bar = ref.masked_mean(out, lens)
    vec = ops.vp_mean_fwd(out.to(dev), lens.to(dev)).cpu().double()
    err = (vec - val).abs()
    print("masked mean: max err / bar", (err / bar.clamp_min(1e-300)).max().item())
    assert (err <= bar).all()
    assert (vec[2] == 0).all()  # len 0
    dvec = ref.inputs(8, N, 2 * H)
    dval, dbar = ref.masked_mean_bwd(dvec, lens, T)
    dout = torch.full((N, T, 2 * H), float("nan"), device=dev)
    ops.vp_mean_bwd(dvec.to(dev), lens.to(dev), dout)
    dout = dout.cpu().double()
    assert not dout.isnan().any()  # every element written
    assert ((dout - dval).abs() <= dbar).all()
    assert (dout[dval == 0] == 0).all() and (dout[2] == 0).all()


@pytest.mark.parametrize("M,C", [(1, 3), (45, 200), (64, 200), (65, 257), (1000, 200), (16064, 200)])
def test_colsum_fixed_order(dev, M, C):
    """The bias gradient's column sum: within its bar of fp64, every element written, and the very bits of its
    stated order (blocks of 64 rows, then the blocks) -- for any M, the training step's 16064 rows among them, where
    ops.colsum adds 63 row blocks atomically."""
    A = ref.inputs(9, M, C)
    val, bar = ref.colsum(A)
    out = torch.full((C,), float("nan"), device=dev)
    ops.vp_colsum(A.to(dev), out, ops.vp_colsum_part(M, C, dev))
    err = (out.cpu().double() - val).abs()
    print(f"colsum M={M}: max err / bar", (err / bar).max().item())
    assert (err <= bar).all()
    assert torch.equal(out.cpu(), ref.colsum_f32(A))


def _memory_run(dev, v, ids, mem, dq):
    vd, idd, md, dqd = v.to(dev), ids.to(dev), mem.to(dev), dq.to(dev)
    keep = md.clone()
    q, u = ops.spk_memory_fwd(vd, idd, md)
    dv = ops.spk_memory_bwd(dqd, vd, u, idd, md)
    assert torch.equal(md, keep)  # mem is read, never written
    return q, u, dv


def test_memory_fwd_bwd_within_bars(dev):
    v, ids, mem, dq = memory_case()
    r = ref.memory(v, ids, mem, dq)
    q, u, dv = _memory_run(dev, v, ids, mem, dq)
    for name, got in (("q", q), ("u", u), ("dv", dv)):
        err = (got.cpu().double() - r[name]).abs()
        bar = r["bar_" + name]
        print(f"memory {name}: max err / bar", (err / bar.clamp_min(1e-300)).max().item())
        assert (err <= bar).all(), name
    assert (q[3] == 0).all() and (dv[3] == 0).all()  # id -1
    assert (u[2] == 0).all()  # the all-zero voiceprint adds nothing ...
    ids2 = ids.clone()
    ids2[2] = -1
    q2, _, _ = _memory_run(dev, v, ids2, mem, dq)
    assert torch.equal(q2[0], q[0])  # ... bit for bit
    qb, ub, dvb = _memory_run(dev, v, ids, mem, dq)
    assert torch.equal(qb, q) and torch.equal(ub, u) and torch.equal(dvb, dv)  # two runs


def test_memory_store_then_forward(dev):
    v, ids, mem, dq = memory_case()
    q, _, _ = _memory_run(dev, v, ids, mem, dq)
    md, idd = mem.to(dev), ids.to(dev)
    ops.spk_memory_store(q, idd, md)
    got = md.cpu()
    for r in range(7):
        rows = [i for i, id_ in enumerate(IDS) if id_ == r]
        assert torch.equal(got[r], q[rows[0]].cpu() if rows else mem[r])
    q2, _ = ops.spk_memory_fwd(torch.zeros_like(v).to(dev), idd, md)
    want = ref.memory(torch.zeros_like(v), ids, got)
    assert ((q2.cpu().double() - want["q"]).abs() <= want["bar_q"]).all()
    for i, id_ in enumerate(IDS):  # the stored rows re-normalised
        w = got[id_].double() / got[id_].double().norm() if id_ >= 0 else torch.zeros(50, dtype=torch.float64)
        assert (q2[i].cpu().double() - w).abs().max() < 1e-6
    # a refused step (status[0] != 0) stores nothing
    md2 = mem.to(dev)
    ops.spk_memory_store(q, idd, md2, status=_i32([1, 0], dev))
    assert torch.equal(md2.cpu(), mem)
    ops.spk_memory_store(q, idd, md2, status=_i32([0, 3], dev))
    assert torch.equal(md2, md)


def test_argument_validation(dev):
    x = torch.zeros(2, 3, 4, device=dev)
    with pytest.raises(ValueError):
        ops.vp_compact(x, "other")
    with pytest.raises(ValueError):
        ops.vp_compact(x, "gt")
    with pytest.raises(RuntimeError):
        ops.vp_shift(x, x, _i32([1, 2], dev), 0, 2, +1)  # in place
    with pytest.raises(RuntimeError):
        ops.vp_shift(x, torch.empty_like(x), _i32([1, 2], dev), 2, 6, +1)  # columns past ld
    with pytest.raises(RuntimeError):
        ops.spk_memory_fwd(torch.zeros(2, 200, device=dev), _i32([0, 1], dev), torch.zeros(3, 200, device=dev))
