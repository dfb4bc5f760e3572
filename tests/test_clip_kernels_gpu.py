"""dl4ss_grad_sumsq and dl4ss_adam_clipped against tests/clip_ref.py (fp64, bars by counted roundings), on the
inputs of small_ref.adam_case: the sum at n = 1, 3, 4, 5, 1027 and at the size whose 1024 ranges each take
several passes of the block and leave a tail of one element; the clipped Adam inactive (bitwise the unclipped
entry), active (within the bars), with bf16 shadow copies, and refusing a gradient with an Inf or a NaN."""
import ctypes
import functools
import math

import pytest
import torch

import clip_ref as cr
import small_ref as sr
from dl4ss_amd import _lib, ops

pytestmark = pytest.mark.gpu

P = _lib.ptr
HP = (2e-4, 0.9, 0.999, 1e-8)
# 1024 ranges of 2049 quads (256 threads: two unrolled passes of 1024 quads and one more quad), the last range
# shorter, and one tail element -- also the second grid-stride pass of adam_kernel
N_LARGE = sr.ADAM_N_LARGE
INF = float("inf")


@functools.lru_cache(maxsize=None)
def _case(n, step):
    """adam_case; at N_LARGE the last 5 elements of g scaled by 1e3, so that they (and the tail element alone)
    carry about a third of the sum of squares.  Shared and read-only."""
    p, g, m, v = sr.adam_case(n, step)
    if n == N_LARGE:
        g[-5:] *= 1e3
        assert n % 4 == 1 and float(g[-1]) != 0.0
        s_all, s_head = cr.sumsq(g), cr.sumsq(g[:-5])
        assert 0.2 < (s_all - s_head) / s_all < 0.5
        assert ops.grad_sumsq_parts(n) == 1024 and (n // 4 + 1023) // 1024 > 2 * 1024
    return p, g, m, v, math.sqrt(cr.sumsq(g))


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- the sum --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sr.ADAM_N + [N_LARGE])
def test_sumsq_matches_fp64_norm_and_repeats_bitwise(dev, n):
    if n == N_LARGE:
        _, g, _, _, nrm = _case(n, 7)
    else:  # (adam_case zeroes every 7th element, at n = 1 the only one)
        g = sr.inputs(40 + n, n, scale=0.1)
        nrm = math.sqrt(cr.sumsq(g))
    gd = g.to(dev)
    n_part = ops.grad_sumsq_parts(n)
    part = torch.full((n_part + 2,), float("nan"), device=dev, dtype=torch.float64)
    out = ops.grad_sumsq(gd, part)
    assert out is part
    torch.cuda.synchronize()
    got = part.cpu()
    assert bool(torch.isnan(got[n_part:]).all())  # nothing written behind the partials
    assert bool(torch.isfinite(got[:n_part]).all()) and bool((got[:n_part] >= 0).all())
    val = math.sqrt(float(got[:n_part].sum()))
    print(f"n={n}: {n_part} partials, sqrt(sum) / fp64 norm - 1 = {val / nrm - 1:.3g}")
    assert abs(val - nrm) <= 2 * cr.U * nrm
    again = ops.grad_sumsq(gd)
    assert again.numel() == n_part and torch.equal(again.view(torch.int64).cpu(), got[:n_part].view(torch.int64))
    assert torch.equal(gd.cpu(), g)


def test_sumsq_ranges_are_contiguous_and_fixed(dev):
    """n = 3 * 4096 + 7: four ranges of 769 quads (the last one 766 quads and the tail of 3): each partial is
    the fp64 sum over exactly its range."""
    n = 3 * 4096 + 7
    g = sr.inputs(5, n, scale=0.1)
    assert ops.grad_sumsq_parts(n) == 4
    part = ops.grad_sumsq(g.to(dev)).cpu()
    per = 4 * (((n // 4) + 3) // 4)
    for j in range(4):
        ref = cr.sumsq(g[j * per:min(n, (j + 1) * per)])
        assert abs(float(part[j]) - ref) <= 1e-12 * ref, j


def test_sumsq_refuses_a_misaligned_gradient(dev):
    g = torch.zeros(1032, device=dev)
    part = torch.zeros(4, device=dev, dtype=torch.float64)
    for off in (1, 2, 3):
        rc = _lib.lib().dl4ss_grad_sumsq(P(g[off:]), 1027, P(part), _lib.stream_ptr())
        assert rc == 1, rc  # hipErrorInvalidValue, before any launch
    with pytest.raises(RuntimeError, match="dl4ss_grad_sumsq"):
        ops.grad_sumsq(g[1:1028])
    with pytest.raises(ValueError):
        ops.grad_sumsq(g, torch.zeros(1, device=dev))  # not float64


# ---- the clipped Adam -----------------------------------------------------------------------------------------------
def _segs(dev, n, fill):
    """Two shadow segments of a flat buffer of n >= 1027 elements: 10 x 33 at offset 4 (odd rows: element by
    element) and 5 x 64 at offset 400 (whole quads), bf16 rows padded to 40 and 64."""
    shapes = [(4, 10, 33, 40), (400, 5, 64, 64)]
    ys = [torch.full((r, ld), fill, device=dev, dtype=torch.int16).view(torch.bfloat16) for _, r, _, ld in shapes]
    k = len(shapes)
    args = (k, (ctypes.c_longlong * k)(*[s[0] for s in shapes]), (ctypes.c_int * k)(*[s[1] for s in shapes]),
            (ctypes.c_int * k)(*[s[2] for s in shapes]), (ctypes.c_void_p * k)(*[y.data_ptr() for y in ys]),
            (ctypes.c_longlong * k)(*[s[3] for s in shapes]))
    return shapes, ys, args


def _run(dev, case, step, gscale, max_norm, shadow=None, status0=0, g=None):
    """max_norm None: dl4ss_adam_guarded_dp_scaled; else grad_sumsq + the clipped adam_."""
    p, g0, m, v, _ = case
    g = g0 if g is None else g
    pd, gd, md, vd = (t.to(dev).clone() for t in (p, g, m, v))
    status = torch.tensor([status0, 0], device=dev, dtype=torch.int32)
    loss = torch.full((3,), 0.25, device=dev)
    gnorm = torch.full((2,), -7.0, device=dev)
    nonfinite = torch.zeros(1, device=dev, dtype=torch.int32)
    if max_norm is None:
        _lib.call("dl4ss_adam_guarded_dp_scaled", P(pd), P(gd), P(md), P(vd), p.numel(), *HP, step, P(status), None,
                  gscale, P(loss), _lib.stream_ptr())
    else:
        part = ops.grad_sumsq(gd)
        ops.adam_(pd, gd, md, vd, step, *HP[:1], HP[1:3], HP[3], status=status, loss=loss, gscale=gscale,
                  shadow=shadow, clip=(part, max_norm, gnorm, nonfinite))
    torch.cuda.synchronize()
    assert torch.equal(gd.cpu().view(torch.int32), g.view(torch.int32))
    return dict(p=pd.cpu(), m=md.cpu(), v=vd.cpu(), pd=pd, status=status.tolist(), loss=loss.cpu(),
                gnorm=gnorm.cpu(), nonfinite=int(nonfinite.item()))


@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("n", [5, 1027, N_LARGE])
def test_inactive_clip_is_bitwise_the_unclipped_update(dev, n, step):
    """max_norm = 2 x the norm, and inf: c == 1, f is bitwise gscale."""
    case = _case(n, step)
    for gscale in (1.0, 0.5):
        want = _run(dev, case, step, gscale, None)
        for max_norm in (2.0 * gscale * case[4], INF):
            got = _run(dev, case, step, gscale, max_norm)
            for k in "pmv":
                assert _same(got[k], want[k]), (k, gscale, max_norm)
            assert float(got["gnorm"][1]) == 1.0
            assert abs(float(got["gnorm"][0]) - gscale * case[4]) <= 2 * cr.U * gscale * case[4]
            assert got["status"] == [0, 0] and got["nonfinite"] == 0 and float(got["loss"][0]) == 0.25
        assert not _same(want["p"], case[0])


@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("n", [5, 1027, N_LARGE])
def test_active_clip_within_the_counted_bars(dev, n, step):
    """max_norm = 0.5 x the norm at gscale 1 and 0.5."""
    case = _case(n, step)
    p, g, m, v, nrm0 = case
    for gscale in ((1.0, 0.5) if n != N_LARGE else (0.5,)):
        max_norm = cr.f32(0.5 * gscale * nrm0)
        (pr, dp), (mr, dm), (vr, dv), (nrm, c, _) = cr.adam_clipped(p, g, m, v, *HP, step, max_norm, gscale)
        assert 0.49 < c < 0.51
        got = _run(dev, case, step, gscale, max_norm)
        print(f"n={n} step={step} gscale={gscale}: gnorm {got['gnorm'].tolist()} ref {(nrm, c)}")
        assert cr.gnorm_close(got["gnorm"], nrm, c)
        for name, ref, b in (("p", pr, dp), ("m", mr, dm), ("v", vr, dv)):
            err = (got[name].double() - ref).abs()
            worst = float((err / b.clamp_min(1e-300)).max())
            print(f"  {name}: max err / bar = {worst:.3g}")
            assert bool(torch.isfinite(got[name]).all())
            assert bool((err <= b).all()), (name, worst)
        # g = m = v = 0: the parameter keeps its bits
        assert _same(got["p"][::7], p[::7])
        assert float(got["m"][::7].abs().max()) == 0.0 and float(got["v"][::7].abs().max()) == 0.0
        # and the clip shows: against the unclipped update the second moment's new term is c^2 of it
        plain = _run(dev, case, step, gscale, None)
        if step == 1:
            moved = g != 0
            ratio = got["v"][moved].double() / plain["v"][moved].double()
            assert float((ratio - c * c).abs().max()) <= 16 * cr.U
        assert got["status"] == [0, 0] and got["nonfinite"] == 0


@pytest.mark.parametrize("rel", [0.5, 2.0])
def test_shadow_copies_are_the_bf16_of_the_new_parameters(dev, rel):
    n, step = 1027, 7
    case = _case(n, step)
    shapes, ys, args = _segs(dev, n, 0)
    got = _run(dev, case, step, 1.0, rel * case[4], shadow=args)
    assert not _same(got["p"], case[0])
    for (off, r, c, ld), y in zip(shapes, ys):
        x = got["pd"][off:off + r * c].view(r, c)
        want = torch.full((r, ld), 0x1234, device=dev, dtype=torch.int16).view(torch.bfloat16)
        _lib.call("dl4ss_f32_to_bf16_2d", P(x), c, r, c, P(want), ld, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert _same(y.cpu(), want.cpu()), off  # (padding columns: zero in both, Adam leaves them alone)
    # the shadow-writing instantiation's update itself: within the bars (the compiler contracts its
    # multiply-adds differently from the plain instantiation's, so the two are not compared bit for bit)
    p, g, m, v, _ = case
    (pr, dp), (mr, dm), (vr, dv), (nrm, c, _) = cr.adam_clipped(p, g, m, v, *HP, step, rel * case[4])
    assert (c < 1.0) == (rel < 1.0) and cr.gnorm_close(got["gnorm"], nrm, c)
    for name, ref, b in (("p", pr, dp), ("m", mr, dm), ("v", vr, dv)):
        assert bool(((got[name].double() - ref).abs() <= b).all()), name


@pytest.mark.parametrize("bad,where", [(INF, 100), (-INF, 3), (float("nan"), 100), (float("nan"), 1026)])
@pytest.mark.parametrize("max_norm", [1.0, INF])
def test_nonfinite_gradient_is_refused_and_counted(dev, bad, where, max_norm):
    """One Inf, then one NaN, inside a quad and in the n % 4 tail: nothing changes, loss[0] = NaN, status[1] and
    the non-finite counter go up by one."""
    n, step = 1027, 7
    case = _case(n, step)
    g = case[1].clone()
    g[where] = bad
    shapes, ys, args = _segs(dev, n, 0x1234)
    got = _run(dev, case, step, 0.5, max_norm, shadow=args, g=g)
    for k, ref in zip("pmv", (case[0], case[2], case[3])):
        assert _same(got[k], ref), k
    for y in ys:
        assert bool((y.view(torch.int16) == 0x1234).all())
    assert math.isnan(float(got["loss"][0])) and float(got["loss"][1]) == 0.25
    assert got["status"] == [0, 1] and got["nonfinite"] == 1
    assert not math.isfinite(float(got["gnorm"][0])) and float(got["gnorm"][1]) == 0.0


def test_hand_off_time_out_takes_precedence(dev):
    """status[0] set: refused as the unclipped entry refuses, the non-finite counter and gnorm untouched --
    also when the gradient holds a NaN."""
    n, step = 1027, 7
    case = _case(n, step)
    g = case[1].clone()
    g[5] = float("nan")
    for gg in (None, g):
        shapes, ys, args = _segs(dev, n, 0x1234)
        got = _run(dev, case, step, 1.0, 0.5 * case[4], shadow=args, status0=1, g=gg)
        for k, ref in zip("pmv", (case[0], case[2], case[3])):
            assert _same(got[k], ref), k
        for y in ys:
            assert bool((y.view(torch.int16) == 0x1234).all())
        assert math.isnan(float(got["loss"][0]))
        assert got["status"] == [1, 1] and got["nonfinite"] == 0
        assert got["gnorm"].tolist() == [-7.0, -7.0]


def test_clip_none_is_the_unclipped_entry_and_bad_arguments_raise(dev):
    case = _case(1027, 7)
    p, g, m, v, nrm = case
    want = _run(dev, case, 7, 0.5, None)
    pd, gd, md, vd = (t.to(dev).clone() for t in (p, g, m, v))
    # part NULL: dl4ss_adam_guarded_dp_scaled_bf16 itself
    _lib.call("dl4ss_adam_clipped", P(pd), P(gd), P(md), P(vd), 1027, *HP, 7, None, None, 0.5, None, 0, None, None,
              None, None, None, None, 0, 0.0, None, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    for k, t in zip("pmv", (pd, md, vd)):
        assert _same(t.cpu(), want[k])
    part = ops.grad_sumsq(gd)
    nf = torch.zeros(1, device=dev, dtype=torch.int32)
    gn = torch.zeros(2, device=dev)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ops.adam_(pd, gd, md, vd, 8, clip=(part, bad, gn, nf))
        rc = _lib.lib().dl4ss_adam_clipped(P(pd), P(gd), P(md), P(vd), 1027, *HP, 8, None, None, 1.0, None, 0, None,
                                           None, None, None, None, P(part), 1, bad, P(gn), P(nf), _lib.stream_ptr())
        assert rc == 1
    with pytest.raises(ValueError):
        ops.adam_(pd, gd, md, vd, 8, clip=(part.float(), 1.0, gn, nf))
    torch.cuda.synchronize()
    for k, t in zip("pmv", (pd, md, vd)):  # none of the refused calls launched
        assert _same(t.cpu(), want[k])
