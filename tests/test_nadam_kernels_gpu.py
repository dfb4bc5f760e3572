"""dl4ss_nadam and dl4ss_adam_clipped_ex against tests/nadam_ref.py (fp64, bars by counted roundings) on the inputs
of small_ref.adam_case: n = 1, 3, 4, 5, 1027 (tails and quads) and once the size that takes a second grid-stride
pass, at steps 1 and 7; unclipped, under Keras's clipnorm (inactive: bitwise the unclipped update; active; at the
threshold; over joint partials), with bf16 shadows, refused, and with bad arguments."""
import functools
import math

import numpy as np
import pytest
import torch

import clip_ref as cr
import nadam_ref as nr
import small_ref as sr
from dl4ss_amd import _lib, adam, ops
from test_clip_kernels_gpu import _same, _segs

pytestmark = pytest.mark.gpu

P = _lib.ptr
HP = (0.002, 0.9, 0.999, 1e-8)
N_LARGE = sr.ADAM_N_LARGE
INF = float("inf")


@functools.lru_cache(maxsize=None)
def _case(n, step):
    """adam_case and the fp64 norm of its gradient.  Shared and read-only."""
    p, g, m, v = sr.adam_case(n, step)
    if n == 1:  # (adam_case zeroes every 7th element: at n = 1 the only one.  One that moves, beside it)
        g, m, v = g + 0.1, m + (0.05 if step > 1 else 0.0), v + (0.01 if step > 1 else 0.0)
    return p, g, m, v, math.sqrt(cr.sumsq(g))


def _run(dev, case, step, gscale=1.0, clipnorm=None, rule=ops.CLIP_KERAS, shadow=None, status0=0, dp=None, g=None,
         part=None, p=None, kind="nadam"):
    """One launch of dl4ss_nadam (kind "adam": ops.adam_ by ``rule``).  part: (buffer, n_part) in place of
    grad_sumsq(g)."""
    p0, g0, m, v, _ = case
    g = g0 if g is None else g
    pd, gd, md, vd = (t.to(dev).clone() for t in (p0 if p is None else p, g, m, v))
    status = torch.tensor([status0, 0], device=dev, dtype=torch.int32)
    loss = torch.full((3,), 0.25, device=dev)
    gnorm = torch.full((2,), -7.0, device=dev)
    nonfinite = torch.zeros(1, device=dev, dtype=torch.int32)
    dp_flag = None if dp is None else torch.tensor([dp], device=dev)
    kw = dict(status=status, loss=loss, dp_flag=dp_flag, gscale=gscale, shadow=shadow)
    if clipnorm is not None:
        buf, n_part = (ops.grad_sumsq(gd), None) if part is None else part
        kw.update(clip=(buf, clipnorm, gnorm, nonfinite), clip_rule=rule, n_part=n_part)
    if kind == "nadam":
        ops.nadam_(pd, gd, md, vd, step, adam.nadam_schedule(step, HP[1]), HP[0], HP[1:3], HP[3], **kw)
    else:
        ops.adam_(pd, gd, md, vd, step, HP[0], HP[1:3], HP[3], **kw)
    torch.cuda.synchronize()
    assert torch.equal(gd.cpu().view(torch.int32), g.view(torch.int32))
    return dict(p=pd.cpu(), m=md.cpu(), v=vd.cpu(), pd=pd, status=status.tolist(), loss=loss.cpu(),
                gnorm=gnorm.cpu(), nonfinite=int(nonfinite.item()))


def _within(got, refs, what):
    for name, (ref, b) in zip("pmv", refs):
        err = (got[name].double() - ref).abs()
        worst = float((err / b.clamp_min(1e-300)).max())
        print(f"  {what} {name}: max err / bar = {worst:.3g}")
        assert bool(torch.isfinite(got[name]).all()), (what, name)
        assert bool((err <= b).all()), (what, name, worst)


# ---- unclipped ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("n", sr.ADAM_N)
def test_unclipped_within_the_counted_bars(dev, n, step):
    case = _case(n, step)
    p, g, m, v, _ = case
    for gscale in (1.0, 0.5):
        got = _run(dev, case, step, gscale)
        _within(got, nr.nadam(p, g, m, v, *HP, step, gscale), f"n={n} step={step} gscale={gscale}")
        assert got["status"] == [0, 0] and float(got["loss"][0]) == 0.25 and got["gnorm"].tolist() == [-7.0, -7.0]
        if n > 1:
            assert not _same(got["p"], p)
            # g = m = v = 0: the parameter keeps its bits
            assert _same(got["p"][::7], p[::7])
            assert float(got["m"][::7].abs().max()) == 0.0 and float(got["v"][::7].abs().max()) == 0.0
    if n > 1:
        assert not _same(_run(dev, case, step, 1.0)["m"], got["m"])  # gscale shows (in m: a first step's p is scale free)


def test_unclipped_second_grid_stride_pass(dev):
    case = _case(N_LARGE, 7)
    p, g, m, v, _ = case
    assert N_LARGE // 4 > 8192 * 256 and N_LARGE % 4 == 1
    got = _run(dev, case, 7)
    _within(got, nr.nadam(p, g, m, v, *HP, 7), f"n={N_LARGE}")
    assert _same(got["p"][::7], p[::7]) and not _same(got["p"][-5:], p[-5:])


def test_parameters_near_zero_show_the_schedule(dev):
    """|p| ~ 1e-6: the bars are the update's own, 7e-5 of which is what mu(t) in place of mu(t + 1) would move
    (test_nadam_ref_cpu.py: such a restatement misses these bars)."""
    case = _case(1027, 7)
    p, g, m, v, _ = case
    p = p * 1e-6
    got = _run(dev, case, 7, p=p)
    refs = nr.nadam(p, g, m, v, *HP, 7)
    _within(got, refs, "p ~ 1e-6")
    (pw, _), _, _ = nr.nadam(p, g, m, v, *HP, 7, mu_next_of=7)
    assert float(((got["p"].double() - pw).abs() > refs[0][1])[m != 0].double().mean()) > 0.9


def test_underflowed_schedule_product_is_accepted(dev):
    """P(t) = 0: what the product of ~0.5s underflows to in double after ~900 updates at beta1 < 0.87 or
    schedule_decay 0 (test_nadam_ref_cpu.py runs the schedule there).  a1 = lr (1 - mu), a2 = lr mu_next: the
    update is within the bars of the reference at the same schedule, clipped and not."""
    n, step = 1027, 1000
    p, g, m, v, nrm = _case(n, 7)
    mu_t, mu_n, P = adam.nadam_schedule(step, 0.8, 0.004, {})
    assert P == 0.0 and 0 < mu_t < 0.5
    hp = (HP[0], 0.8, HP[2], HP[3])
    for clipnorm in (None, cr.f32(0.5 * nrm)):
        pd, gd, md, vd = (t.to(dev).clone() for t in (p, g, m, v))
        gnorm, nf = torch.zeros(2, device=dev), torch.zeros(1, device=dev, dtype=torch.int32)
        clip = None if clipnorm is None else (ops.grad_sumsq(gd), clipnorm, gnorm, nf)
        ops.nadam_(pd, gd, md, vd, step, (mu_t, mu_n, P), hp[0], hp[1:3], hp[3], clip=clip)
        torch.cuda.synchronize()
        f, clipped = 1.0, False
        if clipnorm is not None:
            _, c, f = nr.keras_clip(g, clipnorm)
            f, clipped = cr.f32(f), True
            assert 0.49 < c < 0.51
        refs = nr.nadam(p, g, m, v, *hp, step, f, clipped=clipped, sched=(mu_t, mu_n, P))
        _within(dict(p=pd.cpu(), m=md.cpu(), v=vd.cpu()), refs, f"P = 0, clipnorm {clipnorm}")
        assert not _same(pd.cpu(), p)
        a1, a2, _ = nr.scalars(*hp[:3], step, sched=(mu_t, mu_n, P))
        assert a1 == cr.f32(cr.f32(hp[0]) * (1.0 - mu_t)) and a2 == cr.f32(cr.f32(hp[0]) * mu_n)


# ---- Keras's clipnorm -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("n", sr.ADAM_N)
def test_inactive_clip_is_bitwise_the_unclipped_update(dev, n, step):
    case = _case(n, step)
    for gscale in (1.0, 0.5):
        want = _run(dev, case, step, gscale)
        for clipnorm in (2.0 * gscale * case[4], INF):
            got = _run(dev, case, step, gscale, clipnorm)
            for k in "pmv":
                assert _same(got[k], want[k]), (k, gscale, clipnorm)
            assert float(got["gnorm"][1]) == 1.0
            assert abs(float(got["gnorm"][0]) - gscale * case[4]) <= 2 * cr.U * gscale * case[4]
            assert got["status"] == [0, 0] and got["nonfinite"] == 0 and float(got["loss"][0]) == 0.25


@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("n", sr.ADAM_N)
def test_active_clip_within_the_counted_bars(dev, n, step):
    case = _case(n, step)
    p, g, m, v, nrm0 = case
    for gscale in (1.0, 0.5):
        clipnorm = cr.f32(0.5 * gscale * nrm0)
        *refs, (nrm, c, _) = nr.nadam_clipped(p, g, m, v, *HP, step, clipnorm, gscale)
        assert 0.49 < c < 0.51
        got = _run(dev, case, step, gscale, clipnorm)
        print(f"n={n} step={step} gscale={gscale}: gnorm {got['gnorm'].tolist()} ref {(nrm, c)}")
        assert cr.gnorm_close(got["gnorm"], nrm, c)
        _within(got, refs, "clipped")
        assert (n == 1 or _same(got["p"][::7], p[::7])) and got["status"] == [0, 0] and got["nonfinite"] == 0
        if step == 1:  # the clip shows: the second moment's new term is c^2 of the unclipped one's
            plain = _run(dev, case, step, gscale)
            moved = g != 0
            ratio = got["v"][moved].double() / plain["v"][moved].double()
            assert float((ratio - c * c).abs().max()) <= 16 * cr.U


def test_threshold_takes_the_greater_or_equal_branch(dev):
    """nrm = 5 exactly (g = 3, 4, 0...): clipnorm = 5 gives c = 5 / 5 = 1 by the >= branch where torch's rule gives
    5 / (5 + 1e-6) < 1; the fp32 number below 5 clips (c = clipnorm / nrm < 1, no + 1e-6), the one above does not.
    Then adam_case's own norm: the two fp32 neighbours of the fp64 norm fall on either side of the >=."""
    n, step = 1027, 7
    p, _, m, v, _ = _case(n, step)
    g = torch.zeros(n)
    g[3], g[900] = 3.0, 4.0
    case = (p, g, m, v, 5.0)
    plain = _run(dev, case, step)
    at = _run(dev, case, step, 1.0, 5.0)
    assert at["gnorm"].tolist() == [5.0, 1.0] and all(_same(at[k], plain[k]) for k in "pmv")
    torch_rule = _run(dev, case, step, 1.0, 5.0, rule=ops.CLIP_TORCH)
    assert float(torch_rule["gnorm"][1]) == cr.f32(5.0 / (5.0 + 1e-6)) < 1.0
    below = float(np.nextafter(np.float32(5.0), np.float32(0.0)))
    lo = _run(dev, case, step, 1.0, below)
    assert float(lo["gnorm"][1]) == cr.f32(below / 5.0) < 1.0
    *refs, _ = nr.nadam_clipped(p, g, m, v, *HP, step, below)
    _within(lo, refs, "just below")
    above = float(np.nextafter(np.float32(5.0), np.float32(10.0)))
    hi = _run(dev, case, step, 1.0, above)
    assert float(hi["gnorm"][1]) == 1.0 and all(_same(hi[k], plain[k]) for k in "pmv")
    # a norm that is no fp32 number: two steps below it clips (c rounds below 1), the neighbour above does not
    case = _case(n, step)
    nrm = case[4]
    down = np.nextafter(np.float32(nrm), np.float32(0.0))
    down = float(np.nextafter(down, np.float32(0.0)))
    up = float(np.nextafter(np.float32(nrm), np.float32(INF)))
    assert down < nrm < up and cr.f32(down / nrm) < 1.0
    plain = _run(dev, case, step)
    lo, hi = _run(dev, case, step, 1.0, down), _run(dev, case, step, 1.0, up)
    assert abs(float(lo["gnorm"][1]) - down / nrm) <= 2 * cr.U and float(lo["gnorm"][1]) < 1.0
    assert float(hi["gnorm"][1]) == 1.0 and all(_same(hi[k], plain[k]) for k in "pmv")


def test_joint_partials_give_both_launches_the_same_coefficient(dev):
    """One buffer [parts(g_a) | parts(g_b)], n = 1027 and n = 5: both launches write the same gnorm bits, the
    concatenated gradient's norm and coefficient."""
    step = 7
    a, b = _case(1027, step), _case(5, step)
    na, nb = ops.grad_sumsq_parts(1027), ops.grad_sumsq_parts(5)
    buf = torch.full((na + nb + 1,), float("nan"), device=dev, dtype=torch.float64)
    ops.grad_sumsq(a[1].to(dev), buf[:na])
    ops.grad_sumsq(b[1].to(dev), buf[na:na + nb])
    joint = [a[1], b[1]]
    nrm0 = math.sqrt(cr.sumsq(a[1]) + cr.sumsq(b[1]))
    clipnorm = cr.f32(0.5 * nrm0)
    outs = []
    for case in (a, b):
        p, g, m, v, _ = case
        *refs, (nrm, c, _) = nr.nadam_clipped(p, g, m, v, *HP, step, clipnorm, joint=joint)
        got = _run(dev, case, step, 1.0, clipnorm, part=(buf, na + nb))
        assert cr.gnorm_close(got["gnorm"], nrm, c) and abs(nrm - nrm0) <= 1e-12 * nrm0 and 0.49 < c < 0.51
        _within(got, refs, f"joint n={p.numel()}")
        outs.append(got)
    assert _same(outs[0]["gnorm"], outs[1]["gnorm"])
    alone = _run(dev, b, step, 1.0, clipnorm)  # its own norm is another
    assert not _same(alone["gnorm"], outs[1]["gnorm"])
    assert math.isnan(float(buf[-1]))  # nothing written behind the partials


@pytest.mark.parametrize("rel", [None, 0.5, 2.0])
def test_shadow_copies_are_the_bf16_of_the_new_parameters(dev, rel):
    n, step = 1027, 7
    case = _case(n, step)
    shapes, ys, args = _segs(dev, n, 0)
    clipnorm = None if rel is None else rel * case[4]
    got = _run(dev, case, step, 1.0, clipnorm, shadow=args)
    assert not _same(got["p"], case[0])
    for (off, r, c, ld), y in zip(shapes, ys):
        x = got["pd"][off:off + r * c].view(r, c)
        want = torch.full((r, ld), 0x1234, device=dev, dtype=torch.int16).view(torch.bfloat16)
        _lib.call("dl4ss_f32_to_bf16_2d", P(x), c, r, c, P(want), ld, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert _same(y.cpu(), want.cpu()), off
    # every fused multiply-add is explicit: the shadow-writing instantiation is bitwise the plain one
    plain = _run(dev, case, step, 1.0, clipnorm)
    for k in "pmv":
        assert _same(got[k], plain[k]), k


# ---- refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("how", ["status", "dp_flag"])
def test_refused_update_touches_nothing_and_counts_once(dev, how, clip):
    n, step = 1027, 7
    case = _case(n, step)
    shapes, ys, args = _segs(dev, n, 0x1234)
    kw = dict(status0=1) if how == "status" else dict(dp=1.0)
    got = _run(dev, case, step, 1.0, 0.5 * case[4] if clip else None, shadow=args, **kw)
    for k, ref in zip("pmv", (case[0], case[2], case[3])):
        assert _same(got[k], ref), k
    for y in ys:
        assert bool((y.view(torch.int16) == 0x1234).all())
    assert math.isnan(float(got["loss"][0])) and float(got["loss"][1]) == 0.25
    assert got["status"] == [1 if how == "status" else 0, 1] and got["nonfinite"] == 0
    assert got["gnorm"].tolist() == [-7.0, -7.0]


@pytest.mark.parametrize("bad,where", [(INF, 100), (float("nan"), 1026)])
@pytest.mark.parametrize("sticky", [False, True])
def test_nonfinite_gradient_is_refused_and_counted(dev, bad, where, sticky):
    """An Inf inside a quad, a NaN in the n % 4 tail: nothing changes, loss[0] = NaN, status[1] and the non-finite
    counter go up by one; with the sticky flag bit 2 of status[0] is set, without it status[0] stays 0."""
    n, step = 1027, 7
    case = _case(n, step)
    g = case[1].clone()
    g[where] = bad
    shapes, ys, args = _segs(dev, n, 0x1234)
    pd, gd, md, vd = (t.to(dev).clone() for t in (case[0], g, case[2], case[3]))
    status = torch.zeros(2, device=dev, dtype=torch.int32)
    loss, gnorm = torch.full((3,), 0.25, device=dev), torch.full((2,), -7.0, device=dev)
    nonfinite = torch.zeros(1, device=dev, dtype=torch.int32)
    ops.nadam_(pd, gd, md, vd, step, adam.nadam_schedule(step), *HP[:1], HP[1:3], HP[3], status=status, loss=loss,
               gscale=0.5, shadow=args, clip=(ops.grad_sumsq(gd), 1.0, gnorm, nonfinite),
               n_part=ops.grad_sumsq_parts(n) if sticky else None, sticky=sticky)
    torch.cuda.synchronize()
    for t, ref in zip((pd, md, vd), (case[0], case[2], case[3])):
        assert _same(t.cpu(), ref)
    for y in ys:
        assert bool((y.view(torch.int16) == 0x1234).all())
    assert math.isnan(float(loss[0])) and float(loss[1]) == 0.25
    assert status.tolist() == [ops.STATUS_NONFINITE_GRAD if sticky else 0, 1] and int(nonfinite) == 1
    assert not math.isfinite(float(gnorm[0])) and float(gnorm[1]) == 0.0
    if sticky:  # the bit stays: the next update, of a finite gradient, is refused by it and counts once more
        got = _run(dev, case, step, 1.0, 1.0, status0=ops.STATUS_NONFINITE_GRAD)
        assert _same(got["p"], case[0]) and got["status"] == [ops.STATUS_NONFINITE_GRAD, 1] and got["nonfinite"] == 0


# ---- dl4ss_adam_clipped_ex ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,step,shadow", [(5, 1, False), (1027, 7, False), (1027, 7, True)])
def test_adam_clipped_ex_with_torchs_rule_is_bitwise_adam_clipped(dev, n, step, shadow):
    case = _case(n, step)
    for rel in (0.5, 2.0):
        outs = []
        for n_part in (None, ops.grad_sumsq_parts(n)):  # None: dl4ss_adam_clipped; a number: the _ex entry
            sh = _segs(dev, n, 0) if shadow else None
            part = None if n_part is None else (ops.grad_sumsq(case[1].to(dev)), n_part)
            got = _run(dev, case, step, 0.5, rel * 0.5 * case[4], rule=ops.CLIP_TORCH, shadow=sh and sh[2], part=part,
                       kind="adam")
            outs.append((got, sh))
        (a, sa), (b, sb) = outs
        for k in ("p", "m", "v", "gnorm"):
            assert _same(a[k], b[k]), (k, rel)
        assert not _same(a["p"], case[0]) and (float(a["gnorm"][1]) < 1.0) == (rel < 1.0)
        if shadow:
            for ya, yb in zip(sa[1], sb[1]):
                assert _same(ya.cpu(), yb.cpu())


def test_adam_with_the_keras_rule(dev):
    """dl4ss_adam_clipped_ex, clip_rule 1: Adam's arithmetic (clip_ref.adam_clipped's bars) at Keras's coefficient."""
    n, step = 1027, 7
    case = _case(n, step)
    p, g, m, v, nrm0 = case
    clipnorm = cr.f32(0.5 * nrm0)
    nrm, c, f = nr.keras_clip(g, clipnorm)
    got = _run(dev, case, step, 1.0, clipnorm, kind="adam")
    assert cr.gnorm_close(got["gnorm"], nrm, c)
    f_32 = cr.f32(f)
    (pr, _), (mr, dm), (vr, dv) = sr.adam(p, g, m, v, *HP, step, f_32)
    gs = g.double() * f_32
    dm = dm + 2 * cr.U * gs.abs()
    dv = dv + (4 * cr.U + 4 * cr.U * cr.U) * (1.0 - cr.f32(HP[2])) * gs * gs
    step_sz = cr.f32(HP[0]) / cr.f32(1.0 - cr.f32(HP[1]) ** step)
    denom = vr.sqrt() / cr.f32(np.sqrt(1.0 - cr.f32(HP[2]) ** step)) + cr.f32(HP[3])
    dp = cr.U * pr.abs() + step_sz * dm / denom + 12 * cr.U * (step_sz * mr / denom).abs()
    _within(got, ((pr, dp), (mr, dm), (vr, dv)), "adam, keras rule")
    inactive = _run(dev, case, step, 1.0, 2.0 * nrm0, kind="adam")
    assert float(inactive["gnorm"][1]) == 1.0
    _within(inactive, sr.adam(p, g, m, v, *HP, step), "adam, keras rule, inactive")


# ---- bad arguments --------------------------------------------------------------------------------------------------
def test_bad_arguments_return_invalid_value_before_any_launch(dev):
    n, step = 1027, 7
    case = _case(n, step)
    pd, gd, md, vd = (t.to(dev).clone() for t in case[:4])
    part = torch.zeros(8, device=dev, dtype=torch.float64)
    ops.grad_sumsq(gd, part)
    gn, nf = torch.zeros(2, device=dev), torch.zeros(1, device=dev, dtype=torch.int32)
    status = torch.zeros(2, device=dev, dtype=torch.int32)
    mu, mu_next, mu_prod = adam.nadam_schedule(step)
    good = dict(p=P(pd), g=P(gd), m=P(md), v=P(vd), n=n, lr=HP[0], beta1=HP[1], beta2=HP[2], eps=HP[3], step=step,
                mu=mu, mu_next=mu_next, mu_prod=mu_prod, status=P(status), dp_flag=None, gscale=1.0, loss=None, nseg=0,
                seg_off=None, seg_rows=None, seg_cols=None, seg_y=None, seg_ldy=None, part=P(part), n_part=1,
                clip_rule=1, max_norm=1.0, gnorm=P(gn), nonfinite=P(nf), nonfinite_sticky=0,
                stream=_lib.stream_ptr())
    misaligned = _lib.ctypes.c_void_p(part.data_ptr() + 4)
    bads = [dict(mu=1.0), dict(mu=0.0), dict(mu_next=1.5), dict(mu_prod=-1e-300), dict(mu_prod=1.0), dict(step=0),
            dict(part=misaligned), dict(n_part=0), dict(n_part=4097), dict(clip_rule=2), dict(clip_rule=-1),
            dict(max_norm=0.0), dict(max_norm=float("nan")), dict(nonfinite=None),
            dict(nonfinite_sticky=1, status=None)]
    lib = _lib.lib()
    for bad in bads:
        rc = lib.dl4ss_nadam(*_lib.bind("dl4ss_nadam", (), dict(good, **bad)))
        assert rc == 1, bad  # hipErrorInvalidValue
        with pytest.raises(RuntimeError, match="dl4ss_nadam"):
            _lib.call("dl4ss_nadam", **dict(good, **bad))
    ex = {k: v for k, v in good.items() if k not in ("mu", "mu_next", "mu_prod")}
    for bad in (dict(step=0), dict(part=misaligned), dict(n_part=0), dict(clip_rule=2), dict(max_norm=-1.0)):
        assert lib.dl4ss_adam_clipped_ex(*_lib.bind("dl4ss_adam_clipped_ex", (), dict(ex, **bad))) == 1, bad
    with pytest.raises(ValueError):
        ops.nadam_(pd, gd, md, vd, step, (mu, mu_next, mu_prod), clip=(part.float(), 1.0, gn, nf))
    with pytest.raises(ValueError):
        ops.nadam_(pd, gd, md, vd, step, (mu, mu_next, mu_prod), clip=(part, 0.0, gn, nf))
    torch.cuda.synchronize()
    for t, ref in zip((pd, md, vd), (case[0], case[2], case[3])):  # none of the refused calls launched
        assert _same(t.cpu(), ref)
    assert status.tolist() == [0, 0] and int(nf) == 0
