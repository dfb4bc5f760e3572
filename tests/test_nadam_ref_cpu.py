"""Nadam and Keras's clipnorm without a GPU: tests/nadam_ref.py against torch.optim.NAdam and against its own
wrong variants, adam.nadam_schedule, the Keras rule, what the trainers and GuardedAdam refuse (before any device
call), the third header's binding, the call sites' argument slots and check()'s arithmetic for the sticky bit."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import nadam_ref as nr
import small_ref as sr
from dl4ss_amd import _lib, adam, classifier, engine, infer, ops, plan
from dl4ss_amd.compat import optim as compat_optim
from dl4ss_amd.imagequery import ImageQueryNet
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintNet
from test_lib_bind_cpu import FakeLib, Stand, fake, tag  # noqa: F401 (fake: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = (0.002, 0.9, 0.999, 1e-8)
P, I, LL, F, D = _lib.P, _lib.I, _lib.LL, _lib.F, ctypes.c_double


# ---- the restatement ------------------------------------------------------------------------------------------------
def test_restatement_against_torch_nadam_over_50_steps():
    """torch.optim.NAdam(momentum_decay=0.004) is Keras 1's Nadam.  nr.nadam itself -- the reference every GPU bar
    is measured against, with nr.scalars' fp32-rounded a1, a2, bc2s -- is stepped 50 times beside it on fp64
    tensors: torch keeps mu_product in an fp32 tensor and nr.nadam rounds its three scalars to fp32, so 1e-6 of
    the largest accumulated move is allowed.  The same formulas written out with unrounded scalars agree with
    torch to 1e-9 of it."""
    n = 1027
    p0 = sr.inputs(3, n).double()
    tp = p0.clone().requires_grad_(True)
    opt = torch.optim.NAdam([tp], lr=HP[0], betas=HP[1:3], eps=HP[3], momentum_decay=0.004)
    z = torch.zeros(n, dtype=torch.float64)
    pr, mr, vr = p0.clone(), z.clone(), z.clone()  # nr.nadam's state
    p, m, v = p0.clone(), z.clone(), z.clone()  # the formulas in double throughout
    for t in range(1, 51):
        g = sr.inputs(100 + t, n, scale=0.1).double()
        tp.grad = g.clone()
        opt.step()
        (pr, _), (mr, _), (vr, _) = nr.nadam(pr, g, mr, vr, *HP, t)
        mu_t, mu_n, P_t = nr.schedule(t, HP[1])
        m = HP[1] * m + (1 - HP[1]) * g
        v = HP[2] * v + (1 - HP[2]) * g * g
        den = (v / (1 - HP[2] ** t)).sqrt() + HP[3]
        p = p - HP[0] * ((1 - mu_t) / (1 - P_t) * g + mu_n / (1 - P_t * mu_n) * m) / den
    move = float((p - p0).abs().max())
    err_ref = float((tp.detach() - pr).abs().max())
    err = float((tp.detach() - p).abs().max())
    print(f"largest move {move:.3g}; torch - nr.nadam {err_ref:.3g}, torch - unrounded formulas {err:.3g}")
    assert move > 1e-2 and err_ref <= 1e-6 * move and err <= 1e-9 * move


def test_the_kernels_fp32_sequence_emulated_on_the_cpu_sits_inside_the_bars():
    """nr.nadam (fp32 scalars, as the launcher rounds them) at t = 7 against the kernel's own sequence of fp32
    operations, each emulated in fp64 and rounded once."""
    n, t = 1027, 7
    p, g, m, v = sr.adam_case(n, t)
    (pr, dp), (mr, dm), (vr, dv) = nr.nadam(p, g, m, v, *HP, t)
    pe, me, ve = nr.emulate_f32(p, g, m, v, *HP, t)
    for name, got, ref, b in (("p", pe, pr, dp), ("m", me, mr, dm), ("v", ve, vr, dv)):
        worst = float(((got - ref).abs() / b.clamp_min(1e-300)).max())
        print(f"{name}: fp32 emulation, max err / bar = {worst:.3g}")
        assert bool(((got - ref).abs() <= b).all()), name
        assert worst > 0.02, name  # the bars are not vacuous: the emulation uses a fair part of them
    assert torch.equal(pe[::7], p[::7].double())  # g = m = v = 0: the parameter keeps its bits


@pytest.mark.parametrize("wrong", ["drop_a2", "mu_next"])
def test_a_wrong_restatement_misses_the_bars(wrong):
    n, t = 1027, 7
    p, g, m, v = sr.adam_case(n, t)
    (pr, dp), _, _ = nr.nadam(p, g, m, v, *HP, t)
    if wrong == "drop_a2":  # one element's a2 m' term left out
        (pw, _), _, _ = nr.nadam(p, g, m, v, *HP, t, drop_a2=5)
        bad = (pw - pr).abs() > dp
        assert bool(bad[5]) and int(bad.sum()) == 1
        assert float((pw - pr).abs()[5] / dp[5]) > 100
    else:  # mu(t) used for mu(t + 1): 7e-5 of the update, below u |p| at |p| ~ 1 -- seen with the parameters near
        # zero, where the bars are the update's own (the GPU tests run that case too)
        p = p * 1e-6
        (pr, dp), _, _ = nr.nadam(p, g, m, v, *HP, t)
        (pw, _), _, _ = nr.nadam(p, g, m, v, *HP, t, mu_next_of=t)
        moved = m != 0
        miss = ((pw - pr).abs() > dp)[moved]
        print(f"mu(t) for mu(t+1): {int(miss.sum())} of {int(moved.sum())} elements outside the bars")
        assert float(miss.double().mean()) > 0.9
        pe, _, _ = nr.emulate_f32(p, g, m, v, *HP, t)  # and the right sequence in fp32 stays inside them
        assert bool(((pe - pr).abs() <= dp).all())


# ---- the schedule ---------------------------------------------------------------------------------------------------
def test_schedule_against_a_from_scratch_product():
    for t in (1, 2, 7, 1000):
        assert adam.nadam_schedule(t) == nr.schedule(t), t
        assert adam.nadam_schedule(t, 0.8, 0.01) == nr.schedule(t, 0.8, 0.01), t
    m1 = 0.9 * (1 - 0.5 * 0.96 ** 0.004)
    assert adam.nadam_schedule(1) == (m1, 0.9 * (1 - 0.5 * 0.96 ** 0.008), m1)
    with pytest.raises(ValueError):
        adam.nadam_schedule(0)


def test_schedule_going_back_and_advancing_give_the_same_bits():
    adam._SCHEDULE.clear()
    assert adam.nadam_schedule(7) == nr.schedule(7)
    assert adam.nadam_schedule(5) == nr.schedule(5)  # back (settle() after a refusal): recomputed from 1
    assert adam._SCHEDULE[(0.9, 0.004)][0] == 5
    adam._SCHEDULE.clear()
    for t in range(1, 301):  # one factor per step
        got = adam.nadam_schedule(t)
        assert adam._SCHEDULE[(0.9, 0.004)][0] == t
    assert got == nr.schedule(300)
    adam._SCHEDULE.clear()
    assert adam.nadam_schedule(300) == got  # from scratch: the same bits
    assert all(0 < x < 1 for x in got)
    assert adam.nadam_schedule(3, 0.9, 0.0)[0] == 0.45  # no decay: mu = beta1 / 2 throughout


def test_schedule_past_the_products_underflow():
    """P(t) is a product of factors near 0.5: with mu below 0.5 (beta1 < ~0.87, or schedule_decay 0) it reaches
    exactly 0.0 in double after ~900 updates; the default stays at the smallest denormal.  Either way the
    launcher's scalars stay finite and go to their limits a1 = lr (1 - mu), a2 = lr mu_next, and dl4ss_nadam
    accepts the schedule (0 <= mu_prod < 1: tests/sanitize/optim_abi_check.cpp, test_nadam_kernels_gpu.py)."""
    for b1, d, zero in ((0.8, 0.004, True), (0.85, 0.004, True), (0.5, 0.004, True), (0.9, 0.0, True),
                        (0.9, 0.004, False)):
        cache, first_zero = {}, None
        for t in range(1, 1301):
            mu_t, mu_n, P = adam.nadam_schedule(t, b1, d, cache)
            assert 0.0 < mu_t < 1.0 and 0.0 < mu_n < 1.0 and 0.0 <= P < 1.0, (b1, d, t)
            if P == 0.0 and first_zero is None:
                first_zero = t
            if t in (1, 500, 850, 1000, 1300) or t == first_zero:
                a1, a2, bc2s = nr.scalars(HP[0], b1, HP[2], t, d, sched=(mu_t, mu_n, P))
                assert all(math.isfinite(x) and x > 0.0 for x in (a1, a2, bc2s)), (b1, d, t)
                if t >= 500:  # 1 - P is 1 in double long before the underflow
                    lr = nr.f32(HP[0])
                    assert (a1, a2) == (nr.f32(lr * (1.0 - mu_t)), nr.f32(lr * mu_n)), (b1, d, t)
        print(f"beta1 {b1} decay {d}: P first 0.0 at step {first_zero}, P(1300) = {P!r}")
        assert (first_zero is not None) == zero and (not zero or 500 < first_zero < 1100)
        assert adam.nadam_schedule(1300, b1, d, {}) == (mu_t, mu_n, P) == nr.schedule(1300, b1, d)


def test_every_optimizer_keeps_its_own_schedule_cache():
    """Two optimizers with the same hyper-parameters at different counts, stepped alternately: neither sends the
    other's cache back to 1 (on one shared cache the trailing one would recompute from 1 on every call)."""
    flat, status, loss = torch.zeros(8), torch.zeros(2, dtype=torch.int32), torch.zeros(3)
    a = adam.GuardedAdam(flat, status, loss, 1e-3, kind="nadam")
    b = adam.GuardedAdam(flat, status, loss, 1e-3, kind="nadam")
    assert a._schedule is not b._schedule and a._schedule == {} and a._schedule is not adam._SCHEDULE
    adam._SCHEDULE.clear()
    for t in range(1, 41):
        adam.nadam_schedule(t + 100, 0.9, 0.004, a._schedule)
        adam.nadam_schedule(t, 0.9, 0.004, b._schedule)
        assert a._schedule[(0.9, 0.004)][0] == t + 100 and b._schedule[(0.9, 0.004)][0] == t
    assert adam._SCHEDULE == {}
    assert adam.nadam_schedule(140, 0.9, 0.004, a._schedule) == nr.schedule(140)
    c = compat_optim.Nadam([torch.nn.Parameter(torch.zeros(3))])
    assert c._schedule == {} and c._schedule is not adam._SCHEDULE


# ---- the Keras rule -------------------------------------------------------------------------------------------------
def test_keras_rule():
    g = torch.tensor([3.0, 4.0, 0.0])
    nrm, c, f = nr.keras_clip(g, 6.0)
    assert (nrm, c, f) == (5.0, 1.0, 1.0)  # nrm < clipnorm: exactly 1
    nrm, c, _ = nr.keras_clip(g, 5.0)  # at the threshold: the >= branch, clipnorm / nrm (torch's rule: 5 / (5 + 1e-6))
    assert c == 5.0 / 5.0 and min(1.0, 5.0 / (5.0 + 1e-6)) < 1.0
    nrm, c, f = nr.keras_clip(g, 2.5, gscale=0.5)  # nrm = 2.5: at the threshold again, through gscale
    assert (nrm, c, f) == (2.5, 1.0, 0.5)
    nrm, c, f = nr.keras_clip(g, 2.0)
    assert c == 2.0 / 5.0 and f == c
    below = float(np.nextafter(np.float32(5.0), np.float32(0.0)))
    assert nr.keras_clip(g, below)[1] == below / 5.0 < 1.0
    assert nr.keras_clip(torch.zeros(4), 1.0)[:2] == (0.0, 1.0)  # nrm == 0: 1, no division
    assert nr.keras_clip(g, float("inf"))[1] == 1.0
    joint = nr.keras_clip([g, torch.tensor([12.0])], 1.0)  # the joint norm: sqrt(25 + 144)
    assert joint[0] == 13.0 and joint[1] == 1.0 / 13.0


# ---- refusals -------------------------------------------------------------------------------------------------------
def _net(**kw):
    kw.setdefault("adjust", False)
    return engine.SepNet(cell="gru", num_layers=1, device="cpu", seed=1, **kw)


def _mem():
    return SpeakerMemory(101, 50, device="cpu")


BAD = [(dict(optimizer="sgd"), "optimizer 'sgd'"), (dict(optimizer="Nadam"), "optimizer 'Nadam'"),
       (dict(clipnorm=0.0), "clipnorm must be positive"), (dict(clipnorm=-1.0), "clipnorm must be positive"),
       (dict(clipnorm=float("nan")), "clipnorm must be positive"),
       (dict(clipnorm=1.0, clip_norm=1.0), "given together"),
       (dict(schedule_decay=-0.1), "schedule_decay"), (dict(schedule_decay=float("nan")), "schedule_decay")]


@pytest.mark.parametrize("kw,reason", BAD)
def test_trainers_refuse_before_any_device_call(monkeypatch, kw, reason):
    net = _net()
    cnet = infer.ClassifierNet(hidden=40, num_layers=2, num_labels=11, device="cpu")
    monkeypatch.setattr(_lib, "_load", lambda: pytest.fail("the library was touched"))
    with pytest.raises(ValueError, match=reason):
        engine.SepTrainer(net, 2, 2, 4000, **kw)
    with pytest.raises(ValueError, match=reason):
        classifier.ClassifierTrainer(cnet, 3, 2, 3000, **kw)
    with pytest.raises(ValueError, match=reason):
        plan.check_args(net, 2, 2, 4000, "label", "fp32", None, None, None, None, kw.get("clip_norm"), None, None, None,
                        "reference", **{k: v for k, v in kw.items() if k != "clip_norm"})
    flat = torch.zeros(8)
    gkw = {("kind" if k == "optimizer" else k): v for k, v in kw.items()}
    if "clipnorm" in kw and "clip_norm" not in kw:
        return  # (GuardedAdam takes the threshold its trainer has checked)
    with pytest.raises(ValueError):
        adam.GuardedAdam(flat, torch.zeros(2, dtype=torch.int32), torch.zeros(3), 1e-3, **gkw)


def test_query_encoders_take_clipnorm_and_still_refuse_clip_norm():
    for kw in (dict(voiceprint=VoiceprintNet(device="cpu")), dict(image_query=ImageQueryNet(device="cpu", seed=2))):
        name = next(iter(kw))
        with pytest.raises(ValueError, match=f"{name}: clip_norm is unsupported"):
            engine.SepTrainer(_net(), 2, 2, 4000, memory=_mem(), clip_norm=200.0, **kw)
        tr = engine.SepTrainer(_net(), 2, 2, 4000, memory=_mem(), clipnorm=200.0, optimizer="nadam", **kw)
        n0, n1 = (ops.grad_sumsq_parts(x.flat.numel()) for x in (tr.net, tr.vp.net))
        assert tr.opt.joint and tr.vp.opt.joint and tr.opt.part_all is tr.vp.opt.part_all
        assert tr.opt.part_all.numel() == n0 + n1 and tr.opt.part_all.dtype == torch.float64
        assert tr.opt.part.data_ptr() == tr.opt.part_all.data_ptr() and tr.opt.part.numel() == n0
        assert tr.vp.opt.part.data_ptr() == tr.opt.part_all[n0:].data_ptr() and tr.vp.opt.part.numel() == n1
        assert tr.opt.kind == tr.vp.opt.kind == "nadam" and tr.vp.opt.clipnorm == tr.opt.clipnorm == 200.0
        assert tr.grad_norm is tr.opt.grad_norm and tr.vp.opt.grad_norm is not tr.opt.grad_norm
        plain = engine.SepTrainer(_net(), 2, 2, 4000, memory=_mem(), **kw)
        assert plain.opt.kind == plain.vp.opt.kind == "adam" and not plain.opt.joint and plain.opt.clip is None
    adv = engine.SepTrainer(engine.SepNet(cell="lstm", num_layers=1, hidden=40, device="cpu"), 2, 2, 2048,
                            adversary=engine.DiscNet(17, 129, device="cpu"), optimizer="nadam")
    assert adv.opt.kind == "nadam" and adv.adv_opt.kind == "adam"  # the Discriminator keeps Adam


def test_guarded_adam_arguments():
    flat, status, loss = torch.zeros(5000), torch.zeros(2, dtype=torch.int32), torch.zeros(3)
    with pytest.raises(ValueError, match="given together"):
        adam.GuardedAdam(flat, status, loss, 1e-3, clip_norm=1.0, clipnorm=1.0)
    with pytest.raises(ValueError, match="parts="):
        adam.GuardedAdam(flat, status, loss, 1e-3, parts=(torch.zeros(4, dtype=torch.float64), 0))
    with pytest.raises(ValueError, match="parts"):
        adam.GuardedAdam(flat, status, loss, 1e-3, clipnorm=1.0, parts=(torch.zeros(4, dtype=torch.float64), 3))
    with pytest.raises(ValueError, match="parts"):
        adam.GuardedAdam(flat, status, loss, 1e-3, clipnorm=1.0, parts=(torch.zeros(4), 0))
    opt = adam.GuardedAdam(flat, status, loss, 1e-3, clipnorm=1.0, parts=(torch.zeros(4, dtype=torch.float64), 2),
                           counted=False)
    assert opt.counted and opt.joint and opt.part.numel() == 2 and tuple(opt.grad_norm.shape) == (2,)
    assert adam.GuardedAdam(flat, status, loss, 1e-3, kind="nadam", counted=False).counted
    assert not adam.GuardedAdam(flat, status, loss, 1e-3, counted=False).counted
    opt = adam.GuardedAdam(flat, status, loss, 1e-3, clipnorm=1.0)
    opt.step_count, opt.nonfinite[0] = 10, 2  # settle() as with clip_norm
    assert opt.pending_nonfinite() == 2 and opt.settle(3) == 2
    assert (opt.step_count, opt.skipped_nonfinite, int(opt.nonfinite)) == (5, 2, 0)


def test_check_settles_and_raises_on_the_sticky_bit(monkeypatch):
    """What the kernels leave after a non-finite joint norm followed by k more enqueued steps: the net's update
    counted the refusal and the non-finite gradient once, the encoder's -- refused by the sticky bit -- the
    refusal; every later step two refusals."""
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    tr = engine.SepTrainer(_net(), 2, 2, 4000, voiceprint=VoiceprintNet(device="cpu"), memory=_mem(), clipnorm=1.0,
                           optimizer="nadam")
    for k in (0, 1, 3):
        tr.step_count, tr.skipped_nonfinite = 100, 0
        tr.status[0], tr.status[1] = ops.STATUS_NONFINITE_GRAD, 2 + 2 * k
        tr.opt.nonfinite[0] = 1
        with pytest.raises(RuntimeError, match="non-finite gradient"):
            tr.check()
        assert (tr.step_count, tr.skipped_nonfinite) == (100 - 1 - k, 1 + k)
        assert tr.status.tolist() == [0, 0] and int(tr.opt.nonfinite) == 0 and tr.vp.opt.step_count == 0
    # bit 2 beside bit 1 (a step enqueued behind the refusal whose loss was not finite either): still the gradient's
    # message and accounting, the hand-off workspaces left alone; with bit 0 the time-out comes first
    for s, msg, reset in ((6, "non-finite gradient", False), (5, "hand-off timed out", True),
                          (7, "hand-off timed out", True), (2, "non-finite loss", False)):
        tr.step_count, tr.skipped_nonfinite = 100, 0
        tr.status[0], tr.status[1] = s, 4 if s & 4 else 2
        tr.opt.nonfinite[0] = 1 if s & 4 else 0
        tr.rnn_ws_all.fill_(1)
        with pytest.raises(RuntimeError, match=msg):
            tr.check()
        assert tr.status.tolist() == [0, 0] and bool(tr.rnn_ws_all.any()) == (not reset), s
        assert tr.step_count == (98 if s & 4 else 99) and tr.skipped_nonfinite == ((2 if s == 6 else 1) if s & 4 else 0), s
    tr.rnn_ws_all.zero_()
    # without a query encoder: counted and skipped as clip_norm is, no raise
    solo = engine.SepTrainer(_net(), 2, 2, 4000, clipnorm=1.0)
    solo.step_count = 100
    solo.status[1], solo.opt.nonfinite[0] = 1, 1
    solo.check()
    assert (solo.step_count, solo.skipped_nonfinite) == (99, 1) and solo.status.tolist() == [0, 0]


# ---- the third header -----------------------------------------------------------------------------------------------
ENTRIES = {"dl4ss_nadam", "dl4ss_adam_clipped_ex"}
CORE, OPTIM = _lib.HEADERS["dl4ss_hip.h"], _lib.HEADERS["dl4ss_optim.h"]


def test_optim_params_are_the_headers():
    """The third header's params against a second, independent reading of the header."""
    text = open(os.path.join(ROOT, "include", "dl4ss_optim.h")).read()
    assert set(OPTIM.params) == set(OPTIM.signatures) == ENTRIES == set(_lib.exported_symbols("dl4ss_optim.h"))
    for name, params in OPTIM.params.items():
        m = re.search(r"\b(?:int|long long|void)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert [re.split(r"[\s*]+", p.strip().split("[")[0])[-1] for p in m.group(1).split(",")] == list(params), name
        assert len(set(params)) == len(params) and len(OPTIM.signatures[name]) == len(params), name
        assert OPTIM.restypes[name] is I
    upd = [P, P, P, P, LL, F, F, F, F, I]
    tail = [P, P, F, P, I, P, P, P, P, P, P, I, I, F, P, P, I, P]
    assert OPTIM.signatures["dl4ss_nadam"] == upd + [D, D, D] + tail
    assert OPTIM.signatures["dl4ss_adam_clipped_ex"] == upd + tail
    clipped = CORE.params["dl4ss_adam_clipped"]  # the _ex entry: dl4ss_adam_clipped plus clip_rule and the sticky flag
    assert [p for p in OPTIM.params["dl4ss_adam_clipped_ex"] if p not in ("clip_rule", "nonfinite_sticky")] == \
        list(clipped)
    assert OPTIM.constants == dict(DL4SS_CLIP_TORCH=0, DL4SS_CLIP_KERAS=1, DL4SS_CLIP_MAX_PARTS=4096,
                                   DL4SS_STATUS_NONFINITE_GRAD=4)
    assert (ops.CLIP_TORCH, ops.CLIP_KERAS, ops.CLIP_MAX_PARTS, ops.STATUS_NONFINITE_GRAD) == (0, 1, 4096, 4)


def test_first_two_headers_tables_are_untouched_and_the_library_exports_the_third():
    imgq = _lib.HEADERS["dl4ss_imgq.h"]
    assert not ENTRIES & (set(CORE.signatures) | set(imgq.signatures)) and len(CORE.signatures) == 98
    assert not any(k in CORE.constants or k in imgq.constants for k in OPTIM.constants)
    with open(os.path.join(ROOT, "include", "dl4ss_hip.h")) as f:
        assert CORE == _lib.parse_header(f.read())
    lib = _lib.lib()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes == OPTIM.signatures[name] and fn.restype is I
    with pytest.raises(TypeError, match="dl4ss_optim.h"):
        _lib.bind("dl4ss_nothing", (), {})
    with pytest.raises(TypeError, match="'nonfinite_sticky'"):
        _lib.bind("dl4ss_nadam", (), {p: 0 for p in OPTIM.params["dl4ss_nadam"] if p != "nonfinite_sticky"})


def test_a_library_without_the_third_header_loads_and_a_call_names_the_symbol(monkeypatch):
    import types

    class Old(types.SimpleNamespace):
        def __getattr__(self, name):
            raise AttributeError(f"undefined symbol: {name}")

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Old(
        hipGetErrorString=types.SimpleNamespace(), **{n: types.SimpleNamespace() for n in CORE.signatures}))
    lib = _lib._load()
    assert lib.dl4ss_attn_nblk.argtypes == [I, I]
    with pytest.raises(AttributeError, match="dl4ss_nadam"):
        _lib.call("dl4ss_nadam", *([None] * len(OPTIM.params["dl4ss_nadam"])))
    monkeypatch.setattr(_lib, "_lib", None)  # (the next _load binds the real library again)


# ---- the call sites ---------------------------------------------------------------------------------------------
def check(fake, entry, want):
    """test_lib_bind_cpu.check against the third header's tables."""
    (name, args), = fake.calls
    params, sig = OPTIM.params[entry], OPTIM.signatures[entry]
    assert name == entry and len(args) == len(params) == len(sig)
    for p, a, kind in zip(params, args, sig):
        w = want[p]
        assert a == (tag(w) if isinstance(w, (torch.Tensor, Stand)) else w), (entry, p, a)
        if kind in (F, D):
            assert type(a) is float, (entry, p, a)
        elif kind is P:
            assert a is None or not isinstance(a, (int, float)), (entry, p, a)
        else:
            assert type(a) is int, (entry, p, a)
    fake.calls.clear()


def _stands():
    p, g, m, v = (Stand((1000,)) for _ in range(4))
    status, loss, flag = Stand((2,), torch.int32), Stand((3,)), Stand((1,))
    part, gnorm, nonfinite = Stand((5,), torch.float64), Stand((2,)), Stand((1,), torch.int32)
    want = dict(p=p, g=g, m=m, v=v, n=1000, lr=1e-3, beta1=0.8, beta2=0.9, eps=1e-6, step=7, status=status,
                dp_flag=flag, gscale=0.5, loss=loss, stream="stream")
    return (p, g, m, v), dict(status=status, loss=loss, dp_flag=flag, gscale=0.5), (part, gnorm, nonfinite), want


SEG = (2, "off", "rows", "cols", "ys", "ldy")
NOSEG = (0, None, None, None, None, None)
SEGNAMES = ("nseg", "seg_off", "seg_rows", "seg_cols", "seg_y", "seg_ldy")


@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("clip", [None, "keras", "torch", "joint"])
def test_nadam_form(fake, clip, shadow):
    fake.install()
    fake.returns["dl4ss_grad_sumsq_parts"] = 3
    bufs, kw, (part, gnorm, nonfinite), want = _stands()
    sched = adam.nadam_schedule(7, 0.8)
    ckw = {}
    if clip:
        ckw = dict(clip=(part, 2.0, gnorm, nonfinite))
        if clip == "torch":
            ckw.update(clip_rule=ops.CLIP_TORCH)
        if clip == "joint":
            ckw.update(n_part=5, sticky=True)
    ops.nadam_(*bufs, 7, sched, lr=1e-3, betas=(0.8, 0.9), eps=1e-6, shadow=SEG if shadow else None, **kw, **ckw)
    fake.calls[:] = [c for c in fake.calls if c[0] != "dl4ss_grad_sumsq_parts"]
    want.update(zip(SEGNAMES, SEG if shadow else NOSEG), mu=sched[0], mu_next=sched[1], mu_prod=sched[2])
    if clip:
        want.update(part=part, n_part=5 if clip == "joint" else 3, clip_rule=0 if clip == "torch" else 1, max_norm=2.0,
                    gnorm=gnorm, nonfinite=nonfinite, nonfinite_sticky=int(clip == "joint"))
    else:
        want.update(part=None, n_part=0, clip_rule=1, max_norm=0.0, gnorm=None, nonfinite=None, nonfinite_sticky=0)
    check(fake, "dl4ss_nadam", want)


@pytest.mark.parametrize("how", ["keras", "joint"])
def test_adam_reaches_the_ex_entry_for_the_keras_rule_or_joint_partials_only(fake, how):
    fake.install()
    fake.returns["dl4ss_grad_sumsq_parts"] = 3
    bufs, kw, (part, gnorm, nonfinite), want = _stands()
    ckw = dict(clip_rule=ops.CLIP_KERAS) if how == "keras" else dict(n_part=4, sticky=True)
    ops.adam_(*bufs, 7, lr=1e-3, betas=(0.8, 0.9), eps=1e-6, clip=(part, 2.0, gnorm, nonfinite), **kw, **ckw)
    fake.calls[:] = [c for c in fake.calls if c[0] != "dl4ss_grad_sumsq_parts"]
    want.update(zip(SEGNAMES, NOSEG), part=part, n_part=3 if how == "keras" else 4, clip_rule=int(how == "keras"),
                max_norm=2.0, gnorm=gnorm, nonfinite=nonfinite, nonfinite_sticky=int(how == "joint"))
    check(fake, "dl4ss_adam_clipped_ex", want)
    # today's call sites: today's entry points
    ops.adam_(*bufs, 7, clip=(part, 2.0, gnorm, nonfinite), **kw)
    ops.adam_(*bufs, 7, **kw)
    ops.adam_(*bufs, 7, clip=(part, 2.0, gnorm, nonfinite), clip_rule=ops.CLIP_TORCH, **kw)
    names = [c[0] for c in fake.calls if c[0] != "dl4ss_grad_sumsq_parts"]
    assert names == ["dl4ss_adam_clipped", "dl4ss_adam_guarded_dp_scaled", "dl4ss_adam_clipped"]
    for bad in (dict(clip_rule=2), dict(n_part=0), dict(n_part=4097), dict(n_part=6)):
        with pytest.raises(ValueError):
            ops.adam_(*bufs, 7, clip=(part, 2.0, gnorm, nonfinite), **kw, **bad)


def test_guarded_adam_picks_the_entry_point(fake, monkeypatch):
    """adam (no clip / clip_norm): today's entries; clipnorm: the _ex entry with the Keras rule; nadam: dl4ss_nadam,
    with clip_norm by torch's rule; parts=: the whole shared buffer and the sticky flag."""
    flat, grad = torch.zeros(5000), torch.zeros(5000)
    status, loss = torch.zeros(2, dtype=torch.int32), torch.zeros(3)
    shared = torch.zeros(4, dtype=torch.float64)
    opts = [adam.GuardedAdam(flat, status, loss, 1e-3, **kw) for kw in (
        dict(), dict(clip_norm=1.0), dict(clipnorm=1.0), dict(kind="nadam"), dict(kind="nadam", clip_norm=1.0),
        dict(kind="nadam", clipnorm=1.0, parts=(shared, 2)))]
    fake.install()
    monkeypatch.setattr(ops, "_f32c", lambda t, name: None)  # (host tensors stand in for the device's)
    fake.returns["dl4ss_grad_sumsq_parts"] = 2
    got = []
    for opt in opts:
        opt.step(grad)
        (name, args), = [c for c in fake.calls if c[0] not in ("dl4ss_grad_sumsq_parts", "dl4ss_grad_sumsq")]
        kw = dict(zip(_lib.PARAMS[name], args))
        got.append((name, kw.get("clip_rule"), kw.get("n_part"), kw.get("nonfinite_sticky"), kw["step"]))
        fake.calls.clear()
    assert got == [("dl4ss_adam_guarded_dp_scaled", None, None, None, 1), ("dl4ss_adam_clipped", None, 2, None, 1),
                   ("dl4ss_adam_clipped_ex", 1, 2, 0, 1), ("dl4ss_nadam", 1, 0, 0, 1), ("dl4ss_nadam", 0, 2, 0, 1),
                   ("dl4ss_nadam", 1, 4, 1, 1)]
    opts[-1].step(grad, step=9, summed=True)  # a borrowed count, the sum already taken: one launch
    (name, args), = fake.calls
    kw = dict(zip(OPTIM.params[name], args))
    assert (kw["step"], opts[-1].step_count) == (9, 1)
    assert (kw["mu"], kw["mu_next"], kw["mu_prod"]) == nr.schedule(9)
    assert kw["part"] == tag(shared)


def test_compat_nadam_constructor_and_groups():
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))
    opt = compat_optim.Nadam([{"params": [a]}, {"params": [b], "lr": 0.5}], lr=0.01, beta_1=0.8, beta_2=0.95,
                             epsilon=1e-7, schedule_decay=0.01, clipnorm=200)
    assert [g["lr"] for g in opt.param_groups] == [0.01, 0.5]
    assert opt.param_groups[0]["betas"] == (0.8, 0.95) and opt.param_groups[0]["eps"] == 1e-7
    assert opt.clipnorm == 200.0 and opt.schedule_decay == 0.01
    opt.step()  # no gradient anywhere: nothing to do, no count
    assert opt.step_count == 0 and opt.state == {}
    assert compat_optim.Nadam([a]).param_groups[0]["lr"] == 0.002
    for bad in (dict(clipnorm=0), dict(schedule_decay=-1)):
        with pytest.raises(ValueError):
            compat_optim.Nadam([a], **bad)
    assert math.isinf(compat_optim.Nadam([a], clipnorm=float("inf")).clipnorm)
    assert opt.nonfinite is None and opt.settle() == 0 and opt.skipped_nonfinite == 0  # (no step yet: no buffers)
    # settle(): every parameter's launch of a refused step counted it once
    opt._clip = ([1, 1], None, None, torch.tensor([4], dtype=torch.int32))
    opt.step_count = 10
    assert opt.settle() == 2 and (opt.step_count, opt.skipped_nonfinite, int(opt.nonfinite)) == (8, 2, 0)
