"""A run resumed from checkpoint.save_training_state continues as the run that was never interrupted.

Shapes of tests/test_step_gpu.py::test_step_bitwise_reproducible: SepNet(num_layers=2), B = 4, K = 2, N = 8000, five
fixed batches of synth.SyntheticMixtures; the learning rate is halved between steps (schedule.LRHalving, every=1),
so lr is state that moves.

Yardstick: the uninterrupted five-step run of a case, made twice (once per case, shared, unchanged).  Where the two
agree bit for bit -- the bf16 steps and the fp32 step with splitk_reduce="fixed" do -- the
resumed run must equal them bit for bit.  Where they do not, the state right after the load must still be bitwise
the saved one, and the continued run may differ from an uninterrupted one, quantity by quantity, by no more than
the two uninterrupted runs differ from each other."""
import functools
import shutil

import numpy as np
import pytest
import torch

from dl4ss_amd import checkpoint, classifier, engine, infer, ops, schedule, synth
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, K, N, STEPS, CUT = 4, 2, 8000, 5, 2
T = ops.n_frames(N)
LR = 2e-4
N_LAB = 11
CLS_B = 2  # the classifier's step repeats bit for bit on B T <= 256 rows

# net=: SepNet's arguments, the rest SepTrainer's; adv / vp: the stateful parts
CASES = {
    "bf16-pit-lstm-adam": dict(net=dict(cell="lstm"), precision="bf16", mode="pit"),
    "bf16s-label-lstm-nadam-clipnorm": dict(net=dict(cell="lstm"), precision="bf16s", mode="label", optimizer="nadam",
                                            clipnorm=200),
    "bf16-pit-gru-clip_norm": dict(net=dict(cell="gru", adjust=False), precision="bf16", mode="pit", clip_norm=5.0),
    "fp32-label-lstm-fixed-align": dict(net=dict(cell="lstm", attention="align", adjust=False), precision="fp32",
                                        mode="label", splitk_reduce="fixed"),
    "adversary": dict(net=dict(cell="lstm"), precision="bf16", mode="pit", adv=True),
    "voiceprint": dict(net=dict(cell="lstm", adjust=False), precision="fp32", mode="label", splitk_reduce="fixed",
                       vp=True),
    "classifier": dict(cls=True),
}
RESUME = list(CASES)[:4]
STATEFUL = list(CASES)[4:]


@functools.lru_cache(maxsize=None)
def _batches(cls=False):
    gen = synth.SyntheticMixtures(n_samples=N, k=K, seed=9)
    out = []
    for _ in range(STEPS):
        src, spk, u = gen.batch(CLS_B if cls else B)
        last = torch.from_numpy(spk.astype(np.int32))
        if cls:
            last = torch.zeros(CLS_B, N_LAB)
            for b in range(CLS_B):
                last[b, torch.from_numpy(spk[b] % N_LAB)] = 1.0
        out.append((torch.from_numpy(src.astype(np.float32)).to(DEV),
                    torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(DEV), last.to(DEV)))
    return out


def _build(case, seed):
    """a trainer of the case on nets of ``seed`` (the net, the Discriminator, the encoder; the memory not zero)"""
    kw = dict(CASES[case])
    if kw.pop("cls", False):
        cnet = infer.ClassifierNet(hidden=40, num_layers=1, num_labels=N_LAB, device=DEV, seed=seed)
        tr = classifier.ClassifierTrainer(cnet, CLS_B, K, N, lr=LR)
        assert CLS_B * tr.T <= 256
        return tr
    net = engine.SepNet(num_layers=2, device=DEV, seed=seed, **kw.pop("net"))
    if kw.pop("adv", False):
        kw["adversary"] = engine.DiscNet(T, 129, device=DEV, seed=seed + 1)
    if kw.pop("vp", False):
        kw["voiceprint"] = VoiceprintNet(device=DEV, seed=seed + 2)
        kw["memory"] = SpeakerMemory(101, 50, device=DEV)
        kw["memory"].mem.copy_(torch.randn(101, 50, generator=torch.Generator().manual_seed(seed)) * 0.1)
    return engine.SepTrainer(net, B, K, N, lr=LR, **kw)


def _state(tr):
    """everything a saved state covers: tensors cloned, scalars as they are"""
    out = {"flat": tr.net.flat.clone(), "m": tr.opt.m.clone(), "v": tr.opt.v.clone(), "step_count": tr.step_count,
           "lr": tr.lr, "skipped_nonfinite": tr.skipped_nonfinite}
    if getattr(tr, "adv", None) is not None:
        out.update(disc=tr.adv.disc.flat.clone(), adv_m=tr.adv_opt.m.clone(), adv_v=tr.adv_opt.v.clone(),
                   adv_step_count=tr.adv_step_count, adv_lr=tr.adv_lr)
    if getattr(tr, "vp", None) is not None:
        out.update(enc=tr.vp.net.flat.clone(), enc_m=tr.vp_opt.m.clone(), enc_v=tr.vp_opt.v.clone(),
                   enc_step_count=tr.vp_opt.step_count, enc_lr=tr.vp_lr, mem=tr.memory.mem.clone())
    return out


def _steps(case, tr, sched, first, last, graph=False):
    """steps first .. last - 1 with the learning rate halved in front of every step but the first of the run;
    returns the run's record: the losses, the parameters after step CUT, the final state"""
    batches = _batches(bool(CASES[case].get("cls")))
    rec, losses = {}, []
    for i in range(first, last):
        if i > 0:
            sched.apply(tr, i)
        losses.append((tr.step_graph if graph else tr.step)(*batches[i]).clone())
        if i == CUT:
            rec["flat_after_cut"] = tr.net.flat.clone()
    tr.check()
    rec.update(_state(tr), losses=torch.stack(losses))
    assert rec["losses"].isfinite().all() and rec["skipped_nonfinite"] == 0
    return rec


def _uninterrupted(case):
    return _steps(case, _build(case, seed=11), schedule.LRHalving(LR, every=1), 0, STEPS)


def _diffs(a, b, tail=False):
    """per quantity: equal (scalars) or the largest absolute difference (tensors); tail: b's losses of steps >= CUT"""
    out = {}
    for k, x in a.items():
        y = b[k][CUT:] if (tail and k == "losses") else b[k]
        out[k] = float((x.double() - y.double()).abs().max()) if isinstance(x, torch.Tensor) else (0.0 if x == y else
                                                                                                 float("inf"))
        if isinstance(x, torch.Tensor) and out[k] == 0.0 and not torch.equal(x, y):  # +0 against -0, NaN
            out[k] = float("inf")
    return out


@functools.lru_cache(maxsize=None)
def _yardstick(case):
    """(the uninterrupted run, None where a second one agrees with it bit for bit, else their differences)"""
    a, b = _uninterrupted(case), _uninterrupted(case)
    d = _diffs(a, b)
    bitwise = all(v == 0.0 for v in d.values())
    print(f"{case}: two uninterrupted runs {'agree bit for bit' if bitwise else f'differ by {d}'}")
    assert all(d[k] == 0.0 for k, x in a.items() if not isinstance(x, torch.Tensor)), d
    assert a["step_count"] == STEPS and a["lr"] == LR / 2 ** (STEPS - 1)
    return a, (None if bitwise else d)


def _assert_continues(case, got):
    """``got``: the record of steps CUT .. STEPS - 1 of a resumed run, under the yardstick rule"""
    ref, spread = _yardstick(case)
    d = _diffs(got, ref, tail=True)
    print(f"{case}: resumed against uninterrupted {d}")
    for k, v in d.items():
        assert v <= (0.0 if spread is None else spread[k]), (k, v, spread)
    assert got["lr"] == LR / 2 ** (STEPS - 1) and got["step_count"] == STEPS


@pytest.fixture(scope="module")
def heads(tmp_path_factory):
    """per case, made once: steps 0 .. CUT - 1, then the saved file, the state it was saved from and the weights
    alone; the net and the trainer are dropped"""
    d, cache = tmp_path_factory.mktemp("train_state"), {}

    def get(case):
        if case not in cache:
            tr, sched = _build(case, seed=11), schedule.LRHalving(LR, every=1)
            _steps(case, tr, sched, 0, CUT)
            path = str(d / f"{case}.pt")
            checkpoint.save_training_state(path, tr, schedule=sched, extra={"next_step": CUT})
            cache[case] = (path, _state(tr), tr.net.state_dict())
            del tr
        return cache[case]

    yield get
    shutil.rmtree(d, ignore_errors=True)


def _resume(case, head, seed=12, warm=False, capture=None):
    """a new trainer on nets of another seed, the file loaded (the state right after the load bitwise the saved
    one), steps CUT .. STEPS - 1.  warm: one eager step first; capture "before" / "after" the load: step_graph"""
    path, saved, _ = head
    tr, sched = _build(case, seed), schedule.LRHalving(LR, every=1)
    assert not torch.equal(tr.net.flat, saved["flat"])
    if warm:
        tr.step(*_batches(False)[0])
        tr.check()
    if capture == "before":
        tr.capture()
    extra = checkpoint.load_training_state(path, tr, schedule=sched)
    assert extra == {"next_step": CUT} and sched.lr == saved["lr"]
    d = _diffs(_state(tr), saved)
    assert all(v == 0.0 for v in d.values()), d
    if capture == "after":
        tr.capture()
    return _steps(case, tr, sched, extra["next_step"], STEPS, graph=capture is not None)


@pytest.mark.parametrize("case", RESUME)
def test_resumed_run_equals_the_uninterrupted_run(dev, heads, case):
    _assert_continues(case, _resume(case, heads(case)))


def test_weights_alone_do_not_resume(dev, heads):
    """the control: the same resume from net.load_state_dict, with the right lr even -- zero moments and bias
    corrections from 1 are another optimisation"""
    case = RESUME[0]
    (ref, spread), (_, saved, weights) = _yardstick(case), heads(case)
    tr, sched = _build(case, seed=12), schedule.LRHalving(saved["lr"], every=1)
    tr.net.load_state_dict(weights)
    tr.params_changed()
    tr.lr = saved["lr"]
    assert torch.equal(tr.net.flat, saved["flat"])
    got = _steps(case, tr, sched, CUT, CUT + 1)
    if spread is None:  # same weights, same batch: the loss of step CUT is the uninterrupted one's, the update is not
        assert torch.equal(got["losses"][0], ref["losses"][CUT])
    diff = float((got["flat_after_cut"] - ref["flat_after_cut"]).abs().max())
    print(f"weights alone: parameters after step {CUT} differ by {diff:.3e}")
    assert diff > (0.0 if spread is None else spread["flat"])


@pytest.mark.parametrize("when", ["before", "after"])
@pytest.mark.parametrize("case", RESUME)
def test_captured_graph_replays_on_the_loaded_state(dev, heads, case, when):
    """a graph captured before the load stays valid (the load is copy_ into the buffers it reads, the bf16 weight
    copies are converted again); so does one captured after it"""
    _assert_continues(case, _resume(case, heads(case), warm=True, capture=when))


@pytest.mark.parametrize("case", STATEFUL)
def test_stateful_steps_resume(dev, heads, case):
    """the Discriminator's parameters, moments and both update counts; the voiceprint encoder's state and the
    memory rows; the classifier's trainer"""
    ref, _ = _yardstick(case)
    want = {"adversary": {"disc", "adv_m", "adv_v", "adv_step_count"}, "voiceprint": {"enc", "enc_m", "enc_v", "mem"},
            "classifier": set()}[case]
    assert want <= set(ref)
    if case == "adversary":
        assert ref["adv_step_count"] == 2 * STEPS
    _assert_continues(case, _resume(case, heads(case)))


def test_refused_update_never_reaches_a_file(dev, tmp_path):
    """An update refused on device (a NaN in the gradient, as tests/test_clip_step_gpu.py writes one) is still
    counted in step_count until check(): no state is saved before it, and the state saved after it holds the applied
    count and the skipped one"""
    case = "bf16-pit-gru-clip_norm"
    tr, batches, path = _build(case, seed=11), _batches(False), str(tmp_path / "state.pt")
    tr.step(*batches[0])
    tr.check()
    raw, gains, spk = batches[1]
    tr.spk.copy_(spk)
    tr.features(raw, gains)
    tr.forward()
    tr.loss_and_grad()
    tr.backward()
    tr.net.grad[tr.net.grad.numel() // 2] = float("nan")
    tr.optimizer_step()
    assert tr.step_count == 2  # not yet settled
    with pytest.raises(RuntimeError, match=r"check\(\)"):
        checkpoint.save_training_state(path, tr)
    assert not list(tmp_path.iterdir())
    tr.check()  # returns: a skipped update is not an error
    assert (tr.step_count, tr.skipped_nonfinite) == (1, 1)
    checkpoint.save_training_state(path, tr)
    tr2 = _build(case, seed=12)
    checkpoint.load_training_state(path, tr2)
    assert (tr2.step_count, tr2.skipped_nonfinite) == (1, 1)
    d = _diffs(_state(tr2), _state(tr))
    assert all(v == 0.0 for v in d.values()), d
    a, b = tr.step(*batches[1]).clone(), tr2.step(*batches[1]).clone()
    tr.check(), tr2.check()
    d = _diffs(_state(tr2), _state(tr))
    assert torch.equal(a, b) and all(v == 0.0 for v in d.values()), d
