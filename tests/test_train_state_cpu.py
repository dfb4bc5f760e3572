"""Training state without a GPU: trainers constructed on CPU nets (as tests/test_clip_api_cpu.py does) hold every
buffer a saved state covers, so the round trip, the file format, every refusal, the atomic write, the settled-trainer
rule, the RNG streams and the schedules are checked here; tests/test_train_state_gpu.py runs the steps."""
import os
import pickle
import random

import numpy as np
import pytest
import torch

from dl4ss_amd import checkpoint, classifier, engine, infer, ops, schedule
from dl4ss_amd.imagequery import ImageQueryNet
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintNet

B, K, N, H = 2, 2, 4000, 40
T = ops.n_frames(N)


def _sep(seed=1, num_layers=2, rows=101, **kw):
    """(trainer, net) of one of the kinds below; ``kw``: SepNet's gates / attention / adjust, the rest SepTrainer's"""
    nkw = {k: kw.pop(k) for k in ("gates", "attention", "adjust", "cell") if k in kw}
    query = kw.pop("query", None)
    if query is not None:
        nkw.setdefault("adjust", False)
        kw["memory"] = SpeakerMemory(rows, 50, device="cpu")
        if query == "voiceprint":
            kw["voiceprint"] = VoiceprintNet(device="cpu", seed=seed + 50)
        else:
            kw["image_query"] = ImageQueryNet(device="cpu", seed=seed + 50)
    if kw.pop("adv", False):
        kw["adversary"] = engine.DiscNet(T, 129, device="cpu", seed=seed + 70)
    net = engine.SepNet(num_layers=num_layers, hidden=H, device="cpu", seed=seed, **nkw)
    return engine.SepTrainer(net, B, K, N, **kw)


def _cls(seed=1, **kw):
    cnet = infer.ClassifierNet(hidden=H, num_layers=1, device="cpu", seed=seed)
    return classifier.ClassifierTrainer(cnet, B, K, N, **kw)


KINDS = {"plain": lambda s: _sep(s), "adversary": lambda s: _sep(s, adv=True),
         "voiceprint": lambda s: _sep(s, query="voiceprint"), "image_query": lambda s: _sep(s, query="image_query"),
         "nadam": lambda s: _sep(s, optimizer="nadam", clipnorm=200), "classifier": lambda s: _cls(s)}


def _opts(tr):
    return [o for o in (tr.opt, getattr(tr, "adv_opt", None), getattr(tr, "vp_opt", None)) if o is not None]


def _tensors(tr):
    """every tensor of the trainer's state"""
    out = [tr.net.flat]
    for o in _opts(tr):
        out += [o.m, o.v]
    if getattr(tr, "adv", None) is not None:
        out.append(tr.adv.disc.flat)
    if getattr(tr, "vp", None) is not None:
        out += [tr.vp.net.flat, tr.memory.mem]
    return out


def _scalars(tr):
    return [(o.step_count, o.skipped_nonfinite, o.lr) for o in _opts(tr)]


def _fill(tr, seed):
    g = torch.Generator().manual_seed(seed)
    for t in _tensors(tr):
        t.copy_(torch.randn(t.shape, generator=g))
    for i, o in enumerate(_opts(tr)):
        o.step_count, o.skipped_nonfinite, o.lr = 7 + 10 * i, 2 + i, 1.25e-4 / (i + 3)


def _snapshot(tr):
    return [t.clone() for t in _tensors(tr)], _scalars(tr)


def _rng_streams():
    return random.getstate(), np.random.get_state(), torch.get_rng_state()


def _same_rng(a, b):
    return a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:] \
        and torch.equal(a[2], b[2])


def _assert_unchanged(tr, snap, rng):
    tensors, scalars = snap
    assert all(torch.equal(a, b) for a, b in zip(tensors, _tensors(tr))) and scalars == _scalars(tr)
    assert _same_rng(rng, _rng_streams())


# ---------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_round_trip(tmp_path, kind):
    a, b = KINDS[kind](1), KINDS[kind](2)
    _fill(a, seed=31)
    assert not torch.equal(a.net.flat, b.net.flat) and _scalars(a) != _scalars(b)
    if hasattr(b, "_wb_ver"):
        b._wb_ver, gen = ("made", 0), b.net.generation
    p = str(tmp_path / "state.pt")
    assert checkpoint.save_training_state(p, a, extra={"epoch": 3, "batch": 17, "list": "tr", "best": None}) == p
    extra = checkpoint.load_training_state(p, b)
    assert extra == {"epoch": 3, "batch": 17, "list": "tr", "best": None}
    ta, tb = _tensors(a), _tensors(b)
    assert len(ta) == len(tb) == {"plain": 3, "nadam": 3, "classifier": 3, "adversary": 6}.get(kind, 7)
    for x, y in zip(ta, tb):
        assert torch.equal(x, y)
    assert _scalars(a) == _scalars(b) and len({s for s in _scalars(b)}) == len(_opts(b))
    assert all(type(lr) is float and type(n) is int for n, _, lr in _scalars(b))
    if hasattr(b, "_wb_ver"):  # the net declared the change, the bf16 weight copies are stale
        assert b._wb_ver is None and b.net.generation > gen and b._wb_stale()


def test_load_is_in_place(tmp_path):
    """copy_ into the existing buffers: every pointer a captured graph holds stays what it was"""
    a, b = KINDS["adversary"](1), KINDS["adversary"](2)
    _fill(a, seed=5)
    ptrs = [t.data_ptr() for t in _tensors(b)]
    m = b.m
    p = str(tmp_path / "s.pt")
    checkpoint.save_training_state(p, a)
    checkpoint.load_training_state(p, b)
    assert [t.data_ptr() for t in _tensors(b)] == ptrs and b.m is m and torch.equal(b.m, a.m)


def test_state_dict_round_trip_without_a_file():
    a, b = KINDS["voiceprint"](1), KINDS["voiceprint"](2)
    _fill(a, seed=9)
    b.load_state_dict(a.state_dict())
    assert all(torch.equal(x, y) for x, y in zip(_tensors(a), _tensors(b))) and _scalars(a) == _scalars(b)
    sd = a.opt.state_dict()
    assert sd["kind"] == "adam" and sd["betas"] == [0.9, 0.999] and sd["step_count"] == 7 and "schedule" not in sd
    a.m.add_(1)  # the state is a copy, not a view
    assert not torch.equal(sd["m"], a.m)


# --------------------------------------------------------------------------------------------------- safe format
def _plain(x):
    if isinstance(x, dict):
        return all(type(k) is str and _plain(v) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return all(_plain(v) for v in x)
    return x is None or type(x) in (str, int, float, bool, torch.Tensor)


def test_file_is_plain_and_loads_with_the_safe_loader(tmp_path):
    tr = KINDS["image_query"](1)
    p = str(tmp_path / "state.pt")
    checkpoint.save_training_state(p, tr, schedule=schedule.evalver(), stopper=schedule.EarlyStopping(3))
    sd = torch.load(p, weights_only=True)
    assert sd["format"] == "dl4ss-training-state" and type(sd["version"]) is int and sd["version"] >= 1
    assert _plain(sd)
    assert isinstance(sd["rng"]["numpy"]["key"], torch.Tensor) and sd["rng"]["numpy"]["key"].numel() == 624
    assert set(sd["trainer"]) == {"net", "opt", "image_query"}
    assert set(sd["trainer"]["image_query"]) == {"net", "opt", "memory"}
    lay = sd["trainer"]["net"]["layout"]
    assert [n for n, _ in lay["params"]] == [n for n, _ in tr.net.specs]
    assert [lay[k] for k in ("cell", "gates", "attention", "crm", "adjust")] == ["lstm", "logistic", "dot", False, False]


class _Arbitrary:
    pass


def test_unsafe_payloads_are_refused(tmp_path):
    tr = KINDS["plain"](1)
    p = str(tmp_path / "state.pt")
    checkpoint.save_training_state(p, tr)
    sd = torch.load(p, weights_only=True)
    sd["extra"] = {"thing": _Arbitrary()}
    bad = str(tmp_path / "bad.pt")
    torch.save(sd, bad)
    snap, rng = _snapshot(tr), _rng_streams()
    with pytest.raises(pickle.UnpicklingError):
        checkpoint.load_training_state(bad, tr)
    _assert_unchanged(tr, snap, rng)
    # and the writer puts no such thing into a file
    for extra in ({"thing": _Arbitrary()}, {"a": np.float32(1.0)}, {3: "int key"}):
        with pytest.raises(TypeError, match="extra"):
            checkpoint.save_training_state(p, tr, extra=extra)
    assert sorted(os.listdir(tmp_path)) == ["bad.pt", "state.pt"]
    checkpoint.load_training_state(p, tr)  # the earlier file is intact


# ----------------------------------------------------------------------------------------------------- refusals
def _edited(tmp_path, **fields):
    tr = KINDS["plain"](1)
    p = str(tmp_path / "good.pt")
    checkpoint.save_training_state(p, tr)
    sd = torch.load(p, weights_only=True)
    sd.update(fields)
    q = str(tmp_path / "edited.pt")
    torch.save(sd, q)
    return q


REFUSALS = {
    "num_layers": (lambda: _sep(1, num_layers=1), lambda: _sep(2, num_layers=2), "params"),
    "gates": (lambda: _sep(1, gates="hard"), lambda: _sep(2), "gates"),
    "attention": (lambda: _sep(1, attention="align", adjust=False), lambda: _sep(2, adjust=False), "attention"),
    "kind": (lambda: _sep(1, optimizer="nadam"), lambda: _sep(2), "kind"),
    "betas": (lambda: _sep(1, betas=(0.8, 0.999)), lambda: _sep(2), "betas"),
    "adversary_in_file": (lambda: _sep(1, adv=True), lambda: _sep(2), "adversary"),
    "adversary_in_trainer": (lambda: _sep(1), lambda: _sep(2, adv=True), "adversary"),
    "memory_shape": (lambda: _sep(1, query="voiceprint", rows=101), lambda: _sep(2, query="voiceprint", rows=60),
                     "memory"),
    "voiceprint_vs_image_query": (lambda: _sep(1, query="voiceprint"), lambda: _sep(2, query="image_query"),
                                  "voiceprint"),
    "clipnorm": (lambda: _sep(1, clipnorm=200), lambda: _sep(2, clipnorm=100), "clipnorm"),
    "classifier_file": (lambda: _cls(1), lambda: _sep(2), "layout"),
    "sep_file_into_classifier": (lambda: _sep(1), lambda: _cls(2), "layout"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_mismatch_is_refused_before_anything_changes(tmp_path, case):
    saver, loader, field = REFUSALS[case]
    a, b = saver(), loader()
    _fill(a, seed=3)
    _fill(b, seed=4)
    p = str(tmp_path / "state.pt")
    sched, stop = schedule.evalver(), schedule.EarlyStopping(2)
    checkpoint.save_training_state(p, a, schedule=sched, stopper=stop)
    random.random(), np.random.rand(), torch.rand(1)  # the streams have moved on since the save
    sched.lr, stop.best_epoch = 1e-9, 77
    snap, rng = _snapshot(b), _rng_streams()
    with pytest.raises(ValueError, match=field) as e:
        checkpoint.load_training_state(p, b, schedule=sched, stopper=stop)
    assert "the file has" in str(e.value) and "this trainer has" in str(e.value) and p in str(e.value)
    _assert_unchanged(b, snap, rng)
    assert sched.lr == 1e-9 and stop.best_epoch == 77


@pytest.mark.parametrize("field,value", [("format", "something-else"), ("version", 10 ** 6)])
def test_format_and_version_are_checked(tmp_path, field, value):
    q = _edited(tmp_path, **{field: value})
    tr = KINDS["plain"](2)
    _fill(tr, seed=8)
    snap, rng = _snapshot(tr), _rng_streams()
    with pytest.raises(ValueError, match=field) as e:
        checkpoint.load_training_state(q, tr)
    assert str(value) in str(e.value)
    _assert_unchanged(tr, snap, rng)
    checkpoint.load_training_state(str(tmp_path / "good.pt"), tr)


def test_schedule_and_stopper_mismatches_are_refused(tmp_path):
    tr = KINDS["plain"](1)
    p = str(tmp_path / "state.pt")
    checkpoint.save_training_state(p, tr, schedule=schedule.evalver(), rng=False)
    snap, rng = _snapshot(tr), _rng_streams()
    with pytest.raises(ValueError, match="every"):
        checkpoint.load_training_state(p, tr, schedule=schedule.selfss_db(), rng=False)
    with pytest.raises(ValueError, match="stopper"):  # asked for, not in the file
        checkpoint.load_training_state(p, tr, stopper=schedule.EarlyStopping(1), rng=False)
    with pytest.raises(ValueError, match="rng"):
        checkpoint.load_training_state(p, tr)
    _assert_unchanged(tr, snap, rng)
    checkpoint.load_training_state(p, tr, rng=False)  # a schedule the caller does not pass is left unread


# ------------------------------------------------------------------------------------------------- atomic write
def test_failed_save_leaves_the_previous_file(tmp_path, monkeypatch):
    a = KINDS["plain"](1)
    _fill(a, seed=12)
    p = str(tmp_path / "state.pt")
    checkpoint.save_training_state(p, a, extra={"epoch": 1})
    good = open(p, "rb").read()
    _fill(a, seed=13)

    def torn(obj, f, *args, **kw):
        if hasattr(f, "write"):
            f.write(b"half a file")
        else:
            with open(f, "wb") as fh:
                fh.write(b"half a file")
        raise OSError("disk full")

    with monkeypatch.context() as m:
        m.setattr(torch, "save", torn)
        with pytest.raises(OSError, match="disk full"):
            checkpoint.save_training_state(p, a, extra={"epoch": 2})
    assert os.listdir(tmp_path) == ["state.pt"] and open(p, "rb").read() == good
    b = KINDS["plain"](2)
    assert checkpoint.load_training_state(p, b) == {"epoch": 1}
    assert not torch.equal(b.net.flat, a.net.flat)  # the first save's state, not the torn one's
    checkpoint.save_training_state(p, a, extra={"epoch": 2})  # and the next save replaces it
    assert os.listdir(tmp_path) == ["state.pt"] and checkpoint.load_training_state(p, b) == {"epoch": 2}
    assert torch.equal(b.net.flat, a.net.flat)


# --------------------------------------------------------------------------------------------- unsettled trainer
@pytest.mark.parametrize("kind", ["plain", "classifier"])
def test_unsettled_trainer_is_not_saved(tmp_path, kind):
    tr = KINDS[kind](1)
    p = str(tmp_path / "state.pt")
    for word in (1, 0):
        tr.status[word] = 1  # a host write: a refused update check() has not yet taken out of step_count
        with pytest.raises(RuntimeError, match=r"check\(\)"):
            checkpoint.save_training_state(p, tr)
        with pytest.raises(RuntimeError, match=r"check\(\)"):
            tr.state_dict()
        assert os.listdir(tmp_path) == []
        tr.status[word] = 0
    checkpoint.save_training_state(p, tr)
    tr.status[1] = 2
    with pytest.raises(RuntimeError, match=r"check\(\)"):  # nor is a state loaded over pending refusals
        checkpoint.load_training_state(p, tr)
    tr.status.zero_()
    checkpoint.load_training_state(p, tr)


def test_pending_nonfinite_refusal_is_not_saved(tmp_path):
    tr = _sep(1, clip_norm=5.0)
    tr.opt.nonfinite[0] = 1
    with pytest.raises(RuntimeError, match="non-finite"):
        checkpoint.save_training_state(str(tmp_path / "state.pt"), tr)
    assert os.listdir(tmp_path) == []
    tr.opt.nonfinite.zero_()
    checkpoint.save_training_state(str(tmp_path / "state.pt"), tr)


# ---------------------------------------------------------------------------------------------------------- RNG
def _draws():
    return (random.random(), random.gauss(0, 1), random.randint(0, 10 ** 9), np.random.rand(3).tolist(),
            np.random.randn(3).tolist(), np.random.permutation(7).tolist(), torch.rand(3).tolist(),
            torch.randperm(9).tolist())


def test_rng_streams_resume(tmp_path):
    tr = KINDS["plain"](1)
    random.seed(5), np.random.seed(6), torch.manual_seed(7)
    random.gauss(0, 1), np.random.randn()  # both generators hold a cached normal
    p = str(tmp_path / "state.pt")
    checkpoint.save_training_state(p, tr)
    first = _draws()
    assert _draws() != first
    checkpoint.load_training_state(p, tr)
    assert _draws() == first
    # rng=False touches no generator
    checkpoint.save_training_state(p, tr, rng=False)
    before = _rng_streams()
    checkpoint.load_training_state(p, tr, rng=False)
    assert _same_rng(before, _rng_streams())


# ---------------------------------------------------------------------------------------------------- schedules
def _epochs(sched, stop, tr, losses, first, last):
    out = []
    for e in range(first, last):
        lr = sched.apply(tr, e)
        snap = stop.update(e, losses[e])
        out.append((lr, tr.lr, snap, stop.stop, stop.best_epoch, stop.best_loss))
    return out


@pytest.mark.parametrize("cut", [1, 7, 12, 20])
def test_schedules_resume(tmp_path, cut):
    losses = (np.random.default_rng(3).random(30) + np.linspace(1, 0.5, 30)).tolist()
    losses[5] = float("nan")
    losses[13:] = [x + 1 for x in losses[13:]]  # no improvement after epoch 12: patience runs out
    new = lambda: (schedule.LRHalving(2e-4, every=3, floor=1e-5), schedule.EarlyStopping(4, patience=6, max_epoch=30))
    tr = KINDS["plain"](1)
    sched, stop = new()
    whole = _epochs(sched, stop, tr, losses, 0, 30)
    assert any(w[3] for w in whole) and not whole[12][3] and len({w[0] for w in whole}) > 3

    tr = KINDS["plain"](1)
    sched, stop = new()
    head = _epochs(sched, stop, tr, losses, 0, cut)
    p = str(tmp_path / "state.pt")
    checkpoint.save_training_state(p, tr, schedule=sched, stopper=stop, extra={"epoch": cut})
    tr2 = KINDS["plain"](2)
    sched2, stop2 = new()
    extra = checkpoint.load_training_state(p, tr2, schedule=sched2, stopper=stop2)
    assert tr2.lr == tr.lr and sched2.lr == sched.lr
    tail = _epochs(sched2, stop2, tr2, losses, extra["epoch"], 30)
    assert head + tail == whole
