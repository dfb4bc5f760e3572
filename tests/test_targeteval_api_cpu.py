"""Host side of the target evaluation: the list reader, EarlyStopping against a line-by-line transcription of the
Keras trainer's loop, every refusal (raised before any device call), the fourth header's tables, and the in-memory
weight snapshots.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from dl4ss_amd import _lib, checkpoint, engine, schedule, targeteval
from dl4ss_amd.imagequery import ImageQueryNet
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"dl4ss_bss_gain_ws_bytes", "dl4ss_bss_gain", "dl4ss_te_assemble"}
N = 4000
CORE, EVAL = _lib.HEADERS["dl4ss_hip.h"], _lib.HEADERS["dl4ss_eval.h"]


def _net(**kw):
    kw.setdefault("adjust", False)
    return engine.SepNet(cell="lstm", num_layers=1, hidden=40, device="cpu", seed=1, **kw)


def _vnet(**kw):
    return VoiceprintNet(device="cpu", seed=2, **kw)


def _mem(emb=50):
    return SpeakerMemory(7, emb, device="cpu")


# ------------------------------------------------------------------ the list reader
def test_read_eval_list_both_formats(tmp_path):
    p = tmp_path / "seen.lst"
    p.write_text("a/t1.wav a/b1.wav,a/b2.wav spk01\n  a/t2.wav\ta/b3.wav   spk02  \n")
    got = targeteval.read_eval_list(str(p))
    assert got == [dict(target="a/t1.wav", bg=["a/b1.wav", "a/b2.wav"], spk="spk01", supp=[]),
                   dict(target="a/t2.wav", bg=["a/b3.wav"], spk="spk02", supp=[])]
    q = tmp_path / "unseen.lst"
    q.write_text("a/t1.wav a/b1.wav spk09 a/s1.wav,a/s2.wav\n")
    assert targeteval.read_eval_list(str(q), unk_spk=True) == [
        dict(target="a/t1.wav", bg=["a/b1.wav"], spk="spk09", supp=["a/s1.wav", "a/s2.wav"])]


@pytest.mark.parametrize("text,unk", [("a/t1.wav a/b1.wav spk01\nonlyone\n", False), ("a/t1.wav\n", True),
                                      ("a/t1.wav a/b1.wav\n", False), ("a/t1.wav a/b1.wav spk01\n", True),
                                      ("a/t1.wav a/b1.wav spk01 a/s1.wav\n", False), ("a b c\n\nd e f\n", False)])
def test_read_eval_list_refuses_a_malformed_line(tmp_path, text, unk):
    p = tmp_path / "bad.lst"
    p.write_text(text)
    with pytest.raises(ValueError, match="bad.lst:"):
        targeteval.read_eval_list(str(p), unk_spk=unk)


# ------------------------------------------------------------------ EarlyStopping
def _reference_loop(losses, start, max_epoch):
    """nnet.py:119-172 with the training and the file I/O taken out, line by line: returns (the epochs at which
    save_weights ran, the epoch of the return, the epoch whose weights were loaded); (saves, None, None) when the
    loop runs out without returning."""
    start_ealy_stop = start
    lowest_dev_loss = float('inf')
    lowest_dev_epoch = start_ealy_stop
    saves = []
    for epoch_num in range(max_epoch):
        dev_loss = losses[epoch_num]
        if epoch_num >= start_ealy_stop:
            if dev_loss < lowest_dev_loss:
                lowest_dev_loss = dev_loss
                lowest_dev_epoch = epoch_num
                saves.append(epoch_num)
            if (epoch_num - lowest_dev_epoch >= 10) or (epoch_num == max_epoch - 1):
                return saves, epoch_num, lowest_dev_epoch
    return saves, None, None


NAN = float("nan")
SEQUENCES = {
    "improves late": ([5.0, 4.0, 6.0, 6.1, 6.2, 6.3, 6.4, 6.5, 6.6, 6.7, 6.8, 3.0] + [3.5] * 12, 2, 40),
    "never improves after start": ([1.0, 2.0, 3.0] + [3.0 + 0.1 * i for i in range(20)], 3, 40),
    "hits max_epoch - 1": ([10.0 - i for i in range(8)], 2, 8),
    "holds a NaN": ([5.0, 4.0, NAN, 3.0, NAN, NAN, 2.5] + [2.6] * 14, 1, 40),
    "NaN from the start": ([NAN] * 15, 0, 40),
    "start beyond the run": ([3.0, 2.0, 1.0], 5, 3),
}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_early_stopping_is_the_reference_loop(name):
    losses, start, max_epoch = SEQUENCES[name]
    saves, stop_at, restore = _reference_loop(losses, start, max_epoch)
    es = schedule.EarlyStopping(start, patience=10, max_epoch=max_epoch)
    got_saves, got_stop = [], None
    for epoch in range(min(max_epoch, len(losses))):
        if es.update(epoch, losses[epoch]):
            got_saves.append(epoch)
        if es.stop:
            got_stop = epoch
            break
    assert got_saves == saves and got_stop == stop_at
    if stop_at is not None:
        assert es.best_epoch == restore
    assert not any(math.isnan(losses[e]) for e in got_saves)


def test_early_stopping_patience_and_open_end():
    es = schedule.EarlyStopping(0, patience=2)  # max_epoch None: only the patience stops it
    assert [es.update(e, l) for e, l in enumerate([3.0, 2.0, 2.5, 2.4])] == [True, True, False, False]
    assert es.stop and es.best_epoch == 1 and es.best_loss == 2.0


# ------------------------------------------------------------------ refusals, before any device call
def test_every_refusal_is_a_host_check(monkeypatch):
    net, vnet, mem = _net(), _vnet(), _mem()
    inet40 = ImageQueryNet(device="cpu", seed=2, emb=40)
    tr = engine.SepTrainer(_net(), 2, 2, N, voiceprint=vnet, memory=SpeakerMemory(101, 50, device="cpu"))
    monkeypatch.setattr(_lib, "_load", lambda: pytest.fail("the library was touched"))
    TE = targeteval.TargetEvaluator
    for bad, match in ((dict(B=0), "B 0"), (dict(B=True), "B True"), (dict(N=100), "N 100"), (dict(N=4000.0), "N 4000.0"),
                       (dict(spk_num="2"), "spk_num"), (dict(spk_num=17), "spk_num <= 16"),
                       (dict(precision="bf16s2"), "precision"), (dict(precision="mixed"), "precision"),
                       (dict(bgd_noise=np.zeros(N - 1)), "at least N"), (dict(bgd_noise=np.ones(N)), "constant"),
                       (dict(bgd_noise=np.zeros((2, N))), "1-D")):
        kw = dict(B=2, N=N)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            TE(net, vnet, mem, **kw)
    with pytest.raises(ValueError, match="E = 50"):
        TE(_net(emb=40), _vnet(emb=40), _mem(40), 2, N)
    with pytest.raises(ValueError, match="memory holds rows of 40"):
        TE(net, vnet, _mem(40), 2, N)
    # what EnrolledExtractor refuses
    with pytest.raises(ValueError, match="no cRM"):
        TE(_net(crm=True), vnet, mem, 2, N)
    with pytest.raises(ValueError, match="net.adjust"):
        TE(_net(adjust=True), vnet, mem, 2, N)
    with pytest.raises(ValueError, match="the encoder gives"):
        TE(net, _vnet(input_fre=65), mem, 2, N)
    with pytest.raises(ValueError, match="image encoder gives vectors of 40"):
        TE(net, inet40, mem, 2, N)
    # SepTrainer.eval_loss on a query trainer
    raw, gains, spk = torch.zeros(2, 2, N), torch.ones(2, 2), torch.zeros(2, 2, dtype=torch.int32)
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a kernel was called"))
    with pytest.raises(ValueError, match="TargetEvaluator.eval_loss"):
        tr.eval_loss(raw, gains, spk)


def test_evaluator_builds_and_checks_its_batches(monkeypatch):
    bgd = np.random.default_rng(1).standard_normal(N + 50) * 3 + 2
    ev = targeteval.TargetEvaluator(_net(), _vnet(), _mem(), 2, N, spk_num=1, bgd_noise=bgd)
    assert ev.spk_num == 2 and ev.T == 32 and ev.L == 3968 and ev.count == 0
    want = bgd[:N] - bgd[:N].mean()
    want = (want / np.abs(want).max()).astype(np.float32)
    assert np.array_equal(ev.bgd.numpy(), want) and np.abs(ev.bgd.numpy()).max() == 1.0
    assert targeteval.TargetEvaluator(_net(), _vnet(), None, 2, N, spk_num=3).spk_num == 3
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a kernel was called"))
    raw = torch.zeros(2, 3, N)  # the batch checks come before any launch: CPU tensors are refused first
    with pytest.raises(ValueError, match="on the device"):
        ev.evaluate(raw, None, ids=torch.zeros(2, dtype=torch.int32))


def test_prepare_background_is_numpys_arithmetic():
    rng = np.random.default_rng(4)
    clip = rng.standard_normal(5000) * 0.1 + 0.3
    bg = clip[:N].copy()
    bg -= np.mean(bg)
    bg /= np.max(np.abs(bg))
    assert np.array_equal(targeteval.prepare_background(clip, N), bg.astype(np.float32))
    assert np.array_equal(targeteval.prepare_background(torch.from_numpy(clip), N), bg.astype(np.float32))


# ------------------------------------------------------------------ the fourth header
def test_eval_header_parses_and_collides_with_no_other():
    with open(os.path.join(ROOT, "include", "dl4ss_eval.h")) as f:
        sigs, res, params, consts = _lib.parse_header(f.read(), "dl4ss_eval.h")
    assert set(sigs) == ENTRIES == set(EVAL.signatures) == set(_lib.exported_symbols("dl4ss_eval.h"))
    assert (sigs, res, params, consts) == EVAL
    P, I, LL = _lib.P, _lib.I, _lib.LL
    assert sigs["dl4ss_bss_gain"] == [P, P, P, P, I, I, I, I, P, LL, P, P, P]
    assert params["dl4ss_bss_gain"] == ("src", "est", "index", "n_eff", "M", "J", "Ke", "N", "ws", "ws_bytes", "crit",
                                        "singular", "stream")
    assert params["dl4ss_te_assemble"] == ("srcs", "lengths", "bgd", "B", "S", "N", "spk_num", "mix", "noise",
                                           "target", "mix_len", "stream")
    assert res["dl4ss_bss_gain_ws_bytes"] is LL and res["dl4ss_bss_gain"] is I and res["dl4ss_te_assemble"] is I
    assert params["dl4ss_bss_gain"][-1] == params["dl4ss_te_assemble"][-1] == "stream"
    assert consts == {"DL4SS_BSS_GAIN_MAX_SRC": 4, "DL4SS_BSS_GAIN_CHUNK": 4096}
    others = [h for name, h in _lib.HEADERS.items() if name != "dl4ss_eval.h"]
    assert len(others) >= 3 and not ENTRIES & {n for h in others for n in h.signatures}
    assert not set(consts) & {k for h in others for k in h.constants}
    # the first header's tables stay what dl4ss_hip.h declares
    with open(os.path.join(ROOT, "include", "dl4ss_hip.h")) as f:
        assert CORE == _lib.parse_header(f.read())
    assert _lib.exported_symbols("dl4ss_hip.h") == list(CORE.signatures)
    assert not ENTRIES & set(_lib.exported_symbols("dl4ss_hip.h"))


def test_the_library_exports_the_eval_entry_points_and_sizes_the_workspace():
    lib = _lib.lib()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes == EVAL.signatures[name] and fn.restype is EVAL.restypes[name]
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:  # (binutils present) exactly the declared symbols of targeteval.hip are exported
        exported = {ln.split()[-1] for ln in nm.stdout.splitlines()
                    if "dl4ss_bss_gain" in ln or "dl4ss_te_" in ln}
        assert exported == ENTRIES
    q = _lib.query
    assert q("dl4ss_bss_gain_ws_bytes", 3, 4096) == 3 * (48 + 32) * 8
    assert q("dl4ss_bss_gain_ws_bytes", M=3, N=4097) == 3 * (2 * 48 + 32) * 8
    assert q("dl4ss_bss_gain_ws_bytes", 0, 5) == 0 and q("dl4ss_bss_gain_ws_bytes", -1, 5) == -1
    assert q("dl4ss_bss_gain_ws_bytes", 1, 0) == -1


def test_a_header_that_declares_a_name_again_is_refused():
    """the rule _lib applies to every header at import (merge_headers): neither an entry point nor a constant of an
    earlier header may come back"""
    with open(os.path.join(ROOT, "include", "dl4ss_eval.h")) as f:
        text = f.read()
    again = text.replace("int dl4ss_te_assemble(", "int dl4ss_grad_sumsq(")
    doctored = _lib.Header(*_lib.parse_header(again, "dl4ss_eval.h"))
    assert set(doctored.signatures) & set(CORE.signatures) == {"dl4ss_grad_sumsq"}
    with pytest.raises(ValueError) as e:
        _lib.merge_headers({"dl4ss_hip.h": CORE, "dl4ss_eval.h": doctored})
    assert all(word in str(e.value) for word in ("dl4ss_grad_sumsq", "dl4ss_eval.h", "dl4ss_hip.h"))
    assert str(e.value).index("dl4ss_eval.h") < str(e.value).index("dl4ss_hip.h")  # the one that repeats, then the first
    # a constant: a second header that defines DL4SS_CLIP_MAX_PARTS after dl4ss_optim.h has
    optim = _lib.HEADERS["dl4ss_optim.h"]
    assert "DL4SS_CLIP_MAX_PARTS" in optim.constants
    redefines = _lib.Header(*_lib.parse_header(text + "\n#define DL4SS_CLIP_MAX_PARTS 8\n", "dl4ss_eval.h"))
    assert redefines.signatures == EVAL.signatures and redefines.constants == dict(EVAL.constants, DL4SS_CLIP_MAX_PARTS=8)
    with pytest.raises(ValueError) as e:
        _lib.merge_headers({"dl4ss_hip.h": CORE, "dl4ss_optim.h": optim, "dl4ss_eval.h": redefines})
    assert all(word in str(e.value) for word in ("DL4SS_CLIP_MAX_PARTS", "dl4ss_eval.h", "dl4ss_optim.h"))
    assert "dl4ss_hip.h" not in str(e.value)
    # the controls: the undoctored sets merge, into the tables _lib carries
    merged = _lib.merge_headers({"dl4ss_hip.h": CORE, "dl4ss_optim.h": optim, "dl4ss_eval.h": EVAL})
    assert len(merged.signatures) == 98 + 2 + 3 and merged.constants == {**CORE.constants, **optim.constants,
                                                                         **EVAL.constants}
    assert _lib.merge_headers(_lib.HEADERS) == (_lib.SIGNATURES, _lib.RESTYPES, _lib.PARAMS, _lib.CONSTANTS)
    with pytest.raises(TypeError, match="dl4ss_eval.h"):
        _lib.bind("dl4ss_bss_nothing", (), {})


# ------------------------------------------------------------------ weight snapshots
def test_snapshot_and_restore_round_trip():
    net, vnet, mem = _net(), _vnet(), _mem()
    mem.mem.copy_(torch.randn(7, 50, generator=torch.Generator().manual_seed(3)))
    want = (net.flat.clone(), vnet.flat.clone(), mem.mem.clone())
    snap = checkpoint.snapshot_weights(net, vnet, mem)
    gen = net.generation
    for t in (net.flat, vnet.flat, mem.mem):
        t.add_(1.0)
    assert not torch.equal(net.flat, want[0])
    for (_, _, saved), w in zip(snap, want):  # the snapshot is a copy, not a view
        assert torch.equal(saved, w)
    checkpoint.restore_weights(snap)
    assert all(torch.equal(a, b) for a, b in zip((net.flat, vnet.flat, mem.mem), want))
    assert net.generation == gen + 1  # params_changed(): trainers re-derive their bf16 copies
    checkpoint.restore_weights(snap)  # a snapshot restores any number of times
    assert torch.equal(net.flat, want[0])


def test_snapshot_of_a_trainer_covers_net_encoder_and_memory_but_no_optimizer_state():
    net, vnet = _net(), _vnet()
    memory = SpeakerMemory(101, 50, device="cpu")
    tr = engine.SepTrainer(net, 2, 2, N, voiceprint=vnet, memory=memory)
    snap = checkpoint.snapshot_weights(tr)
    assert [t.data_ptr() for _, t, _ in snap] == [net.flat.data_ptr(), vnet.flat.data_ptr(), memory.mem.data_ptr()]
    m0 = tr.m.clone()
    net.flat.zero_(); memory.mem.fill_(2.0); tr.m.fill_(5.0)
    key = tr._wb_key()
    checkpoint.restore_weights(snap)
    assert torch.equal(net.flat, snap[0][2]) and float(memory.mem.abs().max()) == 0.0
    assert torch.equal(tr.m, torch.full_like(m0, 5.0))  # optimizer state is not part of a snapshot
    assert tr._wb_key() != key and tr._wb_ver is None
    with pytest.raises(TypeError, match="neither flat parameters nor memory rows"):
        checkpoint.snapshot_weights(object())
