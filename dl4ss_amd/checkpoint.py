"""Checkpoint compatibility with the reference's per-module ``params/param_*`` files
(SURVEY section 8f row f4).

The reference saves one ``state_dict`` per module every 5 epochs
(``TDAA_beta/main_run_sstune_EvalVer.py:677-690``: ``..._hidden3d_{epoch}`` = MIX_SPEECH,
``_emblayer_`` = SPEECH_EMBEDDING, ``_adjlayer_`` = ADDJUST, ``_attlayer_`` = ATTENTION,
``_dislayer_`` = Discriminator) and loads them back the same way (``EvalVer.py:545-554``;
the classifier file drops its ``cnn`` keys, ``:547-549``).  The ``_attlayer_`` file is read
and written for nets with the 'align' attention (``SepNet(attention="align")``), whose three
weights it holds; a 'dot' net has none of them.  Key names inside each file are
the module's own: ``layer.weight_ih_l0[_reverse]`` / ``Linear.weight`` (MIX_SPEECH),
``layer.weight`` (embedding, ADDJUST), ``Linear_{1,2,3}.weight`` (attention).

Files are read with ``torch.load(..., weights_only=True)`` only (no arbitrary unpickling):
torch-0.3 / Python-2 files in the legacy (non-zip) format -- protocol-2 pickles of an
``OrderedDict`` of ``torch._utils._rebuild_tensor`` tensors over ``torch.cuda.FloatStorage``
persistent ids saved on ``cuda:N`` (fixture: ``tests/golden/legacy_py2_torch03``, built
opcode by opcode by ``tests/golden/make_legacy_ckpt.py``) -- load through the same safe
path; a file the safe loader refuses raises.  The flat parameter buffers of ``SepNet`` /
``ClassifierNet`` carry the same names under a module prefix (``mix.``, ``emb.``, ``adj.``),
so loading is a rename and a copy; ``save_reference_params`` writes the reference layout
back (one file per module, legacy-compatible keys).

Those files hold weights.  ``save_training_state`` / ``load_training_state`` (at the end of this module) hold a
whole run -- weights, optimizer moments and counts, schedules, the host RNG streams -- so that a run stopped
anywhere continues as the run that was never stopped ("Training state").
"""
import os
import random
import tempfile

import numpy as np
import torch

PREFIX = {"hidden3d": "mix.", "emblayer": "emb.", "adjlayer": "adj.", "attlayer": "att."}


def load_state(path):
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a state_dict")
    return {k: (v.data if hasattr(v, "data") else v) for k, v in sd.items()}


def load_reference_params(net, hidden3d=None, emblayer=None, adjlayer=None, strict=True, attlayer=None):
    """Load the reference's per-module files into a SepNet (in place).  Missing module files
    are skipped; with ``strict`` every key of a given file must map onto the net AND every
    parameter of the net under that file's module prefix must be in the file (torch's
    ``load_state_dict(strict=True)`` in both directions: a 2-layer hidden3d file does not
    silently leave layers 2-3 of a 4-layer net at their random init).  ``attlayer`` is the
    ATTENTION file (``Linear_{1,2,3}.weight``), for a net built with ``attention="align"``; a
    'dot' net has no counterpart for its keys, so a strict load of it raises."""
    for kind, path in (("hidden3d", hidden3d), ("emblayer", emblayer), ("adjlayer", adjlayer),
                       ("attlayer", attlayer)):
        if path is None:
            continue
        sd = load_state(path)
        if strict:
            want = {name[len(PREFIX[kind]):] for name, _ in net.specs if name.startswith(PREFIX[kind])}
            missing = sorted(want - set(sd))
            if missing:
                raise KeyError(f"{path}: missing {missing} for this net")
        for k, v in sd.items():
            name = PREFIX[kind] + k
            if name not in net.offsets:
                if strict:
                    raise KeyError(f"{path}: key {k!r} has no counterpart ({name}) in this net")
                continue
            dst = net.view(name)
            if tuple(dst.shape) != tuple(v.shape):
                raise ValueError(f"{path}: {k} has shape {tuple(v.shape)}, the net expects {tuple(dst.shape)}")
            dst.copy_(v.to(torch.float32))
    return net


def load_reference_classifier(cnet, path, strict=True):
    """MIX_SPEECH_classifier file into a ClassifierNet (the ``cnn`` keys dropped, EvalVer.py:547-549)."""
    sd = {k: v for k, v in load_state(path).items() if "cnn" not in k}
    if strict:
        missing = sorted({name for name, _ in cnet.specs} - set(sd))
        if missing:
            raise KeyError(f"{path}: missing {missing} for this classifier")
    for k, v in sd.items():
        if k not in cnet.offsets:
            if strict:
                raise KeyError(f"{path}: key {k!r} has no counterpart in the classifier")
            continue
        dst = cnet.view(k)
        if tuple(dst.shape) != tuple(v.shape):
            raise ValueError(f"{path}: {k} has shape {tuple(v.shape)}, the classifier expects {tuple(dst.shape)}")
        dst.copy_(v.to(torch.float32))
    return cnet


def save_reference_classifier(cnet, path):
    """A ClassifierNet as the reference saves its classifier (test_multi_labels_speech.py:447-449): one
    plain state_dict with the module's own keys (``layer.*`` / ``Linear.*``) on the CPU.  Round-trips
    through ``load_reference_classifier``; the driver mirrors' ``load_params(classifier=path)`` load it."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    torch.save({name: cnet.view(name).detach().cpu().clone() for name, _ in cnet.specs}, path)
    return path


DIS_KEYS = ("cnn.weight", "cnn.bias", "cnn1.weight", "cnn1.bias", "cnn2.weight", "cnn2.bias", "final.weight",
            "final.bias")


def load_reference_discriminator(module, path):
    """The reference's ``param_{tag}_dislayer_{epoch}`` file (main_run_sstune_dis.py:661-662: the
    Discriminator's plain ``state_dict``) into a ``myNet.Discriminator`` (in place).  The file must hold
    exactly the reference's eight keys with the module's shapes: a file saved at another map size
    (``final.weight`` is (1, 64 H3 W3)) raises instead of loading partly."""
    sd = load_state(path)
    if set(sd) != set(DIS_KEYS):
        raise KeyError(f"{path}: keys {sorted(sd)} are not the Discriminator's {list(DIS_KEYS)}")
    own = module.state_dict()
    for k in DIS_KEYS:
        if tuple(sd[k].shape) != tuple(own[k].shape):
            raise ValueError(f"{path}: {k} has shape {tuple(sd[k].shape)}, the module expects {tuple(own[k].shape)}")
    module.load_state_dict({k: sd[k].to(torch.float32) for k in DIS_KEYS})
    return module


def save_reference_discriminator(module, tag, epoch, directory="params"):
    """Write ``param_{tag}_dislayer_{epoch}`` as the reference does (dis.py:661-662): the module's
    state_dict on the CPU.  Round-trips through ``load_reference_discriminator``."""
    os.makedirs(directory, exist_ok=True)
    p = os.path.join(directory, f"param_{tag}_dislayer_{epoch}")
    torch.save({k: v.detach().cpu().clone() for k, v in module.state_dict().items()}, p)
    return p


def save_reference_params(net, directory, tag, epoch):
    """Write the reference's file layout ``param_{tag}_{hidden3d,emblayer,adjlayer}_{epoch}``, and
    ``param_{tag}_attlayer_{epoch}`` for a net that has the 'align' attention weights.  These files are plain
    state dicts of tensors under the reference's keys and have no place for metadata: ``net.gates`` is NOT
    written, so whoever loads them into a SepNet must build it with the ``gates`` the weights were trained with."""
    os.makedirs(directory, exist_ok=True)
    paths = {}
    for kind, pre in PREFIX.items():
        sd = {name[len(pre):]: net.view(name).detach().cpu().clone() for name, _ in net.specs if name.startswith(pre)}
        if not sd:
            continue
        p = os.path.join(directory, f"param_{tag}_{kind}_{epoch}")
        torch.save(sd, p)
        paths[kind] = p
    return paths


def save_voiceprint(path, vnet, memory):
    """The voiceprint encoder's parameters (``spk.layer.*``) and the speaker memory in one file: plain
    ``torch.save`` of the two state dicts (the Keras tree's weights have no torch layout to mirror), and beside
    them the encoder's cell form ``vnet.gates`` ("logistic" or "hard") as a plain string."""
    torch.save({"voiceprint": {k: v.cpu() for k, v in vnet.state_dict().items()},
                "memory": {k: v.cpu() for k, v in memory.state_dict().items()},
                "gates": str(getattr(vnet, "gates", "logistic"))}, path)


def load_voiceprint(path, vnet, memory):
    """Load a save_voiceprint file into ``vnet`` and ``memory`` (in place; shapes must match).  The file's
    ``gates`` (a file from before the field: "logistic") must be ``vnet.gates``: weights trained through one cell
    form are not weights of the other, so a mismatch raises ValueError before anything is written."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict) or set(sd) - {"gates"} != {"voiceprint", "memory"}:
        raise ValueError(f"{path}: not a save_voiceprint file")
    gates, own = sd.get("gates", "logistic"), getattr(vnet, "gates", "logistic")
    if gates not in ("logistic", "hard"):
        raise ValueError(f"{path}: gates {gates!r}, expected 'logistic' or 'hard'")
    if gates != own:
        raise ValueError(f"{path}: saved from an encoder with gates={gates!r}, this VoiceprintNet has gates={own!r}")
    for name, shape in vnet.specs:
        if name not in sd["voiceprint"] or tuple(sd["voiceprint"][name].shape) != tuple(shape):
            raise ValueError(f"{path}: {name} missing or not of shape {tuple(shape)}")
    mem = sd["memory"].get("mem") if isinstance(sd["memory"], dict) else None
    if mem is None or tuple(mem.shape) != (memory.M, memory.E):  # before either is written
        raise ValueError(f"{path}: mem missing or not of shape {(memory.M, memory.E)}")
    vnet.load_state_dict(sd["voiceprint"])
    memory.load_state_dict(sd["memory"])


def save_image_query(path, inet, memory):
    """The image-query encoder's parameters (``img.*``) and the speaker memory in one file (as save_voiceprint)."""
    torch.save({"image_query": {k: v.cpu() for k, v in inet.state_dict().items()},
                "memory": {k: v.cpu() for k, v in memory.state_dict().items()}}, path)


def load_image_query(path, inet, memory):
    """Load a save_image_query file into ``inet`` and ``memory`` (in place; shapes must match)."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict) or set(sd) != {"image_query", "memory"}:
        raise ValueError(f"{path}: not a save_image_query file")
    for name, shape in inet.specs:
        if name not in sd["image_query"] or tuple(sd["image_query"][name].shape) != tuple(shape):
            raise ValueError(f"{path}: {name} missing or not of shape {tuple(shape)}")
    mem = sd["memory"].get("mem") if isinstance(sd["memory"], dict) else None
    if mem is None or tuple(mem.shape) != (memory.M, memory.E):  # before either is written
        raise ValueError(f"{path}: mem missing or not of shape {(memory.M, memory.E)}")
    inet.load_state_dict(sd["image_query"])
    memory.load_state_dict(sd["memory"])


# --------------------------------------------------------------------------- Keras 1's LSTM weights
KERAS_GATES = ("i", "f", "c", "o")  # this project's row blocks [i | f | g | o]; Keras names the candidate g "c"
KERAS_LSTM_NAMES = tuple(f"{k}_{g}" for g in KERAS_GATES for k in ("W", "U", "b"))


def _keras_layer(net, layer, direction):
    if getattr(net, "gates", "logistic") != "hard":
        raise ValueError("Keras 1's LSTM weights belong to a net with gates='hard' (its cell), this net has "
                         f"gates={getattr(net, 'gates', 'logistic')!r}")
    if not 0 <= int(layer) < net.L:
        raise ValueError(f"layer {layer}: the net has layers 0..{net.L - 1}")
    if direction not in ("forward", "backward"):
        raise ValueError(f"direction {direction!r}: expected 'forward' or 'backward'")
    sfx = f"_l{int(layer)}" + ("_reverse" if direction == "backward" else "")
    return {kind: net.view(f"{net.layer_prefix}{kind}{sfx}") for kind in ("weight_ih", "weight_hh", "bias_ih",
                                                                         "bias_hh")}


def load_keras_lstm(net, layer, direction, weights):
    """One direction of one layer of Keras 1's ``Bidirectional(LSTM(...))`` (DL4SS_Keras/nnet.py:51-68) into a
    ``SepNet`` or ``VoiceprintNet`` built with ``gates="hard"`` (in place).  ``direction``: "forward" or "backward"
    (the wrapper's two LSTMs; "backward" is this project's ``_reverse``).  ``weights`` maps Keras 1's per-gate
    names to arrays (numpy or torch): ``W_i, U_i, b_i, W_f, U_f, b_f, W_c, U_c, b_c, W_o, U_o, b_o`` with
    ``W_*`` (in, H), ``U_*`` (H, H), ``b_*`` (H,).  The mapping is by NAME, never by list position (Keras 1.x
    releases order ``get_weights()`` differently): ``weight_ih`` rows [i | f | g (Keras's c) | o] = ``W_*^T``,
    ``weight_hh`` = ``U_*^T``, ``bias_ih`` = ``b_*``, ``bias_hh`` = 0 (Keras has one bias).  Every name must be
    present with the layer's shape, and no other; nothing is written before all are checked.  Reading the arrays
    out of an ``.h5`` file is the caller's (h5py is not a dependency)."""
    p = _keras_layer(net, layer, direction)
    H, D = net.H, p["weight_ih"].shape[1]
    if set(weights) != set(KERAS_LSTM_NAMES):
        raise ValueError(f"weights: names {sorted(weights)} are not Keras 1's {sorted(KERAS_LSTM_NAMES)}")
    want = {"W": (D, H), "U": (H, H), "b": (H,)}
    t = {}
    for name in KERAS_LSTM_NAMES:
        t[name] = torch.as_tensor(weights[name]).detach().to("cpu", torch.float32)
        if tuple(t[name].shape) != want[name[0]]:
            raise ValueError(f"weights: {name} has shape {tuple(t[name].shape)}, the layer expects {want[name[0]]}")
    for q, g in enumerate(KERAS_GATES):
        rows = slice(q * H, (q + 1) * H)
        p["weight_ih"][rows].copy_(t[f"W_{g}"].t())
        p["weight_hh"][rows].copy_(t[f"U_{g}"].t())
        p["bias_ih"][rows].copy_(t[f"b_{g}"])
    p["bias_hh"].zero_()
    if hasattr(net, "params_changed"):
        net.params_changed()
    return net


def export_keras_lstm(net, layer, direction):
    """The inverse of load_keras_lstm: a dict of the twelve per-gate arrays (CPU fp32 tensors) of one direction of
    one layer of a ``gates="hard"`` net.  Keras's cell has one bias, so ``bias_hh`` must be exactly zero (as
    load_keras_lstm leaves it): a layer trained here with both biases is refused rather than folded silently --
    add ``bias_hh`` into ``bias_ih`` and zero it first (the cell's sum b_ih + b_hh is unchanged up to one
    rounding)."""
    p = _keras_layer(net, layer, direction)
    H = net.H
    if bool((p["bias_hh"] != 0).any()):
        raise ValueError("export_keras_lstm: bias_hh is not zero; Keras's LSTM has one bias (fold bias_hh into "
                         "bias_ih and zero it first)")
    out = {}
    for q, g in enumerate(KERAS_GATES):
        rows = slice(q * H, (q + 1) * H)
        out[f"W_{g}"] = p["weight_ih"][rows].detach().cpu().t().contiguous()
        out[f"U_{g}"] = p["weight_hh"][rows].detach().cpu().t().contiguous()
        out[f"b_{g}"] = p["bias_ih"][rows].detach().cpu().clone()
    return out


# --------------------------------------------------------------------------- in-memory weight snapshots
def _weight_tensors(obj):
    """(owner to notify, tensor) of everything in ``obj`` that Keras's save_weights would cover: a net's or an
    encoder's flat parameter buffer, a SpeakerMemory's rows (a layer weight there), or those of a trainer's net,
    query encoder and memory."""
    if hasattr(obj, "mem") and isinstance(obj.mem, torch.Tensor):  # SpeakerMemory
        return [(None, obj.mem)]
    if hasattr(obj, "flat") and isinstance(obj.flat, torch.Tensor):  # SepNet, VoiceprintNet, ImageQueryNet, ...
        return [(obj, obj.flat)]
    if hasattr(obj, "net") and hasattr(obj, "opt"):  # a trainer: its net, its query encoder, its memory
        out = [(obj, obj.net.flat)]
        for name in ("vnet", "inet"):
            sub = getattr(obj, name, None)
            if sub is not None:
                out.append((sub, sub.flat))
        if getattr(obj, "memory", None) is not None:
            out.append((None, obj.memory.mem))
        return out
    raise TypeError(f"snapshot_weights: {type(obj).__name__} has neither flat parameters nor memory rows")


def snapshot_weights(*objs):
    """Copies, on the tensors' own device, of the flat parameter buffers of the given nets / encoders / trainers and
    of ``SpeakerMemory.mem`` -- what the Keras trees' ``save_weights`` covers at a new lowest validation loss
    (nnet.py:160-165).  Optimizer state is not part of it (``save_training_state`` writes a whole run to a file).
    Give the result to ``restore_weights``."""
    snap = []
    for obj in objs:
        for owner, t in _weight_tensors(obj):
            snap.append((owner, t, t.detach().clone()))
    return snap


def restore_weights(snap):
    """Copy a ``snapshot_weights`` result back into the tensors it was taken from (nnet.py:166-169) and call
    ``params_changed()`` on every owner that has it (a trainer re-derives its bf16 weight copies)."""
    for owner, t, saved in snap:
        t.copy_(saved)
        if owner is not None and hasattr(owner, "params_changed"):
            owner.params_changed()


# --------------------------------------------------------------------------- training state: save and resume a run
TRAINING_STATE_FORMAT = "dl4ss-training-state"
TRAINING_STATE_VERSION = 1


def _check_plain(x, where):
    """The file holds tensors and plain containers of str, int, float, bool and None only (what
    ``torch.load(weights_only=True)`` reads back without an allow-list): TypeError naming the first thing that is
    not."""
    if x is None or isinstance(x, (str, int, float, bool, torch.Tensor)):
        return
    if isinstance(x, dict):
        for k, v in x.items():
            if not isinstance(k, str):
                raise TypeError(f"{where}: key {k!r} is not a str")
            _check_plain(v, f"{where}.{k}")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            _check_plain(v, f"{where}[{i}]")
    else:
        raise TypeError(f"{where}: a {type(x).__name__} cannot go into a training-state file (tensors and plain "
                        "containers of str, int, float, bool and None only)")


def _rng_state():
    """Python ``random``, NumPy's global generator and torch's CPU generator (what the compat loaders draw from),
    the two Mersenne Twister key arrays as int64 tensors."""
    ver, key, gauss = random.getstate()
    name, nkey, pos, has_gauss, cached = np.random.get_state()
    return {"python": {"version": int(ver), "key": torch.tensor(key, dtype=torch.int64), "gauss_next": gauss},
            "numpy": {"name": str(name), "key": torch.from_numpy(nkey.astype(np.int64)), "pos": int(pos),
                      "has_gauss": int(has_gauss), "cached_gaussian": float(cached)},
            "torch": torch.get_rng_state().clone()}


def _check_rng_state(sd, path):
    own = _rng_state()
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: rng: the file holds no generator states (saved with rng=False)")
    for gen in ("python", "numpy"):
        if not isinstance(sd.get(gen), dict):
            raise ValueError(f"{path}: rng.{gen}: not in the file")
        for k in ("version", "name"):
            if k in own[gen] and sd[gen].get(k) != own[gen][k]:
                raise ValueError(f"{path}: rng.{gen}.{k}: the file has {sd[gen].get(k)!r}, this process has "
                                 f"{own[gen][k]!r}")
        key = sd[gen].get("key")
        if not isinstance(key, torch.Tensor) or key.dtype != torch.int64 or key.shape != own[gen]["key"].shape \
                or int(key.min()) < 0 or int(key.max()) >= 2 ** 32:
            raise ValueError(f"{path}: rng.{gen}.key: not a Mersenne Twister key of {own[gen]['key'].numel()} words")
    g = sd["python"].get("gauss_next")
    if g is not None and not isinstance(g, float):
        raise ValueError(f"{path}: rng.python.gauss_next: {g!r} is neither None nor a float")
    for k, types in (("pos", int), ("has_gauss", int), ("cached_gaussian", float)):
        if not isinstance(sd["numpy"].get(k), types):
            raise ValueError(f"{path}: rng.numpy.{k}: {sd['numpy'].get(k)!r} is not a {types.__name__}")
    t = sd.get("torch")
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.shape != own["torch"].shape:
        raise ValueError(f"{path}: rng.torch: not a CPU generator state of {own['torch'].numel()} bytes")


def _set_rng_state(sd):
    p, n = sd["python"], sd["numpy"]
    random.setstate((p["version"], tuple(int(x) for x in p["key"].tolist()), p["gauss_next"]))
    np.random.set_state((n["name"], n["key"].numpy().astype(np.uint32), n["pos"], n["has_gauss"], n["cached_gaussian"]))
    torch.set_rng_state(sd["torch"])


def save_training_state(path, trainer, schedule=None, stopper=None, rng=True, extra=None):
    """Write everything a run needs to continue as if it had not stopped, into one file: ``trainer.state_dict()``
    (a ``SepTrainer`` or ``ClassifierTrainer``: weights, optimizer moments, applied-update and skipped counts, lr,
    and of the parts it has the Discriminator and its Adam or the query encoder, its optimizer and the speaker
    memory), the states of ``schedule`` (``schedule.LRHalving``) and ``stopper`` (``schedule.EarlyStopping``), with
    ``rng`` the host generators the ``compat`` loaders draw from (Python ``random``, NumPy's global one, torch's
    CPU one) and ``extra``, the caller's own small dict of primitives (epoch, batch index, list position, paths of
    best-epoch snapshots).

    Batch size, ``precision``, ``mode``, eager or graph and world size are deliberately NOT part of the state: a
    run may continue at another batch size or precision.  Data parallel: the state is the same on every rank (the
    same all-reduced gradient, the same counts), so one rank saves and every rank loads that file; no broadcast.

    The trainer must be settled: this synchronises, and raises RuntimeError (run ``check()`` first) while a status
    word is non-zero or a non-finite refusal is pending -- step_count would still count refused updates.  The file
    holds tensors and plain containers only and is written atomically: to a temporary name in ``path``'s directory,
    flushed, then ``os.replace``; a save that fails leaves the previous file as it was and no temporary behind."""
    payload = {"format": TRAINING_STATE_FORMAT, "version": TRAINING_STATE_VERSION, "trainer": trainer.state_dict(),
               "schedule": None if schedule is None else schedule.state_dict(),
               "stopper": None if stopper is None else stopper.state_dict(),
               "rng": _rng_state() if rng else None, "extra": dict(extra) if extra else {}}
    _check_plain(payload, "state")
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    fd, tmp = tempfile.mkstemp(dir=d, prefix=os.path.basename(path) + ".", suffix=".tmp")
    try:
        with os.fdopen(fd, "wb") as f:
            torch.save(payload, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return path


def load_training_state(path, trainer, schedule=None, stopper=None, rng=True):
    """Load a ``save_training_state`` file into ``trainer`` (and ``schedule``, ``stopper``, the host generators) in
    place and return the saved ``extra`` dict.  Read with ``torch.load(..., weights_only=True)``: a file the safe
    loader refuses raises.  Everything is validated before anything is written -- format, version, the nets'
    layouts (parameter names and shapes in order, cell, gates, attention, crm, adjust), each optimizer's kind and
    hyper-parameters, a part (adversary, voiceprint, image query) on one side only, the memory's shape, a
    ``schedule`` / ``stopper`` / ``rng`` asked for that the file does not hold: ValueError naming the field and both
    values, with every buffer, counter and generator as it was.  ``lr`` is state and is restored.  Batch size,
    precision, mode, eager or graph and world size are not part of the state and may differ from the saving run's.
    A ``schedule`` or ``stopper`` in the file that the caller does not pass is left unread.

    The buffers are written by ``copy_``: a graph captured before the load stays valid and replays on the loaded
    state, and the bf16 weight copies are converted again by the next step."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict) or sd.get("format") != TRAINING_STATE_FORMAT:
        raise ValueError(f"{path}: format: the file has {sd.get('format') if isinstance(sd, dict) else None!r}, "
                         f"expected {TRAINING_STATE_FORMAT!r}")
    v = sd.get("version")
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= TRAINING_STATE_VERSION:
        raise ValueError(f"{path}: version: the file has {v!r}, this code reads versions 1..{TRAINING_STATE_VERSION}")
    try:
        trainer.check_state_dict(sd.get("trainer"))
        if schedule is not None:
            schedule.check_state_dict(sd.get("schedule"))
        if stopper is not None:
            stopper.check_state_dict(sd.get("stopper"))
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
    if rng:
        _check_rng_state(sd.get("rng"), path)
    extra = sd.get("extra")
    if not isinstance(extra, dict):
        raise ValueError(f"{path}: extra: the file has {type(extra).__name__}, expected a dict")
    trainer.load_state_dict(sd["trainer"], checked=True)
    if schedule is not None:
        schedule.load_state_dict(sd["schedule"], checked=True)
    if stopper is not None:
        stopper.load_state_dict(sd["stopper"], checked=True)
    if rng:
        _set_rng_state(sd["rng"])
    return extra
