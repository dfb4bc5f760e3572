"""The image-query path's host surface without a GPU: the second public header and its binding, what
SepTrainer(image_query=..., memory=...) refuses (before any device call: the nets live on the CPU, nothing here can
launch), ImageQueryNet's names and shapes, and save_image_query / load_image_query."""
import os
import subprocess

import pytest
import torch

import imagequery_ref as ir
from dl4ss_amd import _lib, checkpoint, engine, infer, ops, plan, synth
from dl4ss_amd.imagequery import ImageQueryEncoder, ImageQueryNet
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4000  # 32 frames
ENTRIES = {"dl4ss_imgq_param_count", "dl4ss_imgq_dense_in", "dl4ss_imgq_fwd", "dl4ss_imgq_bwd", "dl4ss_imgq_reduce",
           "dl4ss_imgq_guard"}
CORE, IMGQ = _lib.HEADERS["dl4ss_hip.h"], _lib.HEADERS["dl4ss_imgq.h"]


def _net(**kw):
    kw.setdefault("adjust", False)
    return engine.SepNet(cell="gru", num_layers=1, device="cpu", seed=1, **kw)


def _iq(**kw):
    return ImageQueryNet(device="cpu", seed=2, **kw)


def _mem(emb=50):
    return SpeakerMemory(101, emb, device="cpu")


# ---- the header and the binding ----
def test_header_parses_and_the_library_exports_it():
    with open(os.path.join(ROOT, "include", "dl4ss_imgq.h")) as f:
        sigs, res, params, consts = _lib.parse_header(f.read())
    assert set(sigs) == ENTRIES == set(IMGQ.signatures) == set(_lib.exported_symbols("dl4ss_imgq.h"))
    assert (sigs, res, params, consts) == IMGQ
    assert ENTRIES <= set(_lib.exported_symbols()) and consts.items() <= _lib.CONSTANTS.items()
    P, I, LL = _lib.P, _lib.I, _lib.LL
    assert sigs["dl4ss_imgq_fwd"] == [P, P, I, I, I, I, P, P]
    assert params["dl4ss_imgq_bwd"] == ("images", "dvec", "params", "n", "h", "w", "E", "dpart", "ld",
                                        "dpart_floats", "stream")
    assert sigs["dl4ss_imgq_bwd"] == [P, P, P, I, I, I, I, P, LL, LL, P]
    assert res["dl4ss_imgq_param_count"] is LL and res["dl4ss_imgq_fwd"] is I
    assert consts["DL4SS_IMGQ_MIN_HW"] == 24 and consts["DL4SS_IMGQ_MAX_HW"] >= 48
    assert consts["DL4SS_IMGQ_MAX_E"] == 128 and consts["DL4SS_IMGQ_MAX_N"] == 1024
    lib = _lib.lib()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes == sigs[name] and fn.restype is res[name]
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:  # (binutils present) exactly the declared dl4ss_imgq_ symbols are exported
        exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if "dl4ss_imgq_" in ln}
        assert exported == ENTRIES


def test_a_library_without_the_second_header_loads_and_a_call_names_the_symbol(monkeypatch):
    """A stand-in with the core header's names alone (what tests/test_lib_bind_cpu.py binds) loads; an image-query
    call on it fails in the symbol lookup, by name."""
    import types

    class Old(types.SimpleNamespace):
        def __getattr__(self, name):
            raise AttributeError(f"undefined symbol: {name}")

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Old(
        hipGetErrorString=types.SimpleNamespace(), **{n: types.SimpleNamespace() for n in CORE.signatures}))
    lib = _lib._load()
    assert lib.dl4ss_attn_nblk.argtypes == [_lib.I, _lib.I]
    with pytest.raises(AttributeError, match="dl4ss_imgq_param_count"):
        _lib.query("dl4ss_imgq_param_count", 28, 28, 50)
    with pytest.raises(AttributeError, match="dl4ss_imgq_fwd"):
        _lib.call("dl4ss_imgq_fwd", None, None, 1, 28, 28, 50, None, None)
    monkeypatch.setattr(_lib, "_lib", None)  # (the next _load binds the real library again)


def test_first_header_tables_are_untouched():
    with open(os.path.join(ROOT, "include", "dl4ss_hip.h")) as f:
        assert CORE == _lib.parse_header(f.read())
    assert not any(n.startswith("dl4ss_imgq_") for n in CORE.signatures)
    assert not any(n.startswith("DL4SS_IMGQ_") for n in CORE.constants)
    assert _lib.exported_symbols("dl4ss_hip.h") == list(CORE.signatures)
    assert not ENTRIES & set(_lib.exported_symbols("dl4ss_hip.h"))


def test_bind_orders_keywords_and_refuses_unknown_names():
    want = ("im", "pa", 3, 28, 28, 50, "ve", "st")
    kw = dict(zip(IMGQ.params["dl4ss_imgq_fwd"], want))
    assert _lib.bind("dl4ss_imgq_fwd", (), dict(reversed(kw.items()))) == want
    assert _lib.bind("dl4ss_imgq_fwd", want[:2], {k: kw[k] for k in ("stream", "vec", "E", "w", "h", "n")}) == want
    with pytest.raises(TypeError, match="'vec'") as e:
        _lib.bind("dl4ss_imgq_fwd", want[:6], dict(stream="st"))
    assert "dl4ss_imgq_fwd" in str(e.value)
    with pytest.raises(TypeError, match="'out'"):
        _lib.bind("dl4ss_imgq_fwd", want[:6], dict(out="ve", stream="st"))
    with pytest.raises(TypeError, match="9 given"):
        _lib.bind("dl4ss_imgq_fwd", want + (0,), {})
    with pytest.raises(TypeError, match="dl4ss_imgq_nothing"):
        _lib.bind("dl4ss_imgq_nothing", (), {})
    with pytest.raises(TypeError, match="dl4ss_imgq_nothing"):
        _lib.call("dl4ss_imgq_nothing", 1, 2)


def test_size_queries():
    assert ops.imgq_param_count(28, 28, 50) == 2418
    assert ops.imgq_param_count(24, 24, 50) == 2418 and ops.imgq_param_count(26, 37, 50) == 1568 + 32 * 50 + 50
    assert _lib.query("dl4ss_imgq_dense_in", h=26, w=37) == 32
    for h, w, E in ((23, 28, 50), (28, 23, 50), (28, 49, 50), (28, 28, 0), (28, 28, 129)):
        assert _lib.query("dl4ss_imgq_param_count", h, w, E) == -1
        with pytest.raises(ValueError, match="image query"):
            ops.imgq_param_count(h, w, E)
    for size in ((28, 28), (24, 24), (26, 37), (48, 48), (31, 45)):  # the reference's own shape rule
        c, h3, w3 = ir.stage_shapes(*size)[-1]
        assert _lib.query("dl4ss_imgq_dense_in", size[0], size[1]) == c * h3 * w3


# ---- the net ----
def test_image_query_net_names_shapes_and_count():
    inet = _iq()
    assert (inet.h, inet.w, inet.E, inet.D, inet.image_size) == (28, 28, 50, 16, (28, 28))
    want = ir.param_shapes(28, 28, 50)
    assert [n for n, _ in inet.named_parameters()] == list(ir.NAMES) == list(want)
    assert {k: tuple(t.shape) for k, t in inet.state_dict().items()} == want
    assert inet.num_params == 2418 == sum(t.numel() for _, t in inet.named_parameters())
    assert inet.numel == 2420 and inet.grad.shape == inet.flat.shape and tuple(inet.grad_view("img.conv2.bias").shape) == (8,)
    c = IMGQ.constants  # the flat layout is the kernels' parameter block
    assert inet.offsets["img.conv3.weight"][0] == c["DL4SS_IMGQ_OFF_W3"] == 400
    assert inet.offsets["img.dense.weight"][0] == c["DL4SS_IMGQ_OFF_WD"] == c["DL4SS_IMGQ_CONV_PARAMS"] == 1568
    assert inet.offsets["img.dense.bias"][0] == 1568 + 800
    big = _iq(image_size=(26, 37), emb=128)
    assert big.D == 32 and big.num_params == 1568 + 32 * 128 + 128 == big.numel


def test_initialisation():
    inet = _iq()
    for i, (ci, co, k) in enumerate(((1, 4, 5), (4, 8, 3), (8, 16, 3)), 1):
        w = inet.view(f"img.conv{i}.weight")
        lim = (6.0 / ((ci + co) * k * k)) ** 0.5  # Glorot uniform
        assert float(w.abs().max()) <= lim and float(w.abs().max()) > 0.7 * lim
        assert float(inet.view(f"img.conv{i}.bias").abs().max()) == 0
    d = inet.view("img.dense.weight")
    assert 0.04 < float(d.std()) < 0.06 and float(inet.view("img.dense.bias").abs().max()) == 0
    assert torch.equal(_iq().flat, inet.flat) and not torch.equal(ImageQueryNet(device="cpu", seed=3).flat, inet.flat)


def test_net_and_encoder_argument_checks():
    for kw in (dict(image_size=(23, 28)), dict(image_size=(28, 49)), dict(emb=0), dict(emb=129)):
        with pytest.raises(ValueError):
            _iq(**kw)
    with pytest.raises(ValueError):
        ImageQueryEncoder(object(), 2)
    with pytest.raises(ValueError):
        ImageQueryEncoder(_iq(), 0)
    with pytest.raises(ValueError):
        ImageQueryEncoder(_iq(), 1025)


def test_state_dict_and_checkpoint_round_trip(tmp_path):
    a, m = _iq(), _mem()
    m.mem.copy_(torch.randn(101, 50, generator=torch.Generator().manual_seed(4)))
    p = str(tmp_path / "iq.pt")
    checkpoint.save_image_query(p, a, m)
    b, m2 = ImageQueryNet(device="cpu", seed=9), _mem()
    checkpoint.load_image_query(p, b, m2)
    assert torch.equal(b.flat, a.flat) and torch.equal(m2.mem, m.mem)
    with pytest.raises(ValueError):  # another encoder shape
        checkpoint.load_image_query(p, _iq(image_size=(26, 37)), _mem())
    c = ImageQueryNet(device="cpu", seed=9)
    w = c.flat.clone()
    with pytest.raises(ValueError):  # another memory size: refused before either is written
        checkpoint.load_image_query(p, c, SpeakerMemory(7, 50, device="cpu"))
    assert torch.equal(c.flat, w)
    vp = str(tmp_path / "vp.pt")
    checkpoint.save_voiceprint(vp, VoiceprintNet(device="cpu"), _mem())
    with pytest.raises(ValueError, match="save_image_query"):
        checkpoint.load_image_query(vp, c, _mem())


# ---- the trainer's refusals ----
CASES = {
    "mode": (dict(mode="pit"), {}, "image_query: mode"),
    "crm": (dict(mode="crm"), dict(crm=True), "image_query: (mode|a cRM)"),
    "crm_net": ({}, dict(crm=True), "image_query: a cRM"),
    "adjust": ({}, dict(adjust=True), "image_query: net.adjust"),
    "emb": ({}, dict(emb=40), "image_query: the encoder's vectors have 50 elements"),
    "precision": (dict(precision="bf16"), {}, "image_query: precision"),
    "loss_channels": (dict(loss_channels=101), {}, "image_query: loss_channels"),
    "process_group": (dict(process_group=object()), {}, "image_query: no data-parallel"),
    "clip_norm": (dict(clip_norm=200.0), {}, "image_query: clip_norm"),
    "refresh": (dict(memory_refresh="never"), {}, "memory_refresh"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_trainer_refuses(case):
    kw, nkw, reason = CASES[case]
    with pytest.raises(ValueError, match=reason):
        engine.SepTrainer(_net(**nkw), 2, 2, N, image_query=_iq(), memory=_mem(), **kw)


def test_trainer_refuses_adversary_and_halves_and_types():
    disc = engine.DiscNet(32, 129, device="cpu")
    with pytest.raises(ValueError, match="image_query: an adversary"):
        engine.SepTrainer(_net(), 2, 2, N, image_query=_iq(), memory=_mem(), adversary=disc)
    with pytest.raises(ValueError, match="image_query: the encoder needs memory="):
        engine.SepTrainer(_net(), 2, 2, N, image_query=_iq())
    with pytest.raises(ValueError, match="together with voiceprint="):
        engine.SepTrainer(_net(), 2, 2, N, image_query=_iq(), voiceprint=VoiceprintNet(device="cpu"), memory=_mem())
    with pytest.raises(ValueError, match="memory: a SpeakerMemory needs voiceprint="):  # memory= with neither
        engine.SepTrainer(_net(), 2, 2, N, memory=_mem())
    with pytest.raises(ValueError, match="ImageQueryNet"):
        engine.SepTrainer(_net(), 2, 2, N, image_query=object(), memory=_mem())
    with pytest.raises(ValueError, match="SpeakerMemory"):
        engine.SepTrainer(_net(), 2, 2, N, image_query=_iq(), memory=object())
    with pytest.raises(ValueError, match="rows of 40"):
        engine.SepTrainer(_net(), 2, 2, N, image_query=_iq(), memory=_mem(40))
    with pytest.raises(ValueError, match="1024"):
        engine.SepTrainer(_net(), 600, 2, N, image_query=_iq(), memory=_mem())


@pytest.mark.parametrize("which", ["image_query", "memory"])
def test_trainer_refuses_another_device(which):
    """The net on the CPU, the encoder or the memory declared on another device: refused by name, before any
    buffer is built (check_args reads .device alone)."""
    iq, mem = _iq(), _mem()
    (iq if which == "image_query" else mem).device = torch.device("cuda", 1)
    with pytest.raises(ValueError, match=f"{which}: lives on another device than the net"):
        engine.SepTrainer(_net(), 2, 2, N, image_query=iq, memory=mem)
    with pytest.raises(ValueError, match=f"{which}: lives on another device than the net"):
        plan.check_args(_net(), 2, 2, N, "label", "fp32", None, None, None, None, None, None, None, mem, "reference",
                        inet=iq)
    # the same index of another device type is another device too; both on the net's device pass
    iq2, mem2 = _iq(), _mem()
    (iq2 if which == "image_query" else mem2).device = torch.device("meta")
    with pytest.raises(ValueError, match=f"{which}: lives on another device than the net"):
        plan.check_args(_net(), 2, 2, N, "label", "fp32", None, None, None, None, None, None, None, mem2,
                        "reference", inet=iq2)
    assert plan.check_args(_net(), 2, 2, N, "label", "fp32", None, None, None, None, None, None, None, _mem(),
                           "reference", inet=_iq()) == (None, None)


def test_check_args_runs_before_any_device_call(monkeypatch):
    """plan.check_args alone, with the library out of reach: every refusal is a host check."""
    monkeypatch.setattr(_lib, "_load", lambda: pytest.fail("the library was touched"))
    net, iq, mem = _net(), _iq(), _mem()
    args = (net, 2, 2, N, "label", "fp32", None, None, None, None, None, None, None, mem, "reference")
    assert plan.check_args(*args, inet=iq) == (None, None)
    with pytest.raises(ValueError, match="image_query: mode"):
        plan.check_args(net, 2, 2, N, "pit", *args[5:], inet=iq)
    with pytest.raises(ValueError, match="image_query: the encoder needs memory="):
        plan.check_args(*args[:13], None, "reference", inet=iq)


def test_trainer_builds_takes_images_and_refuses_graph_capture():
    tr = engine.SepTrainer(_net(), 2, 2, N, image_query=_iq(), memory=_mem(), memory_refresh="reuse",
                           image_query_lr=1e-3)
    assert tr.vp_lr == 1e-3 and tr.vp_enc.n == 4 and tr.vp.status is tr.status and tr.vnet is None
    assert tuple(tr.images.shape) == (2, 2, 28, 28)
    assert engine.SepTrainer(_net(), 2, 2, N, image_query=_iq(), memory=_mem(), lr=3e-4).vp_lr == 3e-4
    raw, gains, spk = torch.zeros(2, 2, N), torch.ones(2, 2), torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="image-query"):
        tr.capture()
    with pytest.raises(NotImplementedError, match="image-query"):
        tr.step_graph(raw, gains, spk)
    with pytest.raises(ValueError, match="needs images="):  # required with image_query=
        tr.step(raw, gains, spk)
    with pytest.raises(ValueError, match="expected"):
        tr.step(raw, gains, spk, images=torch.zeros(2, 2, 24, 24))
    imgs = torch.from_numpy(synth.glyphs(4).templates).view(2, 2, 28, 28)
    tr.set_images(imgs)
    assert torch.equal(tr.images, imgs)
    plain = engine.SepTrainer(_net(), 2, 2, N)
    assert plain.inet is None and plain.images is None and not hasattr(plain, "vp_enc")
    with pytest.raises(ValueError, match="image_query="):  # images= without image_query=: before anything runs
        plain.step(raw, gains, spk, images=imgs)


def test_enrolled_extractor_takes_an_image_query_net():
    ex = infer.EnrolledExtractor(_net(), _iq(), 2, 32, 2)
    assert ex.by_image
    with pytest.raises(ValueError, match="queries of 50"):
        infer.EnrolledExtractor(_net(), _iq(emb=40), 2, 32, 2)
    with pytest.raises(ValueError, match="adjust"):
        infer.EnrolledExtractor(_net(adjust=True), _iq(), 2, 32, 2)
    imgs = torch.zeros(4, 28, 28)
    for kw in (dict(rule="gt"), dict(thr=0.5), dict(lengths=torch.zeros(4, dtype=torch.int32))):
        with pytest.raises(ValueError, match="image encoder"):  # the frame mask's arguments: before any launch
            ex.enrol(imgs, **kw)


def test_glyphs():
    g = synth.glyphs(6, (26, 37), seed=2)
    t = g.templates
    assert t.shape == (6, 26, 37) and t.dtype.name == "float32" and t.min() == 0.0 and t.max() <= 1.0
    assert (t == 0).mean() > 0.6 and all((t[i] > 0).sum() > 20 for i in range(6))
    assert (synth.glyphs(6, (26, 37), seed=2).templates == t).all() and not (synth.glyphs(6, (26, 37), seed=3).templates == t).all()
    assert len({t[i].tobytes() for i in range(6)}) == 6
    import numpy as np
    a = g.draw([0, 5, 5], np.random.default_rng(1))
    b = g.draw([0, 5, 5], np.random.default_rng(1))
    assert a.shape == (3, 26, 37) and (a == b).all() and (a == 0).mean() > 0.6 and a.max() <= 1.0
    assert not (a[1] == a[2]).all()  # jittered per draw
