"""The voiceprint path's host surface without a GPU: what SepTrainer(voiceprint=..., memory=...) refuses (before
any device call: the nets live on the CPU, nothing here can launch), VoiceprintNet's keys against nn.LSTM's, the
state dicts' round trips and save_voiceprint / load_voiceprint."""
import pytest
import torch

from dl4ss_amd import _lib, checkpoint, engine, ops
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintEncoder, VoiceprintNet

N = 4000  # 32 frames


def _net(**kw):
    kw.setdefault("adjust", False)
    return engine.SepNet(cell="gru", num_layers=1, device="cpu", seed=1, **kw)


def _vp(**kw):
    return VoiceprintNet(device="cpu", seed=2, **kw)


def _mem(emb=50):
    return SpeakerMemory(101, emb, device="cpu")


def test_new_symbols_are_bound():
    for s in ("dl4ss_vp_compact", "dl4ss_vp_shift", "dl4ss_vp_mean_fwd", "dl4ss_vp_mean_bwd", "dl4ss_spk_memory_fwd",
              "dl4ss_spk_memory_bwd", "dl4ss_spk_memory_store"):
        assert s in _lib.SIGNATURES and hasattr(_lib.lib(), s)


def test_encoder_recurrence_plan_exists():
    """the generic fp32 recurrence at H = 25: J = 20, NG = 2 (a last group of 5 units), a workspace"""
    for B, bc in ((5, 1), (64, 2), (96, 2)):
        p = ops.birnn_plan("lstm", B, 25, precision="fp32", max_wg=240)
        assert p is not None and (p["J"], p["NG"], p["BC"]) == (20, 2, bc), p
    assert _lib.query("dl4ss_birnn_workspace_bytes", 0, 64, 25) >= 0


def test_voiceprint_net_keys_and_defaults():
    v = _vp()
    assert (v.F, v.E, v.H, v.L, v.cell) == (129, 50, 25, 2, "lstm")
    lstm = torch.nn.LSTM(129, 25, 2, batch_first=True, bidirectional=True)
    want = {"spk.layer." + k: tuple(p.shape) for k, p in lstm.named_parameters()}
    assert {k: tuple(t.shape) for k, t in v.state_dict().items()} == want
    assert v.grad.shape == v.flat.shape and all(off % 4 == 0 for off, _ in v.offsets.values())
    k = 25 ** -0.5  # torch's default initialiser: U(+-1/sqrt(H)), not degenerate
    assert float(v.flat.abs().max()) <= k and float(v.view("spk.layer.weight_ih_l0").std()) > 0.4 * k
    assert torch.equal(_vp().flat, v.flat) and not torch.equal(VoiceprintNet(device="cpu", seed=3).flat, v.flat)
    lstm.load_state_dict({k[len("spk.layer."):]: t for k, t in v.state_dict().items()})  # strict
    with pytest.raises(ValueError, match="2 \\* hidden"):
        _vp(emb=50, hidden=24)
    with pytest.raises(ValueError, match="cell"):
        _vp(cell="gru")


def test_state_dicts_round_trip():
    v, v2 = _vp(), VoiceprintNet(device="cpu", seed=9)
    assert not torch.equal(v.flat, v2.flat)
    v2.load_state_dict(v.state_dict())
    assert torch.equal(v.flat, v2.flat)
    m, m2 = _mem(), _mem()
    assert (m.mem == 0).all() and m.mem.shape == (101, 50)
    m.mem.copy_(torch.randn(101, 50))
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m.mem, m2.mem)
    m2.reset()
    assert (m2.mem == 0).all()
    with pytest.raises(ValueError):
        SpeakerMemory(7, 50, device="cpu").load_state_dict(m.state_dict())


def test_save_load_voiceprint_round_trip(tmp_path):
    v, m = _vp(), _mem()
    m.mem.copy_(torch.randn(101, 50))
    p = str(tmp_path / "voiceprint.pt")
    checkpoint.save_voiceprint(p, v, m)
    v2, m2 = VoiceprintNet(device="cpu", seed=9), _mem()
    checkpoint.load_voiceprint(p, v2, m2)
    assert torch.equal(v2.flat, v.flat) and torch.equal(m2.mem, m.mem)
    with pytest.raises(ValueError):  # another encoder shape
        checkpoint.load_voiceprint(p, VoiceprintNet(emb=80, device="cpu"), SpeakerMemory(101, 80, device="cpu"))
    v3 = VoiceprintNet(device="cpu", seed=9)
    w3 = v3.flat.clone()
    with pytest.raises(ValueError):  # another memory size: refused before either is written
        checkpoint.load_voiceprint(p, v3, SpeakerMemory(7, 50, device="cpu"))
    assert torch.equal(v3.flat, w3)


def test_enrolled_extractor_refusals():
    from dl4ss_amd import infer

    with pytest.raises(ValueError, match="adjust"):  # ADDJUST works on embedding rows
        infer.EnrolledExtractor(_net(adjust=True), _vp(), 2, 32, 2)
    with pytest.raises(ValueError, match="cRM"):
        infer.EnrolledExtractor(_net(crm=True), _vp(), 2, 32, 2)


CASES = {
    "mode": (dict(mode="pit"), {}, "mode"),
    "crm": (dict(mode="crm"), dict(crm=True), "mode|cRM"),
    "crm_net": ({}, dict(crm=True), "cRM"),
    "adjust": ({}, dict(adjust=True), "adjust"),
    "emb": ({}, dict(emb=40), "elements"),
    "precision": (dict(precision="bf16"), {}, "precision"),
    "loss_channels": (dict(loss_channels=101), {}, "loss_channels"),
    "process_group": (dict(process_group=object()), {}, "process_group"),
    "clip_norm": (dict(clip_norm=200.0), {}, "clip_norm"),
    "refresh": (dict(memory_refresh="never"), {}, "memory_refresh"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_trainer_refuses(case):
    kw, nkw, reason = CASES[case]
    with pytest.raises(ValueError, match=reason):
        engine.SepTrainer(_net(**nkw), 2, 2, N, voiceprint=_vp(), memory=_mem(), **kw)


def test_trainer_refuses_adversary_and_halves_and_types():
    disc = engine.DiscNet(32, 129, device="cpu")
    with pytest.raises(ValueError, match="adversary"):
        engine.SepTrainer(_net(), 2, 2, N, voiceprint=_vp(), memory=_mem(), adversary=disc)
    with pytest.raises(ValueError, match="memory"):
        engine.SepTrainer(_net(), 2, 2, N, voiceprint=_vp())
    with pytest.raises(ValueError, match="voiceprint"):
        engine.SepTrainer(_net(), 2, 2, N, memory=_mem())
    with pytest.raises(ValueError, match="VoiceprintNet"):
        engine.SepTrainer(_net(), 2, 2, N, voiceprint=object(), memory=_mem())
    with pytest.raises(ValueError, match="SpeakerMemory"):
        engine.SepTrainer(_net(), 2, 2, N, voiceprint=_vp(), memory=object())
    with pytest.raises(ValueError, match="rows of 40"):
        engine.SepTrainer(_net(), 2, 2, N, voiceprint=_vp(), memory=_mem(40))
    with pytest.raises(ValueError, match="1024"):
        engine.SepTrainer(_net(), 600, 2, N, voiceprint=_vp(), memory=_mem())


@pytest.mark.parametrize("attention", ["dot", "align"])
def test_trainer_builds_and_refuses_graph_capture(attention):
    tr = engine.SepTrainer(_net(attention=attention), 2, 2, N, voiceprint=_vp(), memory=_mem(),
                           memory_refresh="reuse", voiceprint_lr=1e-3)
    assert tr.vp_lr == 1e-3 and tr.vp_enc.n == 4 and tr.vp_enc.T == 32 and tr.vp_enc.status is tr.status
    assert engine.SepTrainer(_net(), 2, 2, N, voiceprint=_vp(), memory=_mem(), lr=3e-4).vp_lr == 3e-4
    raw = torch.zeros(2, 2, N)
    with pytest.raises(NotImplementedError):
        tr.capture()
    with pytest.raises(NotImplementedError):
        tr.step_graph(raw, torch.ones(2, 2), torch.zeros(2, 2, dtype=torch.int32))
    plain = engine.SepTrainer(_net(), 2, 2, N)
    assert plain.vnet is None and plain.memory is None and not hasattr(plain, "vp_enc")


def test_encoder_argument_checks():
    with pytest.raises(ValueError):
        VoiceprintEncoder(object(), 2, 9)
    with pytest.raises(ValueError):
        VoiceprintEncoder(_vp(), 2, 4096)
