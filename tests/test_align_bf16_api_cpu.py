"""ATTENTION 'align' on the bf16 steps, host side (no GPU): plan.check_args accepts an align net with precision
"bf16" / "bf16s" / "bf16s2" on the bf16 recurrence and keeps every other refusal, each with its own message; the
fifth header declares dl4ss_mask_attn_align_loss_ex and _lib binds it with the header's parameter names; the
trainer routes the align passes of a bf16 step to it (the library stubbed, as tests/test_lib_bind_cpu.py does)."""
import os

import pytest

from conftest import ROOT
from dl4ss_amd import _lib, engine, imagequery, plan
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintNet

N = 4000
ENTRY = "dl4ss_mask_attn_align_loss_ex"
CORE, ALIGN = _lib.HEADERS["dl4ss_hip.h"], _lib.HEADERS["dl4ss_align.h"]


def _net(**kw):
    kw = dict(dict(cell="lstm", num_layers=1, device="cpu", seed=1, attention="align"), **kw)
    return engine.SepNet(**kw)


def _check(net, precision="bf16", mode="label", rnn_precision=None, loss_channels=None, adversary=None, vnet=None,
           memory=None, inet=None, **kw):
    return plan.check_args(net, 2, 2, N, mode, precision, rnn_precision, loss_channels, None, adversary, None, None,
                           vnet, memory, "reference", inet=inet, **kw)


@pytest.mark.parametrize("precision", ["bf16", "bf16s", "bf16s2"])
@pytest.mark.parametrize("mode", ["label", "pit"])
def test_check_args_accepts_align_on_the_bf16_steps(precision, mode):
    assert _check(_net(), precision, mode) == (None, None)
    assert _check(_net(num_layers=4), precision, mode, optimizer="nadam", clipnorm=200.0) == (None, None)
    assert plan.resolve_rnn_precision(precision) == "bf16"


@pytest.mark.parametrize("precision", ["bf16", "bf16s", "bf16s2"])
def test_check_args_keeps_a_bigru_align_net_on_the_fp32_step(precision):
    """The bf16 align step is built and verified for the BiLSTM nets; a BiGRU align net is refused there, as before
    (tests/test_align_api_gpu.py pins that refusal), and still runs in fp32 and with bf16 GEMMs on the fp32
    recurrence."""
    with pytest.raises(ValueError, match="bf16 / bf16s fast paths is built for cell 'lstm', not 'gru'"):
        _check(_net(cell="gru"), precision)
    assert _check(_net(cell="gru"), "fp32") == (None, None)
    assert _check(_net(cell="gru"), "bf16", rnn_precision="fp32") == (None, None)


def test_check_args_still_accepts_the_fp32_forms():
    assert _check(_net(), "fp32") == (None, None)
    assert _check(_net(), "bf16", rnn_precision="fp32") == (None, None)  # bf16 GEMMs on the fp32 recurrence


@pytest.mark.parametrize("precision", ["bf16", "bf16s", "bf16s2"])
def test_check_args_keeps_its_refusals(precision):
    with pytest.raises(ValueError, match="cRM|crm"):  # (an align net is never a cRM net: SepNet refuses the pair)
        _check(_net(), precision, mode="crm")
    with pytest.raises(ValueError, match="attention='align' does not support loss_channels"):
        _check(_net(), precision, loss_channels=101)
    with pytest.raises(ValueError, match="adversary: attention='align' is unsupported with an adversary"):
        _check(_net(), precision, adversary=engine.DiscNet(32, 129, device="cpu"))
    with pytest.raises(ValueError, match="attention='align' is built for embedding size 50"):
        _check(_net(emb=40), precision)
    with pytest.raises(ValueError, match="gates='hard' .* needs the fp32 recurrence"):
        _check(_net(gates="hard"), precision)
    mem = SpeakerMemory(101, 50, device="cpu")
    with pytest.raises(ValueError, match=f"voiceprint: precision '{precision}' is unsupported"):
        _check(_net(adjust=False), precision, vnet=VoiceprintNet(device="cpu", seed=2), memory=mem)
    with pytest.raises(ValueError, match=f"image_query: precision '{precision}' is unsupported"):
        _check(_net(adjust=False), precision, inet=imagequery.ImageQueryNet(device="cpu"), memory=mem)


def test_crm_mode_message_of_an_align_net():
    """mode 'crm' with an align net: refused as a net / mode mismatch, the first check that sees it."""
    with pytest.raises(ValueError, match="cRM mode needs a cRM net"):
        _check(_net(), "bf16", mode="crm")
    with pytest.raises(ValueError, match="attention='align' with a cRM net is unsupported"):
        _net(crm=True)


def test_hard_gates_align_net_runs_bf16_gemms_on_the_fp32_recurrence_only():
    assert _check(_net(gates="hard"), "bf16", rnn_precision="fp32") == (None, None)
    assert _check(_net(gates="hard"), "fp32") == (None, None)


def test_the_fifth_header_declares_the_entry_point_and_lib_binds_it():
    with open(os.path.join(ROOT, "include", "dl4ss_align.h")) as f:
        sigs, res, params, consts = _lib.parse_header(f.read(), "dl4ss_align.h")
    assert set(sigs) == {ENTRY} == set(ALIGN.signatures) == set(_lib.exported_symbols("dl4ss_align.h"))
    assert (sigs, res, params, consts) == ALIGN and consts == {}
    P, I, LL, F = _lib.P, _lib.I, _lib.LL, _lib.F
    assert sigs[ENTRY] == [I, I, I, I, I, I, P, P, P, P, P, P, P, LL, P, LL, LL, P, F, F, P, P, LL, P, P, LL, P, P, P]
    assert res[ENTRY] is I
    assert params[ENTRY] == ("pass", "B", "K", "T", "F", "E", "V", "V_bf16", "q", "W1", "W2", "w3", "X", "x_bstride",
                             "Y", "y_bstride", "y_kstride", "perm", "s1", "s2", "dPre", "dPre_bf16", "dpre_bf16_ld",
                             "part_loss", "part", "part_floats", "mask_out", "pred_out", "stream")
    # the fp32 entry's parameters with the two bf16 ones of dl4ss_mask_attn_loss_ex / _bf16v added, same names
    old = CORE.params["dl4ss_mask_attn_align_loss"]
    assert tuple(p for p in params[ENTRY] if p not in ("V_bf16", "dPre_bf16", "dpre_bf16_ld")) == old
    assert {"V_bf16", "dPre_bf16", "dpre_bf16_ld"} <= set(CORE.params["dl4ss_mask_attn_loss_bf16v"])
    # no other header has the name, and the first header's tables stay what dl4ss_hip.h declares
    others = [h for name, h in _lib.HEADERS.items() if name != "dl4ss_align.h"]
    assert len(others) >= 4 and not any(ENTRY in h.signatures for h in others)
    assert ENTRY not in _lib.exported_symbols("dl4ss_hip.h") and ENTRY in _lib.exported_symbols()
    with open(os.path.join(ROOT, "include", "dl4ss_hip.h")) as f:
        assert CORE == _lib.parse_header(f.read())
    n = len(params[ENTRY])
    kw = {("pass_" if p == "pass" else p): i for i, p in enumerate(params[ENTRY])}
    assert _lib.bind(ENTRY, (), kw) == tuple(range(n))
    with pytest.raises(TypeError, match="'V_bf16'"):
        _lib.bind(ENTRY, (), {k: v for k, v in kw.items() if k != "V_bf16"})
    with pytest.raises(TypeError, match="dl4ss_align.h"):
        _lib.bind("dl4ss_mask_attn_align_nothing", (), {})


def test_the_library_exports_the_entry_point():
    fn = getattr(_lib.lib(), ENTRY)
    assert fn.argtypes == ALIGN.signatures[ENTRY] and fn.restype is ALIGN.restypes[ENTRY]


class _Fake:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("dl4ss_"):
            raise AttributeError(name)
        return lambda *args: (self.calls.append((name, args)), 0)[1]


@pytest.mark.parametrize("precision", ["bf16", "bf16s", "fp32"])
def test_trainer_routes_the_align_passes(precision, monkeypatch):
    """bf16: V_bf16 = Vb; bf16s: fp32 V; both write dPre into dPreb at its row pitch, in both passes' calls (the
    COST pass writes to neither).  fp32: the fp32 entry, dPre in place over V, as before."""
    tr = engine.SepTrainer(_net(num_layers=2), 2, 2, N, precision=precision, mode="pit")
    assert tr.align and tr.fast == (precision != "fp32")
    assert tr.zero_free == tr.fast and tr._sk == ("auto" if tr.fast else 1)
    fake = _Fake()
    monkeypatch.setattr(_lib, "_lib", fake)
    monkeypatch.setattr(_lib, "ptr", lambda t, strided=False: None if t is None else ("ptr", t.data_ptr()))
    monkeypatch.setattr(_lib, "stream_ptr", lambda stream=None: "stream")
    tag = lambda t: None if t is None else ("ptr", t.data_ptr())  # noqa: E731
    for pass_, grad in ((0, False), (1, True)):
        tr.attn(pass_, tr.perm if grad else None)
        name, args = fake.calls[-1]
        got = dict(zip(_lib.PARAMS[name], args))
        assert got["pass"] == pass_ and got["E"] == 50 and got["part_floats"] == tr.part_att.numel()
        assert got["W1"] == tag(tr.net.view("att.Linear_1.weight")) and got["w3"] == tag(tr.net.view("att.Linear_3.weight"))
        assert got["part"] == (tag(tr.part_att) if grad else None) and got["perm"] == (tag(tr.perm) if grad else None)
        if precision == "fp32":
            assert name == "dl4ss_mask_attn_align_loss"
            assert got["V"] == tag(tr.V) and got["dPre"] == (tag(tr.V) if grad else None)
            continue
        assert name == ENTRY
        assert (got["V"], got["V_bf16"]) == ((None, tag(tr.Vb)) if precision == "bf16" else (tag(tr.V), None))
        assert got["dPre"] is None and got["dPre_bf16"] == tag(tr.dPreb)
        assert got["dpre_bf16_ld"] == tr.dPreb.stride(0) == (129 * 50 + 7) // 8 * 8
