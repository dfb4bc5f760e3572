"""Keras 1's LSTM cell (gates="hard") -- the host surface without a GPU: every refusal (before any device call: the
nets live on the CPU, nothing here can launch), the ABI flag, the new ops' schemas and meta shapes, the Keras weight
mapping (load_keras_lstm / export_keras_lstm, and a numpy Keras-1 step on imported weights against
tests/keras_cell_ref.py), save_voiceprint's ``gates`` field, and the reference's own properties the GPU tests lean on
(the inputs saturate; few gates sit near a kink)."""
import numpy as np
import pytest
import torch

import keras_cell_ref as K
from dl4ss_amd import _lib, checkpoint, engine, infer, library, ops, plan
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintEncoder, VoiceprintNet

N = 4000  # 32 frames


def _net(**kw):
    kw.setdefault("adjust", False)
    kw.setdefault("cell", "lstm")
    return engine.SepNet(num_layers=2, hidden=40, device="cpu", seed=1, **kw)


def _vp(**kw):
    return VoiceprintNet(device="cpu", seed=2, **kw)


# ---- the flag -------------------------------------------------------------------------------------------------
def test_flag_in_the_header():
    c = _lib.CONSTANTS
    assert c["DL4SS_RNN_HARD_GATES"] == 0x800 == ops.HARD_GATES
    others = [c["DL4SS_RNN_WS_ZEROED"], c["DL4SS_RNN_DGH_PAD8"], c["DL4SS_RNN_DEFER_BIAS"],
              c["DL4SS_RNN_DOUT_SLABS_MASK"], 0xFF]  # (0xFF: the base precision's byte)
    assert all(ops.HARD_GATES & o == 0 for o in others)
    assert all(ops.HARD_GATES & ops.DOUT_SLABS(s) == 0 for s in (1, 2, 3, 4))
    assert ops.CELLS == {"lstm": 0, "gru": 1}  # a flag, not a third cell


def test_gate_flags():
    assert ops.gate_flags("logistic") == 0 and ops.gate_flags("logistic", "gru", "bf16") == 0
    assert ops.gate_flags("hard") == ops.HARD_GATES == ops.gate_flags("hard", "lstm", "fp32")
    with pytest.raises(ValueError, match="gates"):
        ops.gate_flags("soft")
    with pytest.raises(ValueError, match="cell"):
        ops.gate_flags("hard", "gru")
    with pytest.raises(ValueError, match="fp32 recurrence"):
        ops.gate_flags("hard", "lstm", "bf16")


# ---- the nets -------------------------------------------------------------------------------------------------
def test_nets_carry_gates_and_keep_their_layout():
    a, b = _net(), _net(gates="hard")
    assert (a.gates, b.gates) == ("logistic", "hard")
    assert a.offsets == b.offsets and torch.equal(a.flat, b.flat)
    va, vb = _vp(), _vp(gates="hard")
    assert (va.gates, vb.gates) == ("logistic", "hard")
    assert va.offsets == vb.offsets and torch.equal(va.flat, vb.flat)
    with pytest.raises(ValueError, match="cell='lstm'"):
        _net(cell="gru", gates="hard")
    with pytest.raises(ValueError, match="gates"):
        _net(gates="soft")
    with pytest.raises(ValueError, match="gates"):
        _vp(gates="soft")
    with pytest.raises(ValueError):
        _vp(cell="gru", gates="hard")


REFUSED = [dict(precision="bf16"), dict(precision="bf16s"), dict(precision="bf16s2"),
           dict(precision="bf16", rnn_precision="bf16")]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_trainer_refuses_hard_gates_off_the_fp32_recurrence(kw):
    with pytest.raises(ValueError, match="fp32 recurrence"):
        engine.SepTrainer(_net(gates="hard"), 2, 2, N, **kw)
    with pytest.raises(ValueError, match="fp32 recurrence"):
        plan.step_plan(_net(gates="hard"), 2, N, kw["precision"], kw.get("rnn_precision"))
    engine.SepTrainer(_net(), 2, 2, N, **kw)  # the logistic net builds


@pytest.mark.parametrize("kw", [dict(precision="fp32"), dict(precision="bf16", rnn_precision="fp32")],
                         ids=["fp32", "bf16-rnn-fp32"])
@pytest.mark.parametrize("attention", ["dot", "align"])
def test_trainer_builds_on_the_fp32_recurrence(kw, attention):
    tr = engine.SepTrainer(_net(gates="hard", attention=attention), 2, 2, N, **kw)
    assert tr.rnn_precision == "fp32" and tr.rnn_flags == ops.HARD_GATES and not tr.fast
    assert engine.SepTrainer(_net(attention=attention), 2, 2, N, **kw).rnn_flags == 0


def test_voiceprint_settings_are_independent():
    mem = SpeakerMemory(101, 50, device="cpu")
    for ng, vg in (("hard", "logistic"), ("logistic", "hard"), ("hard", "hard")):
        tr = engine.SepTrainer(_net(gates=ng), 2, 2, N, voiceprint=_vp(gates=vg), memory=mem)
        assert tr.rnn_flags == ops.gate_flags(ng) and tr.vp_enc.rnn_flags == ops.gate_flags(vg)
    assert VoiceprintEncoder(_vp(), 2, 9).rnn_flags == 0


def test_inference_refuses_hard_gates_on_the_bf16_recurrence():
    net = _net(gates="hard", emb=50)
    for kw in (dict(precision="bf16"), dict(precision="bf16s"), dict(precision="fp32", rnn_precision="bf16")):
        with pytest.raises(ValueError, match="fp32 recurrence"):
            infer.MaskNetForward(net, 2, 32, **kw)
    with pytest.raises(ValueError, match="fp32 recurrence"):
        infer.EnrolledExtractor(net, _vp(gates="hard"), 2, 32, 2, precision="bf16")
    cnet = infer.ClassifierNet(hidden=40, num_layers=1, device="cpu")
    for mode in ("bf16", "mixed", "bf16s"):
        with pytest.raises(ValueError, match="fp32 recurrence"):
            infer.RecursiveExtractor(net, cnet, 2, 32, precision=mode)
    m = infer.MaskNetForward(net, 2, 32, "bf16", "fp32")
    assert m.gates == "hard" and infer.MaskNetForward(_net(), 2, 32, "bf16").gates == "logistic"


# ---- the ops --------------------------------------------------------------------------------------------------
def test_ops_have_schemas_and_meta_shapes():
    assert {"keras_lstm_layer", "keras_lstm_layer_bwd"} <= set(library.OPS)
    f = torch.ops.dl4ss.keras_lstm_layer.default
    b = torch.ops.dl4ss.keras_lstm_layer_bwd.default
    assert f._schema.name == "dl4ss::keras_lstm_layer" and b._schema.name == "dl4ss::keras_lstm_layer_bwd"
    assert [a.name for a in f._schema.arguments] == ["x", "w_ih", "b_ih", "w_hh", "b_hh", "H"]  # no cell, no precision
    B, T, D, H = 3, 7, 23, 25
    e = lambda *s: torch.empty(*s, device="meta")  # noqa: E731
    x, w_ih, b_ih, w_hh, b_hh = e(B, T, D), e(8 * H, D), e(8 * H), e(8 * H, H), e(8 * H)
    out, hprev, act, cs = torch.ops.dl4ss.keras_lstm_layer(x, w_ih, b_ih, w_hh, b_hh, H)
    assert (out.shape, hprev.shape) == ((B, T, 2 * H), (B, T, 2 * H))
    assert (act.shape, cs.shape) == ((B, T, 2, 4 * H), (B, T, 2, H))
    g = torch.ops.dl4ss.keras_lstm_layer_bwd(e(B, T, 2 * H), x, w_ih, w_hh, hprev, act, cs, H, True)
    assert [tuple(t.shape) for t in g] == [(B, T, D), (8 * H, D), (8 * H,), (8 * H, H), (8 * H,)]
    assert torch.ops.dl4ss.keras_lstm_layer_bwd(e(B, T, 2 * H), x, w_ih, w_hh, hprev, act, cs, H, False)[0].numel() == 0
    # the existing ops' schemas did not move
    assert [a.name for a in torch.ops.dl4ss.birnn_layer.default._schema.arguments] == \
        ["x", "w_ih", "b_ih", "w_hh", "b_hh", "cell", "H", "precision"]
    with pytest.raises(ValueError):
        library.birnn(x, w_ih, b_ih, w_hh, b_hh, cell="gru", H=H, gates="hard")
    with pytest.raises(ValueError):
        library.birnn(x, w_ih, b_ih, w_hh, b_hh, H=H, precision="bf16", gates="hard")


# ---- Keras weights ----------------------------------------------------------------------------------------------
def _keras_weights(D, H, seed):
    g = np.random.default_rng(seed)
    shapes = {"W": (D, H), "U": (H, H), "b": (H,)}
    return {n: g.standard_normal(shapes[n[0]]).astype(np.float32) for n in checkpoint.KERAS_LSTM_NAMES}


def test_load_then_export_is_the_identity():
    for net, D in ((_net(gates="hard"), 129), (_vp(gates="hard"), 129)):
        for layer, din in ((0, D), (1, 2 * net.H)):
            for k, direction in enumerate(("forward", "backward")):
                w = _keras_weights(din, net.H, 10 * layer + k)
                # a dict in another order: the mapping is by name
                checkpoint.load_keras_lstm(net, layer, direction, dict(reversed(list(w.items()))))
                back = checkpoint.export_keras_lstm(net, layer, direction)
                assert set(back) == set(checkpoint.KERAS_LSTM_NAMES)
                for n in w:
                    assert np.array_equal(back[n].numpy(), w[n]), n
    net = _net(gates="hard")
    w = _keras_weights(129, 40, 3)
    checkpoint.load_keras_lstm(net, 0, "backward", w)
    H = 40
    wi, bi = net.view("mix.layer.weight_ih_l0_reverse"), net.view("mix.layer.bias_ih_l0_reverse")
    for q, gname in enumerate("ifco"):  # rows [i | f | g (= Keras's c) | o]
        assert np.array_equal(wi[q * H:(q + 1) * H].numpy(), w[f"W_{gname}"].T)
        assert np.array_equal(bi[q * H:(q + 1) * H].numpy(), w[f"b_{gname}"])
    assert bool((net.view("mix.layer.bias_hh_l0_reverse") == 0).all())


def test_keras_weight_refusals():
    w = _keras_weights(129, 40, 1)
    with pytest.raises(ValueError, match="gates='hard'"):
        checkpoint.load_keras_lstm(_net(), 0, "forward", w)
    with pytest.raises(ValueError, match="gates='hard'"):
        checkpoint.export_keras_lstm(_vp(), 0, "forward")
    net = _net(gates="hard")
    keep = net.flat.clone()
    with pytest.raises(ValueError, match="names"):
        checkpoint.load_keras_lstm(net, 0, "forward", {k: v for k, v in w.items() if k != "U_c"})
    with pytest.raises(ValueError, match="names"):
        checkpoint.load_keras_lstm(net, 0, "forward", dict(w, W_g=w["W_c"]))
    with pytest.raises(ValueError, match="shape"):
        checkpoint.load_keras_lstm(net, 1, "forward", w)  # layer 1 reads 2H inputs
    with pytest.raises(ValueError, match="direction"):
        checkpoint.load_keras_lstm(net, 0, "reverse", w)
    with pytest.raises(ValueError, match="layer"):
        checkpoint.load_keras_lstm(net, 2, "forward", w)
    assert torch.equal(net.flat, keep)  # nothing was written
    with pytest.raises(ValueError, match="bias_hh"):  # the torch initialiser's second bias is not zero
        checkpoint.export_keras_lstm(net, 0, "forward")


def _keras1_lstm(x, w, go_backwards):
    """Keras 1's LSTM.step in numpy fp64 from the per-gate names (consume_less='cpu' form): x (B, T, D) -> (B, T, H)."""
    w = {k: v.astype(np.float64) for k, v in w.items()}
    hard = lambda z: np.clip(0.2 * z + 0.5, 0.0, 1.0)  # noqa: E731
    B, T, _ = x.shape
    H = w["b_i"].shape[0]
    h, c = np.zeros((B, H)), np.zeros((B, H))
    out = np.zeros((B, T, H))
    for t in (range(T - 1, -1, -1) if go_backwards else range(T)):
        xt = x[:, t]
        i = hard(xt @ w["W_i"] + w["b_i"] + h @ w["U_i"])
        f = hard(xt @ w["W_f"] + w["b_f"] + h @ w["U_f"])
        c = f * c + i * np.tanh(xt @ w["W_c"] + w["b_c"] + h @ w["U_c"])
        o = hard(xt @ w["W_o"] + w["b_o"] + h @ w["U_o"])
        h = o * np.tanh(c)
        out[:, t] = h
    return out


def test_numpy_keras1_step_agrees_with_the_reference_on_imported_weights():
    B, T, D, H = 3, 6, 129, 25
    net = _vp(gates="hard")
    ws = [_keras_weights(D, H, 40 + k) for k in range(2)]
    for k, direction in enumerate(("forward", "backward")):
        for n in ws[k]:  # large enough that the gates saturate
            ws[k][n] *= 0.3 if n[0] == "W" else 1.0
        checkpoint.load_keras_lstm(net, 0, direction, ws[k])
    x = np.random.default_rng(5).standard_normal((B, T, D))
    want = np.concatenate([_keras1_lstm(x, ws[0], False), _keras1_lstm(x, ws[1], True)], -1)
    xt = torch.from_numpy(x)
    G = (xt.reshape(B * T, D) @ net.cat_view("weight_ih", 0).double().T + net.cat_view("bias_ih", 0).double())
    ref = K.forward(G.view(B, T, 2, 4 * H), net.cat_view("weight_hh", 0).view(2, 4 * H, H),
                    net.cat_view("bias_hh", 0).view(2, 4 * H))
    K.assert_saturates(ref["act"])
    assert np.abs(ref["out"].numpy() - want).max() < 1e-12


# ---- save_voiceprint -------------------------------------------------------------------------------------------
def test_save_load_voiceprint_keeps_gates(tmp_path):
    mem = SpeakerMemory(7, 50, device="cpu")
    for gates in ("hard", "logistic"):
        p = str(tmp_path / f"vp_{gates}.pt")
        v = _vp(gates=gates)
        checkpoint.save_voiceprint(p, v, mem)
        assert torch.load(p, weights_only=True)["gates"] == gates
        v2 = VoiceprintNet(device="cpu", seed=9, gates=gates)
        checkpoint.load_voiceprint(p, v2, mem)
        assert torch.equal(v2.flat, v.flat) and v2.gates == gates
        other = VoiceprintNet(device="cpu", seed=9, gates="logistic" if gates == "hard" else "hard")
        keep = other.flat.clone()
        with pytest.raises(ValueError, match="gates"):
            checkpoint.load_voiceprint(p, other, mem)
        assert torch.equal(other.flat, keep)
    # a file from before the field is a logistic encoder's
    v = _vp()
    old = str(tmp_path / "old.pt")
    torch.save({"voiceprint": v.state_dict(), "memory": mem.state_dict()}, old)
    v2 = VoiceprintNet(device="cpu", seed=9)
    checkpoint.load_voiceprint(old, v2, mem)
    assert torch.equal(v2.flat, v.flat)
    with pytest.raises(ValueError, match="gates"):
        checkpoint.load_voiceprint(old, _vp(gates="hard"), mem)


# ---- the reference itself ---------------------------------------------------------------------------------------
SHAPES = [(5, 9, 25), (64, 3, 25), (3, 1, 40), (4, 2, 40), (9, 4, 300), (32, 3, 300), (1, 5, 600)]


@pytest.mark.parametrize("B,T,H", SHAPES)
def test_reference_inputs_saturate_and_stay_off_the_kinks(B, T, H):
    c = K.case(B, T, H)
    ref = K.forward(c["G"], c["w_hh"], c["b_hh"])
    K.assert_saturates(ref["act"])
    share = K.near_kink(ref["z"]).double().sum().item() / (0.75 * ref["z"].numel())
    print(f"B={B} T={T} H={H}: {share:.2e} of the gates within {K.KINK} of a kink;",
          "shares", K.saturation_shares(ref["act"]))
    assert share <= K.CAP / 4  # the reference's own share stays well inside the cap


def test_reference_bptt_is_the_derivative():
    """The hand-written BPTT with the reference's own pattern equals torch autograd of the same formulae."""
    B, T, H = 3, 5, 8
    c = K.case(B, T, H, seed=3)
    G, w, b = (c[k].double().requires_grad_(True) for k in ("G", "w_hh", "b_hh"))
    outs = []
    for d in range(2):
        h, cc = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
        o_d = [None] * T
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            zi, zf, zg, zo = (G[:, t, d] + h @ w[d].T + b[d]).chunk(4, -1)
            cc = K.hs(zf) * cc + K.hs(zi) * torch.tanh(zg)
            h = K.hs(zo) * torch.tanh(cc)
            o_d[t] = h
        outs.append(torch.stack(o_d, 1))
    out = torch.cat(outs, -1)
    ref = K.forward(c["G"], c["w_hh"], c["b_hh"])
    assert torch.equal(out.detach(), ref["out"])
    dout, bc = c["dOut"].double(), c["dOut_bcast"].double()
    (out * (dout + bc[:, None])).sum().backward()
    r = K.backward(ref, c["w_hh"], dOut=c["dOut"], dOut_bcast=c["dOut_bcast"])
    for got, want in ((r["dG"], G.grad), (r["dw_hh"], w.grad), (r["db_hh"], b.grad)):
        assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    # and through the autograd.Function
    G2, w2, b2 = (c[k].double().requires_grad_(True) for k in ("G", "w_hh", "b_hh"))
    (K.HardLSTMLayer.apply(G2, w2, b2, None) * dout).sum().backward()
    r1 = K.backward(ref, c["w_hh"], dOut=c["dOut"])
    assert torch.equal(G2.grad, r1["dG"]) and torch.equal(w2.grad, r1["dw_hh"]) and torch.equal(b2.grad, r1["db_hh"])
