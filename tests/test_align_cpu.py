"""CPU-side checks of the 'align' attention mode: the SepNet layout (the reference's three extra
ATTENTION weights, TDAA_beta/main_run_sstune_EvalVer.py:207-213, behind an unchanged default
layout), the `_attlayer_` checkpoint file (EvalVer.py:677-690) and the compat module's errors.
No GPU: nets are built on the CPU and no kernel is called."""
import pytest
import torch

from dl4ss_amd import checkpoint, engine

ATT = {"att.Linear_1.weight": (50, 50), "att.Linear_2.weight": (50, 50), "att.Linear_3.weight": (1, 50)}


def _nets(**kw):
    return (engine.SepNet(device="cpu", seed=1, **kw), engine.SepNet(device="cpu", seed=1, attention="dot", **kw),
            engine.SepNet(device="cpu", seed=1, attention="align", **kw))


def test_align_net_has_the_three_reference_keys():
    plain, dot, align = _nets(cell="gru", num_layers=2)
    sd = align.state_dict()
    assert set(sd) - set(plain.state_dict()) == set(ATT)
    assert {k: tuple(sd[k].shape) for k in ATT} == ATT
    # appended behind every existing parameter, in the reference's order
    assert [n for n, _ in align.specs][-3:] == list(ATT)
    assert [n for n, _ in align.specs][:-3] == [n for n, _ in plain.specs]
    # nn.Linear's initialiser: uniform in +-1/sqrt(fan_in), not degenerate
    for k in ATT:
        w = sd[k]
        assert float(w.abs().max()) <= 1.0 / 50 ** 0.5 and float(w.std()) > 0.05


def test_default_net_is_unchanged_by_the_argument():
    plain, dot, align = _nets(cell="lstm", num_layers=2)
    assert plain.attention == "dot" and align.attention == "align"
    assert list(plain.state_dict()) == list(dot.state_dict())
    assert plain.numel == dot.numel and plain.offsets == dot.offsets
    assert torch.equal(plain.flat, dot.flat)
    # the shared parameters draw the same values and sit at the same offsets in the align net
    for k, v in plain.state_dict().items():
        assert torch.equal(v, align.view(k)) and plain.offsets[k] == align.offsets[k]
    assert plain.bucket_split() == dot.bucket_split() == align.bucket_split()
    assert plain.bucket_mid(1) == align.bucket_mid(1)
    # the new weights sit in the late (loss-time) bucket
    assert all(4 + align.offsets[k][0] >= align.bucket_split() for k in ATT)


def test_unknown_or_unsupported_attention_raises():
    with pytest.raises(ValueError):
        engine.SepNet(device="cpu", num_layers=1, attention="general")
    with pytest.raises(ValueError, match="cRM"):
        engine.SepNet(device="cpu", num_layers=1, crm=True, attention="align")


def test_attlayer_checkpoint_round_trip(tmp_path):
    a = engine.SepNet(cell="gru", num_layers=1, device="cpu", seed=1, attention="align")
    paths = checkpoint.save_reference_params(a, str(tmp_path), "t", 5)
    assert set(paths) == {"hidden3d", "emblayer", "adjlayer", "attlayer"}
    assert paths["attlayer"].endswith("param_t_attlayer_5")
    sd = checkpoint.load_state(paths["attlayer"])
    assert list(sd) == ["Linear_1.weight", "Linear_2.weight", "Linear_3.weight"]
    b = engine.SepNet(cell="gru", num_layers=1, device="cpu", seed=2, attention="align")
    assert not torch.equal(a.view("att.Linear_1.weight"), b.view("att.Linear_1.weight"))
    checkpoint.load_reference_params(b, attlayer=paths["attlayer"])
    for k in ATT:
        assert torch.equal(a.view(k), b.view(k))
    # the other modules were not touched by an attlayer-only load
    assert not torch.equal(a.view("emb.layer.weight"), b.view("emb.layer.weight"))
    checkpoint.load_reference_params(b, **paths)
    assert torch.equal(a.flat, b.flat)
    # strict, both directions: a file missing a key raises
    torch.save({k: v for k, v in sd.items() if k != "Linear_3.weight"}, str(tmp_path / "short"))
    with pytest.raises(KeyError):
        checkpoint.load_reference_params(b, attlayer=str(tmp_path / "short"))


def test_attlayer_into_dot_net_raises_and_dot_save_is_unchanged(tmp_path):
    a = engine.SepNet(cell="gru", num_layers=1, device="cpu", seed=1, attention="align")
    d = engine.SepNet(cell="gru", num_layers=1, device="cpu", seed=1)
    pa = checkpoint.save_reference_params(a, str(tmp_path / "a"), "t", 0)
    with pytest.raises(KeyError):
        checkpoint.load_reference_params(d, attlayer=pa["attlayer"])
    before = d.flat.clone()
    checkpoint.load_reference_params(d, attlayer=pa["attlayer"], strict=False)  # nothing to map: a no-op
    assert torch.equal(d.flat, before)
    pd = checkpoint.save_reference_params(d, str(tmp_path / "d"), "t", 0)
    assert set(pd) == {"hidden3d", "emblayer", "adjlayer"}
    assert not (tmp_path / "d" / "param_t_attlayer_0").exists()


def test_align_ops_registered_with_meta_shapes():
    from dl4ss_amd import library as L

    assert {"attention_align", "attention_align_bwd"} <= set(L.OPS)
    m = dict(device="meta")
    V, q = torch.empty(4, 129 * 17, 50, **m), torch.empty(4, 50, **m)
    W1, W2, w3 = torch.empty(50, 50, **m), torch.empty(50, 50, **m), torch.empty(1, 50, **m)
    mask = torch.ops.dl4ss.attention_align(V, q, W1, W2, w3)
    assert mask.shape == (4, 129 * 17) and mask.dtype == torch.float32
    g = torch.ops.dl4ss.attention_align_bwd(mask, V, q, W1, W2, w3, True)
    assert [tuple(x.shape) for x in g] == [(4, 129 * 17, 50), (4, 50), (50, 50), (50, 50), (1, 50)]
    assert torch.ops.dl4ss.attention_align_bwd(mask, V, q, W1, W2, w3, False)[0].shape == (0,)
    with pytest.raises((NotImplementedError, RuntimeError)):  # no CPU kernel
        torch.ops.dl4ss.attention_align(torch.zeros(1, 4, 50), torch.zeros(1, 50), torch.zeros(50, 50),
                                        torch.zeros(50, 50), torch.zeros(1, 50))


def test_compat_attention_modes_without_a_gpu():
    from dl4ss_amd.compat import myNet

    att = myNet.ATTENTION(50, 'align', crm=True)
    assert set(att.state_dict()) == {"Linear_1.weight", "Linear_2.weight", "Linear_3.weight"}
    with pytest.raises(NotImplementedError, match="align"):
        att(torch.zeros(1, 2, 129, 50), torch.zeros(1, 100))
    with pytest.raises(NotImplementedError):
        myNet.ATTENTION(50, 'general', crm=False)(torch.zeros(1, 2, 129, 50), torch.zeros(1, 50))
    # 'align' without cRM reaches the HIP op, which refuses a CPU tensor (no CPU fallback)
    with pytest.raises(RuntimeError):
        myNet.ATTENTION(50, 'align', crm=False)(torch.zeros(1, 2, 129, 50), torch.zeros(1, 50))
