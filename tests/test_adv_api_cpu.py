"""The adversarial step's host surface without a GPU: what SepTrainer(adversary=...) refuses (before any
device call), engine.DiscNet's keys and shapes against the reference Discriminator's, its round trip through
the checkpoint functions and its state_dict exchange with the shapes ``myNet.Discriminator`` declares."""
import pytest
import torch

from dl4ss_amd import _lib, checkpoint, engine

T, F, N = 32, 129, 4000  # ops.n_frames(4000) = 32
FEAT = 64 * 3 * 15  # 32 x 129 -> 15 x 64 -> 7 x 31 -> 3 x 15
SHAPES = {"cnn.weight": (64, 1, 3, 3), "cnn.bias": (64,), "cnn1.weight": (64, 64, 3, 3), "cnn1.bias": (64,),
          "cnn2.weight": (64, 64, 3, 3), "cnn2.bias": (64,), "final.weight": (1, FEAT), "final.bias": (1,)}


def _net(**kw):
    return engine.SepNet(cell="gru", num_layers=1, device="cpu", seed=1, **kw)


def test_new_symbols_are_bound():
    for s in ("dl4ss_mask_attn_loss_adv", "dl4ss_mask_attn_loss_adv_bf16v", "dl4ss_disc_adv_heads"):
        assert s in _lib.SIGNATURES and hasattr(_lib.lib(), s)


def test_discnet_keys_and_shapes():
    d = engine.DiscNet(T, F, device="cpu", seed=5)
    assert tuple(n for n, _ in d.specs) == checkpoint.DIS_KEYS
    sd = d.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == SHAPES
    assert d.feat == FEAT and d.hw == [15, 64, 7, 31, 3, 15]
    assert d.grad_dis.shape == d.flat.shape == d.grad_adv.shape
    assert all(off % 4 == 0 for off, _ in d.offsets.values())  # 16-B aligned views
    # torch-default initialisation: uniform within +-1/sqrt(fan_in), not degenerate
    for k, fan in (("cnn.weight", 9), ("cnn1.bias", 576), ("final.weight", FEAT)):
        v = sd[k]
        assert float(v.abs().max()) <= fan ** -0.5 and float(v.std()) > 0.4 * fan ** -0.5  # (uniform: 0.577)
    assert not torch.equal(engine.DiscNet(T, F, device="cpu", seed=6).flat, d.flat)
    assert torch.equal(engine.DiscNet(T, F, device="cpu", seed=5).flat, d.flat)
    with pytest.raises(ValueError):
        engine.DiscNet(14, F, device="cpu")


def test_discnet_checkpoint_round_trip(tmp_path):
    d = engine.DiscNet(T, F, device="cpu", seed=5)
    p = checkpoint.save_reference_discriminator(d, "adv", 5, str(tmp_path))
    assert p.endswith("param_adv_dislayer_5")
    d2 = engine.DiscNet(T, F, device="cpu", seed=9)
    assert not torch.equal(d2.flat, d.flat)
    checkpoint.load_reference_discriminator(d2, p)
    assert torch.equal(d2.flat, d.flat)
    with pytest.raises(ValueError):  # a file saved at another map size
        checkpoint.load_reference_discriminator(engine.DiscNet(40, F, device="cpu"), p)


def test_discnet_exchanges_state_with_the_module_shapes():
    """myNet.Discriminator's parameters are nn.Conv2d(1, 64, 3) / nn.Conv2d(64, 64, 3) x 2 / nn.Linear(feat, 1)
    under the names cnn, cnn1, cnn2, final: the same declaration, built here without the GPU module."""
    from torch import nn

    class Decl(nn.Module):
        def __init__(self):
            super().__init__()
            self.cnn = nn.Conv2d(1, 64, (3, 3), stride=(2, 2))
            self.cnn1 = nn.Conv2d(64, 64, (3, 3), stride=(2, 2))
            self.cnn2 = nn.Conv2d(64, 64, (3, 3), stride=(2, 2))
            self.final = nn.Linear(FEAT, 1)

    m = Decl()
    d = engine.DiscNet(T, F, device="cpu", seed=5)
    m.load_state_dict(d.state_dict())  # strict
    for k, v in m.state_dict().items():
        assert torch.equal(v, d.view(k))
    torch.manual_seed(1)
    m2 = Decl()
    d.load_state_dict(m2.state_dict())
    for k, v in m2.state_dict().items():
        assert torch.equal(v, d.view(k))


@pytest.mark.parametrize("case", ["crm", "loss_channels", "align", "process_group", "short", "other_map", "type"])
def test_trainer_refuses(case):
    """each refused before any device call: the net lives on the CPU, nothing here can launch"""
    kw, nkw, n, disc = {}, {}, N, engine.DiscNet(T, F, device="cpu")
    if case == "crm":
        kw, nkw = dict(mode="crm"), dict(crm=True)
    elif case == "loss_channels":
        kw = dict(loss_channels=101)
    elif case == "align":
        nkw = dict(attention="align")
    elif case == "process_group":
        kw = dict(process_group=object())
    elif case == "short":
        n, disc = 1700, engine.DiscNet(15, F, device="cpu")  # 14 frames
    elif case == "other_map":
        disc = engine.DiscNet(40, F, device="cpu")
    elif case == "type":
        disc = object()
    with pytest.raises(ValueError, match="adversary"):
        engine.SepTrainer(_net(**nkw), 2, 2, n, adversary=disc, **kw)
