"""The Discriminator's Python surface on the GPU: ``myNet.Discriminator`` against a same-weights fp64
``nn.Conv2d`` / ``nn.Linear`` model (forward and ``.backward()`` of both LSGAN losses), the ``dl4ss::discriminator``
ops against the ``autograd.Function`` (bitwise) and ``torch.library.opcheck``, and the driver mirror's
``train_step`` on a synthetic batch.  fp32 bounds: score rtol 1e-5 / atol 1e-6, every gradient within 1e-4 of
its tensor's largest element."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import disc_ref as R
from dl4ss_amd import autograd as ag, compat, library as L  # noqa: F401  (library registers the ops)

pytestmark = pytest.mark.gpu

compat.install(drivers=True)

SPK = [f"spk{i:03d}" for i in range(101)]
D2I = {s: i for i, s in enumerate(SPK)}
I2D = {i: s for i, s in enumerate(SPK)}


class RefDis(nn.Module):
    """main_run_sstune_dis.py:318-336 without the prints, sized from the map"""

    def __init__(self, feat):
        super().__init__()
        self.cnn = nn.Conv2d(1, 64, (3, 3), stride=(2, 2))
        self.cnn1 = nn.Conv2d(64, 64, (3, 3), stride=(2, 2))
        self.cnn2 = nn.Conv2d(64, 64, (3, 3), stride=(2, 2))
        self.final = nn.Linear(feat, 1)

    def forward(self, spec):
        bs, topk, len_, fre = spec.size()
        spec = spec.reshape(bs * topk, 1, len_, fre)
        for c in (self.cnn, self.cnn1, self.cnn2):
            spec = torch.relu(c(spec))
        return torch.sigmoid(self.final(spec.reshape(bs * topk, -1)))


def _ref_of(module):
    ref = RefDis(module.final.weight.shape[1]).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in module.state_dict().items()})
    return ref


def _close(ours, ref, what):
    e = R.rel_err(ours.detach().cpu(), ref)
    assert e <= 1e-4, (what, e)


@pytest.mark.parametrize("target", [1.0, 0.0])
@pytest.mark.parametrize("shape", [(1, 3, 23, 33), (1, 2, 31, 129)])
def test_module_matches_fp64_model(dev, shape, target):
    import myNet

    bs, topk, T, F = shape
    torch.manual_seed(5)
    d = myNet.Discriminator(T, F, precision="fp32").to(dev)
    ref = _ref_of(d)
    x = R.make_input(bs * topk, T, F, 3).view(bs, topk, T, F)
    xd = x.float().to(dev).requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    score = d(xd)
    assert score.shape == (bs * topk, 1)
    loss = nn.MSELoss()(score, torch.full_like(score, target))
    loss.backward()
    sr = ref(xr)
    lr_ = nn.MSELoss()(sr, torch.full_like(sr, target))
    lr_.backward()
    assert torch.allclose(score.detach().cpu().double(), sr.detach(), rtol=1e-5, atol=1e-6)
    assert abs(float(loss) - float(lr_)) <= 1e-5 * float(lr_)
    for (n, p), (_, q) in zip(d.named_parameters(), ref.named_parameters()):
        _close(p.grad, q.grad, n)
    _close(xd.grad, xr.grad, "spec")
    # no input gradient asked: the parameter gradients are the same bits
    d.zero_grad()
    nn.MSELoss()(d(x.float().to(dev)), torch.full_like(score, target)).backward()
    d2 = {n: p.grad.clone() for n, p in d.named_parameters()}
    d.zero_grad()
    xd.grad = None
    nn.MSELoss()(d(xd), torch.full_like(score, target)).backward()
    for n, p in d.named_parameters():
        assert torch.equal(p.grad, d2[n]), n


def _op_inputs(dev, N, T, F, grad=True):
    P = R.make_params(T, F, 9)
    a = [R.make_input(N, T, F, 9).float().to(dev)] + [P[k].float().to(dev) for k in R.KEYS]
    return [t.requires_grad_(grad) for t in a]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_ops_equal_the_function_bitwise(dev, prec):
    N, T, F = 3, 23, 33
    a, b = _op_inputs(dev, N, T, F), _op_inputs(dev, N, T, F)
    sa = ag.DiscriminatorFn.apply(*a, prec)
    sb, y1, y2, y3 = torch.ops.dl4ss.discriminator(*b, prec)
    assert torch.equal(sa, sb)
    assert y1.dtype == (torch.bfloat16 if prec == "bf16" else torch.float32) and y3.shape == (N, 2, 3, 64)
    ds = torch.randn(N, 1, device=dev)
    ga = torch.autograd.grad(sa, a, ds)
    gb = torch.autograd.grad(sb, b, ds)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)
    # the backward op by itself, without the input gradient
    out = torch.ops.dl4ss.discriminator_bwd(ds, b[0].detach(), b[1].detach(), b[3].detach(), b[5].detach(),
                                            b[7].detach(), sb.detach(), y1, y2, y3, prec, False)
    assert out[0].numel() == 0
    for x, y in zip(out[1:], gb[1:]):
        assert torch.equal(x, y)


def test_op_opcheck(dev):
    a = _op_inputs(dev, 2, 16, 18)
    torch.library.opcheck(torch.ops.dl4ss.discriminator.default, (*a, "fp32"),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    s, y1, y2, y3 = torch.ops.dl4ss.discriminator(*[t.detach() for t in a], "fp32")
    d = [t.detach() for t in a]
    torch.library.opcheck(torch.ops.dl4ss.discriminator_bwd.default,
                          (torch.randn(2, 1, device=dev), d[0], d[1], d[3], d[5], d[7], s, y1, y2, y3, "fp32", True),
                          test_utils=("test_schema", "test_faketensor"))


# --------------------------------------------------------------------------------------------- the driver
def _batch(B, T, F, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    mix = np.abs(r.normal(0.0, 1.0, size=(B, T, F))).astype(np.float32)
    spk = np.stack([np.sort(r.choice(101, size=2, replace=False)) for _ in range(B)])
    Y = (np.abs(r.normal(0.0, 0.7, size=(B, 2, T, F)))).astype(np.float32)
    return {"mix_feas": mix,
            "multi_spk_fea_list": [{SPK[spk[b, k]]: Y[b, k] for k in range(2)} for b in range(B)]}


def _snap(mod):
    return {n: p.detach().clone() for n, p in mod.named_parameters()}


@pytest.mark.parametrize("detach_fake", [False, True])
def test_driver_train_step(dev, detach_fake):
    import main_run_sstune_dis as drv

    B, T, F = 2, 31, 129
    torch.manual_seed(11)
    m, opt = drv.build(F, T, 101, 2)
    assert len(opt.param_groups) == 6
    assert [id(p) for p in opt.param_groups[5]['params']] == [id(p) for p in m['dis_layer'].parameters()]
    before = {k: _snap(v) for k, v in m.items()}
    ref = _ref_of(m['dis_layer'])
    after_first = []
    step = opt.step

    def counting_step():
        step()
        after_first.append(_snap(m['mix_hidden_layer_3d']))

    opt.step = counting_step
    out = drv.train_step(m, opt, _batch(B, T, F, 17), D2I, I2D, 101, detach_fake=detach_fake)
    torch.cuda.synchronize()
    assert len(after_first) == 2  # the two zero_grad / step pairs
    for k in ("loss", "loss_dis", "loss_adv", "loss_mask", "loss_sum"):
        assert np.isfinite(float(out[k])), k
    for n, p in m['dis_layer'].named_parameters():
        assert not torch.equal(p.detach(), before['dis_layer'][n]), f"dis_layer.{n} did not move"
    for n, p in m['mix_speech_classifier'].named_parameters():
        assert torch.equal(p.detach(), before['mix_speech_classifier'][n]), f"classifier {n} moved"
    moved_first = [n for n, p in after_first[0].items() if not torch.equal(p, before['mix_hidden_layer_3d'][n])]
    if detach_fake:
        assert not moved_first, moved_first   # the first step touches the Discriminator alone
    else:
        assert moved_first                    # the reference's undetached fake reaches the mask net
    assert any(not torch.equal(p, before['mix_hidden_layer_3d'][n]) for n, p in after_first[1].items())

    # the Discriminator's gradients of loss_dis and dL/dpred of the adversarial term, against fp64
    pred = out["pred"].cpu().double().requires_grad_(True)
    y_true = out["y_true"].cpu().double()
    st, sf = ref(y_true), ref(pred)
    assert torch.allclose(out["score_true"].cpu().double(), st.detach(), rtol=1e-5, atol=1e-6)
    assert torch.allclose(out["score_false"].cpu().double(), sf.detach(), rtol=1e-5, atol=1e-6)
    mse = nn.MSELoss()
    loss_dis = mse(st, torch.ones_like(st)) + mse(sf, torch.zeros_like(sf))
    assert abs(float(out["loss_dis"]) - float(loss_dis)) <= 1e-5 * float(loss_dis)
    g = torch.autograd.grad(loss_dis, list(ref.parameters()), retain_graph=True)
    for (n, _), gr in zip(ref.named_parameters(), g):
        _close(out["dis_grads"][n], gr, n)
    (dp,) = torch.autograd.grad(mse(sf, torch.ones_like(sf)), pred)
    _close(out["dpred_adv"], dp, "dL/dpred")


def test_driver_other_utterance_true_maps(dev):
    """train_step(..., y_true_map=...): the maps of main_run_sstune_dis_sp.py:613-624 reach the Discriminator"""
    import main_run_sstune_dis as drv

    B, T, F = 2, 31, 129
    torch.manual_seed(12)
    m, opt = drv.build(F, T, 101, 2)
    other = np.abs(np.random.Generator(np.random.PCG64(4)).normal(0, 1, size=(B, 2, T, F))).astype(np.float32)
    out = drv.train_step(m, opt, _batch(B, T, F, 18), D2I, I2D, 101, run_classifier=False, y_true_map=other)
    assert torch.equal(out["y_true"].cpu(), torch.from_numpy(other))
    assert np.isfinite(float(out["loss"])) and np.isfinite(float(out["loss_dis"]))


def test_driver_save_params_writes_the_five_files(dev, tmp_path):
    """dis.py:653-662: emblayer, hidden3d, attlayer, adjlayer, dislayer under param_mix{mode}ag_{DATASET}_*"""
    import config_WSJ0_dB as cfg
    import main_run_sstune_dis as drv
    from dl4ss_amd import checkpoint

    m, _ = drv.build(129, 31, 101, 2)
    paths = drv.save_params(m, 15, str(tmp_path))
    tag = f"mixdotag_{cfg.DATASET}"
    assert sorted(os.path.basename(p) for p in paths.values()) == sorted(
        f"param_{tag}_{kind}_15" for kind in ("emblayer", "hidden3d", "attlayer", "adjlayer", "dislayer"))
    for kind, mod in (("emblayer", "mix_speech_multiEmbedding"), ("hidden3d", "mix_hidden_layer_3d"),
                      ("attlayer", "att_speech_layer"), ("adjlayer", "adjust_layer")):
        sd = torch.load(paths[kind], map_location="cpu", weights_only=True)
        own = m[mod].state_dict()
        assert list(sd) == list(own) and all(torch.equal(sd[k], own[k].cpu()) for k in sd), kind
    fresh = drv.Discriminator(31, 129)
    checkpoint.load_reference_discriminator(fresh, paths["dislayer"])
    for k, v in m["dis_layer"].state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v.cpu()), k


def test_driver_main_loop(dev, tmp_path):
    """main(): loader ('global' + 'once' batches of predata_fromList), the GAN steps, the LR halving"""
    import config_WSJ0_dB as cfg
    import main_run_sstune_dis as drv

    saved = (cfg.BATCH_SIZE, cfg.MAX_LEN, cfg.Load_param)
    cfg.BATCH_SIZE, cfg.MAX_LEN, cfg.Load_param = 2, 4000, False
    try:
        m, hist = drv.main(max_epoch=1, max_batches=2, log=lambda *a: None, save_dir=str(tmp_path))
    finally:
        cfg.BATCH_SIZE, cfg.MAX_LEN, cfg.Load_param = saved
    assert len(hist) == 2 and all(np.isfinite(v) for pair in hist for v in pair)
    assert "dis_layer" in m and not os.listdir(str(tmp_path))  # files are written from epoch 10 on (:649)
