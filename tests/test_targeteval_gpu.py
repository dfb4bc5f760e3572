"""targeteval.TargetEvaluator (the Keras trees' eval_separation / eval_loss on the HIP path) and
SepTrainer.eval_loss (the trainer's own loss, forward only).

Metrics: the evaluator's intermediate pred = mask . |X| and the mixture's spectrum are taken from the device, the
waveform is rebuilt with oracle.dsp.istft in float64 on the CPU and scored with the fp64 restatement of
tests/bss_gain_ref.py.  What separates the two is the fp32 device iSTFT against the oracle's.  Measured on the
MI355X over the six cases below (the test prints each case's figure): the largest deviation of any of the eight
figures of any utterance was 5.771e-06 dB ('align', 3 speakers, unseen; the other cases 4.1e-07 .. 2.8e-06); the
bound is three times that, 1.74e-05 dB -- far inside the 1e-3 dB above which the cause would have to be found (a
relative waveform error of a few 1e-7 against components no more than 40 dB under the estimate bounds it at 4e-4).

SepTrainer.eval_loss: the oracle loss within tests/test_step_gpu.py's own bound for the step's loss (1e-4 fp32,
1e-2 bf16), every trainer buffer that must not change compared bit for bit, and step() after eval_loss() against
step() alone, bit for bit (fp32 with splitk_reduce="fixed", whose step repeats bitwise; the bf16 step does anyway).
"""
import numpy as np
import pytest
import torch

import bss_gain_ref as R
import test_step_gpu as ts
from dl4ss_amd import engine, ops, synth, targeteval
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintNet
from oracle import dsp, model as om

pytestmark = pytest.mark.gpu

MEASURED_DB = 5.8e-6  # the largest |device - oracle| of a dB figure over CASES (see the module docstring)
TOL_DB = 3 * MEASURED_DB
N, B, S, H = 4000, 2, 3, 40
T = ops.n_frames(N)
L_WAV = 128 * (T - 1)
# (attention, spk_num, background noise, seen speakers, log features)
CASES = [("dot", 2, False, True, False), ("dot", 3, True, False, False), ("align", 2, True, True, False),
         ("align", 3, False, False, False), ("dot", 3, False, True, True), ("dot", 2, True, False, True)]
LENGTHS = np.array([[4000, 3500, 3000], [3000, 2800, 3900], [3700, 4000, 2500]], dtype=np.int32)


def _inputs(dev):
    src, _, _ = synth.SyntheticMixtures(n_samples=N, k=S, seed=21).batch(3)
    raw = torch.from_numpy(src.astype(np.float32)).to(dev)
    clean, _, _ = synth.SyntheticMixtures(n_samples=1500, k=1, seed=22).batch(3)
    _, enrol = ops.stft(torch.from_numpy(clean[:, 0].astype(np.float32)).to(dev), complex_out=False)
    bgd = np.random.default_rng(23).standard_normal(N + 100)
    return raw, torch.from_numpy(LENGTHS).to(dev), enrol.contiguous(), bgd


def _evaluator(dev, attention, spk_num, noise, log, bgd, precision="fp32"):
    net = engine.SepNet(cell="lstm", num_layers=2, hidden=H, adjust=False, device=dev, seed=5, attention=attention)
    vnet = VoiceprintNet(hidden=25, device=dev, seed=6)
    memory = SpeakerMemory(5, 50, device=dev)
    memory.mem.copy_(torch.randn(5, 50, generator=torch.Generator().manual_seed(7)))
    return targeteval.TargetEvaluator(net, vnet, memory, B, N, spk_num=spk_num, bgd_noise=bgd if noise else None,
                                      log_features=log, precision=precision)


def _oracle_metrics(ev, n):
    """the eight figures of the first n utterances from the evaluator's device intermediates, on the CPU in fp64"""
    pred = ev.pred[:n].cpu().numpy().astype(np.float64)
    Xc = ev.Xc[:n].cpu().numpy().astype(np.float64)
    spec = Xc[..., 0] + 1j * Xc[..., 1]
    tgt, noi, mix = (x[:n, :L_WAV].cpu().numpy() for x in (ev.target, ev.noise, ev.mix))
    mix_len = ev.mix_len[:n].cpu().numpy()
    out = {k: [] for k in list(targeteval.METRICS) + [m + "_0" for m in targeteval.METRICS]}
    for b in range(n):
        wav = dsp.istft((pred[b] * np.exp(1j * np.angle(spec[b]))).T, dtype=np.float64)
        n_eff = min(int(mix_len[b]), L_WAV)
        m = R.target_metrics(tgt[b], noi[b], wav, mix[b], n_eff)
        m0 = R.target_metrics(tgt[b], noi[b], mix[b], mix[b], n_eff)
        for k in targeteval.METRICS:
            out[k].append(m[k])
            out[k + "_0"].append(m0[k])
    return {k: np.array(v) for k, v in out.items()}


@pytest.mark.parametrize("attention,spk_num,noise,seen,log", CASES)
def test_metrics_against_oracle_istft_and_restatement(dev, attention, spk_num, noise, seen, log):
    raw, lengths, enrol, bgd = _inputs(dev)
    ev = _evaluator(dev, attention, spk_num, noise, log, bgd)
    ids = torch.tensor([3, 0, 4], dtype=torch.int32, device=dev)
    worst, every = 0.0, {k: [] for k in ("SDR", "SIR", "SAR", "NSDR")}
    for lo, hi in ((0, 2), (2, 3)):  # a full batch, then a tail batch of one
        kw = dict(ids=ids[lo:hi]) if seen else dict(enrol=enrol[lo:hi])
        got = ev.evaluate(raw[lo:hi], lengths[lo:hi], **kw)
        ev.check()
        want = _oracle_metrics(ev, hi - lo)
        expect_len = LENGTHS[lo:hi, :max(2, spk_num)].max(1)
        assert (ev.mix_len[:hi - lo].cpu().numpy() == expect_len).all()
        for k, w in want.items():
            g = got[k].cpu().numpy()
            assert g.dtype == np.float64 and g.shape == (hi - lo,) and np.isfinite(w).all(), (k, g, w)
            dev_db = float(np.abs(g - w).max())
            worst = max(worst, dev_db)
            assert dev_db <= TOL_DB, (k, dev_db, g, w)
        for k in every:
            every[k].extend(got[k].cpu().numpy().tolist())
        if not noise and spk_num == 2:  # the mixture is target + noise exactly: no artefact in it
            assert (got["SAR_0"] > 100).all() or torch.isinf(got["SAR_0"]).all()
    print(f"targeteval deviation [{attention} spk{spk_num} noise{int(noise)} seen{int(seen)} log{int(log)}]: "
          f"{worst:.3e} dB  SDR {every['SDR']}")
    s = ev.summary()
    assert s["count"] == 3
    for k, v in every.items():
        assert s["G" + k] == pytest.approx(float(np.mean(v)), rel=1e-12, abs=1e-12)
    ev.reset()
    assert ev.summary()["count"] == 0 and np.isnan(ev.summary()["GSDR"])


@pytest.mark.parametrize("attention,seen", [("dot", True), ("align", False)])
def test_eval_loss_is_the_mse_of_the_first_interferer_mixture(dev, attention, seen):
    raw, lengths, enrol, bgd = _inputs(dev)
    ev = _evaluator(dev, attention, 3, True, False, bgd)  # spk_num 3 and noise: eval_loss must ignore both
    ids = torch.tensor([3, 0, 4], dtype=torch.int32, device=dev)
    for lo, hi in ((0, 2), (2, 3)):
        n = hi - lo
        kw = dict(ids=ids[lo:hi]) if seen else dict(enrol=enrol[lo:hi])
        loss = ev.eval_loss(raw[lo:hi], lengths[lo:hi], **kw)
        assert loss.is_cuda and loss.shape == (1,)
        pred = ev.pred[:n].cpu().numpy().astype(np.float64)
        tgt = ev.mag_tgt[:n].cpu().numpy().astype(np.float64)
        want = float(np.mean((pred - tgt) ** 2))
        assert abs(float(loss) - want) <= 1e-4 * want, (float(loss), want)
        # target + first interferer, no background: the assembled mixture is s_0 + s_1
        two = targeteval.assemble(ev._buffers(S)["srcs"], None, None, 2)[0]
        assert torch.equal(ev.mix[:n], two[:n])
        # and pred is the mask on that mixture's magnitudes: 0 <= pred <= |X|
        assert (ev.pred[:n] >= 0).all() and (ev.pred[:n] <= ev.mag_mix[:n] * (1 + 1e-6)).all()
    again = ev.eval_loss(raw[2:3], lengths[2:3], **(dict(ids=ids[2:3]) if seen else dict(enrol=enrol[2:3])))
    assert torch.equal(again, loss)


def test_evaluate_does_not_synchronise(dev):
    raw, lengths, enrol, bgd = _inputs(dev)
    ev = _evaluator(dev, "dot", 3, True, False, bgd)
    ids = torch.tensor([3, 0], dtype=torch.int32, device=dev)
    ev.evaluate(raw[:2], lengths[:2], ids=ids)  # (the first call allocates)
    ev.evaluate(raw[:2], lengths[:2], enrol=enrol[:2])
    ev.eval_loss(raw[:2], lengths[:2], ids=ids)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.evaluate(raw[:2], lengths[:2], ids=ids)
        ev.evaluate(raw[:1], lengths[:1], enrol=enrol[:1])
        ev.eval_loss(raw[:2], lengths[:2], ids=ids)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ev.check()
    assert ev.summary()["count"] == 7


def test_bf16_mask_net_stays_close(dev):
    """precision "bf16" (V rounded to bf16, as the bf16 training step reads it): the same pipeline, figures within
    1 dB of the fp32 ones on this small net"""
    raw, lengths, enrol, bgd = _inputs(dev)
    ids = torch.tensor([3, 0], dtype=torch.int32, device=dev)
    a = _evaluator(dev, "dot", 2, False, False, bgd).evaluate(raw[:2], lengths[:2], ids=ids)
    b = _evaluator(dev, "dot", 2, False, False, bgd, precision="bf16").evaluate(raw[:2], lengths[:2], ids=ids)
    for k in targeteval.METRICS:
        assert torch.isfinite(b[k]).all() and (a[k] - b[k]).abs().max() < 1.0, (k, a[k], b[k])


# ------------------------------------------------------------------ SepTrainer.eval_loss
# (precision, mode, cell, layers, B, K, N, the step-loss bound of tests/test_step_gpu.py for that precision)
TRAINER_CASES = [("fp32", "label", "lstm", 4, 2, 2, 4000, 1e-4), ("fp32", "pit", "gru", 2, 3, 2, 3000, 1e-4),
                 ("fp32", "crm", "gru", 2, 2, 2, 3000, 1e-4), ("bf16", "label", "lstm", 4, 4, 2, 8000, 1e-2),
                 ("bf16", "pit", "gru", 2, 3, 2, 3000, 1e-2)]


def _trainer(dev, precision, mode, cell, L, Bt, K, Nt):
    net = engine.SepNet(cell=cell, num_layers=L, crm=mode == "crm", device=dev, seed=3)
    kw = dict(splitk_reduce="fixed") if precision == "fp32" else {}
    return net, engine.SepTrainer(net, Bt, K, Nt, mode=mode, precision=precision, **kw)


@pytest.mark.parametrize("precision,mode,cell,L,Bt,K,Nt,tol", TRAINER_CASES)
def test_trainer_eval_loss(dev, precision, mode, cell, L, Bt, K, Nt, tol):
    src, spk, u = synth.SyntheticMixtures(n_samples=Nt, k=K, seed=3).batch(Bt)
    gains = synth.gains_for(u, K)
    batch = (torch.from_numpy(src.astype(np.float32)).to(dev), torch.from_numpy(gains.astype(np.float32)).to(dev),
             torch.from_numpy(spk.astype(np.int32)).to(dev))
    net, tr = _trainer(dev, precision, mode, cell, L, Bt, K, Nt)
    # the oracle's loss of the same batch
    ref = om.SepModel(cell=cell, num_layers=L, crm=mode == "crm")
    ref.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    feats, X, Y = ts._oracle_features(src, gains, mode == "crm")
    with torch.no_grad():
        mask = ref(feats, torch.from_numpy(spk))[0]
        loss_ref = float({"crm": om.loss_crm, "pit": om.loss_pit, "label": om.loss_label_ordered}[mode](mask, X, Y)[0])

    def state():
        return dict(flat=net.flat.clone(), grad=net.grad_ext.clone(), m=tr.m.clone(), v=tr.v.clone(),
                    status=tr.status.clone(), loss=tr.loss.clone(), step=tr.step_count, gen=net.generation)

    before = state()
    l1 = tr.eval_loss(*batch).clone()
    l2 = tr.eval_loss(*batch).clone()
    tr.check()
    assert torch.equal(l1, l2)
    assert abs(float(l1[0]) - loss_ref) <= tol * abs(loss_ref), (float(l1[0]), loss_ref)
    assert float(l1[0]) == pytest.approx(float(l1[1] + l1[2]), rel=1e-6)
    after = state()
    for k, v in before.items():
        assert torch.equal(v, after[k]) if isinstance(v, torch.Tensor) else v == after[k], k
    # step() after eval_loss() against step() alone, from the same seed
    la = tr.step(*batch).clone()
    tr.check()
    net2, tr2 = _trainer(dev, precision, mode, cell, L, Bt, K, Nt)
    lb = tr2.step(*batch).clone()
    tr2.check()
    assert torch.equal(la, lb), (la, lb)
    assert torch.equal(net.flat, net2.flat) and torch.equal(net.grad, net2.grad)
    # the step's loss is the loss eval_loss reported for the same parameters (two kernels: COST and GRAD)
    assert abs(float(la[0]) - float(l1[0])) <= tol * abs(loss_ref)
    # and it is eager on a trainer that holds a captured graph
    if precision == "bf16" and mode == "pit":
        tr.step_graph(*batch)
        p = net.flat.clone()
        e1 = tr.eval_loss(*batch).clone()
        assert torch.equal(net.flat, p) and torch.isfinite(e1).all()
        lg = tr.step_graph(*batch).clone()
        tr.check()
        assert abs(float(lg[0]) - float(e1[0])) <= tol * abs(float(e1[0]))


def test_trainer_eval_loss_ignores_an_adversary_and_refuses_query_trainers(dev):
    from dl4ss_amd.params import DiscNet

    Bt, K, Nt = 2, 2, 4000
    src, spk, u = synth.SyntheticMixtures(n_samples=Nt, k=K, seed=3).batch(Bt)
    batch = (torch.from_numpy(src.astype(np.float32)).to(dev),
             torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(dev),
             torch.from_numpy(spk.astype(np.int32)).to(dev))
    net = engine.SepNet(cell="lstm", num_layers=2, hidden=H, device=dev, seed=3)
    plain = engine.SepTrainer(net, Bt, K, Nt).eval_loss(*batch).clone()
    net_a = engine.SepNet(cell="lstm", num_layers=2, hidden=H, device=dev, seed=3)
    tr = engine.SepTrainer(net_a, Bt, K, Nt, adversary=DiscNet(ops.n_frames(Nt), device=dev))
    d0 = tr.adversary.flat.clone()
    assert torch.equal(tr.eval_loss(*batch), plain)
    assert torch.equal(tr.adversary.flat, d0) and tr.adv_step_count == 0
    net_v = engine.SepNet(cell="lstm", num_layers=2, hidden=H, adjust=False, device=dev, seed=3)
    trv = engine.SepTrainer(net_v, Bt, K, Nt, voiceprint=VoiceprintNet(hidden=25, device=dev),
                            memory=SpeakerMemory(101, 50, device=dev))
    with pytest.raises(ValueError, match="TargetEvaluator.eval_loss"):
        trv.eval_loss(*batch)
