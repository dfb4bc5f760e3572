"""The training step fed from a device-resident corpus: SepTrainer.step_corpus / step_graph_corpus / eval_loss_corpus
and corpus.features give, bit for bit, what step / step_graph / eval_loss and wsj0list.features give for the same
clips uploaded as a zero-padded (B, K, N) array -- only where the sources come from differs.

SepNet(num_layers=2), B = 4, K = 2, N = 8000, a synthetic 16-bit PCM corpus with ragged lengths (so every fp64 sum in
the statistics is exact and the two mixing paths agree bitwise); the bf16 steps and the fp32 step with
splitk_reduce="fixed" repeat bit for bit, so every loss and net.flat must be equal."""
import random

import numpy as np
import pytest
import torch

from dl4ss_amd import checkpoint, corpus as cp, engine, infer, classifier, wsj0list as wl
from test_wsj0list_cpu import _dataset

pytestmark = pytest.mark.gpu
B, K, N, STEPS = 4, 2, 8000, 3
SETTINGS = {"bf16": dict(precision="bf16", mode="pit"),
            "fp32-fixed": dict(precision="fp32", mode="label", splitk_reduce="fixed")}


def _corpus(dev, full=False):
    """6 speakers x 3 clips of 16-bit PCM, lengths ragged in [N / 2, N] (``full``: every clip N samples)"""
    rng = np.random.default_rng(12)
    clips = []
    for s in range(6):
        for j in range(3):
            n = N if (full or j == 0) else int(rng.integers(N // 2, N))
            t = np.arange(n) / 8000.0
            x = np.sin(2 * np.pi * (110 + 23 * s + 7 * j) * t) * (0.5 + 0.4 * np.sin(2 * np.pi * 3 * t + s))
            x = 6000 * x + rng.normal(200, 300, n)
            clips.append((f"spk{s}", f"utt{s}{j}", x.round().astype(np.int16)))
    return cp.DeviceCorpus.from_clips(clips, N).to(dev)


def _batches(c, shifts=False):
    rng = np.random.default_rng(3)
    out = []
    for _ in range(STEPS):
        spk = np.stack([np.sort(rng.choice(6, K, replace=False)) for _ in range(B)]).astype(np.int32)
        clips = (3 * spk + rng.integers(0, 3, (B, K))).astype(np.int32)
        gains = rng.uniform(0.7, 1.6, (B, K)).astype(np.float32)
        sh = (rng.integers(0, N, (B, K)) % c.lengths[clips]).astype(np.int32) if shifts else None
        out.append((clips, gains, spk, sh))
    return out


def _trainer(dev, setting, seed=5):
    net = engine.SepNet(cell="lstm", num_layers=2, device=dev, seed=seed)
    return engine.SepTrainer(net, B, K, N, lr=2e-4, **SETTINGS[setting])


def _uploaded(dev, c, clips, gains, spk):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t(c.gather(clips, N)), t(gains), t(spk), t(c.lengths[clips])


def _run(tr, steps):
    losses = [step().clone() for step in steps]
    tr.check()
    losses = torch.stack(losses)
    assert losses.isfinite().all() and tr.step_count == len(steps)
    return losses, tr.net.flat.clone()


def _same(a, b):
    assert torch.equal(a[0], b[0]), (a[0], b[0])
    assert torch.equal(a[1], b[1]), float((a[1] - b[1]).abs().max())


@pytest.mark.parametrize("augment", [False, True])
def test_features_equal_the_list_loaders(dev, tmp_path, augment):
    lst, data, _ = _dataset(tmp_path)
    max_len = 10000
    c = cp.DeviceCorpus.from_tree(data, "train", max_len, device=dev)
    assert c.pool.dtype == np.int16
    random.seed(3)
    (want,) = list(wl.ListBatches(lst, data, "train", 3, max_len, augment=augment))
    random.seed(3)
    (got,) = list(cp.ListMixSampler(c, lst, 3, augment=augment))
    assert (got["shifts"] is not None) == augment
    a, b = cp.features(c, got, dev), wl.features(want, dev)
    for k in ("src", "mix", "mix_mag", "mix_complex", "src_spec"):
        assert torch.equal(a[k], b[k]), k
    assert a["src"].shape == (3, 2, max_len) and a["src"].abs().max() > 0.5
    cs = cp.features(c, got, dev, complex_sources=True)["src_spec"]
    assert torch.equal(cs, wl.features(want, dev, complex_sources=True)["src_spec"])


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_step_corpus_equals_step_on_uploaded_clips(dev, setting):
    c = _corpus(dev)
    batches = _batches(c)
    a, b = _trainer(dev, setting), _trainer(dev, setting)
    want = _run(a, [lambda x=x: a.step(*_uploaded(dev, c, *x[:3])) for x in batches])
    got = _run(b, [lambda x=x: b.step_corpus(c, x[0], x[1], x[2]) for x in batches])  # (speaker ids from the host)
    _same(got, want)
    # the validation loss likewise, and it leaves the parameters alone
    x = batches[0]
    ea = a.eval_loss(*_uploaded(dev, c, *x[:3])).clone()
    eb = b.eval_loss_corpus(c, x[0], x[1], torch.from_numpy(x[2]).to(dev)).clone()
    assert torch.equal(ea, eb) and torch.equal(b.net.flat, got[1]) and bool(eb.isfinite().all())


def test_step_graph_corpus_equals_step_graph(dev):
    """bf16, full-length clips (step_graph takes no lengths): one eager step each, then two replayed ones"""
    c = _corpus(dev, full=True)
    batches = _batches(c)
    a, b = _trainer(dev, "bf16"), _trainer(dev, "bf16")
    spk = [torch.from_numpy(x[2]).to(dev) for x in batches]
    up = [_uploaded(dev, c, *x[:3]) for x in batches]
    want = _run(a, [lambda: a.step(*up[0])] + [lambda i=i: a.step_graph(*up[i][:3]) for i in (1, 2)])
    got = _run(b, [lambda: b.step_corpus(c, batches[0][0], batches[0][1], spk[0])] +
               [lambda i=i: b.step_graph_corpus(c, batches[i][0], batches[i][1], spk[i]) for i in (1, 2)])
    _same(got, want)


def test_step_graph_corpus_ragged_and_rotated_equals_eager(dev):
    c = _corpus(dev)
    batches = _batches(c, shifts=True)
    assert any((c.lengths[x[0]] < N).any() for x in batches) and all(x[3].any() for x in batches)
    a, b = _trainer(dev, "bf16"), _trainer(dev, "bf16")
    call = lambda fn, x: fn(c, x[0], x[1], torch.from_numpy(x[2]).to(dev), shifts=x[3])
    want = _run(a, [lambda x=x: call(a.step_corpus, x) for x in batches])
    got = _run(b, [lambda: call(b.step_corpus, batches[0])] +
               [lambda x=x: b.step_graph_corpus(c, x[0], x[1], torch.from_numpy(x[2]), shifts=x[3])
                for x in batches[1:]])  # (speaker ids as a CPU tensor)
    _same(got, want)
    # the rotation reached the step: the same batches unrotated train another net
    u = _trainer(dev, "bf16")
    other = _run(u, [lambda x=x: u.step_corpus(c, x[0], x[1], torch.from_numpy(x[2]).to(dev)) for x in batches])
    assert not torch.equal(other[1], want[1])


def test_out_of_range_clip_id_is_reported_by_check(dev):
    c = _corpus(dev)
    tr = _trainer(dev, "bf16")
    clips, gains, spk, _ = _batches(c)[0]
    clips = clips.copy()
    clips[1, 0], clips[3, 1] = len(c), -1
    tr.step_corpus(c, clips, gains, torch.from_numpy(spk).to(dev))
    with pytest.raises(RuntimeError, match=r"2 clip id\(s\)"):
        tr.check()
    tr.check()  # reported once
    with pytest.raises(ValueError, match="max_len"):
        engine.SepTrainer(tr.net, B, K, N - 128, precision="bf16").features_corpus(c, clips, gains)


def test_resume_with_the_samplers_state(dev, tmp_path):
    """save_training_state(extra={"sampler": ...}) after two steps, a fresh trainer and sampler, two more steps:
    the four uninterrupted ones (the draws come from the module-level generators the state file holds)"""
    c = _corpus(dev)
    noise = c.index[("spk5", "utt52")]

    def start(seed, net_seed):
        random.seed(seed)
        np.random.seed(seed)
        return _trainer(dev, "bf16", seed=net_seed), cp.RandomMixSampler(c, B, K, K, db=5, augment=True,
                                                                         noise_clip=noise)

    def steps(tr, s, n):
        out = []
        for _ in range(n):
            b = s.batch()
            assert b["clips"].shape == (B, K + 1)
            out.append(tr.step_corpus(c, b["clips"], b["gains"], torch.from_numpy(b["speakers"]).to(dev),
                                      shifts=b["shifts"]).clone())
        tr.check()
        return out

    tr, s = start(5, 5)
    want = torch.stack(steps(tr, s, 4))
    want_flat = tr.net.flat.clone()
    tr, s = start(5, 5)
    head = steps(tr, s, 2)
    path = str(tmp_path / "state.pt")
    checkpoint.save_training_state(path, tr, extra={"sampler": s.state_dict()})
    tr2, s2 = start(99, 8)
    assert not torch.equal(tr2.net.flat, tr.net.flat)
    s2.load_state_dict(checkpoint.load_training_state(path, tr2)["sampler"])
    got = torch.stack(head + steps(tr2, s2, 2))
    assert torch.equal(got, want) and torch.equal(tr2.net.flat, want_flat) and tr2.step_count == 4


def test_classifier_features_corpus(dev):
    c = _corpus(dev)
    clips, gains, _, sh = _batches(c, shifts=True)[0]
    cnet = infer.ClassifierNet(hidden=40, num_layers=1, num_labels=11, device=dev, seed=2)
    b = classifier.ClassifierTrainer(cnet, B, K, N)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    from dl4ss_amd import ops
    _, mix = ops.mix_sources(t(c.gather(clips, N)), t(gains), lengths=t(c.lengths[clips]), shifts=t(sh))
    want = ops.stft(mix, complex_out=False, mag_out=True)[1]
    got = b.features_corpus(c, clips, gains, shifts=sh)
    assert torch.equal(got, want) and torch.equal(b.mix, mix)
    b.check()
    clips = clips.copy()
    clips[0, 0] = 1000
    b.features_corpus(c, clips, gains)
    with pytest.raises(RuntimeError, match=r"1 clip id\(s\)"):
        b.check()
