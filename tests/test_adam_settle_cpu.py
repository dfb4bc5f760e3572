"""The refusal arithmetic of check(), without a device: adam.timed_out_steps / GuardedAdam.settle behind
SepTrainer.check() and ClassifierTrainer.check() against the formulas those methods carried before the optimizers
became GuardedAdam objects, written out literally below.

The trainers are built on the CPU device (construction only allocates), the status word and the non-finite counters
are set to what the kernels would have left, and check() runs with the device synchronisation stubbed out.
What the kernels leave in status[1] follows from the entry points: a timed-out step is counted once by every update
that goes through a 2-int status form -- the net's Adam, the voiceprint encoder's, each *clipped* Discriminator
update -- and not by the unclipped Discriminator update (dl4ss_adam_guarded, the 1-int form); a non-finite
refusal (clipped updates only, on steps that did not time out) is counted once."""
import itertools

import pytest
import torch

from dl4ss_amd import classifier, engine, infer
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintNet

B, K, N = 2, 2, 2048  # T = 17 frames: above the Discriminator's 15
STEPS, ADV_STEPS = 100, 200  # the counts before check()
CASES = list(itertools.product(range(4), range(3), range(3)))  # timed-out steps, net / Discriminator non-finite


@pytest.fixture(autouse=True)
def no_sync(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)


def old_sep_check(s, refused, nf, nf_adv, n_disc, clip, adv_clip, vnet):
    """SepTrainer.check() as it was: (taken out of step_count, out of adv_step_count, added to skipped_nonfinite,
    to adv_skipped_nonfinite, the RuntimeError's message or None)."""
    if not (s or refused):
        return 0, 0, 0, 0, None
    nf = nf if clip else 0
    nf_adv = nf_adv if adv_clip else 0
    timed_out = (refused - nf - nf_adv) // (1 + (n_disc if adv_clip else 0) + (1 if vnet else 0))
    d_step, d_adv = timed_out + nf, (timed_out * n_disc + nf_adv) if n_disc else 0
    if not (s or timed_out):
        return d_step, d_adv, nf, nf_adv, None
    where = "on this rank" if s else "on a data-parallel peer"
    return d_step, d_adv, nf, nf_adv, f"BiRNN hand-off timed out {where} (status {s}): {timed_out} update(s) refused"


def old_cls_check(s, refused, nonfinite):
    """ClassifierTrainer.check() as it was: (taken out of step_count, added to skipped_nonfinite, message or None)."""
    if not (s or refused):
        return 0, 0, None
    if s or refused > nonfinite:
        return refused, nonfinite, f"BiRNN hand-off timed out (status {s}): {refused - nonfinite} update(s) refused"
    return refused, nonfinite, None


def _sep(n_disc, clip, adv_clip, vnet):
    net = engine.SepNet(cell="lstm", num_layers=1, hidden=40, adjust=not vnet, device="cpu")
    kw = dict(clip_norm=1.0 if clip else None)
    if n_disc:
        kw.update(adversary=engine.DiscNet(17, 129, device="cpu"), disc_adv_update=n_disc == 2,
                  adv_clip_norm=1.0 if adv_clip else None)
    if vnet:
        kw.update(voiceprint=VoiceprintNet(device="cpu"), memory=SpeakerMemory(101, 50, device="cpu"))
    return engine.SepTrainer(net, B, K, N, **kw)


# adversary none / one update / two, each clip on or off; the voiceprint step takes neither clip nor adversary
CONFIGS = [(0, clip, False, False) for clip in (False, True)] + \
    [(n, clip, adv_clip, False) for n in (1, 2) for clip in (False, True) for adv_clip in (False, True)] + \
    [(0, False, False, True)]


@pytest.mark.parametrize("n_disc,clip,adv_clip,vnet", CONFIGS)
def test_sep_trainer_check(n_disc, clip, adv_clip, vnet):
    tr = _sep(n_disc, clip, adv_clip, vnet)
    for (t, nf, nf_adv), s in itertools.product(CASES, (0, 3)):
        if (nf and not clip) or (nf_adv and not adv_clip):
            continue  # (s == 0 with t > 0: a data-parallel peer's time-out; s != 0 with t == 0: checked before Adam)
        # what the kernels leave in status[1]: per timed-out step one count from each counted update
        refused = t * (1 + (n_disc if adv_clip else 0) + (1 if vnet else 0)) + nf + nf_adv
        tr.step_count, tr.skipped_nonfinite = STEPS, 0
        tr.status[0], tr.status[1] = s, refused
        tr.rnn_ws_all.fill_(1)
        if clip:
            tr.opt.nonfinite[0] = nf
        if n_disc:
            tr.adv_step_count, tr.adv_skipped_nonfinite = ADV_STEPS, 0
        if adv_clip:
            tr.adv_opt.nonfinite[0] = nf_adv
        if vnet:
            tr.vp_enc.rnn_ws.fill_(1)
        d_step, d_adv, sk, sk_adv, msg = old_sep_check(s, refused, nf, nf_adv, n_disc, clip, adv_clip, vnet)
        if msg is None:
            tr.check()
        else:
            with pytest.raises(RuntimeError) as e:
                tr.check()
            assert str(e.value) == msg
        what = (t, nf, nf_adv, s)
        assert (tr.step_count, tr.skipped_nonfinite) == (STEPS - d_step, sk), what
        assert tr.adv_skipped_nonfinite == sk_adv, what
        if n_disc:
            assert tr.adv_step_count == ADV_STEPS - d_adv, what
        assert tr.status.tolist() == [0, 0], what
        assert not clip or int(tr.opt.nonfinite) == 0, what
        assert not adv_clip or int(tr.adv_opt.nonfinite) == 0, what
        # the hand-off workspaces are zeroed exactly when check() raises
        assert bool(tr.rnn_ws_all.any()) == (msg is None), what
        assert not vnet or bool(tr.vp_enc.rnn_ws.any()) == (msg is None), what


@pytest.mark.parametrize("clip", [False, True])
def test_classifier_trainer_check(clip):
    cnet = infer.ClassifierNet(hidden=40, num_layers=2, num_labels=11, device="cpu")
    tr = classifier.ClassifierTrainer(cnet, 3, 2, 3000, clip_norm=1.0 if clip else None)
    for t, nf, s in itertools.product(range(4), range(3), (0, 3)):
        if nf and not clip:
            continue
        refused = t + nf
        tr.step_count, tr.skipped_nonfinite = STEPS, 0
        tr.status[0], tr.status[1] = s, refused
        tr.rnn_ws.fill_(1)
        if clip:
            tr.opt.nonfinite[0] = nf
        d_step, sk, msg = old_cls_check(s, refused, nf)
        if msg is None:
            tr.check()
        else:
            with pytest.raises(RuntimeError) as e:
                tr.check()
            assert str(e.value) == msg
        assert (tr.step_count, tr.skipped_nonfinite) == (STEPS - d_step, sk), (t, nf, s)
        assert tr.status.tolist() == [0, 0] and (not clip or int(tr.opt.nonfinite) == 0)
        assert bool(tr.rnn_ws.any()) == (msg is None)
