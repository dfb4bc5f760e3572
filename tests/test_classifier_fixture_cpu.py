"""The reference-pinned classifier training fixture (tests/golden/ref_cls_train.npz, written by
tests/golden/make_ref_classifier_fixture.py from the reference's own MIX_SPEECH_classifier,
count_multi_acc and optimizer / loss / step lines) against the project's CPU restatements."""
import os

import numpy as np
import torch

from conftest import ROOT
from dl4ss_amd import schedule
from dl4ss_amd.compat.multi_labels_acc import count_multi_acc
from oracle import recursive

FIX = os.path.join(ROOT, "tests", "golden", "ref_cls_train.npz")


def load():
    z = np.load(FIX)
    return {k: z[k] for k in z.files}


def test_oracle_step_reproduces_the_reference():
    """oracle.recursive.Classifier + MultiLabelSoftMarginLoss on its sigmoid output + Adam(1e-5):
    probabilities and loss to 1e-6, every gradient to 1e-5 of its largest element."""
    z = load()
    H, L, n_lab, F = (int(z[f"meta/{k}"]) for k in ("hidden", "layers", "n_lab", "F"))
    ref = recursive.Classifier(input_fre=F, hidden=H, num_layers=L, num_labels=n_lab)
    ref.load_state_dict({k[len("weight/"):]: torch.from_numpy(v) for k, v in z.items() if k.startswith("weight/")})
    opt = torch.optim.Adam(ref.parameters(), lr=float(z["meta/lr"]))
    prob = ref(torch.from_numpy(z["in/mix_feas"]))
    loss = torch.nn.MultiLabelSoftMarginLoss()(prob, torch.from_numpy(z["in/y_map"]))
    opt.zero_grad()
    loss.backward()
    assert np.abs(prob.detach().numpy() - z["out/prob"]).max() < 1e-6
    assert abs(float(loss) - float(z["out/loss"])) < 1e-6
    for name, p in ref.named_parameters():
        g = z[f"grad/{name}"]
        assert np.abs(p.grad.numpy() - g).max() <= 1e-5 * np.abs(g).max(), name
    # torch Adam against torch Adam on the same gradients: the updated parameters agree to two fp32 ulps
    # of the largest weight (|w| < 1 / sqrt(H) = 0.25 at H = 16: ulp 1.5e-8) -- 300 times finer than the
    # step itself (lr = 1e-5), so a skipped or reversed step cannot pass
    opt.step()
    for name, p in ref.named_parameters():
        assert np.abs(p.detach().numpy() - z[f"weight/{name}"]).max() > 0.5 * float(z["meta/lr"]), name
        assert np.abs(p.detach().numpy() - z[f"param/{name}"]).max() <= 3e-8, name


def test_count_multi_acc_reproduces_the_reference():
    z = load()
    y_spk = [list(map(int, line)) for line in z["in/y_spk"]]
    for key, kw in (("acc/top2", dict(alpha=-0.1, top_k_num=2)), ("acc/thr", dict(alpha=0.5, top_k_num=0))):
        got = count_multi_acc(z["out/prob"].copy(), y_spk, **kw)
        assert len(got) == 5
        assert [float(x) for x in got] == [float(x) for x in z[key]], (key, got, z[key])
    # the reference's return types: two float accuracies, two int counts, the float recall
    assert isinstance(got[0], float) and isinstance(got[1], float) and isinstance(got[4], float)
    assert int(got[2]) == z["out/prob"].size and int(got[3]) == z["out/prob"].shape[0]


def test_classifier_schedule():
    """lr /= 2 at every epoch_idx % 50 == 0 including epoch 0: 5e-6 for epochs 0-49, 2.5e-6 from 50."""
    s = schedule.classifier()
    lrs = [s.at_epoch_start(e) for e in range(101)]
    assert all(lr == 5e-6 for lr in lrs[:50])
    assert all(lr == 2.5e-6 for lr in lrs[50:100])
    assert lrs[100] == 1.25e-6
