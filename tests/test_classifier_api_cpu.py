"""CPU-side checks of the classifier-training surface: the driver mirror's imports resolve to the
reference's module names, and a ClassifierNet round-trips through the reference checkpoint layout."""
import importlib
import os

import torch

from dl4ss_amd import checkpoint, compat, infer


def test_train_driver_imports_resolve():
    compat.install()
    drv = importlib.import_module("dl4ss_amd.compat.drivers.train_multi_labels_speech")
    for name in ("build", "train_step", "main", "MIX_SPEECH_classifier", "count_multi_acc", "multi_label_vector",
                 "prepare_data"):
        assert hasattr(drv, name), name
    import config
    import myNet
    import test_multi_labels_speech as tmls
    from dl4ss_amd.compat import multi_labels_acc

    assert drv.config is config and drv.myNet is myNet
    # the reference's surface: count_multi_acc under its module name (restated in compat/multi_labels_acc.py)
    assert drv.count_multi_acc is tmls.count_multi_acc is multi_labels_acc.count_multi_acc
    assert drv.multi_label_vector is tmls.multi_label_vector
    # the reference's model: BiLSTM(F, 2 HIDDEN_UNITS, 3 layers) and its parameter names
    net = drv.MIX_SPEECH_classifier(129, 10, 7)
    names = dict(net.named_parameters())
    assert names["layer.weight_hh_l2_reverse"].shape == (4 * 2 * config.HIDDEN_UNITS, 2 * config.HIDDEN_UNITS)
    assert names["Linear.weight"].shape == (7, 4 * config.HIDDEN_UNITS)
    # the save rule of test_multi_labels_speech.py:447
    saved = [e for e in range(40) if e > 10 and e % 5 == 0]
    assert saved == [15, 20, 25, 30, 35] and "epoch15" in drv.save_path(15)


def test_save_reference_classifier_round_trips(tmp_path):
    a = infer.ClassifierNet(hidden=24, num_layers=3, num_labels=9, device="cpu", seed=4)
    path = checkpoint.save_reference_classifier(a, os.path.join(tmp_path, "params", "param_speech_test"))
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert set(sd) == {n for n, _ in a.specs} and all(k.startswith(("layer.", "Linear.")) for k in sd)
    b = infer.ClassifierNet(hidden=24, num_layers=3, num_labels=9, device="cpu", seed=5)
    assert not torch.equal(a.flat, b.flat)
    checkpoint.load_reference_classifier(b, path)
    assert torch.equal(a.flat, b.flat)  # bitwise
    # what the drivers' load_params does with the file: a module load_state_dict of the same keys
    from oracle import recursive

    m = recursive.Classifier(hidden=24, num_layers=3, num_labels=9)
    m.load_state_dict(sd)
    assert sorted(n for n, _ in a.named_parameters()) == sorted(n for n, _ in m.named_parameters())
    for n, p in a.named_parameters():  # (name, tensor) pairs, as torch's
        assert torch.equal(p, sd[n])
