"""Learning-rate schedules of the reference drivers.

* ``TDAA_beta/main_run_sstune_EvalVer.py:570-575``: at the start of every epoch with
  ``epoch_idx % 10 == 0`` each param group's lr is halved while it is ``>= 1e-7`` (so the
  first halving happens at epoch 0: training runs at 1e-4 from the start).
* ``Torch_multi/main_run_multi_selfSS_dB.py:441-444``: halved every 50 epochs, no floor.
* ``main_run_sstune_cRM_EvalVer.py:627-631`` has the 50-epoch / ``>= 5e-6`` form switched
  off (``if 0 and ...``): a constant lr.
* ``Torch_multi/test_multi_labels_speech.py:405-407`` (the speaker classifier): halved every 50
  epochs from epoch 0 on, no floor.

``SepTrainer.lr`` is read by every Adam launch, so applying a schedule is assigning it.
"""


class LRHalving:
    def __init__(self, lr, every, floor=None, enabled=True):
        self.lr, self.every, self.floor, self.enabled = lr, every, floor, enabled

    def at_epoch_start(self, epoch_idx):
        """The reference's per-epoch update; returns the lr for this epoch."""
        if self.enabled and epoch_idx % self.every == 0:
            if self.floor is None or self.lr >= self.floor:
                self.lr /= 2
        return self.lr

    def apply(self, trainer, epoch_idx):
        trainer.lr = self.at_epoch_start(epoch_idx)
        return trainer.lr

    def state_dict(self):
        """``lr`` is the state; ``every``, ``floor``, ``enabled`` say which schedule it is and are checked on load."""
        return {"lr": float(self.lr), "every": self.every, "floor": self.floor, "enabled": bool(self.enabled)}

    def check_state_dict(self, sd, where="schedule"):
        _check_fields(self, sd, where, ("every", "floor", "enabled"), {"lr": (int, float)})

    def load_state_dict(self, sd, checked=False):
        if not checked:
            self.check_state_dict(sd)
        self.lr = float(sd["lr"])


def evalver(lr=2e-4):
    """EvalVer.py:570-575."""
    return LRHalving(lr, every=10, floor=1e-7)


def selfss_db(lr=2e-4):
    """selfSS_dB.py:442-444."""
    return LRHalving(lr, every=50, floor=None)


def classifier(lr=1e-5):
    """Torch_multi/test_multi_labels_speech.py:405-407: halved at every epoch_idx % 50 == 0, epoch 0
    included, no floor -- the optimizer is built with 1e-5 (:395), so epochs 0-49 run at 5e-6."""
    return LRHalving(lr, every=50, floor=None)


def crm_evalver(lr=2e-4):
    """cRM_EvalVer.py:627 (disabled in the reference)."""
    return LRHalving(lr, every=50, floor=5e-6, enabled=False)


def _check_fields(obj, sd, where, fixed, state):
    """ValueError naming the first of the ``fixed`` fields of ``sd`` that is not ``obj``'s, or of the ``state``
    fields ({name: types}) that is missing or of another type; nothing is written."""
    if not isinstance(sd, dict):
        raise ValueError(f"{where}: not in the file")
    for k in fixed:
        if k not in sd or sd[k] != getattr(obj, k):
            raise ValueError(f"{where}.{k}: the file has {sd.get(k)!r}, this object has {getattr(obj, k)!r}")
    for k, types in state.items():
        if not isinstance(sd.get(k), types) or (isinstance(sd[k], bool) and bool not in types):
            want = " or ".join(t.__name__ for t in types)
            raise ValueError(f"{where}.{k}: the file has {sd.get(k)!r}, expected {want}")


class EarlyStopping:
    """The early stopping of the Keras trees (``Cocktail/software/DL4SS_Keras/nnet.py:159-172``), host logic only.

    After every epoch's validation loss, ``update(epoch, dev_loss)`` says whether to snapshot the weights (the
    reference's ``save_weights``): from epoch ``start`` (``START_EALY_STOP``) on, when the loss is below the lowest
    seen so far.  Epochs before ``start`` neither snapshot nor stop.  ``stop`` is then set by the reference's two
    conditions -- ``patience`` (10) epochs since the best one, or the last epoch ``max_epoch - 1`` -- and
    ``best_epoch`` names the snapshot to restore (``start`` itself until one improved: the reference would load a
    file it never wrote).  A NaN loss never counts as an improvement (``nan < x`` is false)."""

    def __init__(self, start, patience=10, max_epoch=None):
        self.start, self.patience, self.max_epoch = int(start), int(patience), max_epoch
        self.best_loss = float("inf")
        self.best_epoch = self.start
        self.stop = False

    def update(self, epoch, dev_loss):
        snapshot = False
        if epoch >= self.start:
            if dev_loss < self.best_loss:
                self.best_loss, self.best_epoch = float(dev_loss), epoch
                snapshot = True
            if epoch - self.best_epoch >= self.patience or \
                    (self.max_epoch is not None and epoch == self.max_epoch - 1):
                self.stop = True
        return snapshot

    def state_dict(self):
        """``best_loss``, ``best_epoch``, ``stop`` are the state; ``start``, ``patience``, ``max_epoch`` are checked."""
        return {"best_loss": float(self.best_loss), "best_epoch": int(self.best_epoch), "stop": bool(self.stop),
                "start": self.start, "patience": self.patience, "max_epoch": self.max_epoch}

    def check_state_dict(self, sd, where="stopper"):
        _check_fields(self, sd, where, ("start", "patience", "max_epoch"),
                      {"best_loss": (float,), "best_epoch": (int,), "stop": (bool,)})

    def load_state_dict(self, sd, checked=False):
        if not checked:
            self.check_state_dict(sd)
        self.best_loss, self.best_epoch, self.stop = sd["best_loss"], sd["best_epoch"], sd["stop"]
