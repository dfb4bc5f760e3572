"""Gradient clipping's host surface without a GPU: the three entry points are bound and exported, the number
of partials is a function of n alone with the documented range, and what SepTrainer(clip_norm=...,
adv_clip_norm=...) refuses -- before any device call, so a CPU net is enough to see it."""
import inspect

import pytest

from dl4ss_amd import _lib, classifier, engine, ops

SYMS = ("dl4ss_grad_sumsq_parts", "dl4ss_grad_sumsq", "dl4ss_adam_clipped")


def test_symbols_are_bound_and_exported():
    for s in SYMS:
        assert s in _lib.SIGNATURES and s in _lib.exported_symbols() and hasattr(_lib.lib(), s)
    # the clipped Adam: the shadow form's arguments, then part, n_part, max_norm, gnorm, nonfinite before the stream
    base = _lib.SIGNATURES["dl4ss_adam_guarded_dp_scaled_bf16"]
    assert _lib.SIGNATURES["dl4ss_adam_clipped"] == base[:-1] + [_lib.P, _lib.I, _lib.F, _lib.P, _lib.P] + base[-1:]
    assert "clip" in inspect.signature(ops.adam_).parameters and callable(ops.grad_sumsq)
    assert inspect.signature(ops.adam_).parameters["clip"].default is None
    for cls, names in ((engine.SepTrainer, ("clip_norm", "adv_clip_norm")), (classifier.ClassifierTrainer, ("clip_norm",))):
        for n in names:
            assert inspect.signature(cls.__init__).parameters[n].default is None


def test_parts_is_a_function_of_n_alone():
    parts = ops.grad_sumsq_parts
    assert parts(1) == 1 and parts(0) == 1
    ns = [1, 2, 3, 4, 5, 1027, 4096, 4097, 8192, 8193, 10 ** 5, 10 ** 6, 11_400_000, 2 ** 22, 2 ** 22 + 1, 2 ** 31 + 5,
          2 ** 40]
    got = [parts(n) for n in ns]
    assert all(1 <= p <= 1024 for p in got), got
    assert got == sorted(got), got
    assert got[-1] == 1024 and parts(11_400_000) == 1024  # the flagship gradient uses the largest grid
    assert [parts(n) for n in ns] == got  # the same answer when asked again


def _net():
    return engine.SepNet(cell="gru", num_layers=1, device="cpu", seed=1)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("-inf")])
def test_clip_norm_must_be_positive(bad):
    with pytest.raises(ValueError, match="clip_norm"):
        engine.SepTrainer(_net(), 2, 2, 4000, clip_norm=bad)
    with pytest.raises(ValueError, match="clip_norm"):
        ops.check_clip_norm(bad)


@pytest.mark.parametrize("bad", [0.0, -2.0, float("nan")])
def test_adv_clip_norm_must_be_positive(bad):
    disc = engine.DiscNet(32, 129, device="cpu")
    with pytest.raises(ValueError, match="adv_clip_norm"):
        engine.SepTrainer(_net(), 2, 2, 4000, adversary=disc, adv_clip_norm=bad)


def test_adv_clip_norm_needs_an_adversary():
    with pytest.raises(ValueError, match="adv_clip_norm needs an adversary"):
        engine.SepTrainer(_net(), 2, 2, 4000, adv_clip_norm=1.0)
    with pytest.raises(ValueError, match="adv_clip_norm needs an adversary"):
        engine.SepTrainer(_net(), 2, 2, 4000, clip_norm=1.0, adv_clip_norm=float("inf"))


def test_inf_is_a_valid_threshold():
    assert ops.check_clip_norm(float("inf")) == float("inf") and ops.check_clip_norm(200) == 200.0
