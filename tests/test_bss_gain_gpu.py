"""dl4ss_bss_gain (BSS Eval 2.0's gain decomposition, batched) against the fp64 restatement of tests/bss_gain_ref.py
fed the same fp32 inputs.

Bound on finite criteria: 1e-6 dB.  Both sides are fp64 and differ by summation order only: <= 4001 x 1.1e-16 x
cond(G) (<= 1e4: tests/test_bss_gain_ref_cpu.py checks it on these inputs) ~ 4e-9 relative, about 2e-8 dB, with
margin.  inf / NaN positions and the singular count must match exactly."""
import numpy as np
import pytest
import torch

import bss_gain_ref as R
from dl4ss_amd import bss

pytestmark = pytest.mark.gpu
TOL_DB = 1e-6


def run(dev, srcs, ests, index, n_eff=None):
    le = None if n_eff is None else torch.as_tensor(n_eff, dtype=torch.int32, device=dev)
    (sdr, sir, sar), sing = bss.bss_eval_gain(torch.as_tensor(srcs).to(dev), torch.as_tensor(ests).to(dev), index, le)
    return torch.stack([sdr, sir, sar], -1).cpu().numpy(), int(sing.item())


def compare(got, want, what):
    assert (np.isnan(got) == np.isnan(want)).all(), (what, got, want)
    assert (np.isposinf(got) == np.isposinf(want)).all(), (what, got, want)
    assert (np.isneginf(got) == np.isneginf(want)).all(), (what, got, want)
    fin = np.isfinite(want)
    if fin.any():
        err = np.abs(got[fin] - want[fin]).max()
        assert err <= TOL_DB, (what, err)


@pytest.mark.parametrize("J,Ke", R.SHAPES)
@pytest.mark.parametrize("N", R.SIZES)
def test_against_restatement(dev, N, J, Ke):
    for M in R.BATCHES:
        srcs, ests, index = R.make_inputs(M, J, Ke, N)
        for kind in R.N_EFF_KINDS:
            n_eff = R.n_eff_of(kind, M, N)
            want, want_sing, _ = R.gain_batch(srcs, ests, index, n_eff)
            got, got_sing = run(dev, srcs, ests, index, n_eff)
            compare(got, want, (M, kind))
            assert got_sing == want_sing, (M, kind, got_sing, want_sing)
        got, got_sing = run(dev, srcs, ests, index, None)  # NULL n_eff = N
        full, full_sing = run(dev, srcs, ests, index, R.n_eff_of("full", M, N))
        assert got.tobytes() == full.tobytes() and got_sing == full_sing


def test_silent_identical_and_short(dev):
    rng = np.random.default_rng(7)
    M, N = 3, 257
    srcs = rng.standard_normal((M, 3, N)).astype(np.float32)
    ests = (srcs[:, :1] + 0.5 * srcs[:, 2:3] + 0.1 * rng.standard_normal((M, 1, N))).astype(np.float32)
    srcs[:, 1] = 0  # a silent source is left out of the span
    want, ws, _ = R.gain_batch(srcs, ests, [0])
    got, gs = run(dev, srcs, ests, [0])
    assert ws == 0 and gs == 0 and np.isfinite(want).all()
    compare(got, want, "silent")
    srcs[1, 1] = srcs[1, 0]  # two identical sources in utterance 1 alone
    want, ws, _ = R.gain_batch(srcs, ests, [0])
    got, gs = run(dev, srcs, ests, [0])
    assert ws == 1 and gs == 1 and np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()
    compare(got, want, "identical")
    srcs[:, 1] = rng.standard_normal((M, N)).astype(np.float32)
    n_eff = np.array([2, 3, 0], dtype=np.int32)  # n_eff < J, = J, and no sample at all
    want, ws, _ = R.gain_batch(srcs, ests, [0], n_eff)
    got, gs = run(dev, srcs, ests, [0], n_eff)
    assert ws == gs == 1 and np.isnan(got[0]).all() and np.isnan(got[2]).all()
    assert (np.isnan(got) == np.isnan(want)).all()


@pytest.mark.parametrize("N", (65, 4001, 9000))
def test_poison_beyond_n_eff_changes_no_bit(dev, N):
    M, J, Ke = 5, 4, 4
    srcs, ests, index = R.make_inputs(M, J, Ke, N)
    n_eff = np.array([N - 1, 1, N // 2, 0, N // 3], dtype=np.int32)
    clean, cs = run(dev, srcs, ests, index, n_eff)
    for m in range(M):
        srcs[m, :, n_eff[m]:] = np.nan
        ests[m, :, n_eff[m]:] = np.nan
    got, gs = run(dev, srcs, ests, index, n_eff)
    assert got.tobytes() == clean.tobytes() and gs == cs
    assert np.isfinite(got[0]).all()


def test_repeatable_and_independent_of_m(dev):
    J, Ke, N = 4, 4, 9000  # three chunks
    srcs, ests, index = R.make_inputs(5, J, Ke, N)
    n_eff = R.n_eff_of("mixed", 5, N)
    a, _ = run(dev, srcs, ests, index, n_eff)
    for _ in range(2):
        b, _ = run(dev, srcs, ests, index, n_eff)
        assert a.tobytes() == b.tobytes()
    one, _ = run(dev, srcs[:1], ests[:1], index, n_eff[:1])
    assert one.tobytes() == a[:1].tobytes()
    want, _, _ = R.gain_batch(srcs, ests, index, n_eff)
    compare(a, want, "three chunks")


def test_bss_eval_target_composes_nsdr(dev):
    rng = np.random.default_rng(9)
    M, N = 3, 1000
    t = rng.standard_normal((M, N)).astype(np.float32)
    n = rng.standard_normal((M, N)).astype(np.float32)
    mix = t + n
    pred = (t + 0.2 * n + 0.05 * rng.standard_normal((M, N))).astype(np.float32)
    n_eff = np.array([N, 700, 999], dtype=np.int32)
    out = bss.bss_eval_target(*(torch.as_tensor(x).to(dev) for x in (t, n, pred, mix)),
                              lengths=torch.as_tensor(n_eff).to(dev))
    assert int(out["singular"].item()) == 0
    for m in range(M):
        want = R.target_metrics(t[m], n[m], pred[m], mix[m], n_eff[m])
        for k in ("SDR", "SIR", "SAR", "NSDR"):  # (NSDR: the difference of two criteria)
            tol = 2 * TOL_DB if k == "NSDR" else TOL_DB
            assert out[k].dtype == torch.float64 and abs(float(out[k][m]) - want[k]) <= tol, (m, k)
    (sdr_mix, _, _), _ = bss.bss_eval_gain(torch.as_tensor(t[:, None]).to(dev), torch.as_tensor(mix[:, None]).to(dev),
                                           [0], torch.as_tensor(n_eff).to(dev))
    assert torch.equal(out["NSDR"], out["SDR"] - sdr_mix[:, 0])


def test_refusals(dev):
    s = torch.zeros(2, 2, 8, device=dev)
    with pytest.raises(ValueError):
        bss.bss_eval_gain(s, s, [0, 2])
    with pytest.raises(ValueError):
        bss.bss_eval_gain(torch.zeros(2, 5, 8, device=dev), s, [0, 1])
    with pytest.raises(ValueError):
        bss.bss_eval_gain(s, s[:, :, :4], [0, 1])
