"""The fp64 restatement of BSS Eval 2.0's gain decomposition (tests/bss_gain_ref.py) against cases computed by
hand, and against np.longdouble on the inputs of tests/test_bss_gain_gpu.py: those inputs have cond(G) <= 1e4 and
every finite criterion under 100 dB, which is what the device test's 1e-6 dB bound rests on."""
import math

import numpy as np
import pytest

import bss_gain_ref as R

INF = float("inf")


def test_orthogonal_sources_by_hand():
    # s0 on samples 0-1, s1 on samples 2-3: G = diag(8, 2).  e = 3 s0 + 2 s1 + artefact (0, 0, 0, 0, 4)
    s = np.array([[2.0, 2, 0, 0, 0], [0, 0, 1, 1, 0]])
    e = np.array([6.0, 6, 2, 2, 4])
    sdr, sir, sar, sing, cond = R.gain_one(s, e, 0)
    # s_target = 3 s0 (energy 72), e_interf = 2 s1 (energy 8), e_artif energy 16
    assert not sing and cond == pytest.approx(4.0)
    assert sdr == pytest.approx(10 * math.log10(72 / 24), abs=1e-12)
    assert sir == pytest.approx(10 * math.log10(72 / 8), abs=1e-12)
    assert sar == pytest.approx(10 * math.log10(80 / 16), abs=1e-12)


def test_estimate_is_the_target():
    s = np.array([[2.0, 2, 0, 0], [0, 0, 1, -1]])
    sdr, sir, sar, sing, _ = R.gain_one(s, s[1].copy(), 1)
    assert (sdr, sir, sar, sing) == (INF, INF, INF, False)


def test_target_plus_noise_leak():
    # e = s_t + beta s_n with orthogonal s_t, s_n: SAR = +inf, SIR = 20 log10(|s_t| / (beta |s_n|))
    s_n = np.array([4.0, 4, 0, 0])
    s_t = np.array([0.0, 0, 1, -1])
    beta = 0.25
    sdr, sir, sar, sing, _ = R.gain_one(np.stack([s_n, s_t]), s_t + beta * s_n, 1)
    want = 20 * math.log10(math.sqrt(2.0) / (beta * math.sqrt(32.0)))
    assert not sing and sar == INF
    assert sir == pytest.approx(want, abs=1e-12) and sdr == pytest.approx(want, abs=1e-12)


def test_one_source():
    rng = np.random.default_rng(3)
    s = rng.standard_normal((1, 50))
    e = 0.7 * s[0] + 0.3 * rng.standard_normal(50)
    sdr, sir, sar, sing, _ = R.gain_one(s, e, 0)
    assert not sing and sir == INF and sdr == sar and 0 < sdr < 30


def test_silent_source_is_left_out_and_identical_sources_are_singular():
    rng = np.random.default_rng(4)
    s = rng.standard_normal((3, 40))
    e = s[0] + 0.5 * s[2] + 0.1 * rng.standard_normal(40)
    s[1] = 0
    with_silent = R.gain_one(s, e, 0)
    without = R.gain_one(s[[0, 2]], e, 0)
    assert with_silent[:4] == without[:4] and not with_silent[3]
    s[1] = s[0]
    assert R.gain_one(s, e, 0)[3] and all(math.isnan(x) for x in R.gain_one(s, e, 0)[:3])
    # fewer samples than sources, and no sample at all (an empty span is not singular: 0 / 0 criteria)
    assert R.gain_one(rng.standard_normal((2, 40)), e, 0, n_eff=1)[3]
    none = R.gain_one(rng.standard_normal((2, 40)), e, 0, n_eff=0)
    assert not none[3] and all(math.isnan(x) for x in none[:3])


def test_nsdr_composition():
    rng = np.random.default_rng(5)
    t, n = rng.standard_normal(300), rng.standard_normal(300)
    mix = t + n
    pred = t + 0.2 * n + 0.05 * rng.standard_normal(300)
    m = R.target_metrics(t, n, pred, mix)
    assert m["SDR"] == R.gain_one(np.stack([n, t]), pred, 1)[0]
    assert m["NSDR"] == m["SDR"] - R.gain_one(t[None], mix, 0)[0]
    assert m["NSDR"] > 5


@pytest.mark.parametrize("J,Ke", R.SHAPES)
@pytest.mark.parametrize("N", R.SIZES)
def test_gpu_inputs_are_well_conditioned_and_match_longdouble(N, J, Ke):
    M = 5
    srcs, ests, index = R.make_inputs(M, J, Ke, N)
    for kind in R.N_EFF_KINDS:
        n_eff = R.n_eff_of(kind, M, N)
        c64, sing64, cond = R.gain_batch(srcs, ests, index, n_eff)
        cld, singld, _ = R.gain_batch(srcs, ests, index, n_eff, dtype=np.longdouble)
        assert cond <= 1e4, (kind, cond)
        assert sing64 == singld
        fin = np.isfinite(c64)
        assert (np.abs(c64[fin]) < 100).all(), (kind, c64[fin].max())
        assert (np.isnan(c64) == np.isnan(cld)).all() and (np.isposinf(c64) == np.isposinf(cld)).all()
        assert not np.isneginf(c64).any()
        if fin.any():  # fp64 against extended precision: far inside the device test's 1e-6 dB
            assert np.abs(c64[fin] - cld[fin]).max() < 1e-9, (kind, np.abs(c64[fin] - cld[fin]).max())
