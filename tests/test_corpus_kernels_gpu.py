"""Device-resident corpus kernels (csrc/corpus.hip) on the GPU: ``ops.mix_corpus`` / ``ops.corpus_stats`` against the
oracle's fp32 restatement of the mixing arithmetic (``oracle.dsp.mix_sources_f32``) on the gathered clips and against
``ops.mix_sources`` on the same inputs uploaded as a zero-padded array.

Every comparison is BITWISE.  The samples are 16-bit PCM (int16 pool, multiples of 2^-15) or 24-bit PCM (fp32 pool,
multiples of 2^-23): for N <= 32000 every fp64 sum of them is exact in any order, so the oracle's rounding-boundary
caveat cannot apply and no tolerance is needed."""
import numpy as np
import pytest
import torch

from dl4ss_amd import corpus as cp, ops
from oracle import dsp

pytestmark = pytest.mark.gpu

B, K = 4, 3
KINDS = ["int16", "fp32"]


def _samples(rng, n, kind):
    """16-bit PCM as int16, or 24-bit PCM as the float64 signal q / 2^23, with a DC offset."""
    if kind == "int16":
        return (rng.normal(300, 5000, n).round().clip(-32768, 32767)).astype(np.int16)
    return (rng.normal(1e5, 1.5e6, n).round().clip(-(1 << 23), (1 << 23) - 1)) / float(1 << 23)


def _corpus(dev, kind, lens, seed=0, max_len=None):
    rng = np.random.default_rng(seed)
    clips = [(f"s{i % 5}", f"c{i}", _samples(rng, n, kind)) for i, n in enumerate(lens)]
    c = cp.DeviceCorpus.from_clips(clips, max(lens) if max_len is None else max_len)
    assert c.pool.dtype == (np.int16 if kind == "int16" else np.float32)
    return c.to(dev)


def _t(dev, a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def _mix(dev, c, clips, gains, shifts, k, n, want_len=False):
    out_len = torch.full(np.shape(clips), -7, device=dev, dtype=torch.int32) if want_len else None
    s, m, bad = c.mix(_t(dev, clips, np.int32), _t(dev, gains, np.float32), k, n, shifts=_t(dev, shifts, np.int32),
                      out_len=out_len)
    torch.cuda.synchronize()
    out = (s.cpu().numpy(), m.cpu().numpy(), int(bad.item()))
    return out + (out_len.cpu().numpy(),) if want_len else out


def _mix_sources(dev, raw, gains, lens, shifts):
    s, m = ops.mix_sources(_t(dev, raw, np.float32), _t(dev, gains, np.float32), lengths=_t(dev, lens, np.int32),
                           shifts=_t(dev, shifts, np.int32))
    torch.cuda.synchronize()
    return s.cpu().numpy(), m.cpu().numpy()


def _case(n, seed=3):
    """Clip lengths {1, 2, 17, n-1, n, 2500}; B x (K + 1) clip ids with clip 1 (2500) in rows 0 and 3; shifts
    {0, 1, len-1, len/2, random, len+5, -3}."""
    lens = [n, 2500, 1, n, n, 17, n - 1, 2, n, 2500]
    clips = np.array([[0, 1, 2, 9], [3, 4, 8, 1], [5, 6, 7, 0], [8, 1, 2, 6]], np.int32)
    L = np.array(lens)[clips]
    rng = np.random.default_rng(seed)
    shifts = np.array([[0, 1, 0, L[0, 3] // 2],
                       [L[1, 0] - 1, L[1, 1] // 2, int(rng.integers(0, n)), L[1, 3] + 5],
                       [L[2, 0] + 5, -3, 1, int(rng.integers(0, n))],
                       [-3, L[3, 1] - 1, 4, L[3, 3] + 5]], np.int32)
    gains = rng.uniform(0.6, 1.8, size=clips.shape).astype(np.float32)
    return lens, clips, L.astype(np.int32), shifts, gains


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [4000, 4002])  # 4002: no 16-B stores, the scalar tail
@pytest.mark.parametrize("rot", [False, True])
def test_mix_corpus_bitwise_vs_oracle_and_mix_sources(dev, kind, n, rot):
    lens, clips, L, shifts, gains = _case(n)
    c = _corpus(dev, kind, lens)
    clips, L, gains = clips[:, :K], L[:, :K], gains[:, :K]
    shifts = shifts[:, :K] if rot else None
    s, m, bad, used = _mix(dev, c, clips, gains, shifts, K, n, want_len=True)
    raw = c.gather(clips, n)
    es, em = dsp.mix_sources_f32(raw, gains, L, shifts)
    assert bad == 0 and np.array_equal(used, L)
    assert np.array_equal(s, es) and np.array_equal(m, em)
    ks, km = _mix_sources(dev, raw, gains, L, shifts)
    assert np.array_equal(s, ks) and np.array_equal(m, km)
    assert s.any() and np.isfinite(s).all()


@pytest.mark.parametrize("kind", KINDS)
def test_background_source_is_mixed_but_not_a_target(dev, kind):
    n = 4000
    lens, clips, L, shifts, gains = _case(n)
    c = _corpus(dev, kind, lens)
    s3, _, _ = _mix(dev, c, clips[:, :K], gains[:, :K], shifts[:, :K], K, n)
    s, m, bad, used = _mix(dev, c, clips, gains, shifts, K, n, want_len=True)  # Ks = K + 1
    es, em = dsp.mix_sources_f32(c.gather(clips, n), gains, L, shifts)
    assert bad == 0 and s.shape == (B, K, n) and np.array_equal(used, L)
    assert np.array_equal(s, s3) and np.array_equal(s, es[:, :K]) and np.array_equal(m, em)
    assert not np.array_equal(m, dsp.mix_sources_f32(c.gather(clips[:, :K], n), gains[:, :K], L[:, :K],
                                                     shifts[:, :K])[1])


@pytest.mark.parametrize("kind", KINDS)
def test_corpus_stats_vs_oracle(dev, kind):
    import math

    lens = [4000, 2500, 1, 3999, 17, 2, 1030, 4]
    c = _corpus(dev, kind, lens, seed=8)
    const = np.full(9, 1234, np.int16) if kind == "int16" else np.full(9, 0.125)
    c = cp.DeviceCorpus.from_clips([(c.speaker_names[s], nm, c.pool[o:o + ln]) for s, nm, o, ln in
                                    zip(c.speaker, c.clip_names, c.offsets, c.lengths)] + [("z", "flat", const)],
                                   4000).to(dev)
    got = c.clip_stats.cpu().numpy()
    assert got.shape == (9, 2) and got.dtype == np.float32
    for i in range(9):
        x = c.clip(i)
        mean = np.float32(math.fsum(x.astype(np.float64).tolist()) / len(x))
        pk = max(np.float32(x.max() - mean), np.float32(mean - x.min()))
        inv = np.float32(1.0) / pk if pk > 0 else np.float32(0.0)
        assert got[i, 0] == mean and got[i, 1] == inv, i
    assert got[8, 1] == 0 and got[2, 1] == 0  # a constant clip, a one-sample clip: silent, not Inf


def test_rows_are_independent_and_launches_repeat(dev):
    n = 4000
    lens, clips, L, shifts, gains = _case(n)
    c = _corpus(dev, "int16", lens)
    a = _mix(dev, c, clips, gains, shifts, K, n)
    b = _mix(dev, c, clips, gains, shifts, K, n)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for r in range(B):
        s, m, _ = _mix(dev, c, clips[r:r + 1], gains[r:r + 1], shifts[r:r + 1], K, n)
        assert np.array_equal(s[0], a[0][r]) and np.array_equal(m[0], a[1][r])


@pytest.mark.parametrize("bad_id", [-1, 10, 2 ** 31 - 1])
def test_out_of_range_clip_is_silent_and_counted(dev, bad_id):
    n = 4000
    lens, clips, L, shifts, gains = _case(n)
    c = _corpus(dev, "fp32", lens)
    clips, L = clips.copy(), L.copy()
    clips[2, 1] = bad_id
    s, m, bad, used = _mix(dev, c, clips, gains, shifts, K, n, want_len=True)
    ok = np.where(clips == bad_id, 0, clips)
    L[2, 1] = 0
    es, em = dsp.mix_sources_f32(c.gather(ok, n), gains, L, shifts)
    assert bad == 1 and np.array_equal(used, L) and not s[2, 1].any()
    assert np.array_equal(s, es[:, :K]) and np.array_equal(m, em)
    # the counter accumulates in a caller's buffer
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)
    clips[0, 3] = bad_id  # (the background source)
    for _ in range(2):
        c.mix(_t(dev, clips, np.int32), _t(dev, gains, np.float32), K, n, bad=cnt)
    assert int(cnt.item()) == 4


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_outside_the_pool_is_read(dev, kind):
    """The pool between guard regions (NaN for fp32, full-scale samples for int16): no output changes."""
    n = 4002
    lens, clips, L, shifts, gains = _case(n)
    c = _corpus(dev, kind, lens)
    want = _mix(dev, c, clips, gains, shifts, K, n)
    stats = c.clip_stats.clone()
    guard, m = 4096, len(c.pool)
    big = torch.full((m + 2 * guard,), float("nan") if kind == "fp32" else -32768, device=dev, dtype=c.d_pool.dtype)
    big[guard:guard + m] = c.d_pool
    c.d_pool = big[guard:guard + m]
    assert c.d_pool.data_ptr() % 16 == 0
    c.clip_stats = ops.corpus_stats(c.d_pool, c.d_offsets, c.d_lengths)
    got = _mix(dev, c, clips, gains, shifts, K, n)
    assert torch.equal(stats, c.clip_stats)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == 0


def test_c2_shape_equals_mix_sources(dev):
    """Once at B = 32, K = 2, N = 32000, ragged lengths, half of the rows rotated."""
    n, b, k = 32000, 32, 2
    rng = np.random.default_rng(6)
    lens = rng.integers(n // 2, n + 1, 80)
    lens[:8] = n
    c = _corpus(dev, "int16", lens.tolist(), seed=6, max_len=n)
    clips = rng.permutation(80)[:b * k].reshape(b, k).astype(np.int32)
    clips[0] = (0, 1)
    L = c.lengths[clips]
    shifts = rng.integers(0, n, size=(b, k)).astype(np.int32) % L
    shifts[:16] = 0
    gains = rng.uniform(0.6, 1.8, size=(b, k)).astype(np.float32)
    s, m, bad = _mix(dev, c, clips, gains, shifts, k, n)
    ks, km = _mix_sources(dev, c.gather(clips, n), gains, L, shifts)
    assert bad == 0 and np.array_equal(s, ks) and np.array_equal(m, km) and s.any()


def test_wrapper_refusals(dev):
    c = _corpus(dev, "int16", [100, 50])
    i32 = lambda *a: torch.zeros(*a, device=dev, dtype=torch.int32)
    g = torch.ones(2, 2, device=dev)
    with pytest.raises(ValueError, match="max_len"):
        c.mix(i32(2, 2), g, 2, 99)
    with pytest.raises(RuntimeError):
        c.mix(i32(2, 2), g, 3, 100)  # K > Ks
    with pytest.raises(RuntimeError):
        c.mix(i32(2, 2).long(), g, 2, 100)
    with pytest.raises(RuntimeError):
        c.mix(i32(2, 2), g, 2, 100, shifts=i32(2, 3))
    with pytest.raises(RuntimeError):
        c.mix(i32(2, 2), g, 2, 100, out_src=torch.empty(2, 2, 101, device=dev))
    with pytest.raises(RuntimeError):
        ops.mix_corpus(c.d_pool[1:], c.d_offsets, c.d_lengths, c.clip_stats, i32(2, 2), g, 2, 100)  # misaligned
