"""Device-resident corpus, host side (no GPU): the pool build, both samplers and the new header.

The dataset is test_wsj0list_cpu._dataset (four 16-bit PCM wavs, a three-line list)."""
import random
import struct

import numpy as np
import pytest

from dl4ss_amd import _lib, corpus as cp, wsj0list as wl
from test_wsj0list_cpu import _dataset

MAX_LEN = 10000  # crops 02b and 04d (12000), keeps 01a (9000) and 03c (5000) whole


def _write_wav(path, x, rate, bits):
    """24-bit PCM or float32 mono wav (write_wav writes 16-bit only)."""
    if bits == 24:
        q = np.round(np.asarray(x) * (1 << 23)).astype(np.int64).clip(-(1 << 23), (1 << 23) - 1)
        body = b"".join(struct.pack("<i", int(v))[:3] for v in q)
        tag = 1
    else:
        body, tag = np.asarray(x, "<f4").tobytes(), 3
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(body), b"WAVE", b"fmt ", 16, tag, 1, rate,
                      rate * bits // 8, bits // 8, bits, b"data", len(body))
    with open(path, "wb") as f:
        f.write(hdr + body)


def _check_layout(c):
    per = 16 // c.pool.dtype.itemsize
    assert c.offsets.dtype == np.int64 and c.lengths.dtype == np.int32 and c.speaker.dtype == np.int32
    assert not (c.offsets * c.pool.dtype.itemsize % 16).any()
    used = np.zeros(len(c.pool), bool)
    for o, n in zip(c.offsets, c.lengths):
        assert not used[o:o + n].any() and o % per == 0
        used[o:o + n] = True
    assert not c.pool[~used].any()  # zero gaps
    assert len(c.pool) == int(((c.lengths.astype(np.int64) + per - 1) // per * per).sum())


def test_pool_from_clips_layout_crop_and_dtype():
    rng = np.random.default_rng(1)
    q = [rng.integers(-3000, 3000, n).astype(np.int16) for n in (1, 2, 17, 4001, 9, 8)]
    clips = [("s%d" % (2 - i % 3), "c%d" % i, x) for i, x in enumerate(q)]
    c = cp.DeviceCorpus.from_clips(clips, max_len=4000)
    assert c.pool.dtype == np.int16 and list(c.lengths) == [1, 2, 17, 4000, 9, 8]  # cropped to max_len
    _check_layout(c)
    assert c.speaker_names == ["s0", "s1", "s2"] and list(c.speaker) == [2, 1, 0, 2, 1, 0]
    assert c.clips_of == [[2, 5], [1, 4], [0, 3]] and c.index[("s2", "c3")] == 3
    for i, x in enumerate(q):
        assert np.array_equal(c.pool[c.offsets[i]:c.offsets[i] + c.lengths[i]], x[:4000])
        assert np.array_equal(c.clip(i), (x[:4000] / 32768.0).astype(np.float32))
    # one float clip: the whole pool is fp32, int16 clips as q / 32768, the float one as float32(x)
    x = rng.standard_normal(33) * 0.1
    f = cp.DeviceCorpus.from_clips(clips + [("s9", "f", x)], max_len=4000)
    assert f.pool.dtype == np.float32
    _check_layout(f)
    assert np.array_equal(f.clip(6), x.astype(np.float32)) and np.array_equal(f.clip(3), c.clip(3))
    assert np.array_equal(f.gather([[3, 6]], 4000)[0, 1, :40], np.concatenate([x.astype(np.float32), np.zeros(7)]))


def test_pool_refusals():
    one = ("a", "x", np.ones(5, np.int16))
    with pytest.raises(ValueError, match="b/empty"):
        cp.DeviceCorpus.from_clips([one, ("b", "empty", np.zeros(0, np.int16))], 100)
    with pytest.raises(ValueError, match="twice"):
        cp.DeviceCorpus.from_clips([one, one], 100)
    c = cp.DeviceCorpus.from_clips([one], 100)
    for kw in (dict(offsets=[4]), dict(lengths=[0]), dict(lengths=[9]), dict(offsets=[8]), dict(speaker=[1])):
        args = dict(pool=c.pool, offsets=c.offsets, lengths=c.lengths, speaker=c.speaker, speaker_names=["a"],
                    clip_names=["x"], max_len=100)
        args.update(kw)
        with pytest.raises(ValueError):
            cp.DeviceCorpus(**args)
    with pytest.raises(ValueError, match="overlap"):
        cp.DeviceCorpus(np.zeros(16, np.int16), [0, 0], [5, 5], [0, 0], ["a"], ["x", "y"], 100)
    # N below the corpus's max_len is refused on the host, before any device call
    with pytest.raises(ValueError, match="max_len = 100"):
        c.mix(None, None, 1, 99)
    with pytest.raises(ValueError, match="max_len = 100"):
        from dl4ss_amd import ops
        ops.mix_corpus(None, None, None, None, None, None, 1, 99, max_len=100)


def test_pool_from_tree_sorted_cropped_int16(tmp_path):
    _, data, lens = _dataset(tmp_path)
    (tmp_path / "data" / "train" / "01a" / "01aa0000.wav").write_bytes(
        (tmp_path / "data" / "train" / "03c" / "03cc0303.wav").read_bytes())
    c = cp.DeviceCorpus.from_tree(data, "train", MAX_LEN)
    assert c.pool.dtype == np.int16
    _check_layout(c)
    assert c.speaker_names == ["01a", "02b", "03c", "04d"]
    assert c.clip_names == ["01aa0000", "01aa0101", "02bb0202", "03cc0303", "04dd0404"]  # files sorted too
    assert list(c.lengths) == [5000, 9000, 10000, 5000, 10000] and list(c.speaker) == [0, 0, 1, 2, 3]
    for i, (spk, name) in enumerate(zip(c.speaker, c.clip_names)):
        x, _ = wl.read_wav(wl.source_path(data, "train", c.speaker_names[spk], name))
        assert np.array_equal(c.clip(i), x[:MAX_LEN].astype(np.float32))  # what ListBatches.load casts


@pytest.mark.parametrize("kind", ["pcm24", "float32", "resampled"])
def test_pool_from_tree_fp32_when_not_pcm16_at_rate(tmp_path, kind):
    _, data, _ = _dataset(tmp_path)
    x = np.random.default_rng(2).standard_normal(3000).clip(-3, 3) / 4
    p = str(tmp_path / "data" / "train" / "04d" / "04dd0505.wav")
    if kind == "resampled":
        wl.write_wav(p, x, 16000)
    else:
        _write_wav(p, x, 8000, 24 if kind == "pcm24" else 32)
    c = cp.DeviceCorpus.from_tree(data, "train", MAX_LEN)
    assert c.pool.dtype == np.float32
    _check_layout(c)
    y, rate = wl.read_wav(p)
    i = c.index[("04d", "04dd0505")]
    assert np.array_equal(c.clip(i), wl.resample(y, rate)[:MAX_LEN].astype(np.float32))
    z, _ = wl.read_wav(wl.source_path(data, "train", "01a", "01aa0101"))
    assert np.array_equal(c.clip(c.index[("01a", "01aa0101")]), z.astype(np.float32))


def test_pool_from_tree_refuses_empty_wav(tmp_path):
    _, data, _ = _dataset(tmp_path)
    wl.write_wav(str(tmp_path / "data" / "train" / "02b" / "02bb0000.wav"), np.zeros(0))
    with pytest.raises(ValueError, match="02bb0000.wav"):
        cp.DeviceCorpus.from_tree(data, "train", MAX_LEN)


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("augment", [False, True])
def test_list_sampler_equals_list_batches(tmp_path, shuffle, augment):
    lst, data, _ = _dataset(tmp_path)
    c = cp.DeviceCorpus.from_tree(data, "train", MAX_LEN)
    lb = wl.ListBatches(lst, data, "train", 1, MAX_LEN, shuffle=shuffle, seed=5, augment=augment)
    ls = cp.ListMixSampler(c, lst, 1, shuffle=shuffle, seed=5, augment=augment)
    assert ls.batch_total == lb.batch_total == 3 and ls.k == lb.k == 2
    for _ in range(2):  # two epochs: the shuffle generator carries on
        random.seed(3)
        want = list(lb)
        random.seed(3)
        got = list(ls)
        assert len(got) == len(want) == 3
        for g, w in zip(got, want):
            assert g["speakers"] == w["speakers"] and g["names"] == w["names"]
            assert g["gains"].dtype == np.float32 and np.array_equal(g["gains"], w["gains"])
            assert g["lengths"].dtype == np.int32 and np.array_equal(g["lengths"], w["lengths"])
            assert g["clips"].dtype == np.int32 and g["clips"].shape == (1, 2)
            if augment:
                assert g["shifts"].dtype == np.int32 and np.array_equal(g["shifts"], w["shifts"])
            else:
                assert g["shifts"] is None and w["shifts"] is None
            assert np.array_equal(c.gather(g["clips"], MAX_LEN), w["raw"])  # (zero beyond each length, too)


def test_list_sampler_state_round_trip(tmp_path):
    lst, data, _ = _dataset(tmp_path)
    c = cp.DeviceCorpus.from_tree(data, "train", MAX_LEN)
    a = cp.ListMixSampler(c, lst, 1, shuffle=True, seed=7)
    it = iter(a)
    first = next(it)
    sd = a.state_dict()
    rest = [b["names"] for b in it] + [b["names"] for b in a]  # the epoch's other two, then a whole one
    b = cp.ListMixSampler(c, lst, 1, shuffle=True, seed=99)
    b.load_state_dict(sd)
    assert [x["names"] for x in b] + [x["names"] for x in b] == rest and len(rest) == 5
    assert first["names"] not in rest[:2]
    from dl4ss_amd.checkpoint import _check_plain
    _check_plain(sd, "sampler")
    with pytest.raises(ValueError):
        b.load_state_dict(dict(sd, order=[0, 0, 1]))
    with pytest.raises(KeyError):
        cp.ListMixSampler(cp.DeviceCorpus.from_clips([("01a", "x", np.ones(4, np.int16))], 8), lst, 1)


def _random_corpus():
    rng = np.random.default_rng(4)
    clips = [(f"s{s}", f"c{s}_{j}", rng.integers(-900, 900, 40 + 3 * s + j).astype(np.int16))
             for s in range(5) for j in range(3)]
    clips.append(("noise", "bgd", rng.integers(-900, 900, 64).astype(np.int16)))
    return cp.DeviceCorpus.from_clips(clips, 64)


def test_random_sampler_draws():
    c = _random_corpus()
    random.seed(11)
    np.random.seed(11)
    s = cp.RandomMixSampler(c, 4, 2, 3, db=5, gain_rule="db3")
    assert 2 <= s.mix_k <= 3
    K, seen = s.mix_k, {i: [] for i in range(6)}
    for b in s.batches(6):
        assert b["K"] == K and b["clips"].shape == (4, K) and b["clips"].dtype == np.int32 and b["shifts"] is None
        assert b["gains"].shape == (4, K) and b["gains"].dtype == np.float32 and (b["gains"] >= 1).all()
        assert np.array_equal(b["lengths"], c.lengths[b["clips"]])
        for spk, clips in zip(b["speakers"], b["clips"]):
            assert len(set(spk.tolist())) == K  # distinct speakers per mixture
            for sp, cl in zip(spk.tolist(), clips.tolist()):
                assert c.speaker[cl] == sp
                seen[sp].append(cl)
    assert sum(len(v) for v in seen.values()) == 24 * K
    for sp, used in seen.items():  # no clip repeats before the speaker's list is exhausted, then the refill
        n = len(c.clips_of[sp])  # (3, and 1 for the speaker that holds the background clip)
        for i in range(0, len(used), n):
            part = used[i:i + n]
            assert len(set(part)) == len(part) and set(part) <= set(c.clips_of[sp])
    assert max(len(v) for v in seen.values()) > 3  # (some list did run out)


def test_random_sampler_noise_clip_augment_and_state():
    c = _random_corpus()
    noise = c.index[("noise", "bgd")]
    random.seed(2)
    np.random.seed(2)
    a = cp.RandomMixSampler(c, 3, 2, 2, db=5, augment=True, noise_clip=noise)
    b0 = a.batch()
    assert b0["K"] == 2 and b0["clips"].shape == (3, 3) and (b0["clips"][:, 2] == noise).all()  # Ks = K + 1
    assert np.allclose(b0["gains"][:, 2], 0.3) and b0["speakers"].shape == (3, 2)
    assert (b0["shifts"] >= 0).all() and (b0["shifts"] < b0["lengths"]).all() and b0["shifts"].any()
    a.batch()
    sd, py, npy = a.state_dict(), random.getstate(), np.random.get_state()
    from dl4ss_amd.checkpoint import _check_plain
    _check_plain(sd, "sampler")
    want = [a.batch() for _ in range(4)]
    random.seed(77)
    b = cp.RandomMixSampler(c, 3, 2, 2, db=5, augment=True, noise_clip=noise)
    b.load_state_dict(sd)
    random.setstate(py)
    np.random.set_state(npy)
    for w in want:
        g = b.batch()
        assert all(np.array_equal(g[k], w[k]) for k in ("clips", "gains", "lengths", "shifts", "speakers"))
    with pytest.raises(ValueError):
        b.load_state_dict({"mix_k": 2, "remaining": {"1": [99]}})
    with pytest.raises(ValueError):
        cp.RandomMixSampler(c, 3, 2, 7)


def test_header_declares_both_entry_points():
    """include/corpus/dl4ss_corpus.h, the extension's header: parsed, bound by keyword, and outside the tables of
    libdl4ss_hip.so (whose exports stay exactly what the headers directly under include/ declare)"""
    assert _lib.exported_symbols("dl4ss_corpus.h") == ["dl4ss_corpus_stats", "dl4ss_mix_corpus"]
    h = _lib.EXT_HEADERS["dl4ss_corpus.h"]
    assert h.params["dl4ss_corpus_stats"] == ("pool", "dtype", "offsets", "lengths", "n_clips", "ws", "clip_stats",
                                              "stream")
    assert h.params["dl4ss_mix_corpus"] == ("pool", "dtype", "offsets", "lengths", "clip_stats", "n_clips", "clips",
                                            "shifts", "gains", "B", "K", "Ks", "N", "out_src", "out_mix", "out_len",
                                            "bad", "stream")
    assert h.restypes["dl4ss_mix_corpus"] is _lib.I and h.restypes["dl4ss_corpus_stats"] is _lib.I
    assert h.constants == _lib.EXT_CONSTANTS == {"DL4SS_CORPUS_I16": 0, "DL4SS_CORPUS_F32": 1}
    assert not set(h.signatures) & set(_lib.SIGNATURES) and "dl4ss_corpus.h" not in _lib.HEADERS
    assert _lib.EXT_LIBS["dl4ss_corpus.h"].endswith("libdl4ss_corpus.so")
    # keywords bind in the prototype's order; a wrong set is refused before any library is touched
    kw = {p: i for i, p in enumerate(h.params["dl4ss_corpus_stats"])}
    assert _lib.bind("dl4ss_corpus_stats", (), dict(reversed(list(kw.items())))) == tuple(range(8))
    with pytest.raises(TypeError, match="no parameter 'Ks'"):
        _lib.bind("dl4ss_corpus_stats", (), dict(kw, Ks=1))
    with pytest.raises(TypeError, match="missing parameter 'stream'"):
        _lib.bind("dl4ss_corpus_stats", (0,) * 7, {})


def test_extension_library_exports_exactly_its_header():
    import ctypes
    import shutil
    import subprocess

    from dl4ss_amd import build

    build.build()
    assert "corpus" in build.extensions()
    path = _lib.EXT_LIBS["dl4ss_corpus.h"]
    assert path == build.ext_lib("corpus")
    lib = ctypes.CDLL(path)
    assert all(hasattr(lib, s) for s in _lib.exported_symbols("dl4ss_corpus.h"))
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        exported = sorted(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.split()[-1].startswith("dl4ss_"))
        assert exported == sorted(_lib.exported_symbols("dl4ss_corpus.h"))
