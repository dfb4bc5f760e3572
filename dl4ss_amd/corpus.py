"""Device-resident corpus: the clips of a training set held once in HBM; a step sends clip ids, gains and shifts.

Everything a loader does per source is determined by the clip and the crop length -- crop to the first MAX_LEN
samples, ``x -= mean; x /= max|x|``, rotate, pad, gain, sum (``TDAA_beta/predata_fromList_cRM_123.py:186-237``,
``Torch_multi/predata_multiAims_dB.py:148-197``) -- so ``DeviceCorpus`` stores every clip cropped, in one flat pool,
computes the per-clip statistics once (``ops.corpus_stats``) and ``ops.mix_corpus`` builds a step's sources and
mixtures in one launch, with the values ``ops.mix_sources`` gives for the same clips uploaded as a zero-padded
``(B, K, N)`` array.  WSJ0 ``si_tr_s`` cropped to 4 s at 8 kHz is under 1 GB as int16.

Pool: int16 when every clip came from 16-bit PCM at the target rate (``q / 32768`` is exact in fp32), else fp32
holding ``float32(x)`` as ``wsj0list.ListBatches.load`` casts it.  Every clip starts 16-B aligned, the gaps are zero.
The host part (pool, tables, validation) needs no GPU; ``to(device)`` uploads it and computes the statistics.

Samplers (host only, they yield index arrays): ``ListMixSampler`` iterates a WSJ0-mix list file as
``wsj0list.ListBatches`` does; ``RandomMixSampler`` restates the on-the-fly draws of the ``predata_multiAims*``
loaders over the corpus's speakers.  Both draw from the module-level ``random`` / ``np.random``, the streams
``checkpoint.save_training_state(rng=True)`` saves; their own position goes through its ``extra=``.
"""
import os
import random
import struct
import types

import numpy as np
import torch

from . import ops, wsj0list
from .compat import _data

ALIGN_BYTES = 16


def _is_pcm16(path):
    """True when the wav's fmt chunk says 16-bit integer PCM (what read_wav scales as q / 32768)."""
    with open(path, "rb") as f:
        data = f.read(4096)
    pos = 12
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        if cid == b"fmt ":
            tag, _, _, _, _, bits = struct.unpack("<HHIIHH", data[pos + 8:pos + 24])
            return tag == 1 and bits == 16
        pos += 8 + size + (size & 1)
    return False


class DeviceCorpus:
    """One flat pool of cropped clips with its tables.

    Host (always): ``pool`` (int16 or float32 numpy), ``offsets`` int64 (in samples), ``lengths`` int32,
    ``speaker`` int32 (index into ``speaker_names``), ``speaker_names``, ``clip_names``, ``clips_of`` (clip ids
    per speaker, in clip order) and ``index`` ``(speaker, name) -> clip id``.  Device, after ``to(device)``:
    ``d_pool``, ``d_offsets``, ``d_lengths``, ``d_speaker``, ``clip_stats`` (n_clips, 2) ``{mean, 1 / peak}``.

    Everything that keeps a kernel inside the pool is validated here, on the host: ``offset + length <= pool_len``,
    16-B aligned clip starts, ``length >= 1``, no two clips overlapping."""

    def __init__(self, pool, offsets, lengths, speaker, speaker_names, clip_names, max_len):
        self.pool = np.ascontiguousarray(pool)
        self.offsets = np.ascontiguousarray(offsets, np.int64)
        self.lengths = np.ascontiguousarray(lengths, np.int32)
        self.speaker = np.ascontiguousarray(speaker, np.int32)
        self.speaker_names, self.clip_names, self.max_len = list(speaker_names), list(clip_names), int(max_len)
        self.validate()
        self.clips_of = [[] for _ in self.speaker_names]
        self.index = {}
        for c, (s, name) in enumerate(zip(self.speaker.tolist(), self.clip_names)):
            self.clips_of[s].append(c)
            if (self.speaker_names[s], name) in self.index:
                raise ValueError(f"clip {self.speaker_names[s]}/{name} is given twice")
            self.index[(self.speaker_names[s], name)] = c
        self.device = None
        self.d_pool = self.d_offsets = self.d_lengths = self.d_speaker = self.clip_stats = None

    def __len__(self):
        return len(self.lengths)

    def validate(self):
        n, per = len(self.offsets), ALIGN_BYTES // self.pool.dtype.itemsize
        if self.pool.dtype not in (np.int16, np.float32) or self.pool.ndim != 1:
            raise ValueError(f"pool must be flat int16 or float32, not {self.pool.dtype} {self.pool.shape}")
        if n < 1 or not (len(self.lengths) == len(self.speaker) == len(self.clip_names) == n):
            raise ValueError("a corpus holds at least one clip, and one table entry per clip")
        if self.max_len < 1 or int(self.lengths.min()) < 1 or int(self.lengths.max()) > self.max_len:
            raise ValueError(f"clip lengths must lie in [1, max_len = {self.max_len}]")
        if (self.offsets % per).any() or int(self.offsets.min()) < 0:
            raise ValueError(f"every clip must start {ALIGN_BYTES}-B aligned ({per} samples)")
        end = self.offsets + self.lengths
        if int(end.max()) > len(self.pool):
            raise ValueError(f"a clip ends at sample {int(end.max())}, past the pool's {len(self.pool)}")
        order = np.argsort(self.offsets, kind="stable")
        if (end[order][:-1] > self.offsets[order][1:]).any():
            raise ValueError("two clips overlap in the pool")
        if int(self.speaker.min()) < 0 or int(self.speaker.max()) >= len(self.speaker_names):
            raise ValueError("a clip's speaker index is outside speaker_names")

    # ------------------------------------------------------------------ builders
    @classmethod
    def from_clips(cls, clips, max_len, device=None):
        """``clips``: a list of ``(speaker, name, samples)``; int16 ``samples`` are 16-bit PCM (x = q / 32768), any
        other dtype is the signal itself.  Each is cropped to its first ``max_len`` samples; an empty one is
        refused (ValueError naming it).  The pool is int16 when every clip is, else fp32.  ``device``: upload
        too (``to``)."""
        clips = [(str(s), str(n), np.asarray(x)) for s, n, x in clips]
        for s, n, x in clips:
            if x.ndim != 1 or len(x) < 1:
                raise ValueError(f"clip {s}/{n}: empty (or not one channel of samples, shape {x.shape})")
        as_i16 = all(x.dtype == np.int16 for _, _, x in clips)
        dtype = np.int16 if as_i16 else np.float32
        per = ALIGN_BYTES // np.dtype(dtype).itemsize
        lengths = np.array([min(len(x), max_len) for _, _, x in clips], np.int32)
        padded = (lengths.astype(np.int64) + per - 1) // per * per
        offsets = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
        pool = np.zeros(int(padded.sum()), dtype)  # the gaps stay zero
        for (_, _, x), o, n in zip(clips, offsets.tolist(), lengths.tolist()):
            x = x[:n]
            if not as_i16 and x.dtype == np.int16:
                x = x.astype(np.float64) / 32768.0
            pool[o:o + n] = x
        names = sorted({s for s, _, _ in clips})
        where = {s: i for i, s in enumerate(names)}
        corpus = cls(pool, offsets, lengths, [where[s] for s, _, _ in clips], names, [n for _, n, _ in clips], max_len)
        return corpus if device is None else corpus.to(device)

    @classmethod
    def from_tree(cls, data_path, split, max_len, rate=wsj0list.FRAME_RATE, device=None):
        """``data_path/<split>/<spk>/*.wav``, speakers and files sorted; ``wsj0list.read_wav``, first channel,
        ``wsj0list.resample`` when a file's rate differs (then, or with any format but 16-bit PCM, the pool is
        fp32).  A clip's name is its file name without ``.wav``."""
        root = os.path.join(data_path, split)
        clips = []
        for spk in sorted(os.listdir(root)):
            if not os.path.isdir(os.path.join(root, spk)):
                continue
            for f in sorted(os.listdir(os.path.join(root, spk))):
                if not f.endswith(".wav"):
                    continue
                path = os.path.join(root, spk, f)
                x, file_rate = wsj0list.read_wav(path)
                if len(x) < 1:
                    raise ValueError(f"{path}: empty clip")
                if file_rate == rate and _is_pcm16(path):
                    x = np.round(x[:max_len] * 32768.0).astype(np.int16)  # (exact: x = q / 32768)
                else:
                    x = wsj0list.resample(x, file_rate, rate)[:max_len]
                clips.append((spk, f[:-4], x))
        if not clips:
            raise ValueError(f"{root}: no <speaker>/*.wav below it")
        return cls.from_clips(clips, max_len, device)

    def to(self, device):
        """Upload the pool and tables and compute ``clip_stats`` (once per corpus)."""
        dev = torch.device(device)
        self.d_pool = torch.from_numpy(self.pool).to(dev)
        self.d_offsets = torch.from_numpy(self.offsets).to(dev)
        self.d_lengths = torch.from_numpy(self.lengths).to(dev)
        self.d_speaker = torch.from_numpy(self.speaker).to(dev)
        self.clip_stats = ops.corpus_stats(self.d_pool, self.d_offsets, self.d_lengths)
        self.device = dev
        return self

    # ------------------------------------------------------------------ use
    def clip(self, c):
        """Clip ``c``'s samples as the float32 signal the kernels see (host)."""
        x = self.pool[self.offsets[c]:self.offsets[c] + self.lengths[c]]
        return x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x

    def gather(self, clips, n):
        """(…, n) float32 zero-padded signals of the clip ids ``clips`` (host): what a host loader would upload."""
        clips = np.asarray(clips)
        raw = np.zeros(clips.shape + (n,), np.float32)
        for idx in np.ndindex(*clips.shape):
            x = self.clip(int(clips[idx]))
            raw[idx][:len(x)] = x
        return raw

    def check_n(self, n):
        if n < self.max_len:
            raise ValueError(f"N = {n} is below the corpus's max_len = {self.max_len} (the clip statistics are over "
                             "the stored crop)")

    def mix(self, clips, gains, K, N, shifts=None, **out):
        """``ops.mix_corpus`` over this corpus: clips, gains, shifts (B, Ks) device tensors -> (src, mix, bad)."""
        self.check_n(N)
        if self.device is None:
            raise RuntimeError("the corpus is on the host only: call to(device) first")
        return ops.mix_corpus(self.d_pool, self.d_offsets, self.d_lengths, self.clip_stats, clips, gains, K, N,
                              shifts=shifts, max_len=self.max_len, **out)


class CorpusFeed:
    """A trainer's side of the corpus step: device buffers for one batch's index arrays -- clips, gains, shifts
    (B, Ks) and, when the caller has them on the host, the speaker ids (B, K), in ONE int32 block, so a step uploads
    once, asynchronously, from pinned memory -- and the ``bad`` counter of out-of-range clip ids."""

    def __init__(self, batch, device):
        self.B, self.device = batch, device
        self.bad = torch.zeros(1, device=device, dtype=torch.int32)
        self._buf = {}

    def mix(self, corpus, clips, gains, shifts, K, N, out_src, out_mix, spk=None, spk_out=None):
        """clips, gains, shifts: host arrays (B, Ks), shifts may be None.  spk (host, (B, K) integers) rides in
        the same upload and lands in ``spk_out`` (the trainer's int32 speaker buffer)."""
        clips = np.asarray(clips)
        if clips.ndim != 2 or clips.shape[0] != self.B or not K <= clips.shape[1] <= ops.MAX_MIX_SOURCES:
            raise ValueError(f"clips {clips.shape}: expected ({self.B}, Ks) with {K} <= Ks <= {ops.MAX_MIX_SOURCES}")
        corpus.check_n(N)
        B, Ks = clips.shape
        n = B * Ks
        host = np.zeros(3 * n + B * K, np.int32)
        host[:n] = clips.reshape(-1)
        host[n:2 * n] = np.ascontiguousarray(np.broadcast_to(np.asarray(gains, np.float32), clips.shape)) \
            .view(np.int32).reshape(-1)
        if shifts is not None:
            host[2 * n:3 * n] = np.asarray(shifts).reshape(-1)
        if spk is not None:
            host[3 * n:] = np.asarray(spk).reshape(-1)
        if (Ks, K) not in self._buf:
            self._buf[Ks, K] = torch.empty(3 * n + B * K, device=self.device, dtype=torch.int32)
        buf = self._buf[Ks, K]
        # (a pinned source: the copy is asynchronous and the host allocator keeps the block until it has run)
        buf.copy_(torch.from_numpy(host).pin_memory(), non_blocking=True)
        part = lambda i: buf[i * n:(i + 1) * n].view(B, Ks)
        if spk is not None:
            spk_out.copy_(buf[3 * n:].view(B, K))
        corpus.mix(part(0), part(1).view(torch.float32), K, N, shifts=None if shifts is None else part(2),
                   out_src=out_src, out_mix=out_mix, bad=self.bad)

    def check(self):
        """After a synchronise: RuntimeError naming the count of out-of-range clip ids since the last check."""
        n = int(self.bad.item())
        if n:
            self.bad.zero_()
            raise RuntimeError(f"mix_corpus: {n} clip id(s) outside the corpus since the last check (those sources "
                               "were silent)")


def features(corpus, batch, device, complex_sources=False):
    """A sampler's batch -> the dict ``wsj0list.features`` returns for the same mixtures: src (B, K, N), mix (B, N),
    mix_complex, mix_mag, src_spec.  N = the corpus's max_len; a background clip (Ks = K + 1) is in the mixture only."""
    dev = torch.device(device)
    clips = torch.from_numpy(np.ascontiguousarray(batch["clips"], np.int32)).to(dev)
    gains = torch.from_numpy(np.ascontiguousarray(batch["gains"], np.float32)).to(dev)
    shifts = batch.get("shifts")
    shifts = None if shifts is None else torch.from_numpy(np.ascontiguousarray(shifts, np.int32)).to(dev)
    K, N = batch.get("K", clips.shape[1]), corpus.max_len
    B = clips.shape[0]
    src, mix, bad = corpus.mix(clips, gains, K, N, shifts=shifts)
    if int(bad.item()):
        raise RuntimeError(f"mix_corpus: {int(bad.item())} clip id(s) outside the corpus")
    Xc, Xm = ops.stft(mix, complex_out=True, mag_out=True)
    if complex_sources:
        Sc, _ = ops.stft(src.view(B * K, N), complex_out=True, mag_out=False)
        S = Sc.view(B, K, *Sc.shape[1:])
    else:
        _, Sm = ops.stft(src.view(B * K, N), complex_out=False, mag_out=True)
        S = Sm.view(B, K, *Sm.shape[1:])
    return dict(src=src, mix=mix, mix_complex=Xc, mix_mag=Xm, src_spec=S)


class ListMixSampler:
    """The iteration of ``wsj0list.ListBatches`` over a corpus: ``parse_line`` per line, ``batch_total = lines //
    batch``, ``random.Random(seed).shuffle`` of the line order per epoch, and with ``augment`` each source's shift
    drawn ``random.sample(range(len), 1)[0]`` in line order on the module-level ``random``.  Yields host arrays
    only: clips, lengths, shifts (B, k) int32 (shifts None without augment), gains (B, k) float32 = 10^(dB/20),
    speakers and names per row.  A line naming a clip the corpus does not hold raises KeyError at construction.

    ``state_dict()`` after a batch holds the epoch's order, the position in it and the shuffle generator;
    ``load_state_dict`` makes the next ``iter()`` continue that epoch behind that batch."""

    def __init__(self, corpus, list_path, batch, shuffle=False, seed=1, augment=False):
        with open(list_path) as f:
            lines = [l for l in f.readlines() if l.strip()]
        self.items = [wsj0list.parse_line(l) for l in lines]
        ks = {len(it) for it in self.items}
        if len(ks) != 1:
            raise ValueError("a list file holds mixtures of one size (mix_{k}_spk_*.txt)")
        self.k = ks.pop()
        self.corpus, self.B, self.shuffle, self.augment = corpus, batch, shuffle, augment
        self.rng = random.Random(seed)
        self.ids = np.array([[corpus.index[(s, n)] for s, n, _ in it] for it in self.items], np.int32)
        self.gains = np.array([[10.0 ** (db / 20.0) for _, _, db in it] for it in self.items], np.float32)
        self.batch_total = len(self.items) // batch
        self._order, self._pos, self._resume = None, 0, False

    def __iter__(self):
        if self._resume:
            order, start, self._resume = self._order, self._pos, False
        else:
            order, start = list(range(len(self.items))), 0
            if self.shuffle:
                self.rng.shuffle(order)
        self._order = order
        for bi in range(start, self.batch_total):
            rows = order[bi * self.B:(bi + 1) * self.B]
            clips = self.ids[rows]
            lengths = self.corpus.lengths[clips]
            shifts = _data.draw_shifts(lengths) if self.augment else None
            self._pos = bi + 1
            yield dict(clips=clips, gains=self.gains[rows], lengths=lengths, shifts=shifts,
                       speakers=[[s for s, _, _ in self.items[i]] for i in rows],
                       names=[[n for _, n, _ in self.items[i]] for i in rows])

    def state_dict(self):
        ver, key, gauss = self.rng.getstate()
        return {"order": None if self._order is None else list(self._order), "pos": self._pos,
                "rng": {"version": ver, "key": list(key), "gauss_next": gauss}}

    def load_state_dict(self, sd):
        order = sd["order"]
        if order is not None and sorted(order) != list(range(len(self.items))):
            raise ValueError("sampler state: the saved order is not a permutation of this list's lines")
        r = sd["rng"]
        self.rng.setstate((r["version"], tuple(int(x) for x in r["key"]), r["gauss_next"]))
        self._order = None if order is None else [int(i) for i in order]
        self._pos = int(sd["pos"])
        self._resume = order is not None and self._pos < self.batch_total


class RandomMixSampler:
    """The on-the-fly draws of ``Torch_multi/predata_multiAims_dB.py:107-145`` over a corpus's speakers: one
    ``mix_k = random.randint(min_mix, max_mix)`` per generator, per mixture ``random.sample(speakers, mix_k)``, the
    dB uniforms (two of ``np.random`` per mixture when ``db`` is set and the gain rule applies; a batch's are taken
    together, which leaves that stream's order unchanged), then per speaker one clip
    ``random.sample(remaining, 1)[0]`` that is removed after use; gains through ``compat._data.gains_of``;
    with ``augment`` a shift per source, ``random.sample(range(len), 1)[0]``, applied as the list loaders' rotation.
    ``noise_clip`` (a clip id): the background of ``predata_multiAims_noisedB.py:198-222``, rotated per mixture by a
    drawn shift and mixed at ``noise_gain`` as source K of Ks = K + 1 -- in the mixture, not a target.

    Stated deviations: a speaker whose list has run out is refilled (the reference raises there); the speakers and
    each speaker's clips stand in the corpus's sorted order, while the reference's come from ``os.listdir``, whose
    order is the file system's -- so the reference's exact RNG stream is not reproduced, only its draws.

    ``batches(n)`` (or iteration, endless) yields host arrays: clips, lengths, shifts (B, Ks) int32, gains (B, Ks)
    float32, speakers (B, K) int32 indices into ``corpus.speaker_names``, ``K``."""

    def __init__(self, corpus, batch, min_mix, max_mix, db=0, gain_rule="db2", augment=False, noise_clip=None,
                 noise_gain=0.3):
        if not 1 <= min_mix <= max_mix <= len(corpus.speaker_names):
            raise ValueError(f"1 <= min_mix <= max_mix <= {len(corpus.speaker_names)} speakers needed")
        if noise_clip is not None and not 0 <= noise_clip < len(corpus):
            raise ValueError(f"noise_clip {noise_clip} is outside the corpus")
        if max_mix + (noise_clip is not None) > ops.MAX_MIX_SOURCES:
            raise ValueError(f"at most {ops.MAX_MIX_SOURCES} sources per mixture")
        self.corpus, self.B, self.augment = corpus, batch, augment
        self.noise_clip, self.noise_gain, self.gain_rule = noise_clip, float(noise_gain), gain_rule
        self.cfg = types.SimpleNamespace(dB=db, MIN_MIX=min_mix, MAX_MIX=max_mix)
        self.mix_k = random.randint(min_mix, max_mix)
        self.remaining = {}  # speaker index -> clip ids not yet used, registered at the speaker's first draw

    def _mixture(self):
        corpus = self.corpus
        spk = random.sample(range(len(corpus.speaker_names)), self.mix_k)
        clips, shifts = [], []
        for s in spk:
            left = self.remaining.get(s)
            if not left:  # first use, or run out: the refill
                left = self.remaining[s] = list(corpus.clips_of[s])
            c = random.sample(left, 1)[0]
            left.remove(c)
            clips.append(c)
            shifts.append(random.sample(range(int(corpus.lengths[c])), 1)[0] if self.augment else 0)
        if self.noise_clip is not None:
            clips.append(self.noise_clip)
            shifts.append(random.sample(range(int(corpus.lengths[self.noise_clip])), 1)[0])
        return spk, clips, shifts

    def batch(self):
        B, K = self.B, self.mix_k
        # the dB uniforms come from np.random, the other draws from random: two streams, so taking a batch's
        # uniforms first leaves each stream's order as the reference's (two per mixture, in mixture order)
        u = np.random.rand(B, 2) if (self.cfg.dB and self.gain_rule != "none") else np.zeros((B, 2))
        gains = _data.gains_of(self.cfg, u, K, self.gain_rule)
        if self.noise_clip is not None:
            gains = np.concatenate([gains, np.full((B, 1), self.noise_gain)], 1)
        rows = [self._mixture() for _ in range(B)]
        clips = np.array([r[1] for r in rows], np.int32)
        return dict(clips=clips, gains=gains.astype(np.float32), lengths=self.corpus.lengths[clips],
                    shifts=np.array([r[2] for r in rows], np.int32) if (self.augment or self.noise_clip is not None)
                    else None, speakers=np.array([r[0] for r in rows], np.int32), K=K)

    def batches(self, n):
        for _ in range(n):
            yield self.batch()

    def __iter__(self):
        while True:
            yield self.batch()

    def state_dict(self):
        return {"mix_k": self.mix_k, "remaining": {str(s): list(v) for s, v in self.remaining.items()}}

    def load_state_dict(self, sd):
        remaining = {int(s): [int(c) for c in v] for s, v in sd["remaining"].items()}
        for s, v in remaining.items():
            if not 0 <= s < len(self.corpus.clips_of) or not set(v) <= set(self.corpus.clips_of[s]):
                raise ValueError(f"sampler state: speaker {s}'s remaining clips are not this corpus's")
        self.mix_k, self.remaining = int(sd["mix_k"]), remaining
