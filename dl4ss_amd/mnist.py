"""MNIST in the IDX format the reference's ``input_data.read_data_sets`` reads (``*-images-idx3-ubyte`` /
``*-labels-idx1-ubyte``, plain or ``.gz``), and the reference's draw of the picture that names a speaker.
No dataset is shipped or fetched: the caller points at files it has."""
import gzip
import struct

import numpy as np

IMAGE_MAGIC, LABEL_MAGIC = 0x00000803, 0x00000801


def _read(path):
    with (gzip.open if str(path).endswith(".gz") else open)(path, "rb") as f:
        return f.read()


def read_images(path):
    """(N, h, w) float32 in [0, 1] (the bytes / 255) of an idx3-ubyte file."""
    raw = _read(path)
    if len(raw) < 16:
        raise ValueError(f"{path}: {len(raw)} bytes, shorter than an idx3 header")
    magic, n, h, w = struct.unpack(">IIII", raw[:16])
    if magic != IMAGE_MAGIC:
        raise ValueError(f"{path}: magic {magic:#010x}, expected {IMAGE_MAGIC:#010x} (idx3-ubyte images)")
    if len(raw) != 16 + n * h * w:
        raise ValueError(f"{path}: {len(raw) - 16} bytes of pixels, the header says {n} x {h} x {w}")
    return (np.frombuffer(raw, dtype=np.uint8, offset=16).reshape(n, h, w) / 255.0).astype(np.float32)


def read_labels(path):
    """(N) int64 labels of an idx1-ubyte file."""
    raw = _read(path)
    if len(raw) < 8:
        raise ValueError(f"{path}: {len(raw)} bytes, shorter than an idx1 header")
    magic, n = struct.unpack(">II", raw[:8])
    if magic != LABEL_MAGIC:
        raise ValueError(f"{path}: magic {magic:#010x}, expected {LABEL_MAGIC:#010x} (idx1-ubyte labels)")
    if len(raw) != 8 + n:
        raise ValueError(f"{path}: {len(raw) - 8} labels, the header says {n}")
    return np.frombuffer(raw, dtype=np.uint8, offset=8).astype(np.int64)


def read(images_path, labels_path):
    """(images (N, h, w) float32 / 255, labels (N) int64) of an IDX pair; the two counts must agree."""
    images, labels = read_images(images_path), read_labels(labels_path)
    if images.shape[0] != labels.shape[0]:
        raise ValueError(f"{images_path}: {images.shape[0]} images, {labels_path}: {labels.shape[0]} labels")
    return images, labels


def pick(images, labels, spk_idx, rng):
    """The reference's draw (prepare_data.py:186-187): for every speaker index spk (any shape, 1-based as the
    reference counts its speakers) a random image whose label is spk - 1.  Returns spk_idx.shape + (h, w)."""
    spk = np.asarray(spk_idx)
    out = np.empty(spk.shape + images.shape[1:], dtype=images.dtype)
    for pos in np.ndindex(spk.shape):
        where = np.flatnonzero(labels == int(spk[pos]) - 1)
        if where.size == 0:
            raise ValueError(f"mnist.pick: no image of class {int(spk[pos]) - 1} (speaker {int(spk[pos])})")
        out[pos] = images[rng.choice(where)]
    return out
