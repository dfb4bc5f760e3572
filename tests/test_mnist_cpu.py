"""dl4ss_amd/mnist.py: the IDX reader (plain and gzip, magic and sizes checked) and the reference's draw of the
picture that names a speaker.  No dataset: each test writes a tiny IDX pair into tmp_path."""
import gzip

import numpy as np
import pytest

import imagequery_ref as ir
from dl4ss_amd import mnist


def _pair(n=12, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(n, 28, 28), dtype=np.uint8), (np.arange(n) % 4).astype(np.uint8)


def _write(path, data, gz):
    with (gzip.open if gz else open)(path, "wb") as f:
        f.write(data)


@pytest.mark.parametrize("gz", [False, True])
def test_round_trip(tmp_path, gz):
    img, lab = _pair()
    bi, bl = ir.idx_bytes(img, lab)
    ext = ".gz" if gz else ""
    pi, pl = tmp_path / ("t10k-images-idx3-ubyte" + ext), tmp_path / ("t10k-labels-idx1-ubyte" + ext)
    _write(pi, bi, gz)
    _write(pl, bl, gz)
    images, labels = mnist.read(pi, pl)
    assert images.shape == (12, 28, 28) and images.dtype == np.float32 and labels.dtype == np.int64
    assert np.array_equal(images, (img / 255.0).astype(np.float32)) and np.array_equal(labels, lab)
    assert images.min() >= 0.0 and images.max() <= 1.0


def test_bad_files_are_refused(tmp_path):
    img, lab = _pair()
    bi, bl = ir.idx_bytes(img, lab)
    pi, pl = tmp_path / "images-idx3-ubyte", tmp_path / "labels-idx1-ubyte"
    _write(pl, bl, False)
    _write(pi, bl[:4] + bi[4:], False)  # the labels' magic on the image file
    with pytest.raises(ValueError, match="magic"):
        mnist.read(pi, pl)
    _write(pi, bi[:-5], False)  # short
    with pytest.raises(ValueError, match="pixels"):
        mnist.read(pi, pl)
    _write(pi, bi[:10], False)  # shorter than the header
    with pytest.raises(ValueError, match="header"):
        mnist.read(pi, pl)
    _write(pi, bi, False)
    _write(pl, bi[:4] + bl[4:], False)  # the images' magic on the label file
    with pytest.raises(ValueError, match="magic"):
        mnist.read(pi, pl)
    _write(pl, bl + b"\x00", False)  # one label more than the header says
    with pytest.raises(ValueError, match="labels"):
        mnist.read(pi, pl)
    _write(pl, ir.idx_bytes(img, lab[:-1])[1], False)  # a consistent file of 11 labels for 12 images
    with pytest.raises(ValueError, match="12 images"):
        mnist.read(pi, pl)


def test_pick_returns_images_of_the_asked_class_only():
    img, lab = _pair(40)
    images = (img / 255.0).astype(np.float32)
    rng = np.random.default_rng(3)
    spk = np.array([[1, 2], [4, 3], [2, 2]])  # 1-based speakers: classes 0 .. 3
    seen = set()
    for _ in range(20):
        out = mnist.pick(images, lab.astype(np.int64), spk, rng)
        assert out.shape == (3, 2, 28, 28) and out.dtype == np.float32
        for pos in np.ndindex(spk.shape):
            hits = [i for i in range(40) if np.array_equal(images[i], out[pos])]
            assert len(hits) == 1 and lab[hits[0]] == spk[pos] - 1
            seen.add(hits[0])
    assert len(seen) > 8  # a random draw, not always the first image of the class
    with pytest.raises(ValueError, match="class 7"):
        mnist.pick(images, lab.astype(np.int64), np.array([8]), rng)
