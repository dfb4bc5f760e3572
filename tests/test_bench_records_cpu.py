"""The bench line's roofline fields read committed profile records (no GPU): the PMC traffic of
the STFT launch, the MFMA-busy counter of the in-step Linear GEMM and the measured
streaming ceiling must all resolve, so a renamed kernel (rocprofv3 spells template arguments
out) or a missing profile shows up here instead of as a silent null in BENCH_*.json."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_pmc_records_resolve():
    traffic = bench.pmc_traffic("stft_fwd_kernel", [bench.stft_grid_threads(4096, 251)])
    assert traffic is not None and 2.0e9 < traffic < 2.4e9  # algorithmic 2.116 GB per launch
    busy = bench.pmc_mfma_busy(bench.GEMM_GL_LINEAR)
    assert busy is not None and 0.0 < busy < 1.0


def test_stream_ceiling_resolves():
    c = bench.stream_ceiling("r1w3")
    assert c is not None and 3000.0 < c < bench.HBM_PEAK_GBS


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_float32_and_seeded_sample(tmp_path, monkeypatch):
    import numpy as np
    import torch

    monkeypatch.setattr(bench, "DUMP_BUDGET", 4 * 2 * 100)  # two arrays -> 100 elements each
    big = torch.arange(1000, dtype=torch.float64).view(10, 100)
    small = torch.tensor([3, -1], dtype=torch.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (100,) and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and set(a) <= set(range(1000))  # a sorted sample of the elements, no repeats
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.tolist() == [3.0, -1.0]  # within its part: whole, in its own shape


def test_standin_dump_is_reproducible(tmp_path, monkeypatch):
    """--dump-outputs end to end on the CPU stand-in step: same arguments, same arrays."""
    import numpy as np
    import torch

    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    threads = torch.get_num_threads()
    try:
        for d in ("a", "b"):
            bench.main(["--standin", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / d)])
    finally:
        torch.set_num_threads(threads)
    for name in ("loss", "params"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and a.size > 0 and np.all(np.isfinite(a)) and np.array_equal(a, b)
