"""The Discriminator's host side (no GPU): the size queries of the C ABI, the bound symbols, the meta
shapes of the two custom ops, the module's reference state_dict, the ``_dislayer_`` checkpoint and the
driver mirror's import surface."""
import ctypes
import importlib

import pytest
import torch

from dl4ss_amd import _lib, build, checkpoint, compat

REF_KEYS = {"cnn.weight": (64, 1, 3, 3), "cnn.bias": (64,), "cnn1.weight": (64, 64, 3, 3), "cnn1.bias": (64,),
            "cnn2.weight": (64, 64, 3, 3), "cnn2.bias": (64,), "final.weight": (1, 36480), "final.bias": (1,)}
SYMBOLS = ["dl4ss_disc_dims", "dl4ss_disc_ws_bytes", "dl4ss_disc_conv1_fwd", "dl4ss_disc_conv64_fwd",
           "dl4ss_disc_head_fwd", "dl4ss_disc_head_bwd", "dl4ss_disc_conv64_bwd", "dl4ss_disc_conv1_bwd"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def test_dims():
    hw = (ctypes.c_int * 6)()
    assert _lib.query("dl4ss_disc_dims", 313, 129, hw) == 36480
    assert list(hw) == [156, 64, 77, 31, 38, 15]
    assert _lib.query("dl4ss_disc_dims", 251, 129, hw) == 28800
    assert _lib.query("dl4ss_disc_dims", 15, 15, hw) == 64 and list(hw) == [7, 7, 3, 3, 1, 1]
    assert _lib.query("dl4ss_disc_dims", 15, 15, None) == 64
    assert _lib.query("dl4ss_disc_dims", 14, 15, hw) == -1
    assert _lib.query("dl4ss_disc_dims", 15, 14, hw) == -1


def test_workspace_query_positive_and_monotone():
    for T, F in ((15, 15), (31, 129), (313, 129)):
        sizes = [_lib.query("dl4ss_disc_ws_bytes", n, T, F) for n in (1, 2, 3, 8, 64, 256)]
        assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
    assert _lib.query("dl4ss_disc_ws_bytes", 0, 313, 129) == -1
    assert _lib.query("dl4ss_disc_ws_bytes", 4, 14, 129) == -1


def test_symbols_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s


def test_compute_entry_points_refuse_bad_sizes_before_any_device_call():
    """No GPU here: a call that reached the device would fail differently (or crash on the fake pointers)."""
    INVALID = 1  # hipErrorInvalidValue
    lib = _lib.lib()
    p = ctypes.c_void_p(64)
    assert lib.dl4ss_disc_conv1_fwd(0, p, p, p, 1, 2, 15, p, None) == INVALID
    assert lib.dl4ss_disc_conv1_fwd(2, p, p, p, 1, 15, 15, p, None) == INVALID
    assert lib.dl4ss_disc_conv64_fwd(0, p, p, p, 1, 7, 2, p, None) == INVALID
    assert lib.dl4ss_disc_conv64_fwd(0, None, p, p, 1, 7, 7, p, None) == INVALID
    assert lib.dl4ss_disc_head_fwd(0, p, p, p, 0, 1, 1, p, p, None) == INVALID
    assert lib.dl4ss_disc_head_bwd(0, p, p, p, None, 1.0, 1, 0, 1, None, p, p, p, p, None) == INVALID
    assert lib.dl4ss_disc_conv64_bwd(0, p, p, p, p, 1, 7, 7, None, p, p, p, 16, None) == INVALID  # workspace too small
    assert lib.dl4ss_disc_conv1_bwd(0, p, p, p, p, 1, 2, 15, None, p, p, p, 1 << 30, None) == INVALID


def test_meta_shapes_of_the_ops():
    from dl4ss_amd import library as L

    assert {"discriminator", "discriminator_bwd"} <= set(L.OPS)
    m = dict(device="meta")
    e = lambda *s: torch.empty(*s, **m)  # noqa: E731
    args = (e(64, 1, 3, 3), e(64), e(64, 64, 3, 3), e(64), e(64, 64, 3, 3), e(64))
    for prec, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        score, y1, y2, y3 = torch.ops.dl4ss.discriminator(e(4, 313, 129), *args, e(1, 36480), e(1), prec)
        assert score.shape == (4, 1) and score.dtype == torch.float32
        assert y1.shape == (4, 156, 64, 64) and y2.shape == (4, 77, 31, 64) and y3.shape == (4, 38, 15, 64)
        assert y1.dtype == y2.dtype == y3.dtype == dt
        for need_dx in (True, False):
            out = torch.ops.dl4ss.discriminator_bwd(e(4, 1), e(4, 313, 129), args[0], args[2], args[4], e(1, 36480),
                                                    score, y1, y2, y3, prec, need_dx)
            assert [tuple(t.shape) for t in out] == [(4, 313, 129) if need_dx else (0,), (64, 1, 3, 3), (64,),
                                                     (64, 64, 3, 3), (64,), (64, 64, 3, 3), (64,), (1, 36480), (1,)]
            assert all(t.dtype == torch.float32 for t in out)


def test_module_state_dict_is_the_references():
    compat.install()
    import myNet

    assert "Discriminator" in myNet.__all__
    d = myNet.Discriminator()
    assert {k: tuple(v.shape) for k, v in d.state_dict().items()} == REF_KEYS
    assert list(d.state_dict()) == list(REF_KEYS)
    assert myNet.Discriminator(251, 129).final.weight.shape == (1, 28800)
    with pytest.raises(RuntimeError):
        myNet.Discriminator(14, 129)


def test_dislayer_checkpoint_round_trip(tmp_path):
    compat.install()
    import myNet

    torch.manual_seed(3)
    a, b = myNet.Discriminator(31, 41), myNet.Discriminator(31, 41)
    p = checkpoint.save_reference_discriminator(a, "mixdotag_WSJ0", 15, str(tmp_path))
    assert p.endswith("param_mixdotag_WSJ0_dislayer_15")
    checkpoint.load_reference_discriminator(b, p)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    # a plain torch.save of the reference's eight keys, as the reference writes it
    plain = str(tmp_path / "plain")
    sd = {k: torch.randn_like(v) for k, v in a.state_dict().items()}
    torch.save(sd, plain)
    checkpoint.load_reference_discriminator(b, plain)
    for k in sd:
        assert torch.equal(sd[k], b.state_dict()[k]), k
    # another map size, a missing key: refused whole
    with pytest.raises(ValueError):
        checkpoint.load_reference_discriminator(myNet.Discriminator(31, 57), plain)
    sd.pop("cnn2.bias")
    torch.save(sd, plain)
    with pytest.raises(KeyError):
        checkpoint.load_reference_discriminator(b, plain)


def test_driver_mirror_imports():
    compat.install(drivers=True)
    m = importlib.import_module("main_run_sstune_dis")
    for n in ("Discriminator", "MIX_SPEECH", "MIX_SPEECH_classifier", "SPEECH_EMBEDDING", "ADDJUST", "ATTENTION",
              "top_k_mask", "build", "train_step", "save_params", "main"):
        assert hasattr(m, n), n
    assert m.Discriminator().final.weight.shape == (1, 36480)
