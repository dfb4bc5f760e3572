"""Host-side contract of the fixed-order split-K (no device): the slab ranges and workspace sizes the library
reports, the refusals dl4ss_gemm_fixed makes in front of any launch, the workspace that is never grown inside
a graph capture, and SepTrainer's / VoiceprintEncoder's argument checks."""
import ctypes
import types

import pytest
import torch

from dl4ss_amd import _lib, ops, plan

INVALID = 1  # hipErrorInvalidValue


def _kps(K, s):
    return int(_lib.query("dl4ss_gemm_fixed_kps", K, s))


@pytest.mark.parametrize("K,splitk,kps,S", [(64, 4, 16, 4), (129, 3, 48, 3), (1004, 7, 144, 7), (1000, 31, 48, 21),
                                            (40, 4, 16, 3), (2, 4, 16, 1), (16064, 31, 528, 31), (7, 0, 16, 1)])
def test_slab_ranges(K, splitk, kps, S):
    """kps = ceil(ceil(K / splitk) / 16) * 16, S = ceil(K / kps); the workspace is S dense M x N fp32 slabs"""
    assert _kps(K, splitk) == kps and -(-K // kps) == S
    M, N = 100, 25
    assert ops.gemm_fixed_ws_bytes(M, N, K, splitk) == (S * M * N * 4 if S > 1 else 0)


def test_ws_bytes_edge_cases():
    assert ops.gemm_fixed_ws_bytes(0, 25, 1000, 4) == 0 and ops.gemm_fixed_ws_bytes(100, 25, 0, 4) == 0
    assert _kps(0, 4) == 0
    with pytest.raises(RuntimeError):
        ops.gemm_fixed_ws_bytes(-1, 25, 1000, 4)
    assert ops.gemm_fixed_ws_bytes(100, 25, 16064, "auto") == \
        ops.gemm_fixed_ws_bytes(100, 25, 16064, ops.auto_splitk(100, 25, 16064)) > 0
    # no 32-bit overflow in the size
    assert ops.gemm_fixed_ws_bytes(40000, 40000, 64, 4) == 4 * 40000 * 40000 * 4


def test_split_order_stays_inside_the_any_order_bound():
    """The bound tests/test_voiceprint_wgrad_split_gpu.py relies on, |fl(sum) - sum| <= K 2^-24 sum|a||b| for an
    fp32 sum of K exact products in any order (each product passes through at most K - 1 rounded additions:
    gamma_{K-1} = (K - 1) u / (1 - (K - 1) u) <= K u while K (K - 1) u <= 1, i.e. K <= 4096), checked on a numpy
    restatement of the split order -- per slab an fp32 chain over its k-range, the slabs added in order -- at the
    voiceprint dW_hh shape (M = 100, N = 25, K = n T = 1280, auto's factor) with operands of the encoder's kind:
    dG rows exactly zero behind each utterance's length, h_{t-1} in (-1, 1)."""
    import numpy as np

    M, N, n, T = 100, 25, 8, 160
    K = n * T
    assert K * (K - 1) * 2.0 ** -24 <= 1
    rng = np.random.default_rng(4)
    a = (rng.standard_normal((K, M)) * 1e-3).astype(np.float32)
    b = np.tanh(rng.standard_normal((K, N))).astype(np.float32)
    for u, length in enumerate([160, 0, 37, 160, 1, 96, 129, 64]):
        a[u * T + length:(u + 1) * T] = 0
    splitk = ops.auto_splitk(M, N, K)
    kps = _kps(K, splitk)
    assert splitk > 1 and kps < K
    total = None
    for k0 in range(0, K, kps):
        acc = np.zeros((M, N), np.float32)
        for k in range(k0, min(K, k0 + kps)):  # exact products (fp64 holds them), one rounded fp32 add each
            acc = (acc.astype(np.float64) + np.outer(a[k].astype(np.float64), b[k].astype(np.float64))).astype(np.float32)
        total = acc if total is None else total + acc
    ref = a.astype(np.float64).T @ b.astype(np.float64)
    bound = K * 2.0 ** -24 * (np.abs(a).astype(np.float64).T @ np.abs(b).astype(np.float64))
    err = np.abs(total.astype(np.float64) - ref)
    assert total.dtype == np.float32 and (err <= bound).all()
    assert err.max() > 0


def _call(epi=0, prec=0, ws=64, ws_bytes=1 << 40, M=130, N=257, K=129, splitk=3, A=64):
    """dl4ss_gemm_fixed on fake (never dereferenced) pointers: only calls that are refused before any launch"""
    P = ctypes.c_void_p
    return _lib.lib().dl4ss_gemm_fixed(0, 0, M, N, K, P(A), K, P(64), N, P(64), N, None, epi, 0.0, prec, splitk,
                                       P(ws) if ws else None, ws_bytes, None)


def test_entry_point_refusals_before_any_launch():
    need = 3 * 130 * 257 * 4
    assert _call(ws_bytes=need - 1) == INVALID  # short workspace
    assert _call(ws=None, ws_bytes=0) == INVALID  # missing workspace
    assert _call(prec=1, ws_bytes=need) == INVALID  # bf16 operands with S > 1
    assert _call(epi=1, ws_bytes=need) == INVALID  # an epilogue with S > 1
    assert _call(A=None, ws_bytes=need) == INVALID
    assert _call(M=-1, ws_bytes=need) == INVALID
    assert _call(M=0, ws=None, ws_bytes=0) == 0  # an empty problem launches nothing


def test_workspace_never_grows_inside_a_capture(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(cuda_stream=12345))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    monkeypatch.setattr(ops, "_fixed_ws", {})
    with pytest.raises(RuntimeError, match="before graph capture"):
        ops._fixed_workspace(torch.device("cpu"), 1 << 21)
    # a workspace sized by an earlier eager call is handed out, capture or not
    have = torch.empty(1 << 21, dtype=torch.uint8)
    ops._fixed_ws[(torch.device("cpu"), 12345)] = have
    assert ops._fixed_workspace(torch.device("cpu"), 1 << 21) is have
    with pytest.raises(RuntimeError, match="before graph capture"):
        ops._fixed_workspace(torch.device("cpu"), (1 << 21) + 1)


def test_gemm_argument_checks():
    with pytest.raises(ValueError, match="reduce"):
        ops.gemm(None, None, reduce="tree")
    with pytest.raises(ValueError, match="ws"):
        ops.gemm(None, None, ws=torch.empty(4))


def _net(**kw):
    d = dict(attention="dot", crm=False, adjust=False, E=50, F=129, device=torch.device("cpu"))
    d.update(kw)
    return types.SimpleNamespace(**d)


def _check(precision, splitk_reduce, **kw):
    return plan.check_args(_net(), 8, 2, 16384, kw.pop("mode", "label"), precision, kw.pop("rnn_precision", None),
                           None, None, None, None, None, None, None, "reference", splitk_reduce=splitk_reduce)


@pytest.mark.parametrize("precision", ["bf16", "bf16s", "bf16s2"])
def test_fixed_reduce_is_fp32_only(precision):
    """refused by plan.check_args, in front of any device call"""
    with pytest.raises(ValueError, match="splitk_reduce"):
        _check(precision, "fixed")
    assert _check(precision, "atomic") == (None, None)


def test_fixed_reduce_accepted_on_fp32():
    assert _check("fp32", "fixed") == (None, None)
    assert _check("fp32", "fixed", mode="pit") == (None, None)
    with pytest.raises(ValueError, match="splitk_reduce"):
        _check("fp32", "slabs")
    # the argument is a trailing keyword with a default: the existing positional call is unchanged
    assert plan.check_args(_net(), 8, 2, 16384, "label", "fp32", None, None, None, None, None, None, None, None,
                           "reference") == (None, None)


def test_trainer_refuses_fixed_on_bf16_before_any_device_call(monkeypatch):
    from dl4ss_amd import engine

    def no_device(*a, **k):
        raise AssertionError("a device call in front of the refusal")

    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "query", no_device)
    with pytest.raises(ValueError, match="splitk_reduce"):
        engine.SepTrainer(_net(), 8, 2, 16384, precision="bf16", splitk_reduce="fixed")


def test_encoder_wgrad_split_argument():
    from dl4ss_amd.voiceprint import VoiceprintEncoder, VoiceprintNet

    vnet = VoiceprintNet(device="cpu")
    for bad in (0, -2, 2.0, "fixed", True, None):
        with pytest.raises(ValueError, match="wgrad_split"):
            VoiceprintEncoder(vnet, 8, 160, wgrad_split=bad)
