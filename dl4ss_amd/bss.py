"""BSS-eval SDR / SIR / SAR with the permutation search, on the GPU.

Replaces ``separation.bss_eval_sources`` as called by ``bss_test.cal``
(``Torch_multi/bss_test.py:12-61``).  The reference's ``separation`` module is not vendored
(SURVEY 8c item 3): the algorithm is BSS_EVAL v3 as published (512-tap time-invariant
distortion filters; restated explicitly in ``oracle/bss_eval.py``) -- parity unpinned
against the reference's own copy, pinned against the restatement.

Closed form used here (exact for the least-squares projections BSS_EVAL defines): with
G the Gram matrix of the delays 0..511 of the K references, D_e = <delayed refs, est_e>
and E_e = |est_e|^2,

    Q_all = D^T G^{-1} D          = |P_all(e)|^2
    Q_j   = D_j^T G_jj^{-1} D_j   = |P_j(e)|^2 = |s_true|^2
    SDR = 10 log10(Q_j / (E - Q_j)),  SIR = 10 log10(Q_j / (Q_all - Q_j)),
    SAR = 10 log10(Q_all / (E - Q_all))

(P_j(e) lies in the span P_all projects on, so every cross term collapses to these.)
The correlations (the only O(N L) work: 4.2 GMAC fp64 for 32 two-speaker mixtures of 4 s)
and the Gram assembly are HIP kernels (``bss.hip``); the dense SPD solves are batched fp64
Cholesky factorisations through torch.linalg (rocSOLVER) on the same stream.
"""
import ctypes
import itertools

import numpy as np
import torch

from . import _lib

FLEN = 512


def _criteria_db(num, den):
    den = torch.where(den > 0, den, torch.zeros_like(den))
    return torch.where(den > 0, 10.0 * torch.log10(num / den), torch.full_like(num, float("inf")))


def _spd_solve(G, D):
    """Batched G^{-1} D (G symmetric positive (semi)definite): Cholesky, pseudo-inverse for
    the batches whose factorisation fails (singular Gram, e.g. a silent reference; the
    restated algorithm falls back to least squares there)."""
    Lc, info = torch.linalg.cholesky_ex(G)
    C = torch.cholesky_solve(D, Lc)
    bad = torch.nonzero(info).flatten()
    if bad.numel():
        C[bad] = torch.linalg.pinv(G[bad], hermitian=True) @ D[bad]
    return C


def bss_eval_matrices(refs, ests, flen=FLEN):
    """refs (M, K, N), ests (M, Ke, N) float32 on the device -> sdr, sir, sar (M, Ke, K)
    float64 on the device: the criteria of every (estimate, true source) pair."""
    refs, ests = refs.float(), ests.float()
    if not refs.is_cuda:
        raise RuntimeError("bss_eval runs on the GPU (no CPU fallback)")
    M, K, N = refs.shape
    Ke = ests.shape[1]
    P = K + Ke
    L = flen
    dev = refs.device
    x = torch.cat([refs, ests], 1).contiguous()
    R = torch.empty(M, P, P, L, dtype=torch.float64, device=dev)
    st = _lib.stream_ptr()
    _lib.call("dl4ss_bss_corr", _lib.ptr(x), M, P, N, L, _lib.ptr(R), st)
    KL = K * L
    G = torch.empty(M, KL, KL, dtype=torch.float64, device=dev)
    Gd = torch.empty(M, K, L, L, dtype=torch.float64, device=dev)
    D = torch.empty(M, KL, Ke, dtype=torch.float64, device=dev)
    _lib.call("dl4ss_bss_gram", _lib.ptr(R), M, P, K, L, _lib.ptr(G), _lib.ptr(Gd), _lib.ptr(D), st)
    q_all = (D * _spd_solve(G, D)).sum(1)  # (M, Ke)
    Dj = D.view(M, K, L, Ke).reshape(M * K, L, Ke)
    q_j = (Dj * _spd_solve(Gd.view(M * K, L, L), Dj)).sum(1).view(M, K, Ke).transpose(1, 2)  # (M, Ke, K)
    idx = torch.arange(K, P, device=dev)
    E = R[:, idx, idx, 0][:, :, None]  # (M, Ke, 1)
    qa = q_all[:, :, None]
    sdr = _criteria_db(q_j, E - q_j)
    sir = _criteria_db(q_j, qa - q_j)
    sar = _criteria_db(qa.expand_as(q_j), E - qa)
    return sdr, sir, sar


def bss_eval_gain(srcs, ests, index, lengths=None):
    """BSS Eval 2.0's gain decomposition (``bss_decomp_gain`` + ``bss_crit``; include/dl4ss_eval.h), batched:
    srcs (M, J, N), ests (M, Ke, N) float32 on the device, ``index`` Ke ints (estimate e estimates source
    index[e]), ``lengths`` (M) int32 on the device (None: N) -- only the first lengths[m] samples of utterance m
    exist.  Returns ((sdr, sir, sar), singular): three (M, Ke) float64 device tensors and the int32 device count
    (1 element) of (utterance, estimate) pairs whose Gram matrix was singular (their criteria are NaN).  Nothing
    syncs with the host."""
    if not (srcs.is_cuda and ests.is_cuda):
        raise RuntimeError("bss_eval_gain runs on the GPU (no CPU fallback)")
    if srcs.dim() != 3 or ests.dim() != 3 or srcs.shape[0] != ests.shape[0] or srcs.shape[2] != ests.shape[2]:
        raise ValueError(f"bss_eval_gain: srcs {tuple(srcs.shape)} and ests {tuple(ests.shape)} must be (M, J, N) "
                         "and (M, Ke, N)")
    if srcs.dtype != torch.float32 or ests.dtype != torch.float32:
        raise ValueError("bss_eval_gain: float32 signals")
    M, J, N = srcs.shape
    Ke = ests.shape[1]
    index = [int(i) for i in index]
    if not (1 <= J <= 4 and 1 <= Ke <= 4) or len(index) != Ke or any(not 0 <= i < J for i in index) or N < 1:
        raise ValueError(f"bss_eval_gain: J = {J}, Ke = {Ke} must be 1..4, N >= 1, and index {index} Ke entries "
                         "in [0, J)")
    if lengths is not None and (lengths.dtype != torch.int32 or tuple(lengths.shape) != (M,) or not lengths.is_cuda):
        raise ValueError("bss_eval_gain: lengths must be (M) int32 on the device")
    dev = srcs.device
    ws_bytes = _lib.query("dl4ss_bss_gain_ws_bytes", M, N)
    ws = torch.empty(max(ws_bytes, 8) // 8, dtype=torch.float64, device=dev)
    crit = torch.empty(M, Ke, 3, dtype=torch.float64, device=dev)
    singular = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("dl4ss_bss_gain", src=_lib.ptr(srcs), est=_lib.ptr(ests), index=(ctypes.c_int * Ke)(*index),
              n_eff=_lib.ptr(lengths), M=M, J=J, Ke=Ke, N=N, ws=_lib.ptr(ws), ws_bytes=ws_bytes,
              crit=_lib.ptr(crit), singular=_lib.ptr(singular), stream=_lib.stream_ptr())
    return (crit[..., 0], crit[..., 1], crit[..., 2]), singular


def bss_eval_target(target, noise, pred, mix, lengths=None):
    """``BSS_EVAL.m`` of the Keras trees (DL4SS_Keras/predict.py:259-282), batched: target, noise, pred, mix (M, N)
    float32 on the device.  SDR / SIR / SAR: the gain decomposition of ``pred`` on [noise; target] with the target
    as the source it estimates; NSDR = SDR - SDR(mix decomposed on [target] alone).  Returns a dict of (M) float64
    device tensors ``SDR, SIR, SAR, NSDR`` and ``singular`` (the int32 device count over both decompositions)."""
    srcs = torch.stack([noise, target], 1).contiguous()
    (sdr, sir, sar), s1 = bss_eval_gain(srcs, pred[:, None].contiguous(), [1], lengths)
    (sdr_mix, _, _), s2 = bss_eval_gain(target[:, None].contiguous(), mix[:, None].contiguous(), [0], lengths)
    return dict(SDR=sdr[:, 0], SIR=sir[:, 0], SAR=sar[:, 0], NSDR=sdr[:, 0] - sdr_mix[:, 0], singular=s1 + s2)


def bss_eval_sources(refs, ests, flen=FLEN):
    """Batched bss_eval_sources: refs / ests (M, K, N) (torch on the GPU, or numpy / CPU
    tensors that are moved there) -> numpy (sdr, sir, sar, perm), each (M, K): row m holds the
    criteria of (estimate perm[m][j], source j), perm maximising the mean SIR (first maximum
    in itertools order), as separation.bss_eval_sources returns per mixture."""
    refs = torch.as_tensor(refs)
    ests = torch.as_tensor(ests)
    if not refs.is_cuda:
        refs, ests = refs.cuda(), ests.cuda()
    if refs.dim() == 2:
        refs, ests = refs[None], ests[None]
    if refs.shape != ests.shape:
        raise ValueError("bss_eval_sources needs as many estimates as references")
    sdr, sir, sar = (t.cpu().numpy() for t in bss_eval_matrices(refs, ests, flen))
    M, K = refs.shape[:2]
    perms = list(itertools.permutations(range(K)))
    dum = np.arange(K)
    out = [np.empty((M, K)) for _ in range(3)] + [np.empty((M, K), dtype=np.int64)]
    for m in range(M):
        mean_sir = np.array([np.mean(sir[m][list(p), dum]) for p in perms])
        popt = list(perms[int(np.argmax(mean_sir))])
        out[0][m], out[1][m], out[2][m] = sdr[m][popt, dum], sir[m][popt, dum], sar[m][popt, dum]
        out[3][m] = popt
    return tuple(out)
