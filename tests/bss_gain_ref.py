"""BSS Eval 2.0's gain decomposition (bss_decomp_gain + bss_crit), restated with explicit vectors for the tests of
dl4ss_bss_gain.  Written from the published formulae, not from the kernel:

    G = [<s_i, s_j>],  d = [<e, s_j>],  c = G^{-1} d,  P = sum_j c_j s_j,  a = <e, s_idx> / <s_idx, s_idx>
    s_target = a s_idx,  e_interf = P - s_target,  e_artif = e - P
    SDR = 10 log10(|s_target|^2 / |e_interf + e_artif|^2),  SIR = 10 log10(|s_target|^2 / |e_interf|^2),
    SAR = 10 log10(|s_target + e_interf|^2 / |e_artif|^2)

+inf where the denominator is 0 and the numerator is not, NaN where both are.  A source of zero energy is left out
of the span (coefficient 0); if a Cholesky pivot of what remains is <= 1e-12 of its diagonal entry the pair is
singular: three NaNs, counted.  ``dtype`` np.float64 solves with np.linalg.solve; np.longdouble (which LAPACK does
not take) with Gaussian elimination in that type.
"""
import numpy as np

PIVOT_TOL = 1e-12
H4 = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], dtype=np.float32)


def _db(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(num / den)


def _singular(G):
    """A Cholesky pivot (the squared diagonal entry of the factor, before its root) <= 1e-12 of G's diagonal."""
    n = G.shape[0]
    L = np.zeros_like(G)
    D = np.ones(n, dtype=G.dtype)
    for j in range(n):
        piv = G[j, j] - sum(L[j, k] * L[j, k] * D[k] for k in range(j))
        if not piv > PIVOT_TOL * G[j, j]:
            return True
        D[j] = piv
        for i in range(j + 1, n):
            L[i, j] = (G[i, j] - sum(L[i, k] * L[j, k] * D[k] for k in range(j))) / piv
    return False


def _solve(G, d):
    if G.dtype == np.float64:
        return np.linalg.solve(G, d)
    A = np.concatenate([G, d[:, None]], 1).copy()  # Gaussian elimination with partial pivoting
    n = G.shape[0]
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        A[[j, p]] = A[[p, j]]
        for i in range(j + 1, n):
            A[i] -= A[i, j] / A[j, j] * A[j]
    x = np.zeros(n, dtype=G.dtype)
    for j in range(n - 1, -1, -1):
        x[j] = (A[j, n] - A[j, j + 1:n] @ x[j + 1:]) / A[j, j]
    return x


def gain_one(srcs, est, idx, n_eff=None, dtype=np.float64):
    """srcs (J, N), est (N) -> (sdr, sir, sar, singular, cond): the criteria of one estimate, whether its Gram
    matrix was singular, and the condition number of the Gram matrix that was solved (1 for an empty span)."""
    n = srcs.shape[1] if n_eff is None else int(n_eff)
    S = np.asarray(srcs)[:, :n].astype(dtype)
    e = np.asarray(est)[:n].astype(dtype)
    J = S.shape[0]
    G = np.array([[np.sum(S[i] * S[j]) for j in range(J)] for i in range(J)], dtype=dtype).reshape(J, J)
    d = np.array([np.sum(e * S[j]) for j in range(J)], dtype=dtype)
    act = np.array([G[j, j] > 0 for j in range(J)], dtype=bool)
    Ga = G[np.ix_(act, act)]
    nan = float("nan")
    if act.any() and _singular(Ga):
        return nan, nan, nan, True, float("inf")
    c = np.zeros(J, dtype=dtype)
    cond = 1.0
    if act.any():
        c[act] = _solve(Ga, d[act])
        cond = float(np.linalg.cond(Ga.astype(np.float64)))
    P = np.zeros(n, dtype=dtype)
    for j in range(J):
        P = P + c[j] * S[j]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = d[idx] / G[idx, idx]
    s_target = a * S[idx]
    e_interf = P - s_target
    e_artif = e - P
    sdr = _db(np.sum(s_target ** 2), np.sum((e_interf + e_artif) ** 2))
    sir = _db(np.sum(s_target ** 2), np.sum(e_interf ** 2))
    sar = _db(np.sum((s_target + e_interf) ** 2), np.sum(e_artif ** 2))
    return float(sdr), float(sir), float(sar), False, cond


def gain_batch(srcs, ests, index, n_eff=None, dtype=np.float64):
    """srcs (M, J, N), ests (M, Ke, N) -> crit (M, Ke, 3) float64, the singular count and the largest condition
    number among the pairs that were solved."""
    M, Ke = ests.shape[:2]
    crit = np.empty((M, Ke, 3))
    count, worst = 0, 1.0
    for m in range(M):
        for k in range(Ke):
            *c3, sing, cond = gain_one(srcs[m], ests[m, k], index[k], None if n_eff is None else n_eff[m], dtype)
            crit[m, k] = c3
            count += int(sing)
            if not sing:
                worst = max(worst, cond)
    return crit, count, worst


def target_metrics(target, noise, pred, mix, n_eff=None):
    """BSS_EVAL.m for one utterance: pred on [noise; target] with the target estimated; NSDR = SDR - SDR(mix on
    [target] alone)."""
    sdr, sir, sar, _, _ = gain_one(np.stack([noise, target]), pred, 1, n_eff)
    sdr_mix, _, _, _, _ = gain_one(target[None], mix, 0, n_eff)
    return dict(SDR=sdr, SIR=sir, SAR=sar, NSDR=sdr - sdr_mix)


# ---- the inputs the CPU and the GPU tests share ----
SIZES = (1, 2, 63, 64, 65, 255, 257, 4001)
SHAPES = ((1, 1), (2, 2), (3, 1), (4, 4))  # (J, Ke)
BATCHES = (1, 5)
N_EFF_KINDS = ("full", "minus1", "one", "mixed")


def index_of(J, Ke):
    return [1 % J] if Ke == 1 else [e % J for e in range(Ke)]


def make_inputs(M, J, Ke, N):
    """fp32 (srcs (M, J, N), ests (M, Ke, N), index).  Normal sources; each estimate is its source plus 0.4 of every
    other source plus 0.2 of fresh noise (criteria of 5 - 15 dB).  The first two samples of every signal are small
    dyadic numbers, the sources' taken from the columns of a 4 x 4 Hadamard matrix, so that the utterances whose
    whole length is 1 or 2 samples -- where the estimate lies in the span and a criterion is 0 / 0 or x / 0 -- are
    exact in fp64 in any summation order."""
    rng = np.random.default_rng(1000 * N + 100 * J + 10 * Ke)  # (not of M: row 0 of M = 5 is the M = 1 input)
    index = index_of(J, Ke)
    srcs = np.empty((M, J, N), dtype=np.float32)
    ests = np.empty((M, Ke, N), dtype=np.float32)
    for m in range(M):
        s = rng.standard_normal((J, N)).astype(np.float32)
        noise = rng.standard_normal((Ke, N)).astype(np.float32)
        e = np.empty((Ke, N), dtype=np.float32)
        for k in range(Ke):
            others = sum((s[j] for j in range(J) if j != index[k]), np.zeros(N, dtype=np.float32))
            e[k] = s[index[k]] + np.float32(0.4) * others + np.float32(0.2) * noise[k]
        w = min(N, 2)
        s[:, :w] = 0.5 * H4[:J, :w]
        e[:, :w] = (np.array([[3, 1], [-1, 2], [2, -3], [1, 1]], dtype=np.float32) / 4)[:Ke, :w]
        srcs[m], ests[m] = s, e
    return srcs, ests, index


def n_eff_of(kind, M, N):
    if kind == "full":
        return np.full(M, N, dtype=np.int32)
    if kind == "minus1":
        return np.full(M, N - 1, dtype=np.int32)
    if kind == "one":
        return np.ones(M, dtype=np.int32)
    return np.array([(N, N - 1, 1, max(1, N // 2), N)[m % 5] for m in range(M)], dtype=np.int32)
