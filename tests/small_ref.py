"""fp64 torch-CPU restatements of the step's small kernels (csrc/small.hip, csrc/modules.hip, the column
sums of csrc/convert.hip) shared by test_small_ref_cpu.py and the test_small_* GPU files, each taken from
the SAME fp32 inputs the kernel gets, with the a-priori error bar of its fp32 arithmetic.

Sums of products.  Every such output is returned as a `Sum`: the fp64 value, S = sum |terms| (fp64) and the
term count n.  A product of two fp32 numbers is exact in fp64, so the fp64 terms are the exact terms.  In
fp32, whatever the order or tree of the additions, a term passes through at most one product rounding and
n - 1 additions, so the error of the sum is at most ((1 + u)^n - 1) S <= (n + 1) u S while n^2 u <= 1
(n <= 4096: every sum here); the bar is

    bar = (n + c) u S,     u = 2^-24,

where c counts that second-order unit and the further roundings after the sum (each at most u |result|
<= u S).  c is stated beside each operation below.  No bar here comes from what a GPU returned.
"""
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
CRM_K = 10.0  # the cRM branch's 10 tanh

Sum = namedtuple("Sum", "val S n c terms scale")


def bar(s):
    """the a-priori bound (n + c) u S of a Sum (n may be a tensor: ragged term counts)"""
    return (s.n + s.c) * U * s.S


def _sum(terms, c, scale=1.0, n=None):
    terms = terms.double()
    return Sum(terms.sum(-1) * scale, terms.abs().sum(-1) * scale, terms.shape[-1] if n is None else n, c, terms,
               scale)


def inputs(seed, *shape, scale=1.0):
    """Seeded standard normals with the magnitude clamped to [0.7, 1.5] (fp32): every term of a sum built
    from them is within a factor ~5 of the mean term, so no term is negligible against S and a kernel that
    leaves ONE term out misses the bar several times over (test_small_ref_cpu.py checks exactly that)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(*shape, generator=g)
    return (torch.sign(z) + (z == 0)) * z.abs().clamp(0.7, 1.5) * scale


def seq_f32(s, drop_last=False):
    """A sequential fp32 emulation of a Sum: products rounded to fp32, added left to right in fp32, then the
    scale applied as one fp32 division / multiplication.  drop_last: the last term (the last term of the last
    chunk, the last row) left out -- what a kernel with an off-by-one bound would compute."""
    t = s.terms.numpy().astype(np.float32)
    n = t.shape[-1] - (1 if drop_last else 0)
    acc = np.zeros(t.shape[:-1], np.float32)
    for i in range(n):
        acc = (acc + t[..., i]).astype(np.float32)
    if s.scale != 1.0:
        acc = (acc * np.float32(s.scale)).astype(np.float32)
    return torch.from_numpy(acc.astype(np.float64))


# ---- time mean, speaker queries -------------------------------------------------------------------------
def time_mean(h):
    """mean_t h (B, T, D) -> (B, D).  n = T; c = 2: the division by T and the second-order unit."""
    return _sum(h.double().permute(0, 2, 1), 2, 1.0 / h.shape[1])


def query_fwd(mean, idx, emb, wadj):
    """q[b,k,o] = Emb[id][o] + sum_c W[o][c] mean[b][c] + sum_c W[o][D+c] Emb[id][c]; an id of -1 gives a zero
    query (no term at all).  n = D + W + 1 terms (the products and the embedding value); c = 1: the second-order
    unit (the last addition, + Emb[id][o], is one of the n - 1 additions).  wadj None: the plain gather, exact."""
    B, K = idx.shape
    W = emb.shape[1]
    valid = (idx >= 0)
    e = emb.double()[idx.clamp_min(0)] * valid[..., None]  # (B, K, W)
    if wadj is None:
        return _sum(e[..., None], 0)
    D = mean.shape[1]
    wa = wadj.double()
    tm = wa[None, None, :, :D] * mean.double()[:, None, None, :]  # (B, 1, W, D)
    te = wa[None, None, :, D:] * e[:, :, None, :]                 # (B, K, W, W)
    terms = torch.cat([tm.expand(B, K, W, D), te, e[..., None]], -1) * valid[..., None, None]
    return _sum(terms, 1)


def query_bwd(dq, idx, emb, wadj, mean, T, n_labels, old_emb=None, old_wadj=None):
    """Backward of query_fwd from dq (B, K, W); rows with id -1 contribute to nothing.  Returns a dict of Sums:
      dh   (B, D)        = sum_{k,o} W[o][c] dq[b,k,o] / T            n = K W      (wadj given)
      demb (n_labels, W) = old + sum_{rows of the label} (dq[r][c] + sum_o W[o][D+c] dq[r][o])
                                                                        n = rows (W + 1) + 1 (rows: 1 without wadj)
      dwadj (W, D + W)   = old + sum_b (sum_k dq[b,k,o]) mean[b][c]      n = B K + 1   (c < D)
                           old + sum_{b,k} dq[b,k,o] Emb[id][c - D]       n = B K + 1   (c >= D)
    The kernels form u = sum_k dq first, then the products: a term then passes through K - 1 additions, one
    product, the remaining additions, the division by T or the beta product, and the final addition -- never
    more than the n + 3 roundings that c = 3 allows (K - 1 + 1 + W - 1 + 1 <= K W + 1; the other sums are
    plain chains).  old_*: the prefilled gradient (beta 1), None for beta 0."""
    B, K, W = dq.shape
    valid = (idx >= 0)
    d = dq.double() * valid[..., None]
    e = emb.double()[idx.clamp_min(0)] * valid[..., None]
    out = {}
    if wadj is not None:
        D = wadj.shape[1] - W
        wa = wadj.double()
        # dh[b][c]: terms over (k, o)
        t = d[:, :, :, None] * wa[None, None, :, :D]          # (B, K, W, D)
        out["dh"] = _sum(t.permute(0, 3, 1, 2).reshape(B, D, K * W), 3, 1.0 / T)
        # dwadj
        tm = d[:, :, :, None] * mean.double()[:, None, None, :]   # (B, K, W, D)
        te = d[:, :, :, None] * e[:, :, None, :]                  # (B, K, W, W)
        t = torch.cat([tm, te], -1).permute(2, 3, 0, 1).reshape(W, D + W, B * K)
        o = torch.zeros(W, D + W, 1, dtype=torch.float64) if old_wadj is None else old_wadj.double()[..., None]
        out["dwadj"] = _sum(torch.cat([o, t], -1), 3)
    # demb[label][c]: per row the W products and dq[r][c], rows of other labels masked out
    flat = idx.reshape(-1)
    own = (flat[None, :] == torch.arange(n_labels)[:, None]).double()   # (L, BK)
    dr = d.reshape(B * K, W)
    per = [dr[:, :, None]]                                               # (BK, W(c), 1): dq[r][c]
    if wadj is not None:
        per.append(dr[:, None, :] * wa[:, D:].T[None, :, :])             # (BK, W(c), W(o)): W[o][D+c] dq[r][o]
    per = torch.cat(per, -1)                                             # (BK, W, m)
    m = per.shape[-1]
    t = (own[:, :, None, None] * per[None]).permute(0, 2, 1, 3).reshape(n_labels, W, B * K * m)
    o = torch.zeros(n_labels, W, 1, dtype=torch.float64) if old_emb is None else old_emb.double()[..., None]
    nrows = own.sum(1)[:, None]                                          # (L, 1)
    out["demb"] = _sum(torch.cat([o, t], -1), 3, n=nrows * m + 1)
    return out


# ---- column sums ------------------------------------------------------------------------------------------
def colsum(A, old=None):
    """out[n] = old[n] + sum_m A[m][n] (A fp32 or bf16, exact in fp64).  n = M + 1 terms (the rows and the old
    value; M when old is None); c = 2: the second-order unit and the beta product of the _ex form."""
    t = A.double().T
    if old is not None:
        t = torch.cat([old.double()[:, None], t], -1)
    return _sum(t, 2)


# ---- element-wise ---------------------------------------------------------------------------------------------
def tanh_bwd(v, dv):
    """dpre = dv (1 - v^2); the bar 3 u |dv| (v^2, 1 - v^2 and the product, |1 - v^2| <= 1 for a tanh output;
    a fused 1 - v v saves one of them)."""
    return dv.double() * (1.0 - v.double() ** 2), 3 * U * dv.double().abs()


# ---- ATTENTION 'dot' --------------------------------------------------------------------------------------------
def attn_dot_logits(V, q):
    """e[b][r] = sum_e V[b][r][e] q[b][e]: n = E, c = 1 (the second-order unit)."""
    return _sum(V.double() * q.double()[:, None, :], 1)


def attn_dot_fwd(V, q, act):
    """mask = sigmoid(e) (act 0) or 10 tanh(e) (act 1).  The logit's bound goes through the activation's slope
    (<= 1/4, <= 10); the device exponential / tanh is not derivable and takes the bar the project already
    uses for this kernel, 1e-5 of the largest reference value."""
    lg = attn_dot_logits(V, q)
    ref = torch.sigmoid(lg.val) if act == 0 else CRM_K * torch.tanh(lg.val)
    slope = 0.25 if act == 0 else CRM_K
    return ref, slope * bar(lg) + 1e-5 * ref.abs().max()


def attn_dot_bwd(V, q, mask, dmask, act, dV_old=None):
    """From the fp32 mask the forward saved: dE = dmask act'(e), act' = m (1 - m) or 10 (1 - (m/10)^2);
    dV = dV_old + dE q; dq[b][e] = sum_r dE V.
    dE's own bar: sigmoid: 1 - m, the product and the product with dmask, three relative roundings of a value
    <= |dmask| / 4; tanh: t = m * fp32(0.1) (2), t^2 (1 more: 5 u relative on t^2 <= 1), 1 - t^2 (1), the
    products with 10 and dmask (2): <= 8 u * 10 |dmask|.  Both fit  dE_bar = 8 u amax |dmask|, amax = 1/4 or 10.
    dV (one fused multiply-add, or a product and an addition): dE_bar |q| + 2 u (|dE q| + |dV_old|).
    dq: n = R terms, c = 2 (second order, and the partials' tree is part of the n - 1 additions), plus the
    terms' own dE_bar |V| summed."""
    m, dm = mask.double(), dmask.double()
    if act == 0:
        de = dm * m * (1.0 - m)
        amax = 0.25
    else:
        t = m / CRM_K
        de = dm * CRM_K * (1.0 - t * t)
        amax = CRM_K
    de_bar = 8 * U * amax * dm.abs()
    old = torch.zeros_like(V, dtype=torch.float64) if dV_old is None else dV_old.double()
    prod = de[..., None] * q.double()[:, None, :]
    dV = old + prod
    dV_bar = de_bar[..., None] * q.double().abs()[:, None, :] + 2 * U * (prod.abs() + old.abs())
    s = _sum((de[..., None] * V.double()).permute(0, 2, 1), 2)
    dq_bar = bar(s) + (de_bar[..., None] * V.double().abs()).sum(1)
    return dV, dV_bar, s, dq_bar


# ---- Adam -----------------------------------------------------------------------------------------------------
def adam(p, g, m, v, lr, b1, b2, eps, step, gscale=1.0):
    """torch.optim.Adam's update evaluated in fp64 from the fp32 p, g, m, v, with lr, betas, eps as the fp32
    values the kernel receives and the bias corrections as the launcher forms them (double, then rounded to
    fp32):  gs = g gscale;  m' = m + (1 - b1)(gs - m);  v' = b2 v + (1 - b2) gs^2;
            p' = p - (lr / bc1) m' / (sqrt(v') / bc2s + eps).
    Bars by counted fp32 roundings (u = 2^-24; 1 - b1 and 1 - b2 are exact: Sterbenz):
      m': gs, gs - m, the product, the sum: 4 roundings, each of a value <= |m| + |gs|, and the second-order
          unit:  |dm| <= 5 u (|m| + |gs|)
      v': the g^2 term carries gs twice (2), two products (2) and the sum (1); the b2 v term a product and the
          sum:  |dv| <= 5 u v'
      p': the final subtraction u |p'|; the error of m' through the quotient, step |dm| / denom; and on the
          update x = step m' / denom: dv through the root (2.5), sqrtf (1), / bc2s (1), + eps (1), the quotient
          m' / denom (1), step = lr / bc1 (1), the product with step (1) = 8.5 u, within the 12 u allowed:
          |dp| <= u |p'| + step |dm| / denom + 12 u |x|."""
    f = lambda x: float(np.float32(x))
    lr, b1, b2, eps, gscale = f(lr), f(b1), f(b2), f(eps), f(gscale)
    bc1 = f(1.0 - b1 ** step)
    bc2s = f(np.sqrt(1.0 - b2 ** step))
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gs = g * gscale
    m2 = m + (1.0 - b1) * (gs - m)
    v2 = b2 * v + (1.0 - b2) * gs * gs
    step_sz = lr / bc1
    denom = v2.sqrt() / bc2s + eps
    x = step_sz * m2 / denom
    p2 = p - x
    dm = 5 * U * (m.abs() + gs.abs())
    dv = 5 * U * v2
    dp = U * p2.abs() + step_sz * dm / denom + 12 * U * x.abs()
    return (p2, dp), (m2, dm), (v2, dv)


# ---- top-k ---------------------------------------------------------------------------------------------------
def sort_desc(row):
    """ids of one row by descending value, ties lower id first (a stable sort)"""
    return np.argsort(-row.astype(np.float64), kind="stable")


def top_k_mask(prob, alpha, top_k):
    """mask (B, N) of the first min(top_k, #{p > alpha}) ids in descending order; idx (B, top_k) the selected
    ids ascending, -1 padded; count (B)."""
    prob = np.asarray(prob)
    B, N = prob.shape
    mask = np.zeros((B, N), np.float32)
    idx = np.full((B, top_k), -1, np.int32)
    count = np.zeros(B, np.int32)
    for b in range(B):
        lim = min(top_k, int((prob[b] > np.float32(alpha)).sum()))
        sel = np.sort(sort_desc(prob[b])[:lim])
        mask[b, sel] = 1.0
        idx[b, :lim] = sel
        count[b] = lim
    return mask, idx, count


def classifier_select(prob, alpha, top_k, prev):
    """From the probabilities: sort_index (B, top_k) descending (ties lower id, -1 beyond N); chosen (B) the
    first of them not in prev (n_prev, B) when any prob exceeds alpha, else -1."""
    prob = np.asarray(prob)
    B, N = prob.shape
    si = np.full((B, top_k), -1, np.int32)
    chosen = np.full(B, -1, np.int32)
    for b in range(B):
        order = sort_desc(prob[b])[:top_k]
        si[b, :len(order)] = order
        if (prob[b] > np.float32(alpha)).any():
            seen = set(int(x) for x in prev[:, b]) if prev is not None and len(prev) else set()
            for k in order:
                if int(k) not in seen:
                    chosen[b] = k
                    break
    return si, chosen


# ---- the cases both test files use (fp32 CPU tensors, seeded) ---------------------------------------------------
N_LABELS = 12
MEAN_SHAPES = [(1, 1, 1), (2, 15, 63), (3, 17, 65), (2, 83, 130), (1, 251, 600)]            # (B, T, D)
QFWD_SHAPES = [(3, 2, 11, 600, 50), (2, 4, 5, 63, 64), (2, 5, 5, 130, 70), (1, 9, 3, 600, 50)]  # (B, K, T, D, W)
# (B, K, D, W, ids): one row; a small odd case, also with ONE speaker in all 15 rows (a longer single-label sum
# would have n^2 u near 1, where the a-priori bar no longer tells one missing term from rounding); a partial
# last QCH = 32 chunk of the sums over b (B = 33, 66 rows: two 64-row ballots); 70 rows with the same speaker
# at rows 2 and 66 (two ballots); K = 5
QBWD_SHAPES = [(1, 1, 600, 50, "mixed"), (5, 3, 63, 64, "mixed"), (5, 3, 63, 64, "single"),
               (33, 2, 600, 50, "mixed"), (70, 1, 130, 70, "far"), (17, 5, 600, 50, "mixed")]
COLSUM_SHAPES = [(1, 1, 1), (255, 63, 63), (257, 65, 72), (1000, 130, 130)]                   # (M, N, lda)
COLSUM_BF16_VEC = [(300, 513, 520), (1, 8, 8), (256, 512, 512), (257, 520, 520)]
COLSUM_BF16_SCALAR = [(300, 129, 129, 0), (70, 65, 66, 1)]                                    # (.., pointer offset)
DOT_SHAPES = [(1, 1), (2, 255), (2, 256), (3, 257), (2, 903)]                                 # (Bq, R), E = 50
ADAM_N = [1, 3, 4, 5, 1027]
ADAM_N_LARGE = 8192 * 1024 + 5   # the second grid-stride pass of adam_kernel


def query_ids(B, K, kind, seed):
    """(B, K) int64 speaker ids.  mixed: a repeat within the first row (or across rows when K = 1), the last
    label, one -1; the last row stays valid.  single: one speaker throughout.  far: the same speaker at rows
    2 and 66 only (two 64-row ballots of query_bwd_emb), a -1 at row 40."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, N_LABELS - 1, (B * K,), generator=g)
    if kind == "single":
        idx[:] = 5
    elif kind == "far":
        idx[idx == 7] = 3
        idx[2] = idx[66] = 7
        idx[40] = -1
    else:
        if B * K >= 2:
            idx[1] = idx[0]
        if B * K >= 3:
            idx[2] = N_LABELS - 1
        if B * K >= 5:
            idx[B * K // 2] = -1
    return idx.view(B, K)


def query_case(B, K, T, D, W, kind="mixed", seed=0):
    s = 1000 * B + 10 * K + D + seed
    return dict(h=inputs(s, B, T, D), mean=inputs(s + 1, B, D), idx=query_ids(B, K, kind, s + 2),
                emb=inputs(s + 3, N_LABELS, W), wadj=inputs(s + 4, W, D + W, scale=0.3), dq=inputs(s + 5, B, K, W),
                old_emb=inputs(s + 6, N_LABELS, W), old_wadj=inputs(s + 7, W, D + W))


def dot_case(Bq, R, seed=0, E=50):
    s = 77 * Bq + R + seed
    return dict(V=inputs(s, Bq, R, E), q=inputs(s + 1, Bq, 2 * E, scale=0.05), dmask=inputs(s + 2, Bq, R),
                dV_old=inputs(s + 3, Bq, R, E))


def adam_case(n, step, seed=0):
    """p, g, m, v of n elements; non-zero moments for step > 1 (zero at step 1, as a first step has them);
    every 7th element has g = m = v = 0: its p must not move."""
    s = 13 * step + seed + (n % 1000)
    p, g = inputs(s, n), inputs(s + 1, n, scale=0.1)
    m = inputs(s + 2, n, scale=0.05) if step > 1 else torch.zeros(n)
    v = inputs(s + 3, n, scale=0.01).abs() if step > 1 else torch.zeros(n)
    for t in (g, m, v):
        t[::7] = 0.0
    return p, g, m, v
