"""fp64 torch-CPU restatements of the voiceprint kernels (csrc/voiceprint.hip) -- the frame mask, the compaction,
the row shift, the masked mean and the speaker memory -- shared by test_voiceprint_ref_cpu.py and the
test_voiceprint_* GPU files, each taken from the SAME fp32 inputs the kernel gets, with the a-priori error bar of
its fp32 arithmetic (u = 2^-24, one unit per rounding, as tests/small_ref.py counts them).

Mask, compaction and shift move values and compare bitwise: no bar.

Sums.  A sum of n exact terms in fp32 errs, whatever the order, by at most (n - 1 + 1) u S = n u S, S = sum |terms|
(n - 1 additions and the second-order unit, as in small_ref); a sum of n products by (n + 1) u S.  A division or a
square root adds one u of its result.  Through y = a / N an absolute error e_a of a and e_N of N arrive as
e_a / N + |a| e_N / N^2 (first order).  The memory's bars below are built from exactly these rules, stage by
stage, from the fp64 values; the products of two first-order errors (each below 1e-5 relative) are covered by the
factor SECOND = 1.01 on the final bar.  No bar here comes from what a GPU returned.
"""
import torch

from small_ref import U, inputs  # noqa: F401 (inputs: the tests' clamped normals)

EPS = 2.220446049250313e-16  # np.spacing(1); 2^-52, exact in fp32
SECOND = 1.01
LENS = [9, 4, 0, 1, 8]   # the tests' utterance lengths of T = 9
IDS = [2, 5, 2, -1, 0, 5]  # and speaker ids


# ---- frame mask, compaction, shift (exact) ------------------------------------------------------------------
def frame_mask(x, rule="nonzero", thr=None, lengths=None):
    """(n, T) bool.  nonzero: any bin != 0 (Masking(0.), nnet.py:46); gt: any bin > thr (MaskingGt, nnet.py:44);
    lengths: the prefix [0, len) instead."""
    n, T, _ = x.shape
    if lengths is not None:
        return torch.arange(T)[None, :] < lengths.long().clamp(0, T)[:, None]
    return (x != 0).any(-1) if rule == "nonzero" else (x > thr).any(-1)


def compact(x, mask):
    """The valid frames of each utterance, in their own order, as a prefix: (xc, len int32, idx int32 (-1 behind))."""
    n, T, _ = x.shape
    xc = torch.zeros_like(x)
    idx = torch.full((n, T), -1, dtype=torch.int32)
    for b in range(n):
        t = torch.nonzero(mask[b]).flatten()
        xc[b, :len(t)] = x[b, t]
        idx[b, :len(t)] = t.int()
    return xc, mask.sum(1).int(), idx


def shift(src, lens, c0, c1, direction, other=0, dst=None):
    """dl4ss_vp_shift with torch indexing: columns [c0, c1) of src (n, T, ld) moved by d = T - len rows (+1: to
    the right-aligned frame, rows < d zero; -1: back, rows >= len zero); the other columns by ``other`` (0: dst's
    own, 1: src with rows >= len zeroed, 2: src)."""
    n, T, ld = src.shape
    dst = torch.full_like(src, float("nan")) if dst is None else dst.clone()
    rest = [c for c in range(ld) if not c0 <= c < c1]
    for b in range(n):
        L = int(lens[b])
        d = T - L
        blk = torch.zeros(T, c1 - c0, dtype=src.dtype)
        if direction > 0:
            blk[d:] = src[b, :L, c0:c1]
        else:
            blk[:L] = src[b, d:, c0:c1]
        dst[b, :, c0:c1] = blk
        if other and rest:
            o = src[b][:, rest].clone()
            if other == 1:
                o[L:] = 0
            dst[b][:, rest] = o
    return dst


# ---- masked mean (MeanPool, extend_layers.py:105-125) -------------------------------------------------------------
def mean_terms(out, lens):
    """The terms of the masked mean of out (n, T, 2H) in the recurrence's frame, zero padded: (n, 2H, T) fp64 --
    term j of column c is the j-th own frame (forward half rows [0, len), reverse half rows [T - len, T))."""
    n, T, D = out.shape
    H = D // 2
    terms = torch.zeros(n, D, T, dtype=torch.float64)
    for b in range(n):
        L = int(lens[b])
        terms[b, :H, :L] = out[b, :L, :H].double().T
        terms[b, H:, :L] = out[b, T - L:, H:].double().T
    return terms


def masked_mean(out, lens):
    """(val (n, 2H) fp64, bar).  vec = sum over the len own frames / (len + eps) (extend_layers.py:121-122);
    n = len exact terms, c = 2: the division (len + eps rounds to len exactly for len >= 1) and one unit to spare.
    len = 0: exactly zero."""
    terms = mean_terms(out, lens)
    den = (lens.double() + EPS)[:, None]
    return terms.sum(-1) / den, (lens.double()[:, None] + 2) * U * terms.abs().sum(-1) / den


def masked_mean_bwd(dvec, lens, T):
    """(val (n, T, 2H) fp64, bar).  dOut = dvec / (len + eps) on the rows the mean read, exact zeros elsewhere; one
    division: bar = u |val|."""
    n, D = dvec.shape
    H = D // 2
    val = torch.zeros(n, T, D, dtype=torch.float64)
    for b in range(n):
        L = int(lens[b])
        g = dvec[b].double() / (L + EPS)
        val[b, :L, :H] = g[:H]
        val[b, T - L:, H:] = g[H:]
    return val, U * val.abs()


# ---- fixed-order column sum (the encoder's bias gradient) ------------------------------------------------------
CS_ROWS = 64  # rows per first-stage block of dl4ss_vp_colsum (include/dl4ss_hip.h states it)


def colsum(A):
    """(val (C) fp64, bar) of the column sums of A (M, C).  M exact terms, summed in whatever grouping, take M - 1
    additions: M u S with the second-order unit, S = sum |terms| (the module docstring's rule)."""
    Ad = A.double()
    return Ad.sum(0), A.shape[0] * U * Ad.abs().sum(0)


def colsum_f32(A, drop_last=False):
    """The kernel's order in sequential fp32: blocks of CS_ROWS rows in ascending row, then the blocks' sums in
    ascending block.  Additions only, so the kernel must give these very bits.  (C) fp32."""
    import numpy as np

    a = A.numpy().astype(np.float32)
    if drop_last:
        a = a[:-1]
    out = np.zeros(a.shape[1], np.float32)
    for r0 in range(0, a.shape[0], CS_ROWS):
        s = np.zeros(a.shape[1], np.float32)
        for r in range(r0, min(r0 + CS_ROWS, a.shape[0])):
            s = (s + a[r]).astype(np.float32)
        out = (out + s).astype(np.float32)
    return torch.from_numpy(out)


# ---- speaker memory (SpkLifeLongMemory / SelectSpkMemory, extend_layers.py:149-216) ------------------------------
def _through_norm(g, eg, a, ea, N, eN, y, ey):
    """Error bound of da = g / N - ((g . a) / N) (a / N) / N, the kernel's backward of y = a / N(a), from the
    bounds of its inputs (y = a / N with bound ey), by the rules in the module docstring."""
    E = a.shape[-1]
    p = g * a
    ga = p.sum(-1, keepdim=True)
    e_ga = (a.abs() * eg + g.abs() * ea).sum(-1, keepdim=True) + (E + 1) * U * p.abs().sum(-1, keepdim=True)
    t1 = g / N
    e_t1 = eg / N + g.abs() * eN / N ** 2 + U * t1.abs()
    x = ga / N
    e_x = e_ga / N + ga.abs() * eN / N ** 2 + U * x.abs()
    z = x * y
    e_z = y.abs() * e_x + x.abs() * ey + U * z.abs()
    w = z / N
    e_w = e_z / N + z.abs() * eN / N ** 2 + U * w.abs()
    return e_t1 + e_w + U * (t1.abs() + w.abs())


def memory(v, ids, mem, dq=None):
    """The memory forward in fp64 from fp32 v (n, E), ids (n), mem (M, E), and (dq given) its backward by autograd.
    Returns a dict: q, u, bar_q, bar_u and dv, bar_dv.  An id outside [0, M) gives a zero query and adds nothing."""
    n, E = v.shape
    M = mem.shape[0]
    vd = v.double().clone().requires_grad_(True)
    eps = torch.full_like(vd, EPS)
    w = torch.where(vd == 0, eps, vd)                           # extend_layers.py:162 (switch: no gradient to eps)
    nv = (w ** 2).sum(1, keepdim=True).sqrt()                   # :163-164
    u = vd / nv                                                 # :165
    valid = (ids >= 0) & (ids < M)
    iv = ids[valid].long()
    A = mem.double().index_add(0, iv, u[valid])                 # :167 inc_subtensor: duplicate ids accumulate
    wA = torch.where(A == 0, torch.full_like(A, EPS), A)        # :169
    NA = (wA ** 2).sum(1, keepdim=True).sqrt()                  # :170-171
    An = A / NA                                                 # :172
    q = torch.where(valid[:, None], An[ids.long().clamp(0, M - 1)], torch.zeros_like(vd))  # :208 gather
    out = dict(q=q.detach(), u=u.detach())
    with torch.no_grad():
        # a norm of exact inputs: E squares summed ((E + 1) u relative), halved by the root, + the root's own unit
        rN = (E + 1) / 2 + 1
        e_u = (rN + 1) * U * u.abs()                            # + the division
        m = torch.zeros(M, 1, dtype=torch.float64).index_add(0, iv, torch.ones(len(iv), 1, dtype=torch.float64))
        S_A = mem.double().abs().index_add(0, iv, u[valid].abs())
        # m + 1 terms (the stored row and m unit vectors, each within e_u): m additions and the second-order unit
        e_A = torch.zeros(M, E, dtype=torch.float64).index_add(0, iv, e_u[valid]) + (m + 1) * U * S_A
        e_N = (A.abs() * e_A).sum(1, keepdim=True) / NA + rN * U * NA
        e_An = e_A / NA + A.abs() * e_N / NA ** 2 + U * An.abs()
        gi = ids.long().clamp(0, M - 1)
        out["bar_u"] = SECOND * e_u
        out["bar_q"] = SECOND * e_An[gi] * valid[:, None]
    if dq is None:
        return out
    dqd = dq.double()
    out["dv"], = torch.autograd.grad(q, vd, dqd)
    with torch.no_grad():
        dqv = dqd * valid[:, None]
        g = torch.zeros(M, E, dtype=torch.float64).index_add(0, iv, dqv[valid])
        Sg = torch.zeros(M, E, dtype=torch.float64).index_add(0, iv, dqv[valid].abs())
        e_dA = _through_norm(g, m * U * Sg, A, e_A, NA, e_N, An, e_An)   # per row (M, E)
        # the vector stage: a = v exact, its norm with the rN bound, y = u
        gA = g / NA - ((g * A).sum(1, keepdim=True) / NA) * (A / NA) / NA
        e_dv = _through_norm(gA[gi], e_dA[gi], vd, torch.zeros_like(vd), nv, rN * U * nv, u, e_u)
        out["bar_dv"] = SECOND * e_dv * valid[:, None]
    return out


# ---- the masked encoder: per-utterance nn.LSTM over the valid prefix, and the alignment scheme -----------------
def encoder_ref(xc, lens, sd, F, H, L, dvec, prefix="spk.layer."):
    """The contract in fp64: nn.LSTM(F, H, L, bidirectional) over each utterance's valid prefix xc[b, :len], the
    voiceprint = sum of the top layer / (len + eps), and the gradients of sum(vec * dvec) by autograd.
    Returns (vec (n, 2H), {name: grad})."""
    lstm = torch.nn.LSTM(F, H, L, batch_first=True, bidirectional=True).double()
    lstm.load_state_dict({k[len(prefix):]: v.detach().double().cpu() for k, v in sd.items()})
    n = xc.shape[0]
    vec = []
    for b in range(n):
        Lb = int(lens[b])
        if Lb == 0:
            vec.append(torch.zeros(2 * H, dtype=torch.float64))
            continue
        o, _ = lstm(xc[b:b + 1, :Lb].double())
        vec.append(o[0].sum(0) / (Lb + EPS))
    vec = torch.stack(vec)
    grads = {}
    if vec.requires_grad:
        (vec * dvec.double()).sum().backward()
        grads = {prefix + k: p.grad.clone() for k, p in lstm.named_parameters()}
    return vec.detach(), grads


def _shift_rows(src, lens, direction):
    """differentiable row shift by d = T - len with zero fill (torch indexing)"""
    n, T, _ = src.shape
    t = torch.arange(T)[None, :]
    d = (T - lens.long())[:, None]
    ts, ok = (t - d, t >= d) if direction > 0 else (t + d, t < lens.long()[:, None])
    g = src.gather(1, ts.clamp(0, T - 1)[:, :, None].expand_as(src))
    return g * ok[:, :, None]


def _lstm_dir(G, w_hh, b_hh, reverse):
    """one direction of a full-length LSTM over G (n, T, 4H) = x W_ih^T + b_ih (torch gate order i, f, g, o)"""
    n, T, _ = G.shape
    H = w_hh.shape[1]
    h = torch.zeros(n, H, dtype=G.dtype)
    c = torch.zeros(n, H, dtype=G.dtype)
    outs = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        i, f, g, o = (G[:, t] + h @ w_hh.T + b_hh).chunk(4, -1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        outs[t] = h
    return torch.stack(outs, 1)


def aligned_encoder(xc, lens, P, L, prefix="spk.layer."):
    """The alignment scheme with torch indexing in fp64: FULL-length recurrences over the compacted batch with the
    reverse direction's rows right-aligned ("Voiceprint memory").  P: {name: fp64 tensor}."""
    n, T, _ = xc.shape
    x = xc.double()
    valid = (torch.arange(T)[None, :] < lens.long()[:, None])[:, :, None]
    for l in range(L):
        w = lambda kind, r: P[f"{prefix}{kind}_l{l}{'_reverse' if r else ''}"]  # noqa: E731
        Gf = x @ w("weight_ih", 0).T + w("bias_ih", 0)
        Gr = _shift_rows(x @ w("weight_ih", 1).T + w("bias_ih", 1), lens, +1)
        of = _lstm_dir(Gf, w("weight_hh", 0), w("bias_hh", 0), False)
        orv = _lstm_dir(Gr, w("weight_hh", 1), w("bias_hh", 1), True)
        x = torch.cat([of * valid, _shift_rows(orv, lens, -1)], -1)
    right = (torch.arange(T)[None, :] >= (T - lens.long())[:, None])[:, :, None]
    s = torch.cat([(of * valid).sum(1), (orv * right).sum(1)], -1)
    return s / (lens.double()[:, None] + EPS)


# ---- the tests' memory case --------------------------------------------------------------------------------------
def memory_case():
    """M = 7, E = 50, ids [2, 5, 2, -1, 0, 5]; mem: two unit rows (row 5 touched, row 3 not), zeros elsewhere;
    v[2] (a duplicate of id 2) all zero."""
    v = inputs(21, 6, 50)
    v[2] = 0
    mem = torch.zeros(7, 50)
    for r, seed in ((5, 22), (3, 23)):
        x = inputs(seed, 50).double()
        mem[r] = (x / x.norm()).float()
    dq = inputs(24, 6, 50)
    return v, torch.tensor(IDS, dtype=torch.int32), mem, dq
