"""The voiceprint references check themselves on the CPU: a sequential fp32 emulation of each kernel's arithmetic
meets the a-priori bar of tests/voiceprint_ref.py, the same emulation with ONE term left out (the last valid frame
of the mean, the last row of the column sum, the last duplicate's contribution to a memory row) misses it, and the alignment scheme of the masked
encoder -- full-length recurrences with the reverse direction's rows right-aligned -- equals per-utterance
nn.LSTM over the valid prefix in fp64."""
import numpy as np
import torch

import voiceprint_ref as ref

f32 = np.float32
EPS32 = f32(ref.EPS)
LENS, IDS, memory_case = ref.LENS, ref.IDS, ref.memory_case


def _mean_f32(out, lens, drop_last=False):
    terms = ref.mean_terms(out, lens).numpy().astype(f32)
    n, D, _ = terms.shape
    vec = np.zeros((n, D), f32)
    for b in range(n):
        L = int(lens[b])
        acc = np.zeros(D, f32)
        for t in range(L - (1 if drop_last else 0)):
            acc = (acc + terms[b, :, t]).astype(f32)
        vec[b] = acc / (f32(L) + EPS32)
    return torch.from_numpy(vec.astype(np.float64))


def test_masked_mean_bar():
    out = ref.inputs(11, 5, 9, 50)
    lens = torch.tensor(LENS, dtype=torch.int32)
    val, bar = ref.masked_mean(out, lens)
    assert (val[2] == 0).all() and (bar[2] == 0).all()  # len 0: exactly zero
    got = _mean_f32(out, lens)
    assert ((got - val).abs() <= bar).all()
    miss = _mean_f32(out, lens, drop_last=True)
    has = lens > 0
    assert ((miss - val).abs() > 3 * bar)[has].all()


def test_masked_mean_bwd_bar():
    dvec = ref.inputs(12, 5, 50)
    lens = torch.tensor(LENS, dtype=torch.int32)
    val, bar = ref.masked_mean_bwd(dvec, lens, 9)
    got = np.zeros((5, 9, 50), f32)
    for b, L in enumerate(LENS):
        g = dvec[b].numpy() / (f32(L) + EPS32)
        got[b, :L, :25] = g[:25]
        got[b, 9 - L:, 25:] = g[25:]
    got = torch.from_numpy(got.astype(np.float64))
    assert ((got - val).abs() <= bar).all()
    assert (val[2] == 0).all() and (val[1, 4:, :25] == 0).all() and (val[1, :5, 25:] == 0).all()


def test_colsum_bar():
    A = ref.inputs(13, 3 * ref.CS_ROWS + 7, 11)  # three full blocks and a short one
    val, bar = ref.colsum(A)
    assert ((ref.colsum_f32(A).double() - val).abs() <= bar).all()
    assert ((ref.colsum_f32(A, drop_last=True).double() - val).abs() > 3 * bar).all()


def _norm32(a):
    w = np.where(a == 0, EPS32, a).astype(f32)
    s = f32(0)
    for e in range(len(w)):
        s = f32(s + f32(w[e] * w[e]))
    return f32(np.sqrt(s))


def _dot32(a, b):
    s = f32(0)
    for e in range(len(a)):
        s = f32(s + f32(a[e] * b[e]))
    return s


def _through_norm32(g, a, N):
    ga = _dot32(g, a)
    return (g / N - (f32(ga / N) * (a / N)).astype(f32) / N).astype(f32)


def _memory_f32(v, ids, mem, dq, drop_last_dup=False):
    """the kernels' arithmetic, sequential, in fp32; drop_last_dup: the last duplicate of the first duplicated id
    is left out of its row's accumulation"""
    v, mem, dq = (t.numpy().astype(f32) for t in (v, mem, dq))
    n, E = v.shape
    M = mem.shape[0]
    u = np.stack([v[i] / _norm32(v[i]) for i in range(n)]).astype(f32)
    skip = None
    if drop_last_dup:
        dup = next(i for i in ids if i >= 0 and ids.count(i) > 1)
        skip = max(j for j in range(n) if ids[j] == dup)
    q, dv = np.zeros((n, E), f32), np.zeros((n, E), f32)
    for i, id_ in enumerate(ids):
        if not 0 <= id_ < M:
            continue
        A, g = mem[id_].copy(), np.zeros(E, f32)
        for j in range(n):
            if ids[j] == id_:
                if j != skip:
                    A = (A + u[j]).astype(f32)
                g = (g + dq[j]).astype(f32)
        N = _norm32(A)
        q[i] = A / N
        dv[i] = _through_norm32(_through_norm32(g, A, N), v[i], _norm32(v[i]))
    return (torch.from_numpy(x.astype(np.float64)) for x in (q, u, dv))


def test_memory_bars():
    v, ids, mem, dq = memory_case()
    r = ref.memory(v, ids, mem, dq)
    assert (r["q"][3] == 0).all() and (r["dv"][3] == 0).all() and (r["u"][2] == 0).all()
    q, u, dv = _memory_f32(v, IDS, mem, dq)
    assert ((u - r["u"]).abs() <= r["bar_u"]).all()
    assert ((q - r["q"]).abs() <= r["bar_q"]).all()
    assert ((dv - r["dv"]).abs() <= r["bar_dv"]).all()
    # the bars are tight enough to see one missing contribution: id 5's second voiceprint left out of its row
    # (reordered so that the left-out duplicate is a non-zero voiceprint)
    ids5 =[5, 2, 5, -1, 0, 2]  # the first duplicated id is now 5 (two non-zero voiceprints)
    r5 = ref.memory(v[[1, 0, 5, 3, 4, 2]], torch.tensor(ids5, dtype=torch.int32), mem, dq)
    q3, _, dv3 = _memory_f32(v[[1, 0, 5, 3, 4, 2]], ids5, mem, dq, drop_last_dup=True)
    rows = [0, 2]
    assert ((q3 - r5["q"]).abs() > 3 * r5["bar_q"])[rows].all()
    assert ((dv3 - r5["dv"]).abs() > 3 * r5["bar_dv"])[rows].any(1).all()


def test_memory_reference_semantics():
    """Store then a forward with all-zero v returns the stored rows re-normalised; mem is never written."""
    v, ids, mem, _ = memory_case()
    keep = mem.clone()
    r = ref.memory(v, ids, mem)
    assert torch.equal(mem, keep)
    mem2 = mem.clone()
    for i, id_ in enumerate(IDS):
        if id_ >= 0:
            mem2[id_] = r["q"][i].float()
    r2 = ref.memory(torch.zeros_like(v), ids, mem2)
    for i, id_ in enumerate(IDS):
        want = mem2[id_].double() / mem2[id_].double().norm() if id_ >= 0 else torch.zeros(50, dtype=torch.float64)
        assert (r2["q"][i] - want).abs().max() < 1e-15


def test_alignment_scheme_equals_per_utterance_lstm():
    """len = 9, 4, 0, 1 of T = 9, two layers, fp64: the voiceprint and every weight gradient."""
    n, T, F, H, L = 4, 9, 23, 25, 2
    lens = torch.tensor([9, 4, 0, 1], dtype=torch.int32)
    x = ref.inputs(31, n, T, F)
    xc, l2, _ = ref.compact(x, ref.frame_mask(x, lengths=lens))
    assert torch.equal(l2, lens)
    torch.manual_seed(3)
    lstm = torch.nn.LSTM(F, H, L, batch_first=True, bidirectional=True).double()
    sd = {"spk.layer." + k: p.detach().clone() for k, p in lstm.named_parameters()}
    dvec = ref.inputs(32, n, 2 * H)
    vec, grads = ref.encoder_ref(xc, lens, sd, F, H, L, dvec)
    P = {k: p.clone().requires_grad_(True) for k, p in sd.items()}
    got = ref.aligned_encoder(xc, lens, P, L)
    assert (got[2] == 0).all()
    assert (got - vec).abs().max() < 1e-14
    (got * dvec.double()).sum().backward()
    for k, p in P.items():
        assert (p.grad - grads[k]).abs().max() <= 1e-13 * max(1.0, float(grads[k].abs().max())), k


def test_compact_and_shift_reference():
    x = ref.inputs(41, 3, 5, 4)
    x[0, 1] = 0
    x[1] = 0
    m = ref.frame_mask(x)
    xc, lens, idx = ref.compact(x, m)
    assert lens.tolist() == [4, 0, 5] and idx[0].tolist() == [0, 2, 3, 4, -1]
    assert torch.equal(xc[0, :4], x[0, [0, 2, 3, 4]]) and (xc[0, 4] == 0).all()
    assert ref.frame_mask(x, "gt", 0.0).sum() <= m.sum()
    s = ref.shift(xc, lens, 2, 4, +1, other=2)
    assert torch.equal(s[0, 1:, 2:], xc[0, :4, 2:]) and (s[0, 0, 2:] == 0).all()
    assert torch.equal(s[..., :2], xc[..., :2])
    back = ref.shift(s, lens, 2, 4, -1, other=1)
    assert torch.equal(back, xc)
