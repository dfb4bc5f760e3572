"""torch.autograd.Functions over the HIP kernels, for the reference-API modules
(``dl4ss_amd.compat.myNet``): a driver that composes MIX_SPEECH / ATTENTION /
SPEECH_EMBEDDING / ADDJUST with torch autograd (as the reference's ``main_run_*``
scripts do) runs the recurrence, the GEMMs, the attention and the query gather
on the gfx950 kernels.  The fused single-call training step is
``dl4ss_amd.engine.SepTrainer``; these Functions are the modular path.

Every tensor reaching a kernel must be a contiguous fp32 CUDA tensor (``_lib.ptr``
enforces it); there is no CPU fallback.
"""
import ctypes

import torch

from . import _lib, ops
from .ops import CELLS


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _check_status(status, what):
    s = int(status.item())
    if s != 0:
        raise RuntimeError(f"{what}: BiRNN hand-off timed out (status {s})")


def birnn_fwd_impl(x, w_ih, b_ih, w_hh, b_hh, cell, H, precision, gates="logistic"):
    """One bidirectional layer's forward: (out (B,T,2H), hprev, act, cs or None).  Shared by
    BiRNNLayerFn and the dl4ss::birnn_layer / dl4ss::keras_lstm_layer custom ops (dl4ss_amd.library).
    gates "hard": Keras 1's LSTM cell (ops.HARD_GATES; fp32 LSTM only)."""
    flags = ops.gate_flags(gates, cell, precision)
    x = _c(x)
    B, T, D = x.shape
    cid = CELLS[cell]
    dev = x.device
    G = ops.gemm(x.view(B * T, D), _c(w_ih), transB=True, bias=_c(b_ih), precision=precision)
    out = torch.empty(B, T, 2 * H, device=dev)
    hprev = torch.empty_like(out)
    act = torch.empty(B, T, 2, 4 * H, device=dev)
    cs = torch.empty(B, T, 2, H, device=dev) if cell == "lstm" else None
    wsn = _birnn_ws_bytes(cid, B, H)
    ws = torch.empty((wsn + 7) // 8, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.birnn_fwd(cell, B, T, H, G=G, w_hh=_c(w_hh), b_hh=_c(b_hh), out=out, hprev=hprev, act=act, cs=cs, ws=ws,
                  ws_bytes=wsn, status=status, precision=precision, flags=flags)
    _check_status(status, "dl4ss_birnn_fwd")
    return out, hprev, act, cs


def _birnn_ws_bytes(cid, B, H):
    wsn = _lib.query("dl4ss_birnn_workspace_bytes", cid, B, H)
    if wsn < 0:
        raise RuntimeError(f"BiRNN shape unsupported (B={B}, H={H})")
    return wsn


def birnn_bwd_impl(dout, x, w_ih, w_hh, hprev, act, cs, cell, H, precision, need_dx=True, gates="logistic"):
    """BPTT + the layer's weight / bias / input gradients: (dx or None, dw_ih, db_ih, dw_hh, db_hh).
    gates: as birnn_fwd_impl (act must come from a forward of the same setting)."""
    flags = ops.gate_flags(gates, cell, precision)
    B, T, D = x.shape
    dev = x.device
    NGH = (4 if cell == "lstm" else 3) * H
    wsn = _birnn_ws_bytes(CELLS[cell], B, H)
    dout = _c(dout.float())
    dG = torch.empty(B * T, 2 * NGH, device=dev)
    dGh = torch.empty_like(dG) if cell == "gru" else None
    ws = torch.empty((wsn + 7) // 8, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    # (one entry point for every H: the H = 600 classifier runs its large-hidden BPTT, the generic kernel)
    ops.birnn_bwd(cell, B, T, H, dOut=dout, w_hh=_c(w_hh), act=act, cs=cs if cell == "lstm" else None, hprev=hprev,
                  dG=dG, dGh=dGh, ws=ws, ws_bytes=wsn, status=status, precision=precision, flags=flags)
    _check_status(status, "dl4ss_birnn_bwd")
    dGh = dG if dGh is None else dGh
    w_ih = _c(w_ih)
    x2 = _c(x).view(B * T, D)
    dx = ops.gemm(dG, w_ih, precision=precision).view(B, T, D) if need_dx else None
    dw_ih = torch.zeros_like(w_ih)
    ops.gemm(dG, x2, transA=True, out=dw_ih, beta=1.0, splitk="auto", precision=precision)
    db_ih = torch.zeros(2 * NGH, device=dev)
    ops.colsum(dG, db_ih)
    dw_hh = torch.zeros_like(w_hh)
    hp = hprev.view(B * T, 2 * H)
    for d in range(2):
        ops.gemm(dGh[:, d * NGH:(d + 1) * NGH], hp[:, d * H:(d + 1) * H], transA=True,
                 out=dw_hh[d * NGH:(d + 1) * NGH], beta=1.0, splitk="auto", precision=precision)
    db_hh = torch.zeros(2 * NGH, device=dev)
    ops.colsum(dGh, db_hh)
    return dx, dw_ih, db_ih, dw_hh, db_hh


class BiRNNLayerFn(torch.autograd.Function):
    """One bidirectional LSTM/GRU layer (torch gate order / two-bias semantics).

    x (B,T,D); w_ih (2*G*H, D), b_ih (2*G*H), w_hh (2*G*H, H), b_hh (2*G*H) with the
    forward direction's rows first (G = 4 LSTM / 3 GRU)  ->  out (B,T,2H) = [fwd | rev].
    Replaces one layer of nn.LSTM / nn.GRU(batch_first, bidirectional)
    (TDAA_beta/main_run_sstune_EvalVer.py:282-293, Torch_multi/main_run.py:263-273).
    gates "hard": Keras 1's LSTM cell instead (hard_sigmoid i / f / o gates; one layer of
    Bidirectional(LSTM(...)) at DL4SS_Keras/nnet.py:51-68), fp32 LSTM only.
    """

    @staticmethod
    def forward(ctx, x, w_ih, b_ih, w_hh, b_hh, cell, H, precision, *gates):  # gates: optional, "logistic"
        if len(gates) > 1:
            raise TypeError("BiRNNLayerFn.apply(x, w_ih, b_ih, w_hh, b_hh, cell, H, precision[, gates])")
        g = gates[0] if gates else "logistic"
        out, hprev, act, cs = birnn_fwd_impl(x, w_ih, b_ih, w_hh, b_hh, cell, H, precision, g)
        ctx.save_for_backward(_c(x), _c(w_ih), _c(w_hh), hprev, act, cs if cs is not None else act)
        ctx.meta = (cell, H, precision, g)
        ctx.n_opt = len(gates)  # backward returns one gradient per argument apply() was given
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w_ih, w_hh, hprev, act, cs = ctx.saved_tensors
        cell, H, precision, gates = ctx.meta
        dx, dw_ih, db_ih, dw_hh, db_hh = birnn_bwd_impl(dout, x, w_ih, w_hh, hprev, act,
                                                        cs if cell == "lstm" else None, cell, H, precision,
                                                        bool(ctx.needs_input_grad[0]), gates)
        return (dx, dw_ih, db_ih, dw_hh, db_hh, None, None, None) + (None,) * ctx.n_opt


def linear_tanh_bwd_impl(dv, x2d, w, v, precision, need_dx=True):
    """(dx or None, dW, db) of V = tanh(x W^T + b), from the saved V."""
    dv = _c(dv.float())
    dpre = torch.empty_like(v)
    _lib.call("dl4ss_tanh_bwd", _lib.ptr(v), _lib.ptr(dv), _lib.ptr(dpre), v.numel(), _lib.stream_ptr())
    dw = torch.zeros_like(w)
    ops.gemm(dpre, x2d, transA=True, out=dw, beta=1.0, splitk="auto", precision=precision)
    db = torch.zeros(w.shape[0], device=w.device)
    ops.colsum(dpre, db)
    dx = ops.gemm(dpre, w, precision=precision) if need_dx else None
    return dx, dw, db


class LinearTanhFn(torch.autograd.Function):
    """V = tanh(x W^T + b), the MIX_SPEECH output head (EvalVer.py:290,298-299)."""

    @staticmethod
    def forward(ctx, x2d, w, b, precision):
        x2d, w = _c(x2d), _c(w)
        v = ops.gemm(x2d, w, transB=True, bias=_c(b), epilogue=ops.EPI_TANH, precision=precision)
        ctx.save_for_backward(x2d, w, v)
        ctx.precision = precision
        return v

    @staticmethod
    def backward(ctx, dv):
        x2d, w, v = ctx.saved_tensors
        dx, dw, db = linear_tanh_bwd_impl(dv, x2d, w, v, ctx.precision, bool(ctx.needs_input_grad[0]))
        return dx, dw, db, None


class LinearFn(torch.autograd.Function):
    """y = x W^T (+ b) on the GEMM kernel (ADDJUST's bias-free Linear, EvalVer.py:366;
    the classifier head)."""

    @staticmethod
    def forward(ctx, x2d, w, b, precision):
        x2d, w = _c(x2d.float()), _c(w)
        y = ops.gemm(x2d, w, transB=True, bias=_c(b) if b is not None else None, precision=precision)
        ctx.save_for_backward(x2d, w)
        ctx.precision, ctx.has_b = precision, b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x2d, w = ctx.saved_tensors
        dy = _c(dy.float())
        dw = ops.gemm(dy, x2d, transA=True, precision=ctx.precision)
        db = None
        if ctx.has_b:
            db = torch.zeros(w.shape[0], device=w.device)
            ops.colsum(dy, db)
        dx = ops.gemm(dy, w, precision=ctx.precision) if ctx.needs_input_grad[0] else None
        return dx, dw, db, None


def attention_dot_fwd_impl(V, q, crm):
    """mask (Bq,R) = sigmoid(V . q), or (Bq,R,2) = 10 tanh(V . q_half) for the cRM branch."""
    return torch.stack(_attention_dot_masks(V, q, crm), dim=-1) if crm else _attention_dot_masks(V, q, crm)[0]


def _attention_dot_masks(V, q, crm):
    V, q = _c(V.float()), _c(q.float())
    Bq, R, E = V.shape
    st = _lib.stream_ptr()
    masks = []
    for h in range(2 if crm else 1):
        m = torch.empty(Bq, R, device=V.device)
        _lib.call("dl4ss_attn_dot_fwd", _lib.ptr(V), ctypes.c_void_p(q.data_ptr() + 4 * h * E), q.shape[1], Bq, R,
                  E, int(crm), _lib.ptr(m), st)
        masks.append(m)
    return masks


def attention_dot_bwd_impl(dmask, V, q, masks, crm, need_dV=True):
    """(dV or None, dq) from the per-half masks of the forward."""
    V, q = _c(V.float()), _c(q.float())
    Bq, R, E = V.shape
    st = _lib.stream_ptr()
    dV = torch.zeros_like(V) if need_dV else None
    nblk = _lib.query("dl4ss_attn_dot_nblk", R)
    part = torch.empty(Bq * nblk * E, device=V.device)
    dq = torch.zeros_like(q)
    dqh = torch.empty(Bq, E, device=V.device)
    for h, m in enumerate(masks):
        dm = _c(dmask[..., h].float()) if crm else _c(dmask.float())
        _lib.call("dl4ss_attn_dot_bwd", V=_lib.ptr(V), q=ctypes.c_void_p(q.data_ptr() + 4 * h * E), q_stride=q.shape[1],
                  mask=_lib.ptr(m), dmask=_lib.ptr(dm), Bq=Bq, R=R, E=E, act=int(crm),
                  dV=_lib.ptr(dV) if dV is not None else None, part_dq=_lib.ptr(part), dq=_lib.ptr(dqh), stream=st)
        dq[:, h * E:(h + 1) * E] = dqh
    return dV, dq


class AttentionDotFn(torch.autograd.Function):
    """ATTENTION 'dot' (EvalVer.py:216-226): mask (Bq,R) = sigmoid(V (Bq,R,E) . q (Bq,E));
    crm=True: the cRM branch (cRM_EvalVer.py:259-271), q (Bq,2E) split in halves,
    mask (Bq,R,2) = 10 tanh(V . q_half)."""

    @staticmethod
    def forward(ctx, V, q, crm):
        V, q = _c(V.float()), _c(q.float())
        masks = _attention_dot_masks(V, q, crm)
        ctx.save_for_backward(V, q, *masks)
        ctx.crm = crm
        return torch.stack(masks, dim=-1) if crm else masks[0]

    @staticmethod
    def backward(ctx, dmask):
        V, q, *masks = ctx.saved_tensors
        dV, dq = attention_dot_bwd_impl(dmask, V, q, masks, ctx.crm, bool(ctx.needs_input_grad[0]))
        return dV, dq, None


def attention_align_fwd_impl(V, q, W1, W2, w3):
    """mask (Bq,R) = sigmoid(w3 . tanh(W1 V + W2 q)): V (Bq,R,E), q (Bq,E), W1 / W2 (E,E), w3 (1,E)."""
    V, q, W1, W2, w3 = (_c(t.float()) for t in (V, q, W1, W2, w3))
    Bq, R, E = V.shape
    m = torch.empty(Bq, R, device=V.device)
    _lib.call("dl4ss_attn_align_fwd", V=_lib.ptr(V), q=_lib.ptr(q), q_stride=q.shape[1], W1=_lib.ptr(W1),
              W2=_lib.ptr(W2), w3=_lib.ptr(w3), Bq=Bq, R=R, E=E, mask=_lib.ptr(m), mask_stride=R,
              stream=_lib.stream_ptr())
    return m


def attention_align_bwd_impl(dmask, V, q, W1, W2, w3, need_dV=True):
    """(dV or None, dq, dW1, dW2, dw3) from dmask; s and the mask are recomputed from V."""
    V, q, W1, W2, w3 = (_c(t.float()) for t in (V, q, W1, W2, w3))
    dmask = _c(dmask.float())
    Bq, R, E = V.shape
    dev = V.device
    dq, dW1, dW2, dw3 = torch.empty_like(q), torch.empty_like(W1), torch.empty_like(W2), torch.empty_like(w3)
    if Bq == 0 or R == 0:
        return (torch.zeros_like(V) if need_dV else None), dq.zero_(), dW1.zero_(), dW2.zero_(), dw3.zero_()
    dV = torch.zeros_like(V) if need_dV else None
    n = _lib.query("dl4ss_attn_align_part_floats", Bq, 1, _lib.query("dl4ss_attn_align_nblk", R))
    part = torch.empty(n, device=dev)
    _lib.call("dl4ss_attn_align_bwd", V=_lib.ptr(V), q=_lib.ptr(q), q_stride=q.shape[1], W1=_lib.ptr(W1),
              W2=_lib.ptr(W2), w3=_lib.ptr(w3), dmask=_lib.ptr(dmask), Bq=Bq, R=R, E=E, dV=_lib.ptr(dV),
              part=_lib.ptr(part), part_floats=n, dq=_lib.ptr(dq), dW1=_lib.ptr(dW1), dW2=_lib.ptr(dW2),
              dw3=_lib.ptr(dw3), stream=_lib.stream_ptr())
    return dV, dq, dW1, dW2, dw3


class AttentionAlignFn(torch.autograd.Function):
    """ATTENTION 'align' (EvalVer.py:228-239; DL4SS_Keras/extend_layers.py:50-64): mask (Bq,R) =
    sigmoid(Linear_3(tanh(Linear_1(V) + Linear_2(q)))), V (Bq,R,E), q (Bq,E), the three bias-free
    Linear weights W1 (E,E), W2 (E,E), w3 (1,E)."""

    @staticmethod
    def forward(ctx, V, q, W1, W2, w3):
        V, q, W1, W2, w3 = (_c(t.float()) for t in (V, q, W1, W2, w3))
        ctx.save_for_backward(V, q, W1, W2, w3)
        return attention_align_fwd_impl(V, q, W1, W2, w3)

    @staticmethod
    def backward(ctx, dmask):
        V, q, W1, W2, w3 = ctx.saved_tensors
        need = ctx.needs_input_grad
        dV, dq, dW1, dW2, dw3 = attention_align_bwd_impl(dmask, V, q, W1, W2, w3, bool(need[0]))
        return (dV, dq if need[1] else None, dW1 if need[2] else None, dW2 if need[3] else None,
                dw3 if need[4] else None)


class EmbeddingGatherFn(torch.autograd.Function):
    """q (B,K,W) = Emb[idx]: SPEECH_EMBEDDING gather (EvalVer.py:355-360)."""

    @staticmethod
    def forward(ctx, emb, idx):
        emb = _c(emb)
        idx = _c(idx.to(torch.int32))
        B, K = idx.shape
        W = emb.shape[1]
        q = torch.empty(B, K, W, device=emb.device)
        # query kernel without ADJUST: a pure gather (h / mean unused)
        _lib.call("dl4ss_query_fwd", h=_lib.ptr(emb), B=B, T=1, D=1, idx=_lib.ptr(idx), emb=_lib.ptr(emb), w_adj=None,
                  K=K, W=W, q=_lib.ptr(q), mean_out=None, stream=_lib.stream_ptr())
        ctx.save_for_backward(idx)
        ctx.shape = emb.shape
        return q

    @staticmethod
    def backward(ctx, dq):
        (idx,) = ctx.saved_tensors
        B, K = idx.shape
        n, W = ctx.shape
        demb = torch.zeros(n, W, device=dq.device)
        dq = _c(dq.float())
        _lib.call("dl4ss_query_bwd", dq=_lib.ptr(dq), B=B, T=1, D=1, idx=_lib.ptr(idx), emb=None, w_adj=None, mean=None,
                  K=K, W=W, d_emb=_lib.ptr(demb), d_wadj=None, dh_bcast=None, stream=_lib.stream_ptr())
        return demb, None


def top_k_mask_device(prob, alpha, top_k):
    """(mask (B,N) float, idx (B,top_k) int32 ascending, -1 padded, count (B,) int32) on device."""
    prob = _c(prob.float())
    B, N = prob.shape
    mask = torch.empty(B, N, device=prob.device)
    idx = torch.empty(B, max(top_k, 1), dtype=torch.int32, device=prob.device)
    cnt = torch.empty(B, dtype=torch.int32, device=prob.device)
    _lib.call("dl4ss_top_k_mask", _lib.ptr(prob), B, N, float(alpha), int(top_k), _lib.ptr(mask), _lib.ptr(idx),
              _lib.ptr(cnt), _lib.stream_ptr())
    return mask, idx[:, :top_k], cnt


# --------------------------------------------------------------------------- Discriminator
def disc_dims(T, F):
    """(features, [H1, W1, H2, W2, H3, W3]) of a (T, F) map through the three stride-2 3x3 'valid' convs
    (host only); raises for a map smaller than 15 x 15."""
    hw = (ctypes.c_int * 6)()
    feat = _lib.query("dl4ss_disc_dims", int(T), int(F), hw)
    if feat < 0:
        raise RuntimeError(f"Discriminator: a ({T}, {F}) map is smaller than the 15 x 15 minimum")
    return feat, list(hw)


def _disc_act_dtype(precision):
    return torch.bfloat16 if ops.PREC[precision] == 1 else torch.float32


def disc_fwd_impl(spec, w1, b1, w2, b2, w3, b3, wf, bf, precision):
    """spec (N, T, F) -> (score (N, 1), y1, y2, y3): the saved post-ReLU activations are channels-last
    (N, H, W, 64), fp32 or (precision 'bf16') bfloat16.  Shared by DiscriminatorFn and dl4ss::discriminator."""
    spec = _c(spec.float())
    N, T, F = spec.shape
    feat, hw = disc_dims(T, F)
    if wf.numel() != feat:
        raise RuntimeError(f"Discriminator: final.weight has {wf.numel()} features, a ({T}, {F}) map gives {feat}")
    dt, dev = _disc_act_dtype(precision), spec.device
    ys = [torch.empty(N, hw[2 * l], hw[2 * l + 1], 64, dtype=dt, device=dev) for l in range(3)]
    score = torch.empty(N, 1, device=dev)
    ops.disc_forward(ops.PREC[precision], spec, [_c(p) for p in (w1, b1, w2, b2, w3, b3, wf, bf)], ys,
                     torch.empty(N, device=dev), score)
    return (score, *ys)


def disc_bwd_impl(dscore, spec, w1, w2, w3, wf, score, y1, y2, y3, precision, need_dx=True, target=None):
    """(dspec or None, dw1, db1, dw2, db2, dw3, db3, dwf, dbf) from dscore (N, 1).  With ``dscore`` None the
    head fuses the loss mean_n (score_n - target)^2 (target 1 or 0) and its scalar is appended to the result."""
    spec = _c(spec.float())
    N, T, F = spec.shape
    disc_dims(T, F)
    dev = spec.device
    w1, w2, w3, wf = _c(w1), _c(w2), _c(w3), _c(wf)
    wsn = _lib.query("dl4ss_disc_ws_bytes", N, T, F)
    if wsn < 0:
        raise RuntimeError(f"Discriminator shape unsupported (N={N}, T={T}, F={F})")
    ws = torch.empty((wsn + 3) // 4, device=dev)
    dz = torch.empty(N, device=dev)
    grads = [torch.empty_like(w) if b is None else torch.empty(b, device=dev)  # dw1, db1, ..., dwf, dbf
             for w, n in ((w1, 64), (w2, 64), (w3, 64), (wf, 1)) for b in (None, n)]
    loss = torch.empty(1, device=dev) if dscore is None else None
    dx = torch.empty_like(spec) if need_dx else None
    ops.disc_backward(ops.PREC[precision], spec, (w1, w2, w3, wf), (y1, y2, y3),
                      [torch.empty_like(y) for y in (y1, y2, y3)], _c(score),
                      _c(dscore.float()) if dscore is not None else None, target if target is not None else 0.0, loss,
                      dz, grads, dx, ws, wsn)
    return (dx, *grads) if dscore is not None else (dx, *grads, loss[0])


class DiscriminatorFn(torch.autograd.Function):
    """The reference's Discriminator (TDAA_beta/main_run_sstune_dis.py:318-336): three Conv2d(., 64, 3x3,
    stride 2) + ReLU on spec (N, T, F), Linear(64 H3 W3, 1) + sigmoid -> score (N, 1).  Parameters in the
    reference's layouts: cnn*.weight (64, Cin, 3, 3), final.weight (1, 64 H3 W3) in (c, h, w) order.  The input
    gradient (the generator's adversarial gradient) is computed only when spec requires it."""

    @staticmethod
    def forward(ctx, spec, w1, b1, w2, b2, w3, b3, wf, bf, precision):
        spec = _c(spec.float())
        score, y1, y2, y3 = disc_fwd_impl(spec, w1, b1, w2, b2, w3, b3, wf, bf, precision)
        ctx.save_for_backward(spec, _c(w1), _c(w2), _c(w3), _c(wf), score, y1, y2, y3)
        ctx.precision = precision
        return score

    @staticmethod
    def backward(ctx, dscore):
        spec, w1, w2, w3, wf, score, y1, y2, y3 = ctx.saved_tensors
        dx, dw1, db1, dw2, db2, dw3, db3, dwf, dbf = disc_bwd_impl(dscore, spec, w1, w2, w3, wf, score, y1, y2, y3,
                                                                   ctx.precision, bool(ctx.needs_input_grad[0]))
        return dx, dw1, db1, dw2, db2, dw3, db3, dwf.view_as(wf), dbf, None


# --------------------------------------------------------------------------- voiceprint encoder
class VoiceprintFn(torch.autograd.Function):
    """vec (n, E) = the masked voiceprint encoder of a VoiceprintNet over feats (n, T, F) (DL4SS_Keras/nnet.py:64-80:
    Masking, the BiLSTM, MeanPool); differentiable in the net's flat parameter buffer (the gradient has its
    layout).  lengths (n) int32 or None; rule / thr as ops.vp_compact."""

    @staticmethod
    def forward(ctx, feats, flat, vnet, lengths, rule, thr):
        from .voiceprint import VoiceprintEncoder

        if flat.data_ptr() != vnet.flat.data_ptr():
            raise RuntimeError("VoiceprintFn: flat must be vnet.flat")
        n, T, _ = feats.shape
        enc = VoiceprintEncoder(vnet, n, T)
        vec = enc.forward(_c(feats.float()), rule, thr, lengths).clone()
        _check_status(enc.status[:1], "voiceprint forward")
        ctx.enc = enc
        return vec

    @staticmethod
    def backward(ctx, dvec):
        enc = ctx.enc
        keep, enc.net.grad = enc.net.grad, torch.zeros_like(enc.net.flat)
        try:
            g = enc.backward(_c(dvec.float()))
        finally:
            enc.net.grad = keep
        _check_status(enc.status[:1], "voiceprint backward")
        return None, g, None, None, None, None


def voiceprint(feats, vnet, lengths=None, rule="nonzero", thr=None, flat=None):
    """The voiceprints of feats (n, T, F) under autograd; ``flat``: vnet.flat as a leaf that requires grad."""
    return VoiceprintFn.apply(feats, vnet.flat if flat is None else flat, vnet, lengths, rule, thr)
