"""Variant-library check of the fused attention + loss kernels: every entry point of attn_loss.hip and
attn_align.hip on fixed-seed inputs with the library named by DL4SS_LIB (default: the shipped one); writes SHA-256
digests of everything each call writes to argv[1] (JSON).  `--compare a b` reports whether two such records are
bitwise equal, and which entries are not.

  DL4SS_LIB=dl4ss_amd/libdl4ss_hip_parent.so python tools/attn_bitwise.py parent.json
  python tools/attn_bitwise.py new.json && python tools/attn_bitwise.py --compare parent.json new.json

Covered, at (B, T, F, ld_pad) = (3, 7, 129, 6) and (2, 33, 129, 2), K = 1, 2, 3:
  dl4ss_mask_attn_loss_ex / _bf16v        magnitude and cRM; COST, dl4ss_pit_select, GRAD; fp32 / bf16 V x fp32 / bf16 dPre
  dl4ss_mask_attn_loss_adv / _adv_bf16v   the same four I/O forms
  dl4ss_mask_attn_align_loss / _ex        fp32 V + fp32 dPre (both entry points), fp32 V + bf16 dPre, bf16 V + bf16 dPre
  dl4ss_attn_align_fwd / _bwd             K = 1
each followed by dl4ss_loss_finalize / dl4ss_attn_align_finalize.  Digested: part_loss (after each pass), part_dq or
the 'align' partial records, dPre with its row padding, mask_out, pred_out, perm, the loss triple, dq, dW1, dW2, dw3.
Every output buffer is prefilled, so what a call leaves unwritten is compared too."""
import hashlib
import json
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])

E = 50
SHAPES = [(3, 7, 129, 6), (2, 33, 129, 2)]


def run(out):
    from dl4ss_amd import _lib

    dev = torch.device("cuda")
    P, st = _lib.ptr, _lib.stream_ptr()
    rec = {}

    def put(tag, **tensors):
        torch.cuda.synchronize()
        for n, t in tensors.items():
            if t is not None:
                rec[f"{tag}/{n}"] = hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()

    def filled(shape, bf16=False):
        t = torch.full(shape, float("nan"), device=dev)
        return t.to(torch.bfloat16) if bf16 else t

    for B, T, F, ld_pad in SHAPES:
        R, ldpb = T * F, F * E + ld_pad
        for K in (1, 2, 3):
            g = torch.Generator(device="cpu").manual_seed(100 * K + T)
            V = torch.tanh(torch.randn(B, R, E, generator=g)).to(dev)
            Vs = {"fp32": V, "bf16": V.to(torch.bfloat16)}
            rperm = torch.stack([torch.randperm(K, generator=g) for _ in range(B)]).to(torch.int32).to(dev)
            s1 = 1.0 / (B * K * R)
            # ---- 'dot': dl4ss_mask_attn_loss_ex / _bf16v / _adv / _adv_bf16v
            nblk = _lib.query("dl4ss_attn_nblk", T, F)
            for crm in (0, 1):
                QW, NC = (2 * E, 2) if crm else (E, 1)
                s2 = 0.0 if crm else 0.5 / (B * R)
                q = ((0.05 if crm else 0.3) * torch.randn(B, K, QW, generator=g)).to(dev)
                X = torch.rand(B, R * NC, generator=g).to(dev)
                Y = torch.rand(B, K, R * NC, generator=g).to(dev)
                gext = (8.0 * s1 * torch.randn(B, K, R, generator=g)).to(dev)
                for vt, Vd in Vs.items():
                    sfx = "_bf16v" if vt == "bf16" else ""
                    for dp in ("fp32", "bf16"):
                        for adv in ((False, True) if not crm else (False,)):
                            tag = f"dot{'_adv' if adv else ''}/{(B, T, F)}/K{K}/crm{crm}/V{vt}/dPre{dp}"
                            bf = dp == "bf16"
                            dpre = None if bf else filled((B, R, E))
                            dpreb = filled((B * T, ldpb), True) if bf else None
                            pl, pdq = filled((B, nblk, K * K + 1)), filled((B, nblk, K, QW))
                            perm = rperm.clone()
                            head = (B, K, T, F, E, P(Vd), P(q), P(X), R, P(Y), K * R, R)
                            io = (P(dpreb), ldpb if bf else 0, P(pl))
                            if adv:
                                _lib.call("dl4ss_mask_attn_loss_adv" + sfx, *head, P(perm), s1, s2, P(gext), P(dpre), *io,
                                          P(pdq), None, None, st)
                            else:
                                mask, pred = filled((B, K, R * NC)), filled((B, K, R * NC))
                                _lib.call("dl4ss_mask_attn_loss" + (sfx or "_ex"), 0, crm, *head, None, s1, s2, None, *io,
                                          None, P(mask), P(pred), st)
                                _lib.call("dl4ss_pit_select", P(pl), B, K, nblk, P(perm), st)
                                put(tag, part_loss_cost=pl, mask=mask, pred=pred, perm=perm)
                                _lib.call("dl4ss_mask_attn_loss" + (sfx or "_ex"), 1, crm, *head, P(perm), s1, s2, P(dpre),
                                          *io, P(pdq), None, None, st)
                            loss, dq = filled((3,)), filled((B, K, QW))
                            _lib.call("dl4ss_loss_finalize", P(pl), B, K, nblk, P(perm), s1, s2, P(loss), P(pdq), QW,
                                      P(dq), st)
                            put(tag, part_loss=pl, part_dq=pdq, dpre=dpre, dpre_bf16=dpreb, loss=loss, dq=dq)
            # ---- 'align': dl4ss_mask_attn_align_loss / _ex, dl4ss_attn_align_finalize
            k = 1.0 / E ** 0.5
            q = torch.randn(B, K, E, generator=g).to(dev)
            W1, W2 = (torch.empty(E, E).uniform_(-k, k, generator=g).to(dev) for _ in range(2))
            w3 = torch.empty(1, E).uniform_(-k, k, generator=g).to(dev)
            X = torch.rand(B, R, generator=g).to(dev)
            Y = torch.rand(B, K, R, generator=g).to(dev)
            s2 = 0.5 / (B * R)
            nba = _lib.query("dl4ss_attn_align_nblk", R)
            npart = _lib.query("dl4ss_attn_align_part_floats", B, K, nba)
            for form, vt, dp in (("old", "fp32", "fp32"), ("ex", "fp32", "fp32"), ("ex", "fp32", "bf16"),
                                 ("ex", "bf16", "bf16")):
                tag = f"align_{form}/{(B, T, F)}/K{K}/V{vt}/dPre{dp}"
                bf = dp == "bf16"
                dpre = None if bf else filled((B, R, E))
                dpreb = filled((B * T, ldpb), True) if bf else None
                pl, part = filled((B, nba, K * K + 1)), torch.zeros(npart, device=dev)
                mask, pred = filled((B, K, R)), filled((B, K, R))
                perm = rperm.clone()
                for pass_ in (0, 1):
                    Vp = ((P(Vs["fp32"]),) if form == "old" else
                          (P(Vs["fp32"]) if vt == "fp32" else None, P(Vs["bf16"]) if vt == "bf16" else None))
                    dpp = (P(dpre) if pass_ else None,) + ((P(dpreb), ldpb if bf else 0) if form == "ex" else ())
                    _lib.call("dl4ss_mask_attn_align_loss" + ("_ex" if form == "ex" else ""), pass_, B, K, T, F, E, *Vp,
                              P(q), P(W1), P(W2), P(w3), P(X), R, P(Y), K * R, R, P(perm) if pass_ else None, s1, s2,
                              *dpp, P(pl), P(part) if pass_ else None, npart, None if pass_ else P(mask),
                              None if pass_ else P(pred), st)
                    if pass_ == 0:
                        _lib.call("dl4ss_pit_select", P(pl), B, K, nba, P(perm), st)
                        put(tag, part_loss_cost=pl, mask=mask, pred=pred, perm=perm)
                loss = filled((3,))
                dq, dW1, dW2, dw3 = filled((B, K, E)), filled((E, E)), filled((E, E)), filled((E,))
                _lib.call("dl4ss_loss_finalize", P(pl), B, K, nba, P(perm), s1, s2, P(loss), None, E, None, st)
                _lib.call("dl4ss_attn_align_finalize", P(part), npart, B, K, T, F, P(q), P(W2), P(dq), P(dW1), P(dW2),
                          P(dw3), st)
                put(tag, part_loss=pl, part=part, dpre=dpre, dpre_bf16=dpreb, loss=loss, dq=dq, dW1=dW1, dW2=dW2, dw3=dw3)
            # ---- the module-level forward / backward (one query per utterance)
            if K == 1:
                tag = f"align_module/{(B, T, F)}"
                mask = filled((B, R))
                _lib.call("dl4ss_attn_align_fwd", P(V), P(q), E, P(W1), P(W2), P(w3), B, R, E, P(mask), R, st)
                dmask = torch.randn(B, R, generator=g).to(dev)
                dV, part = torch.zeros(B, R, E, device=dev), torch.zeros(npart, device=dev)
                dq, dW1, dW2, dw3 = filled((B, E)), filled((E, E)), filled((E, E)), filled((E,))
                _lib.call("dl4ss_attn_align_bwd", P(V), P(q), E, P(W1), P(W2), P(w3), P(dmask), B, R, E, P(dV), P(part),
                          npart, P(dq), P(dW1), P(dW2), P(dw3), st)
                put(tag, mask=mask, dV=dV, part=part, dq=dq, dW1=dW1, dW2=dW2, dw3=dw3)
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
    print(f"{len(rec)} digests -> {out}")


def compare(a, b):
    x, y = json.load(open(a)), json.load(open(b))
    diff = sorted(k for k in set(x) | set(y) if x.get(k) != y.get(k))
    n = len(set(x) | set(y))
    print(f"bitwise equal: all {n} digests" if not diff else f"DIFFERENT: {len(diff)} of {n}", *diff)
    return not diff


if __name__ == "__main__":
    if len(sys.argv) not in (2, 4) or (len(sys.argv) == 4) != (sys.argv[1] == "--compare"):
        sys.exit("usage: attn_bitwise.py OUT.json | attn_bitwise.py --compare A.json B.json")
    if sys.argv[1] == "--compare":
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    run(sys.argv[1])
