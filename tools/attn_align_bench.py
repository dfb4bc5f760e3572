"""Time the fused 'align' attention passes (dl4ss_mask_attn_align_loss COST / GRAD, attn_align.hip)
against the 'dot' passes (dl4ss_mask_attn_loss_ex, fp32 V, row-per-lane kernel) on the same buffers in
one process, at the C2 shape (B = 32, K = 2, T = 251, F = 129, E = 50, fp32 V), and a plain device
copy V -> dPre as the measured streaming ceiling for the same 414 MB.

Each launch is timed by its own pair of HIP events after a warm-up; the variants alternate inside
every repetition.  One JSON line: median and [min, max] per variant in microseconds, the align / dot
ratios, and the achieved fraction of the two floors of the GRAD pass (its FMAs at the fp32 vector
rate; V read + dPre written at the measured copy rate).

  python tools/attn_align_bench.py [reps] [B]
"""
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from dl4ss_amd import _lib  # noqa: E402

E = 50
FP32_VECTOR_FLOPS = 157.3e12  # MI355X fp32 vector (packed FMA) = fp32 MFMA peak


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    K, T, F = 2, 251, 129
    R = T * F
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1)
    k = 1.0 / E ** 0.5
    V = torch.tanh(torch.randn(B, R, E, generator=g)).to(dev)
    dPre = torch.empty_like(V)
    q = torch.randn(B, K, E, generator=g).to(dev)
    W1, W2 = (torch.empty(E, E).uniform_(-k, k, generator=g).to(dev) for _ in range(2))
    w3 = torch.empty(1, E).uniform_(-k, k, generator=g).to(dev)
    X = torch.rand(B, R, generator=g).to(dev)
    Y = torch.rand(B, K, R, generator=g).to(dev)
    perm = torch.tensor([[1, 0]] * B, dtype=torch.int32, device=dev)
    s1, s2 = 1.0 / (B * K * R), 0.5 / (B * R)
    st = _lib.stream_ptr()
    nb_a = _lib.query("dl4ss_attn_align_nblk", R)
    npart = _lib.query("dl4ss_attn_align_part_floats", B, K, nb_a)
    pl_a = torch.empty(B, nb_a, K * K + 1, device=dev)
    part = torch.empty(npart, device=dev)
    nb_d = _lib.query("dl4ss_attn_nblk", T, F)
    pl_d = torch.empty(B, nb_d, K * K + 1, device=dev)
    pdq = torch.empty(B, nb_d, K, E, device=dev)

    def align(pass_):
        _lib.call("dl4ss_mask_attn_align_loss", pass_, B, K, T, F, E, _lib.ptr(V), _lib.ptr(q), _lib.ptr(W1),
                  _lib.ptr(W2), _lib.ptr(w3), _lib.ptr(X), R, _lib.ptr(Y), K * R, R, _lib.ptr(perm), s1, s2,
                  _lib.ptr(dPre) if pass_ else None, _lib.ptr(pl_a), _lib.ptr(part) if pass_ else None, npart, None,
                  None, st)

    def dot(pass_):
        _lib.call("dl4ss_mask_attn_loss_ex", pass_, 0, B, K, T, F, E, _lib.ptr(V), _lib.ptr(q), _lib.ptr(X), R,
                  _lib.ptr(Y), K * R, R, _lib.ptr(perm), s1, s2, _lib.ptr(dPre) if pass_ else None, None, 0,
                  _lib.ptr(pl_d), _lib.ptr(pdq) if pass_ else None, None, None, st)

    variants = {"align_cost": lambda: align(0), "align_grad": lambda: align(1), "dot_cost": lambda: dot(0),
                "dot_grad": lambda: dot(1), "copy": lambda: dPre.copy_(V)}
    for _ in range(3):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(reps):
        for n, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3)
    out = {"shape": dict(B=B, K=K, T=T, F=F, E=E), "reps": reps}
    med = {}
    for n, ts in times.items():
        med[n] = statistics.median(ts)
        out[n + "_us"] = {"median": round(med[n], 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}
    rows = B * R
    # FMAs per row of the GRAD pass: U, dV and the dW1 outer-product sum (3 E^2) + the K tanh / logit /
    # dS columns (~4 K E); 2 FLOP each
    flop = 2.0 * rows * (3 * E * E + 4 * K * E)
    nbytes = 2.0 * rows * E * 4
    copy_rate = nbytes / (med["copy"] * 1e-6)
    out["grad_ratio_align_over_dot"] = round(med["align_grad"] / med["dot_grad"], 2)
    out["cost_ratio_align_over_dot"] = round(med["align_cost"] / med["dot_cost"], 2)
    out["grad_gflop"] = round(flop / 1e9, 2)
    out["grad_tflops"] = round(flop / (med["align_grad"] * 1e-6) / 1e12, 1)
    out["grad_frac_of_fp32_vector_floor"] = round(flop / FP32_VECTOR_FLOPS / (med["align_grad"] * 1e-6), 3)
    out["copy_TB_s"] = round(copy_rate / 1e12, 2)
    out["grad_frac_of_stream_floor"] = round(med["copy"] / med["align_grad"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
