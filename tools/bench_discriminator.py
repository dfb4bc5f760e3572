"""Time the Discriminator kernels (disc.hip) at the reference size (N, T, F) = (64, 313, 129) -- B = 16, K = 2,
32 true + 32 fake maps -- in both precisions, and ``torch.nn.functional.conv2d`` (the vendor-library path the
reference takes) on the same GPU in the same dtype.

Per precision: every C-ABI launch of the forward and of the backward timed by its own pair of HIP events
after a warm-up, the whole forward and forward + backward the same way, and the library model (three
conv2d + relu, matmul + sigmoid; autograd backward; the default NCHW call, not tuned further) likewise; the
variants alternate inside every repetition.  One JSON line per case (median and [min, max] in microseconds)
is written to the output file, which every run rewrites.  A per-launch figure is one launch between two
events and includes the host's enqueue gap.  The conv2 line carries its FLOPs (2 M 64 576, from the shapes)
and the achieved fraction of the MFMA peak of its precision.
A library path that cannot run is recorded as such, with the error, not skipped silently.

  python tools/bench_discriminator.py [--reps R] [--n N] [--out profiles/dis_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from dl4ss_amd import _lib, autograd as ag, ops  # noqa: E402

PEAK = {"fp32": 157.3e12, "bf16": 2.5e15}  # MFMA peaks: v_mfma_f32_32x32x2_f32, v_mfma_f32_32x32x16_bf16


def timed(fns, reps, warmup=3):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[n].append(e0.elapsed_time(e1) * 1e3)
    return {n: {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
            for n, t in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--out", default="profiles/dis_bench.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_discriminator: no GPU (a timing needs the device; there is no fallback)")
    N, T, F = a.n, 313, 129
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1)
    feat, hw = ag.disc_dims(T, F)
    u = lambda shape, fan: ((torch.rand(shape, generator=g) * 2 - 1) * fan ** -0.5).to(dev)  # noqa: E731
    w1, b1, w2, b2, w3, b3 = u((64, 1, 3, 3), 9), u((64,), 9), u((64, 64, 3, 3), 576), u((64,), 576), \
        u((64, 64, 3, 3), 576), u((64,), 576)
    wf, bf = u((1, feat), feat), u((1,), feat)
    x = torch.randn(N, T, F, generator=g).abs().to(dev)
    st = _lib.stream_ptr()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def write(rec):
        line = json.dumps(rec)
        out.write(line + "\n")
        out.flush()
        print(line, flush=True)

    # every HIP case of both precisions is on record before the library runs its first convolution
    for phase, prec in (("hip", "fp32"), ("hip", "bf16"), ("lib", "fp32"), ("lib", "bf16")):
        p, dt = ops.PREC[prec], (torch.bfloat16 if prec == "bf16" else torch.float32)
        y = [torch.empty(N, hw[2 * l], hw[2 * l + 1], 64, dtype=dt, device=dev) for l in range(3)]
        dy = [torch.empty_like(t) for t in y]
        z, score, dz = torch.empty(N, device=dev), torch.empty(N, 1, device=dev), torch.empty(N, device=dev)
        dw = [torch.empty_like(t) for t in (w1, w2, w3, wf)]
        db = [torch.empty(64, device=dev) for _ in range(3)] + [torch.empty(1, device=dev)]
        dx, loss = torch.empty_like(x), torch.empty(1, device=dev)
        wsn = _lib.query("dl4ss_disc_ws_bytes", N, T, F)
        ws = torch.empty((wsn + 3) // 4, device=dev)
        P = _lib.ptr
        launches = {
            "conv1_fwd": lambda: _lib.call("dl4ss_disc_conv1_fwd", p, P(x), P(w1), P(b1), N, T, F, P(y[0]), st),
            "conv2_fwd": lambda: _lib.call("dl4ss_disc_conv64_fwd", p, P(y[0]), P(w2), P(b2), N, hw[0], hw[1], P(y[1]),
                                           st),
            "conv3_fwd": lambda: _lib.call("dl4ss_disc_conv64_fwd", p, P(y[1]), P(w3), P(b3), N, hw[2], hw[3], P(y[2]),
                                           st),
            "head_fwd": lambda: _lib.call("dl4ss_disc_head_fwd", p, P(y[2]), P(wf), P(bf), N, hw[4], hw[5], P(z),
                                          P(score), st),
            "head_loss_bwd": lambda: _lib.call("dl4ss_disc_head_bwd", p, P(y[2]), P(wf), P(score), None, 1.0, N, hw[4],
                                               hw[5], P(loss), P(dz), P(dw[3]), P(db[3]), P(dy[2]), st),
            "conv3_bwd": lambda: _lib.call("dl4ss_disc_conv64_bwd", p, P(y[1]), P(y[2]), P(dy[2]), P(w3), N, hw[2],
                                           hw[3], P(dy[1]), P(dw[2]), P(db[2]), P(ws), wsn, st),
            "conv2_bwd": lambda: _lib.call("dl4ss_disc_conv64_bwd", p, P(y[0]), P(y[1]), P(dy[1]), P(w2), N, hw[0],
                                           hw[1], P(dy[0]), P(dw[1]), P(db[1]), P(ws), wsn, st),
            "conv2_bwd_no_dx": lambda: _lib.call("dl4ss_disc_conv64_bwd", p, P(y[0]), P(y[1]), P(dy[1]), P(w2), N,
                                                 hw[0], hw[1], None, P(dw[1]), P(db[1]), P(ws), wsn, st),
            "conv1_bwd": lambda: _lib.call("dl4ss_disc_conv1_bwd", p, P(x), P(y[0]), P(dy[0]), P(w1), N, T, F, P(dx),
                                           P(dw[0]), P(db[0]), P(ws), wsn, st),
            "conv1_bwd_no_dx": lambda: _lib.call("dl4ss_disc_conv1_bwd", p, P(x), P(y[0]), P(dy[0]), P(w1), N, T, F,
                                                 None, P(dw[0]), P(db[0]), P(ws), wsn, st),
        }
        fwd = ("conv1_fwd", "conv2_fwd", "conv3_fwd", "head_fwd")
        bwd = ("head_loss_bwd", "conv3_bwd", "conv2_bwd", "conv1_bwd")

        def whole(names):
            def run():
                for n in names:
                    launches[n]()
            return run

        # the library path: the reference's nn.Conv2d / F.relu / nn.Linear / F.sigmoid in the same dtype
        lp = [t.to(dt).requires_grad_(True) for t in (w1, b1, w2, b2, w3, b3, wf, bf)]
        xl = x.to(dt).view(N, 1, T, F).requires_grad_(True)

        def lib_fwd():
            h = xl
            for i in range(3):
                h = torch.relu(Fn.conv2d(h, lp[2 * i], lp[2 * i + 1], stride=2))
            s = torch.sigmoid(h.reshape(N, -1) @ lp[6].T + lp[7])
            return ((s.float() - 1.0) ** 2).mean()

        def lib_fwd_bwd():
            torch.autograd.grad(lib_fwd(), lp + [xl])

        def lib_conv2():
            with torch.no_grad():
                Fn.conv2d(y1_nchw, lp[2], lp[3], stride=2)

        cases = dict(launches)
        cases["hip_fwd"] = whole(fwd)
        cases["hip_fwd_bwd"] = whole(fwd + bwd)
        M2 = N * hw[2] * hw[3]
        flop2 = 2.0 * M2 * 64 * 576

        def emit(res):
            for name, t in res.items():
                rec = {"case": name, "precision": prec, "shape": [N, T, F], "reps": a.reps, "us": t}
                if name in ("conv2_fwd", "lib_conv2_fwd"):
                    rec["gflop"] = round(flop2 / 1e9, 2)
                    rec["tflops"] = round(flop2 / (t["median"] * 1e-6) / 1e12, 1)
                    rec["frac_of_mfma_peak"] = round(flop2 / PEAK[prec] / (t["median"] * 1e-6), 4)
                write(rec)

        if phase == "hip":
            emit(timed(cases, a.reps))
            continue
        try:  # its first convolutions may build or search kernels
            y1_nchw = torch.rand(N, 64, hw[0], hw[1], device=dev).to(dt)
            with torch.no_grad():
                lib_fwd()
            lib_fwd_bwd()
            lib_conv2()
            torch.cuda.synchronize()
            emit(timed(dict(lib_fwd=lambda: torch.no_grad()(lib_fwd)(), lib_fwd_bwd=lib_fwd_bwd,
                            lib_conv2_fwd=lib_conv2), a.reps))
        except Exception as e:  # the library path cannot run here: say so in the record
            write({"case": "lib", "precision": prec, "shape": [N, T, F], "error": f"{type(e).__name__}: {e}"[:300]})
    out.close()


if __name__ == "__main__":
    main()
