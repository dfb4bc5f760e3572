"""Timing of one speaker-classifier training step (dl4ss_amd.classifier.ClassifierTrainer) at the
reference's size -- B = 32, T = 251 (N = 32000 samples), H = 600, 3 layers, N_lab = 101 -- in fp32 and
bf16, and of the large-hidden BPTT launch beside the large-hidden forward launch of the same (middle)
layer in the same process.  HIP events after a warm-up; median and [min, max] of --reps repetitions.
One JSON line per measurement on stdout and appended to --out.

    python tools/bench_classifier.py [--reps 30] [--warmup 3] [--out profiles/cls_train_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dl4ss_amd import classifier, infer, ops, synth  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, K, N, H, L, C = args.batch, 2, args.samples, 600, 3, 101
    src, spk, u = synth.SyntheticMixtures(n_samples=N, k=K, seed=1).batch(B)
    raw = torch.from_numpy(src.astype(np.float32)).to(dev)
    gains = torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(dev)
    y_map = np.zeros((B, C), np.float32)
    for b in range(B):
        y_map[b, np.asarray(spk[b]) % C] = 1.0
    y = torch.from_numpy(y_map).to(dev)
    lines = []
    for precision in ("fp32", "bf16"):
        cnet = infer.ClassifierNet(hidden=H, num_layers=L, num_labels=C, device=dev, seed=1)
        tr = classifier.ClassifierTrainer(cnet, B, K, N, precision=precision)
        r = timed(lambda: tr.step(raw, gains, y), args.reps, args.warmup)
        tr.check()
        r.update(what="classifier_step", precision=precision, B=B, T=tr.T, H=H, L=L, n_lab=C,
                 mixtures_per_s=B / (r["median_ms"] * 1e-3), loss=float(tr.loss[0].item()))
        lines.append(r)
        # one forward and one BPTT launch of the middle layer on the step's own buffers
        l, T = 1, tr.T
        G = tr.G.clone()

        def fwd():
            ops.birnn_fwd("lstm", B, T, H, G=G, w_hh=cnet.cat_view("weight_hh", l), b_hh=cnet.cat_view("bias_hh", l),
                          out=tr.out[l], hprev=tr.hprev[l], act=tr.act[l], cs=tr.cs[l], ws=tr.rnn_ws,
                          ws_bytes=tr.ws_bytes, status=tr.status, precision=precision)

        dH, dG = torch.randn(B * T, 2 * H, device=dev) * 1e-3, torch.empty_like(G)

        def bwd():
            ops.birnn_bwd("lstm", B, T, H, dOut=dH, w_hh=cnet.cat_view("weight_hh", l), act=tr.act[l], cs=tr.cs[l],
                          hprev=tr.hprev[l], dG=dG, ws=tr.rnn_ws, ws_bytes=tr.ws_bytes, status=tr.status,
                          precision=precision)

        ops.gemm(tr.out[0].view(B * T, 2 * H), cnet.cat_view("weight_ih", l), transB=True,
                 bias=cnet.cat_view("bias_ih", l), out=G, precision=precision)
        for what, fn in (("birnn_fwd_launch", fwd), ("birnn_bwd_launch", bwd)):
            r = timed(fn, args.reps, args.warmup)
            r.update(what=what, precision=precision, B=B, T=T, H=H, us_per_step=r["median_ms"] * 1e3 / T)
            lines.append(r)
        tr.check()
        del tr, cnet
    for r in lines:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
