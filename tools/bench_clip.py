"""The training step with the on-device gradient clip against the plain step, same process, graph replay.

  python tools/bench_clip.py [--steps K] [--warmup W] [--rounds R] [--precision bf16] [--clip-norm X] [--eager]

C2 (bench.py's workload): BiLSTM-4L, B = 32, N = 32000 (4 s), 2-spk PIT, bf16 -- once as SepTrainer(...)
(clip_norm=None: the unclipped step, no extra launch), once as SepTrainer(..., clip_norm=inf): the
sum-of-squares launch over the 11.4 M-float gradient and the clipped Adam (the partials summed in every block,
the non-finite guard), with c == 1 so both sides train the same weights.  The two trainers are timed in
alternating rounds of ``--steps`` replayed steps each (A B A B ...), so that clock and thermal drift fall on
both alike; the result is each side's median round and the difference.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dl4ss_amd import engine, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "bf16s", "bf16s2"])
    ap.add_argument("--clip-norm", type=float, default=float("inf"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--eager", action="store_true", help="step() instead of step_graph()")
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, K, N = a.batch, 2, a.samples
    src, spk, u = synth.SyntheticMixtures(n_samples=N, k=K, seed=1).batch(B)
    batch = (torch.from_numpy(src.astype(np.float32)).to(dev),
             torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(dev),
             torch.from_numpy(spk.astype(np.int32)).to(dev))

    def make(clip_norm):
        net = engine.SepNet(cell="lstm", num_layers=4, device=dev, seed=1)
        tr = engine.SepTrainer(net, B, K, N, mode="pit", precision=a.precision, clip_norm=clip_norm)
        tr.step(*batch)  # eager first step: plans and workspaces exist before the capture
        fn = tr.step if a.eager else tr.step_graph
        for _ in range(a.warmup):
            fn(*batch)
        tr.check()
        return tr, fn

    sides = {"plain": make(None), "clipped": make(a.clip_norm)}
    ms = {k: [] for k in sides}
    for _ in range(a.rounds):
        for name, (tr, fn) in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = fn(*batch)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            tr.check()
            assert bool(torch.isfinite(loss).all())
    tr = sides["clipped"][0]
    med = {k: statistics.median(v) for k, v in ms.items()}
    same = bool(torch.equal(sides["plain"][0].net.flat, tr.net.flat)) if a.clip_norm == float("inf") else None
    print(json.dumps({
        "config": f"C2 clipped step vs plain: BiLSTM-4L, B={B}, N={N}, 2-spk PIT, {a.precision}, "
                  f"{'eager' if a.eager else 'graph replay'}, clip_norm={a.clip_norm}",
        "ms_per_step": med, "extra_ms_per_step": med["clipped"] - med["plain"],
        "extra_percent": 100.0 * (med["clipped"] - med["plain"]) / med["plain"],
        "mixtures_per_s": {k: B / v * 1e3 for k, v in med.items()}, "rounds_ms": ms, "steps_per_round": a.steps,
        "grad_floats": tr.net.grad.numel(), "grad_norm": [float(x) for x in tr.grad_norm.tolist()],
        "skipped_nonfinite": tr.skipped_nonfinite, "weights_bitwise_equal": same, "loss": float(tr.loss[0]),
        "data": "synthetic", "n_gpus": 1}), flush=True)


if __name__ == "__main__":
    main()
