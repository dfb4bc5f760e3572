"""The fp32 training step with Keras 1's LSTM cell (gates="hard") against the step with the logistic cell, same process.

  python tools/bench_keras_cell.py [--steps K] [--warmup W] [--rounds R] [--pair logistic,hard] [--graph]

C2's shapes (bench.py's workload): BiLSTM-4L, H = 300, B = 32, N = 32000 (4 s), 2-spk PIT -- in fp32, eager, the only
recurrence the hard cell has: the generic kernels, where the logistic H = 300 plan runs the compile-time-sliced
instantiations and the hard cell the runtime-bounds ones.  ``--pair A,B`` names the two sides, each ``logistic`` or
``hard``.  The default runs logistic against hard and logistic against logistic -- two sides built alike, whose
difference is the spread a difference between unlike sides has to exceed.  The two trainers of a pair are timed in
alternating rounds of ``--steps`` steps each (A B A B ...), so that clock and thermal drift fall on both alike; the
result is each side's median round and the difference.  One JSON line.
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

SIDES = ("logistic", "hard")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pair", action="append", help="A,B of logistic / hard (repeatable); default: "
                    "logistic,logistic  logistic,hard")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--graph", action="store_true", help="step_graph() instead of step()")
    a = ap.parse_args()
    pairs = [tuple(p.split(",")) for p in (a.pair or ["logistic,logistic", "logistic,hard"])]
    for p in pairs:
        if len(p) != 2 or any(s not in SIDES for s in p):
            ap.error(f"--pair {','.join(p)}: two of {SIDES}")
    dev = torch.device("cuda")
    B, K, N = a.batch, 2, a.samples
    src, spk, u = synth.SyntheticMixtures(n_samples=N, k=K, seed=1).batch(B)
    batch = (torch.from_numpy(src.astype(np.float32)).to(dev),
             torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(dev),
             torch.from_numpy(spk.astype(np.int32)).to(dev))

    def make(side):
        net = engine.SepNet(cell="lstm", num_layers=4, device=dev, seed=1, gates=side)
        tr = engine.SepTrainer(net, B, K, N, mode="pit", precision="fp32")
        tr.step(*batch)  # eager first step: plans and workspaces exist before a capture
        fn = tr.step_graph if a.graph else tr.step
        for _ in range(a.warmup):
            fn(*batch)
        tr.check()
        return tr, fn

    out = []
    for pa, pb in pairs:
        sides = [(pa, *make(pa)), (pb, *make(pb))]  # (two trainers even when pa == pb: the spread)
        ms = [[], []]
        for _ in range(a.rounds):
            for i, (_, tr, fn) in enumerate(sides):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loss = fn(*batch)
                torch.cuda.synchronize()
                ms[i].append((time.perf_counter() - t0) / a.steps * 1e3)
                tr.check()
                assert bool(torch.isfinite(loss).all())
        med = [statistics.median(v) for v in ms]
        (_, ta, _), (_, tb, _) = sides
        out.append({"a": pa, "b": pb, "ms_per_step": med, "b_minus_a_ms": med[1] - med[0],
                    "b_minus_a_percent": 100.0 * (med[1] - med[0]) / med[0], "rounds_ms": ms,
                    "loss": [float(ta.loss[0]), float(tb.loss[0])]})
        del sides, ta, tb
        torch.cuda.empty_cache()
    print(json.dumps({
        "config": f"C2 step by LSTM cell: BiLSTM-4L, B={B}, N={N}, 2-spk PIT, fp32, "
                  f"{'graph replay' if a.graph else 'eager'}",
        "pairs": out, "steps_per_round": a.steps, "rounds": a.rounds, "data": "synthetic", "n_gpus": 1}), flush=True)


if __name__ == "__main__":
    main()
