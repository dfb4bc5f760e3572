"""The training step with Nadam against the step with Adam, same process, graph replay.

  python tools/bench_nadam.py [--steps K] [--warmup W] [--rounds R] [--precision bf16] [--pair adam,nadam] [--eager]

C2 (bench.py's workload): BiLSTM-4L, B = 32, N = 32000 (4 s), 2-spk PIT, bf16.  ``--pair A,B`` names the two
sides, each one of

  adam        SepTrainer(...): today's step
  nadam       SepTrainer(..., optimizer="nadam"): the same seven fp32 streams and the bf16 shadows, a few more FMAs
  nadam-clip  SepTrainer(..., optimizer="nadam", clipnorm=inf): the sum-of-squares launch over the 11.4 M-float
              gradient and the clipped update (Keras's rule, c == 1)

The default runs all three questions in one process: adam against nadam, nadam against nadam-clip, and adam against
adam -- two sides built alike, whose difference is the spread a difference between unlike sides has to exceed.  The
two trainers of a pair are timed in alternating rounds of ``--steps`` replayed steps each (A B A B ...), so that
clock and thermal drift fall on both alike; the result is each side's median round and the difference.  One JSON
line.
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

SIDES = {"adam": {}, "nadam": dict(optimizer="nadam"), "nadam-clip": dict(optimizer="nadam", clipnorm=float("inf"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "bf16s", "bf16s2"])
    ap.add_argument("--pair", action="append", help="A,B of adam / nadam / nadam-clip (repeatable); default: "
                    "adam,adam  adam,nadam  nadam,nadam-clip")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--eager", action="store_true", help="step() instead of step_graph()")
    a = ap.parse_args()
    pairs = [tuple(p.split(",")) for p in (a.pair or ["adam,adam", "adam,nadam", "nadam,nadam-clip"])]
    for p in pairs:
        if len(p) != 2 or any(s not in SIDES for s in p):
            ap.error(f"--pair {','.join(p)}: two of {sorted(SIDES)}")
    dev = torch.device("cuda")
    B, K, N = a.batch, 2, a.samples
    src, spk, u = synth.SyntheticMixtures(n_samples=N, k=K, seed=1).batch(B)
    batch = (torch.from_numpy(src.astype(np.float32)).to(dev),
             torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(dev),
             torch.from_numpy(spk.astype(np.int32)).to(dev))

    def make(side):
        net = engine.SepNet(cell="lstm", num_layers=4, device=dev, seed=1)
        tr = engine.SepTrainer(net, B, K, N, mode="pit", precision=a.precision, **SIDES[side])
        tr.step(*batch)  # eager first step: plans and workspaces exist before the capture
        fn = tr.step if a.eager else tr.step_graph
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
        same = bool(torch.equal(ta.net.flat, tb.net.flat)) if SIDES[pa].get("optimizer") == SIDES[pb].get("optimizer") \
            else None
        out.append({"a": pa, "b": pb, "ms_per_step": med, "b_minus_a_ms": med[1] - med[0],
                    "b_minus_a_percent": 100.0 * (med[1] - med[0]) / med[0], "rounds_ms": ms,
                    "weights_bitwise_equal": same, "loss": [float(ta.loss[0]), float(tb.loss[0])],
                    "grad_norm_b": [float(x) for x in tb.grad_norm.tolist()] if hasattr(tb, "grad_norm") else None})
        del sides, ta, tb
        torch.cuda.empty_cache()
    print(json.dumps({
        "config": f"C2 step by optimizer: BiLSTM-4L, B={B}, N={N}, 2-spk PIT, {a.precision}, "
                  f"{'eager' if a.eager else 'graph replay'}",
        "pairs": out, "steps_per_round": a.steps, "rounds": a.rounds, "data": "synthetic", "n_gpus": 1}), flush=True)


if __name__ == "__main__":
    main()
