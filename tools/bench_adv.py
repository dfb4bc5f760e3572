"""The adversarial training step against the plain step, same process, graph replay.

  python tools/bench_adv.py [--steps K] [--warmup W] [--rounds R] [--precision bf16] [--adv-weight L] [--eager]

C2 (bench.py's workload): BiLSTM-4L, B = 32, N = 32000 (4 s), 2-spk PIT, bf16 -- once as
SepTrainer(...), once as SepTrainer(..., adversary=DiscNet) (the Discriminator over the 2 B K maps, its two
backwards, the adversarial GRAD pass, two more Adam launches).  The two trainers are timed in alternating
rounds of ``--steps`` replayed steps each (A B A B ...), so that clock and thermal drift fall on both alike; the
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

from dl4ss_amd import engine, ops, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "bf16s", "bf16s2"])
    ap.add_argument("--adv-weight", type=float, default=1.0)
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

    def make(adv):
        net = engine.SepNet(cell="lstm", num_layers=4, device=dev, seed=1)
        kw = {}
        if adv:
            kw = dict(adversary=engine.DiscNet(ops.n_frames(N), net.F, device=dev, seed=2), adv_weight=a.adv_weight)
        tr = engine.SepTrainer(net, B, K, N, mode="pit", precision=a.precision, **kw)
        tr.step(*batch)  # eager first step: plans and workspaces exist before the capture
        fn = tr.step if a.eager else tr.step_graph
        for _ in range(a.warmup):
            fn(*batch)
        tr.check()
        return tr, fn

    sides = {"plain": make(False), "adversarial": make(True)}
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
    tr = sides["adversarial"][0]
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        "config": f"C2 adversarial step vs plain: BiLSTM-4L, B={B}, N={N}, 2-spk PIT, {a.precision}, "
                  f"{'eager' if a.eager else 'graph replay'}, lambda={a.adv_weight}",
        "ms_per_step": med, "extra_ms_per_step": med["adversarial"] - med["plain"],
        "mixtures_per_s": {k: B / v * 1e3 for k, v in med.items()}, "rounds_ms": ms, "steps_per_round": a.steps,
        "adv_loss": [float(x) for x in tr.adv_loss.tolist()], "loss": float(tr.loss[0]),
        "disc_updates": tr.adv_step_count, "data": "synthetic", "n_gpus": 1}), flush=True)


if __name__ == "__main__":
    main()
