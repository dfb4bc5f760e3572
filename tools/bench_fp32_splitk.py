"""The fp32 step with the fixed-order split-K against the default step, same process, eager launches.

  python tools/bench_fp32_splitk.py [--steps K] [--warmup W] [--rounds R] [--batch B] [--samples N]

C2's shapes (BiLSTM-4L, B = 32, K = 2, N = 32000), mode "label", fp32, eager, for ATTENTION 'dot' and 'align':
SepTrainer(..., splitk_reduce="atomic") -- on 'dot' the backward GEMMs split with float atomics, on 'align' they
run unsplit -- against SepTrainer(..., splitk_reduce="fixed") (every backward GEMM split through fp32 slabs added
in a fixed order, fixed-order bias column sums: the step that repeats bit for bit).  The four trainers are timed
in alternating rounds of ``--steps`` steps each (A B C D A B C D ...), so that clock and thermal drift fall on all
alike; the result is each side's median round, the rounds themselves and their spread, and the slab bytes each
"fixed" step writes and reads again (computed from the shapes).  One JSON line.
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
from dl4ss_amd.params import _ngate  # noqa: E402


def slab_bytes(net, B, T):
    """Bytes of split-K slabs one "fixed" backward writes (and the combines read again): per GEMM
    gemm_fixed_ws_bytes at the auto factor."""
    BT, H, FE = B * T, net.H, net.F * net.E
    NGH = _ngate(net.cell) * H
    shapes = [(FE, 2 * H, BT), (BT, 2 * H, FE)]
    for l in range(net.L):
        shapes += [(2 * NGH, net.F if l == 0 else 2 * H, BT), (NGH, H, BT), (NGH, H, BT)]
        if l > 0:
            shapes.append((BT, 2 * H, 2 * NGH))
    return sum(ops.gemm_fixed_ws_bytes(*s, "auto") for s in shapes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=32000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fp32_splitk: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda")
    B, K, N = a.batch, 2, a.samples
    src, spk, u = synth.SyntheticMixtures(n_samples=N, k=K, seed=1).batch(B)
    batch = (torch.from_numpy(src.astype(np.float32)).to(dev),
             torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(dev),
             torch.from_numpy(spk.astype(np.int32)).to(dev))

    def make(attention, reduce):
        net = engine.SepNet(cell="lstm", num_layers=4, adjust=False, device=dev, seed=1, attention=attention)
        tr = engine.SepTrainer(net, B, K, N, mode="label", precision="fp32", splitk_reduce=reduce)
        for _ in range(a.warmup):
            tr.step(*batch)
        tr.check()
        return tr

    sides = {f"{att}_{red}": make(att, red) for att in ("dot", "align") for red in ("atomic", "fixed")}
    ms = {k: [] for k in sides}
    for _ in range(a.rounds):
        for name, tr in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = tr.step(*batch)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            tr.check()
            assert bool(torch.isfinite(loss).all())
    med = {k: statistics.median(v) for k, v in ms.items()}
    tr = sides["dot_fixed"]
    print(json.dumps({
        "config": f"C2 fp32 step, splitk_reduce atomic vs fixed: BiLSTM-4L, B={B}, K={K}, N={N}, label order, fp32, "
                  "eager, no ADDJUST ('align' atomic = the unsplit step)",
        "ms_per_step": med,
        "fixed_minus_atomic_ms": {att: med[f"{att}_fixed"] - med[f"{att}_atomic"] for att in ("dot", "align")},
        "fixed_minus_atomic_percent": {att: 100.0 * (med[f"{att}_fixed"] - med[f"{att}_atomic"]) / med[f"{att}_atomic"]
                                       for att in ("dot", "align")},
        "rounds_ms": ms, "round_spread_ms": {k: max(v) - min(v) for k, v in ms.items()},
        "steps_per_round": a.steps, "slab_mb_per_step": slab_bytes(tr.net, B, tr.T) / 1e6,
        "workspace_mb": tr.fixed_ws.numel() * 4 / 1e6, "loss": {k: float(t.loss[0]) for k, t in sides.items()},
        "data": "synthetic", "n_gpus": 1}), flush=True)


if __name__ == "__main__":
    main()
