"""The training step with voiceprint queries against the plain step, same process, eager launches.

  python tools/bench_voiceprint.py [--steps K] [--warmup W] [--rounds R] [--batch B] [--samples N]

C2's shapes (BiLSTM-4L, B = 32, K = 2, N = 32000), mode "label", fp32, eager, a mask net without ADDJUST -- once
as SepTrainer(...) (queries gathered from emb.layer.weight), once each as SepTrainer(..., voiceprint=, memory=)
with memory_refresh "reference" (a second encoder pass after the update) and "reuse".  The voiceprint encoder is
the default VoiceprintNet (BiLSTM-2L, H = 25) over the step's B K = 64 clean magnitude maps; and both voiceprint
trainers again with splitk_reduce="fixed" (the mask net's backward GEMMs and the encoder's six weight gradients
split through fixed-order slabs: the step that repeats bit for bit).  The five trainers are timed in alternating
rounds of ``--steps`` steps each (A B C D E A B ...), so that clock and thermal drift fall on all alike; the
result is each side's median round and the differences.  One JSON line.
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
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=32000)
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, K, N = a.batch, 2, a.samples
    src, spk, u = synth.SyntheticMixtures(n_samples=N, k=K, seed=1).batch(B)
    batch = (torch.from_numpy(src.astype(np.float32)).to(dev),
             torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(dev),
             torch.from_numpy(spk.astype(np.int32)).to(dev))

    def make(refresh, reduce="atomic"):
        net = engine.SepNet(cell="lstm", num_layers=4, adjust=False, device=dev, seed=1)
        kw = dict(splitk_reduce=reduce)
        if refresh is not None:
            kw.update(voiceprint=VoiceprintNet(device=dev, seed=2), memory=SpeakerMemory(net.num_labels, net.E, dev),
                      memory_refresh=refresh)
        tr = engine.SepTrainer(net, B, K, N, mode="label", precision="fp32", **kw)
        for _ in range(a.warmup):
            tr.step(*batch)
        tr.check()
        return tr

    sides = {"plain": make(None), "reference": make("reference"), "reuse": make("reuse"),
             "reference_fixed": make("reference", "fixed"), "reuse_fixed": make("reuse", "fixed")}
    vp = [k for k in sides if k != "plain"]
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
    print(json.dumps({
        "config": f"C2 voiceprint step vs plain: BiLSTM-4L, B={B}, K={K}, N={N}, label order, fp32, eager, no ADDJUST; "
                  "encoder BiLSTM-2L H=25",
        "ms_per_step": med,
        "extra_ms_per_step": {k: med[k] - med["plain"] for k in vp},
        "extra_percent": {k: 100.0 * (med[k] - med["plain"]) / med["plain"] for k in vp},
        "fixed_minus_unsplit_ms": {k: med[k + "_fixed"] - med[k] for k in ("reference", "reuse")},
        "round_spread_ms": {k: max(v) - min(v) for k, v in ms.items()},
        "mixtures_per_s": {k: B / v * 1e3 for k, v in med.items()}, "rounds_ms": ms, "steps_per_round": a.steps,
        "encoder_floats": sides["reuse"].vnet.flat.numel(), "loss": {k: float(t.loss[0]) for k, t in sides.items()},
        "data": "synthetic", "n_gpus": 1}), flush=True)


if __name__ == "__main__":
    main()
