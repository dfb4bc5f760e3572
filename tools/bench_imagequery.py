"""The training step with image queries against the plain step, same process, eager launches.

  python tools/bench_imagequery.py [--steps K] [--warmup W] [--rounds R] [--batch B] [--samples N]

C2's shapes (BiLSTM-4L, B = 32, K = 2, N = 32000), mode "label", fp32, eager, a mask net without ADDJUST -- once
as SepTrainer(...) (queries gathered from emb.layer.weight), once each as SepTrainer(..., image_query=, memory=)
with memory_refresh "reference" (a second encoder pass after the update) and "reuse".  The encoder is the default
ImageQueryNet (28 x 28, E = 50, 2418 parameters) over the step's B K = 64 synth.glyphs images.  The three
trainers are timed in alternating rounds of ``--steps`` steps each (A B C A B ...), so that clock and thermal drift
fall on all alike; the result is each side's median round and the differences.  The encoder's three launches
(forward, backward, reduce) are event-timed alone as well, 200 back-to-back launches each, and next to the reduce
``ops.vp_colsum`` over the same rows (the serial-order column sum it stands in for).  One JSON line.
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
from dl4ss_amd.imagequery import ImageQueryEncoder, ImageQueryNet  # noqa: E402
from dl4ss_amd.voiceprint import SpeakerMemory  # noqa: E402


def event_us(fn, reps=200, rounds=5):
    """Median over ``rounds`` of the mean time of ``reps`` back-to-back launches of fn, in microseconds."""
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return statistics.median(out)


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
    images = torch.from_numpy(synth.glyphs(101).draw(spk, np.random.default_rng(1))).view(B, K, 28, 28).to(dev)

    def make(refresh):
        net = engine.SepNet(cell="lstm", num_layers=4, adjust=False, device=dev, seed=1)
        kw = {}
        if refresh is not None:
            kw.update(image_query=ImageQueryNet(device=dev, seed=2), memory=SpeakerMemory(net.num_labels, net.E, dev),
                      memory_refresh=refresh)
        tr = engine.SepTrainer(net, B, K, N, mode="label", precision="fp32", **kw)
        step = (lambda: tr.step(*batch, images=images)) if refresh is not None else (lambda: tr.step(*batch))
        for _ in range(a.warmup):
            step()
        tr.check()
        return tr, step

    sides = {"plain": make(None), "reference": make("reference"), "reuse": make("reuse")}
    iq = [k for k in sides if k != "plain"]
    ms = {k: [] for k in sides}
    for _ in range(a.rounds):
        for name, (tr, step) in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = step()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            tr.check()
            assert bool(torch.isfinite(loss).all())
    med = {k: statistics.median(v) for k, v in ms.items()}

    inet = ImageQueryNet(device=dev, seed=2)
    enc = ImageQueryEncoder(inet, B * K)
    flat_images = images.view(B * K, 28, 28)
    dvec = torch.randn(B * K, inet.E, device=dev)
    enc.forward(flat_images)
    kernels = {"forward": event_us(lambda: enc.forward(flat_images)),
               "backward": event_us(lambda: ops.imgq_bwd(flat_images, dvec, inet.flat, enc.dpart)),
               "reduce": event_us(lambda: ops.imgq_reduce(enc.dpart, inet.grad))}
    # the alternative the pairwise reduce replaced: ops.vp_colsum's two serial-order launches over the same rows
    part, out2 = ops.vp_colsum_part(B * K, inet.numel, dev), torch.empty_like(inet.grad)
    kernels["reduce_vp_colsum"] = event_us(lambda: ops.vp_colsum(enc.dpart, out2, part))
    print(json.dumps({
        "config": f"C2 image-query step vs plain: BiLSTM-4L, B={B}, K={K}, N={N}, label order, fp32, eager, no ADDJUST; "
                  f"encoder CNN 28x28 -> {inet.E}, {B * K} images",
        "ms_per_step": med,
        "extra_ms_per_step": {k: med[k] - med["plain"] for k in iq},
        "extra_percent": {k: 100.0 * (med[k] - med["plain"]) / med["plain"] for k in iq},
        "round_spread_ms": {k: max(v) - min(v) for k, v in ms.items()},
        "mixtures_per_s": {k: B / v * 1e3 for k, v in med.items()}, "rounds_ms": ms, "steps_per_round": a.steps,
        "encoder_kernel_us": kernels, "encoder_params": inet.num_params,
        "loss": {k: float(t.loss[0]) for k, (t, _) in sides.items()}, "data": "synthetic", "n_gpus": 1}), flush=True)


if __name__ == "__main__":
    main()
