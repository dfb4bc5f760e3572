"""What feeding the step costs: the replayed C2 step on resident inputs, behind a host loader, behind the corpus.

  python tools/bench_corpus.py [--steps K] [--warmup W] [--rounds R] [--clips C] [--out FILE]

C2 (bench.py's workload): BiLSTM-4L, B = 32, N = 32000 (4 s), 2-spk PIT, bf16, graph replay.  The corpus is synthetic:
``--clips`` sources of synth.speech_like quantised to 16-bit PCM (seed 1), ``--speakers`` speakers, an int16 pool on
the device and the same clips on the host.  One trainer, three loops, timed in alternating rounds of ``--steps``
steps each (A B C A' ...: clock and thermal drift fall on all alike):

  resident  step_graph on four batches that stay on the device: bench.py's way, the ceiling; timed twice per round
            (A and A'), and the difference of the two medians is the spread a difference between loops has to exceed
  host      a host loader: RandomMixSampler's draws, numpy assembly of the (B, K, N) fp32 array from the host clips,
            upload, step_graph
  corpus    the same draws, step_graph_corpus: 1 KB of indices goes up from pinned memory, one launch gathers and mixes

and the mixing launches' own device time from HIP events around ``--launches`` launches each, replayed from a
captured graph: ops.mix_sources (dl4ss_mix_sources_rot: statistics + mixing, two kernels) on an uploaded array
against ops.mix_corpus (one launch).
One JSON line, appended to ``--out`` when given.
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

from dl4ss_amd import corpus as cp, engine, ops, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--speakers", type=int, default=101)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, K, N = a.batch, 2, a.samples
    import random

    random.seed(1)
    np.random.seed(1)
    rng = np.random.Generator(np.random.PCG64(1))
    clips = []
    for i in range(a.clips):
        x = synth.speech_like(rng, N) * rng.uniform(0.2, 1.0)
        q = np.round(x / np.abs(x).max() * 0.9 * 32767).astype(np.int16)
        clips.append((f"s{i % a.speakers:03d}", f"c{i:05d}", q))
    corpus = cp.DeviceCorpus.from_clips(clips, N, device=dev)
    sampler = cp.RandomMixSampler(corpus, B, K, K, db=5)

    net = engine.SepNet(cell="lstm", num_layers=4, device=dev, seed=1)
    tr = engine.SepTrainer(net, B, K, N, mode="pit", precision="bf16")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    resident = []
    for _ in range(4):
        b = sampler.batch()
        resident.append((up(corpus.gather(b["clips"], N)), up(b["gains"]), up(b["speakers"])))

    def step_resident(i):
        return tr.step_graph(*resident[i % 4])

    def step_host(i):
        b = sampler.batch()
        return tr.step_graph(up(corpus.gather(b["clips"], N)), up(b["gains"]), up(b["speakers"]))

    def step_corpus(i):
        b = sampler.batch()
        return tr.step_graph_corpus(corpus, b["clips"], b["gains"], b["speakers"])  # (one pinned upload, no wait)

    tr.step(*resident[0])  # eager first step: plans and workspaces exist before the capture
    loops = [("resident", step_resident), ("host", step_host), ("corpus", step_corpus), ("resident2", step_resident)]
    for _, fn in loops[:3]:
        for i in range(a.warmup):
            fn(i)
    tr.check()
    ms = {name: [] for name, _ in loops}
    for _ in range(a.rounds):
        for name, fn in loops:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                loss = fn(i)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            tr.check()
            assert bool(torch.isfinite(loss).all())
    med = {k: statistics.median(v) for k, v in ms.items()}

    # the mixing launches alone, device time
    b = sampler.batch()
    raw, gains, clips_d = up(corpus.gather(b["clips"], N)), up(b["gains"]), up(b["clips"])
    lens = up(b["lengths"])
    bad = torch.zeros(1, device=dev, dtype=torch.int32)

    def timed(fn, reps=10):
        """device time of one call of fn: ``reps`` calls captured into one HIP graph, replayed between two events
        (kernel time plus in-graph gaps, not the host's launch path)"""
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
        g.replay()
        n = max(1, a.launches // reps)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (n * reps) * 1e3

    def mix_rot():
        ops.mix_sources(raw, gains, out_src=tr.src, out_mix=tr.mix, stats_ws=tr.stats, lengths=lens)

    def mix_corpus():
        corpus.mix(clips_d, gains, K, N, out_src=tr.src, out_mix=tr.mix, bad=bad)

    us = {"mix_sources_rot": [], "mix_corpus": []}
    for _ in range(5):
        us["mix_sources_rot"].append(timed(mix_rot))
        us["mix_corpus"].append(timed(mix_corpus))
    assert int(bad.item()) == 0

    spread = abs(med["resident"] - med["resident2"])
    line = {
        "config": f"C2 step by input path: BiLSTM-4L, B={B}, N={N}, 2-spk PIT, bf16, graph replay; synthetic int16 "
                  f"corpus of {a.clips} clips ({corpus.pool.nbytes / 2 ** 20:.0f} MiB), {a.speakers} speakers",
        "ms_per_step": med, "mixtures_per_s": {k: B / v * 1e3 for k, v in med.items()}, "rounds_ms": ms,
        "resident_spread_ms": spread, "corpus_minus_resident_ms": med["corpus"] - med["resident"],
        "host_minus_resident_ms": med["host"] - med["resident"],
        "corpus_within_resident_spread": bool(abs(med["corpus"] - med["resident"]) <= spread),
        "mix_launch_us": {k: statistics.median(v) for k, v in us.items()}, "mix_launch_rounds_us": us,
        "steps_per_round": a.steps, "rounds": a.rounds, "loss": float(tr.loss[0]), "data": "synthetic", "n_gpus": 1}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
