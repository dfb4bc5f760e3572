"""Target evaluation (targeteval.TargetEvaluator) at C2's shapes, same process, eager launches.

  python tools/bench_targeteval.py [--steps K] [--warmup W] [--rounds R] [--batch B] [--samples N]

BiLSTM-4L (H = 300, no ADDJUST), B = 32, N = 32000, fp32, seen speakers (queries from the speaker memory), three
source slots: evaluate() with spk_num 2 and 3, with and without the background clip, timed in alternating rounds of
``--steps`` batches each; the result is each configuration's median round as evaluated mixtures per second (the
mixture itself is scored too: two BSS_EVAL.m compositions, four gain decompositions per batch).  The two new
kernels are event-timed alone, 200 back-to-back calls each: dl4ss_te_assemble over the batch, and dl4ss_bss_gain
(its four launches) on the batch's own waveforms as evaluate() calls it -- the prediction on [noise; target] -- with
the bytes it moves (2 (J + Ke) N 4 B per utterance) over that time.  For context, bss.bss_eval_sources (BSS_EVAL
v3: 512-tap filters, permutation search; host-synchronous) on the same waveforms, [noise; target] against
[mixture - prediction; prediction].  One JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dl4ss_amd import _lib, bss, engine, synth, targeteval  # noqa: E402
from dl4ss_amd.voiceprint import SpeakerMemory, VoiceprintNet  # noqa: E402


def event_us(fn, reps=200, rounds=5):
    """Median over ``rounds`` of the mean time of ``reps`` back-to-back calls of fn, in microseconds."""
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
    B, S, N = a.batch, 3, a.samples
    src, _, _ = synth.SyntheticMixtures(n_samples=N, k=S, seed=1).batch(B)
    raw = torch.from_numpy(src.astype(np.float32)).to(dev)
    ids = torch.arange(B, dtype=torch.int32, device=dev) % 101
    bgd = np.random.default_rng(2).standard_normal(N)

    net = engine.SepNet(cell="lstm", num_layers=4, adjust=False, device=dev, seed=1)
    vnet = VoiceprintNet(device=dev, seed=2)
    memory = SpeakerMemory(net.num_labels, net.E, dev)
    memory.mem.copy_(torch.randn(net.num_labels, net.E, generator=torch.Generator().manual_seed(3)))
    sides = {}
    for spk_num in (2, 3):
        for noise in (False, True):
            ev = targeteval.TargetEvaluator(net, vnet, memory, B, N, spk_num=spk_num, bgd_noise=bgd if noise else None)
            for _ in range(a.warmup):
                ev.evaluate(raw, None, ids=ids)
            ev.check()
            sides[f"spk{spk_num}" + ("_noise" if noise else "")] = ev
    ms = {k: [] for k in sides}
    for _ in range(a.rounds):
        for name, ev in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                ev.evaluate(raw, None, ids=ids)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            ev.check()
    med = {k: statistics.median(v) for k, v in ms.items()}
    summaries = {k: ev.summary() for k, ev in sides.items()}

    # the two new kernels alone, on the last configuration's own buffers
    ev = sides["spk3_noise"]
    bf = ev._buffers(S)
    asm_us = event_us(lambda: targeteval.assemble(bf["srcs"], bf["lengths"], ev.bgd, 3,
                                                  out=(ev.mix, ev.noise, ev.target, ev.mix_len)))
    L = ev.L
    srcs = torch.stack([ev.noise[:, :L], ev.target[:, :L]], 1).contiguous()
    est = ev.pred_wav[:, None].contiguous()
    J, Ke = 2, 1
    ws_bytes = _lib.query("dl4ss_bss_gain_ws_bytes", B, L)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    crit = torch.empty(B, Ke, 3, dtype=torch.float64, device=dev)
    sing = torch.empty(1, dtype=torch.int32, device=dev)
    index = (ctypes.c_int * Ke)(1)
    gain_us = event_us(lambda: _lib.call(
        "dl4ss_bss_gain", src=_lib.ptr(srcs), est=_lib.ptr(est), index=index, n_eff=_lib.ptr(ev.n_eff), M=B, J=J, Ke=Ke,
        N=L, ws=_lib.ptr(ws), ws_bytes=ws_bytes, crit=_lib.ptr(crit), singular=_lib.ptr(sing), stream=_lib.stream_ptr()))
    gain_bytes = 2 * (J + Ke) * L * 4 * B
    # BSS_EVAL v3 on the same waveforms, for context (host-synchronous: it returns numpy)
    refs = srcs
    ests = torch.stack([ev.mix[:, :L] - ev.pred_wav, ev.pred_wav], 1).contiguous()
    bss.bss_eval_sources(refs, ests)
    v3 = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bss.bss_eval_sources(refs, ests)
        v3.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({
        "config": f"target evaluation at C2's shapes: BiLSTM-4L H=300, B={B}, N={N} (T={ev.T}), fp32, eager, seen "
                  f"speakers, {S} source slots; prediction and mixture both scored",
        "ms_per_batch": med, "mixtures_per_s": {k: B / v * 1e3 for k, v in med.items()},
        "round_spread_ms": {k: max(v) - min(v) for k, v in ms.items()}, "rounds_ms": ms, "batches_per_round": a.steps,
        "te_assemble_us": asm_us, "te_assemble_GBps": (3 + 3) * B * N * 4 / asm_us / 1e3,
        "bss_gain_us": gain_us, "bss_gain_bytes": gain_bytes, "bss_gain_GBps": gain_bytes / gain_us / 1e3,
        "bss_gain_shape": dict(M=B, J=J, Ke=Ke, N=L, chunks=-(-L // 4096)),
        "bss_eval_sources_v3_ms": statistics.median(v3), "bss_eval_sources_v3_shape": dict(M=B, K=2, N=L),
        "summary": summaries, "singular": int(sing.item()), "data": "synthetic", "n_gpus": 1}), flush=True)


if __name__ == "__main__":
    main()
