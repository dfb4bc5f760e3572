"""Time the ATTENTION 'align' training step on the bf16 fast paths against the bf16 'dot' step, at C2's shapes
(BiLSTM-4L, B = 32, K = 2, N = 32000 -> T = 251, PIT), in one process:

  * the bf16 'dot' step, the bf16 'align' step, the bf16s 'align' step and the fp32 'align' step with
    splitk_reduce="fixed" -- each captured and replayed (step_graph), timed in alternating rounds of `--steps`
    replays between two HIP events, median over the rounds;
  * the attention launches of each pass on the trainers' own buffers, each timed by its own pair of events, the
    variants alternating: 'dot' COST / GRAD and 'align' COST / GRAD in their bf16-V forms (and 'align' on fp32 V
    with bf16 dPre, the bf16s step's form);
  * X = (bf16 'align' step) - (bf16 'dot' step) and Y = ('align' COST + GRAD) - ('dot' COST + GRAD): X <= 1.25 Y says
    the attention kernels are all the align step pays for (no stray conversion, zeroing or copy pass, no GEMM that
    fell back to an unsplit or fp32 form);
  * before any update, on one batch and the same weights: the masked magnitudes (the COST pass's predictions) of the
    bf16 and bf16s 'align' forwards against the fp32 'align' forward, relative L2 -- next to the project's 1e-3 bar.

One JSON line, printed and appended to --out (default profiles/align_bf16_c2.jsonl).

  python tools/bench_align_step.py [--rounds 9] [--steps 10] [--reps 30] [--out PATH]
"""
import argparse
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from dl4ss_amd import engine, synth  # noqa: E402

B, K, N, L = 32, 2, 32000, 4
STEPS = {"dot_bf16": dict(attention="dot", precision="bf16"), "align_bf16": dict(attention="align", precision="bf16"),
         "align_bf16s": dict(attention="align", precision="bf16s"),
         "align_fp32_fixed": dict(attention="align", precision="fp32", splitk_reduce="fixed")}


def stats(ts, nd=1):
    return {"median": round(statistics.median(ts), nd), "min": round(min(ts), nd), "max": round(max(ts), nd)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=__file__.rsplit("/tools/", 1)[0] + "/profiles/align_bf16_c2.jsonl")
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = synth.SyntheticMixtures(n_samples=N, k=K, seed=1)
    batches = []
    for _ in range(2):
        src, spk, u = gen.batch(B)
        batches.append((torch.from_numpy(src.astype(np.float32)).to(dev),
                        torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(dev),
                        torch.from_numpy(spk.astype(np.int32)).to(dev)))
    trs = {}
    for name, kw in STEPS.items():
        kw = dict(kw)
        net = engine.SepNet(cell="lstm", num_layers=L, device=dev, seed=1, attention=kw.pop("attention"))
        trs[name] = engine.SepTrainer(net, B, K, N, mode="pit", **kw)
    out = {"shape": dict(cell="lstm", L=L, B=B, K=K, N=N, T=trs["dot_bf16"].T, mode="pit"), "rounds": a.rounds,
           "steps_per_round": a.steps, "attn_reps": a.reps}

    # ---- masked magnitude of the align forwards, same weights and batch, before any update
    preds = {}
    for name in ("align_fp32_fixed", "align_bf16", "align_bf16s"):
        tr = trs[name]
        raw, gains, spk = batches[0]
        tr.spk.copy_(spk)
        tr.features(raw, gains)
        tr.forward()
        preds[name] = torch.empty(B, K, tr.T * tr.F, device=dev)
        tr.attn(0, pred_out=preds[name])
    torch.cuda.synchronize()
    ref = preds["align_fp32_fixed"].double()
    out["masked_rel_l2_vs_fp32_align"] = {n: float((preds[n].double() - ref).norm() / ref.norm())
                                          for n in ("align_bf16", "align_bf16s")}
    del preds, ref

    # ---- step times: graph replay, alternating rounds
    for tr in trs.values():
        tr.step(*batches[0])
        tr.capture()
        for b in batches:
            tr.step_graph(*b)
        tr.check()
    ms = {n: [] for n in trs}
    for r in range(a.rounds):
        for name, tr in trs.items():
            b = batches[r % 2]
            ms[name].append(timed(lambda: [tr.step_graph(*b) for _ in range(a.steps)]) / a.steps)
    losses = {}
    for name, tr in trs.items():
        tr.check()
        losses[name] = float(tr.loss[0])
        out[name + "_step_ms"] = stats(ms[name], 3)
    out["loss_after"] = losses

    # ---- the attention launches, each by its own events, on the buffers the last step left
    launches = {}
    for name, tag in (("dot_bf16", "dot_bf16v"), ("align_bf16", "align_bf16v"), ("align_bf16s", "align_fp32v_bf16dpre")):
        tr = trs[name]
        launches[tag + "_cost"] = lambda tr=tr: tr.attn(0)
        launches[tag + "_grad"] = lambda tr=tr: tr.attn(1, tr.perm)
    for _ in range(3):
        for fn in launches.values():
            fn()
    torch.cuda.synchronize()
    us = {n: [] for n in launches}
    for _ in range(a.reps):
        for n, fn in launches.items():
            us[n].append(timed(fn) * 1e3)
    for n, ts in us.items():
        out[n + "_us"] = stats(ts)
    med = {n: statistics.median(ts) for n, ts in us.items()}
    x = (statistics.median(ms["align_bf16"]) - statistics.median(ms["dot_bf16"])) * 1e3
    y = med["align_bf16v_cost"] + med["align_bf16v_grad"] - med["dot_bf16v_cost"] - med["dot_bf16v_grad"]
    out["X_step_delta_us"], out["Y_attn_delta_us"] = round(x, 1), round(y, 1)
    out["X_over_Y"] = round(x / y, 3)
    out["X_le_1.25_Y"] = bool(x <= 1.25 * y)
    xs = (statistics.median(ms["align_bf16s"]) - statistics.median(ms["dot_bf16"])) * 1e3
    out["bf16s_step_minus_dot_bf16_us"] = round(xs, 1)
    out["mixtures_per_s"] = {n: round(B / (statistics.median(t) * 1e-3), 1) for n, t in ms.items()}
    line = json.dumps(out)
    print(line, flush=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
