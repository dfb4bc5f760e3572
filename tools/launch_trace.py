"""The ordered list of C-ABI launches of two eager SepTrainer (or ClassifierTrainer) step() calls, in a form two
trees can compare.

    python tools/launch_trace.py CASE out.json [--tree DIR]     record (DIR: the tree to import, default this one)
    python tools/launch_trace.py --compare a.json b.json        print the first difference, or "identical"
    python tools/launch_trace.py --list                         the case names

``_lib.call`` is wrapped (record, then forward); what is recorded is the bound positional tuple (``_lib.bind`` puts
keyword arguments into the prototype's order; a tree without it calls positionally, and its arguments are taken as
given), so records of both kinds of tree compare.  Integers and floats are recorded verbatim.  Every pointer --
also each element of a ctypes pointer array, so the GroupedGemm tables and the conversion / bias-reduce lists --
becomes (region, byte offset): a region is the torch storage that contains the address, numbered by first
appearance in the trace; the storages are found after the steps by walking the trainer's and the net's
attributes (tensors, lists, GroupedGemm objects) and the batch.  Stream handles are numbered the same way (the
default stream is the null handle).  The short entry points (dl4ss_birnn_fwd, _fwd_ex, _fwd_xw, _bwd) are
rewritten to their superset forms, padded with nulls where birnn.hip pads them, so that a tree that calls the
short forms and one that calls the supersets compare equal.  Uses only _lib.call, the public constructors (engine.SepNet
/ DiscNet / SepTrainer, the voiceprint and classifier modules) and synth, so the same file runs against an older
checkout (--tree).

Besides the calls a record holds ``digest``, the sha256 of every parameter buffer after the two steps (net.flat, and
where present the adversary's flat, the encoder's flat, memory.mem), and ``norms``, each step's grad_norm /
adv_grad_norm where the trainer clips.  --compare compares the digest for the cases of DIGEST_STABLE only: those
whose digest one tree reproduced in two runs of its own on the MI355X (the others add with float atomics)."""
import bisect
import ctypes
import hashlib
import json
import os
import sys

C2 = dict(B=32, N=32000, K=2, net=dict(cell="lstm", num_layers=4), tr=dict(mode="pit", precision="bf16"))
GRU2 = dict(cell="gru", num_layers=2, adjust=False)
LSTM2 = dict(cell="lstm", num_layers=2)
LSTM2_NOADJ = dict(LSTM2, adjust=False)


def small(net, K=2, **tr):
    return dict(B=4, N=8000, K=K, net=net, tr=tr)


CASES = {
    "c2": C2,
    "gru2_k3_pit_bf16": small(GRU2, K=3, mode="pit", precision="bf16"),
    "gru2_label_bf16s": small(GRU2, mode="label", precision="bf16s"),
    "gru2_label_bf16s2": small(GRU2, mode="label", precision="bf16s2"),
    "lstm2_label_fp32": small(dict(cell="lstm", num_layers=2), mode="label", precision="fp32"),
    "gru2_crm_bf16": small(dict(cell="gru", num_layers=2, crm=True), mode="crm", precision="bf16"),
    "gru2_crm_fp32": small(dict(cell="gru", num_layers=2, crm=True), mode="crm", precision="fp32"),
    "lstm2_align_fp32": small(dict(cell="lstm", num_layers=2, attention="align"), mode="label", precision="fp32"),
    "lstm6_bf16": small(dict(cell="lstm", num_layers=6), mode="pit", precision="bf16"),
    "lstm2_bf16_rnn_fp32": small(dict(cell="lstm", num_layers=2), mode="pit", precision="bf16", rnn_precision="fp32"),
    "c2_side0": dict(C2, env={"DL4SS_SIDE_DWLIN": "0"}),
    "c2_slabs0": dict(C2, env={"DL4SS_DH_SLABS": "0"}),
    # the optional optimizers (T = 63 frames, above the Discriminator's 15).  Clip thresholds: below the first
    # step's grad_norm as read on the tree this table was written against, so the clip is active -- the net 0.05
    # (norm 18.5, bf16 and fp32; 17.6 in 'pit'), the Discriminator 0.01 (grad_dis 0.74, grad_adv 2.05), the
    # classifier 0.01 (0.062); every record keeps its norms and coefficients ("norms")
    "lstm2_clip_bf16": small(LSTM2, mode="label", precision="bf16", clip_norm=0.05),
    "lstm2_clip_fp32": small(LSTM2, mode="label", precision="fp32", clip_norm=0.05),
    "lstm2_adv_bf16": dict(small(LSTM2, mode="label", precision="bf16"), adv={}),
    "lstm2_adv_fp32": dict(small(LSTM2, mode="label", precision="fp32"), adv={}),
    "lstm2_adv_dis_only_bf16": dict(small(LSTM2, mode="label", precision="bf16", disc_adv_update=False), adv={}),
    "lstm2_adv_clip_bf16": dict(small(LSTM2, mode="pit", precision="bf16", clip_norm=0.05, adv_clip_norm=0.01), adv={}),
    "lstm2_vp_reference_fp32": dict(small(LSTM2_NOADJ, mode="label", memory_refresh="reference"), vp={}),  # (fp32)
    "lstm2_vp_reuse_fp32": dict(small(LSTM2_NOADJ, mode="label", memory_refresh="reuse"), vp={}),
    "lstm2_vp_align_fp32": dict(small(dict(LSTM2_NOADJ, attention="align"), mode="label"), vp={}),
    # ClassifierTrainer at the smallest shape of its own tests (H = 40, two layers, B = 3, N = 3000)
    "cls_fp32": dict(B=3, N=3000, K=2, cls=dict(hidden=40, num_layers=2, num_labels=11), tr=dict(precision="fp32")),
    "cls_clip_fp32": dict(B=3, N=3000, K=2, cls=dict(hidden=40, num_layers=2, num_labels=11),
                          tr=dict(precision="fp32", clip_norm=0.01)),
}

# the cases whose parameter digest a tree reproduces run after run (measured: two records of one tree, MI355X).
# The others -- the fp32 'dot' steps and bf16 with an fp32 recurrence -- add split-K partial sums with float atomics
DIGEST_STABLE = ("c2", "c2_side0", "c2_slabs0", "gru2_k3_pit_bf16", "gru2_label_bf16s", "gru2_label_bf16s2",
                 "gru2_crm_bf16", "lstm2_align_fp32", "lstm6_bf16", "lstm2_clip_bf16", "lstm2_adv_bf16",
                 "lstm2_adv_dis_only_bf16", "lstm2_adv_clip_bf16", "lstm2_vp_align_fp32", "cls_fp32", "cls_clip_fp32")

# short entry point -> (superset, index at which birnn.hip inserts null pointers, how many)
SUPERSET = {"dl4ss_birnn_fwd": ("dl4ss_birnn_fwd_mean", 12, 3), "dl4ss_birnn_fwd_ex": ("dl4ss_birnn_fwd_mean", 14, 1),
            "dl4ss_birnn_fwd_xw": ("dl4ss_birnn_fwd_xw_ex", 18, 1), "dl4ss_birnn_bwd": ("dl4ss_birnn_bwd_ex", 13, 4)}


def raw(a):
    """One argument as recorded at call time: numbers verbatim, pointers tagged "p", arrays element-wise."""
    if isinstance(a, ctypes.Array):
        if a._type_ is ctypes.c_void_p:
            return ["pa"] + [("p", v) for v in a]
        return ["a"] + list(a)
    if isinstance(a, ctypes.c_void_p):
        return ("p", a.value)
    if a is None:
        return ("p", None)
    assert isinstance(a, (int, float)), type(a)
    return a


def storages(roots):
    """{base address: bytes} of every torch storage reachable from the roots through lists, tuples, dicts and
    the attributes of the package's own objects (the trainer, the net, GroupedGemm)."""
    import torch

    found, seen, todo = {}, set(), list(roots)
    while todo:
        o = todo.pop()
        if id(o) in seen:
            continue
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            s = o.untyped_storage()
            found[s.data_ptr()] = max(found.get(s.data_ptr(), 0), s.nbytes())
        elif isinstance(o, (list, tuple)):
            todo += o
        elif isinstance(o, dict):
            todo += o.values()
        elif type(o).__module__.startswith("dl4ss_amd") and hasattr(o, "__dict__"):
            todo += vars(o).values()
    return found


def normalise(trace, regions, streams):
    bases = sorted(regions)
    rnum, snum, unknown = {}, {}, {}

    def ptr(v):
        if v is None:
            return None
        i = bisect.bisect_right(bases, v) - 1
        if i >= 0 and v < bases[i] + max(regions[bases[i]], 1):
            return ["r", rnum.setdefault(bases[i], len(rnum)), v - bases[i]]
        if v in streams:
            return ["s", snum.setdefault(v, len(snum))]
        return ["?", unknown.setdefault(v, len(unknown))]

    def arg(a):
        if isinstance(a, tuple):
            return ptr(a[1])
        if isinstance(a, list):
            return [arg(x) for x in a[1:]]
        return a

    out = []
    for name, args in trace:
        args = [arg(a) for a in args]
        if name in SUPERSET:
            name, at, n = SUPERSET[name]
            args[at:at] = [None] * n
        out.append([name, args])
    return out, len(unknown)


def record(case, out, tree):
    sys.path.insert(0, tree)
    cfg = CASES[case]
    os.environ.update(cfg.get("env", {}))
    import numpy as np
    import torch

    from dl4ss_amd import _lib, engine, ops, synth

    dev = torch.device("cuda")
    B, K, N = cfg["B"], cfg["K"], cfg["N"]
    src, spk, u = synth.SyntheticMixtures(n_samples=N, k=K, seed=7).batch(B)
    batch = (torch.from_numpy(src.astype(np.float32)).to(dev),
             torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(dev),
             torch.from_numpy(spk.astype(np.int32)).to(dev))
    extra, kw = [], dict(cfg["tr"])
    if "cls" in cfg:
        from dl4ss_amd import classifier, infer

        net = infer.ClassifierNet(device=dev, seed=3, **cfg["cls"])
        tr = classifier.ClassifierTrainer(net, B, K, N, **kw)
        y = np.zeros((B, net.num_labels), np.float32)
        for b in range(B):
            y[b, np.asarray(spk[b]) % net.num_labels] = 1.0
        batch = batch[:2] + (torch.from_numpy(y).to(dev),)
    else:
        net = engine.SepNet(device=dev, seed=11, **cfg["net"])
        if "adv" in cfg:
            extra.append(engine.DiscNet(ops.n_frames(N), net.F, device=dev, seed=2))
            kw["adversary"] = extra[0]
        if "vp" in cfg:
            from dl4ss_amd import voiceprint

            extra += [voiceprint.VoiceprintNet(device=dev, seed=3), voiceprint.SpeakerMemory(101, 50, device=dev)]
            kw.update(voiceprint=extra[-2], memory=extra[-1])
        tr = engine.SepTrainer(net, B, K, N, **kw)
    trace, call, losses, norms = [], _lib.call, [], []

    bind = getattr(_lib, "bind", lambda name, args, kw: args)  # (an older tree: positional calls only)

    def recording_call(name, *args, **kw):
        args = bind(name, args, kw)
        trace.append((name, [raw(a) for a in args]))
        return call(name, *args)

    _lib.call = recording_call
    try:
        for _ in range(2):
            losses.append(float(tr.step(*batch)[0]))
            norms.append({n: getattr(tr, n).tolist() for n in ("grad_norm", "adv_grad_norm") if hasattr(tr, n)})
    finally:
        _lib.call = call
    tr.check()
    digest = hashlib.sha256()
    for t in [net.flat] + [o.mem if hasattr(o, "mem") else o.flat for o in extra]:
        digest.update(t.detach().cpu().numpy().tobytes())
    streams = {s.cuda_stream for s in (torch.cuda.current_stream(), getattr(tr, "_side_stream", None)) if s is not None}
    calls, unknown = normalise(trace, storages([tr, net, batch, extra, getattr(ops, "_gl_ws", {})]), streams)
    with open(out, "w") as f:
        json.dump(dict(case=case, losses=losses, norms=norms, digest=digest.hexdigest(), unresolved_pointers=unknown,
                       calls=calls), f)
    print(f"{case}: {len(calls)} calls, {unknown} unresolved pointers, losses {losses}, norms {norms}, "
          f"digest {digest.hexdigest()[:16]}")


def compare(a, b):
    x, y = json.load(open(a)), json.load(open(b))
    bad = [n for n, t in ((a, x), (b, y)) if t["unresolved_pointers"]]
    if bad:
        print(f"{x['case']}: unresolved pointers in {bad}: not comparable")
        return False
    for i, (p, q) in enumerate(zip(x["calls"], y["calls"])):
        if p != q:
            j = next((j for j, (s, t) in enumerate(zip(p[1], q[1])) if s != t), min(len(p[1]), len(q[1])))
            where = "entry point" if p[0] != q[0] else f"argument {j}"
            print(f"{x['case']}: call {i} differs ({where})\n  {a}: {p}\n  {b}: {q}")
            return False
    # (the first step's loss only: the fp32 step's split-K backward GEMMs add with float atomics, so its second
    # loss varies in the last bits from run to run of one tree)
    if len(x["calls"]) != len(y["calls"]) or x["losses"][:1] != y["losses"][:1]:
        print(f"{x['case']}: {len(x['calls'])} vs {len(y['calls'])} calls, losses {x['losses']} vs {y['losses']}")
        return False
    if x["case"] in DIGEST_STABLE and x.get("digest") != y.get("digest"):
        print(f"{x['case']}: the parameters after two steps differ (digest {x.get('digest')} vs {y.get('digest')})")
        return False
    print(f"{x['case']}: identical ({len(x['calls'])} calls"
          f"{', parameter digest' if x['case'] in DIGEST_STABLE else ''})")
    return True


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if sys.argv[1] == "--list":
        print("\n".join(CASES))
    elif sys.argv[1] == "--compare":
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    else:
        tree = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else here
        record(sys.argv[1], sys.argv[2], os.path.abspath(tree))  # (--compare refuses a trace with unresolved pointers)
