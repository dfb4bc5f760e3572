"""Golden fixture of the reference's own speaker-classifier training step (run where the reference tree
is available: ``python tests/golden/make_ref_classifier_fixture.py``; ``$DL4SS_REFERENCE``).

Like ``make_ref_align_fixture.py`` this reads the py2 file as text and translates it in memory with
``lib2to3`` (``make_ref_fixtures`` helpers; the file as a whole does not parse, so by line range):
``MIX_SPEECH_classifier`` (Torch_multi/test_multi_labels_speech.py:235-273) and ``count_multi_acc``
(:300-351) are taken out by AST, and the optimizer / loss / backward / step statements of ``main`` (:389-397,
:437, :443-445) are run as they stand, on torch-CPU fp32 at a small size: HIDDEN_UNITS = 8 (H = 16),
3 layers, (B, T, F) = (3, 6, 129), N_lab = 7.  Nothing of the reference is written into the repository:
only data goes into ``tests/golden/ref_cls_train.npz``:

    in/mix_feas (B,T,F), in/y_map (B,N_lab), in/y_spk (B,2), weight/<name> (initial state_dict),
    out/prob (B,N_lab), out/loss, grad/<name>, param/<name> (after the one Adam step, lr 1e-5),
    acc/top2 and acc/thr: count_multi_acc(prob, y_spk, alpha=-0.1, top_k_num=2) and
    (..., alpha=0.5, top_k_num=0) as 5 float64 each
"""
import ast
import os
import warnings

import numpy as np
import torch

import make_ref_fixtures as mr

HERE = os.path.dirname(os.path.abspath(__file__))
REL = "Torch_multi/test_multi_labels_speech.py"


def statements(rel, ranges):
    """The statements at the given reference line ranges (inside main()), dedented and translated."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from lib2to3 import refactor

        tool = refactor.RefactoringTool(refactor.get_fixers_from_package("lib2to3.fixes"))
    with open(os.path.join(mr.REF, rel), encoding="utf-8") as f:
        lines = f.read().splitlines()
    body = []
    for a, b in ranges:
        chunk = [l for l in lines[a - 1:b] if l.strip()]
        ind = min(len(l) - len(l.lstrip()) for l in chunk)
        tree = ast.parse(str(tool.refactor_string("\n".join(l[ind:] for l in chunk) + "\n", rel)), rel)
        body += [s for s in tree.body if not mr._is_logging(s)]
    return compile(ast.Module(body=body, type_ignores=[]), os.path.join(mr.REF, rel), "exec")


def check(rel, n, text):
    with open(os.path.join(mr.REF, rel), encoding="utf-8") as f:
        got = f.read().splitlines()[n - 1].replace(" ", "")
    assert text.replace(" ", "") in got, (rel, n, got)


def main(B=3, T=6, F=129, n_lab=7, hidden_units=8, seed=31):
    for n, t in [(242, "hidden_size=config.HIDDEN_UNITS*2"), (243, "num_layers=3"), (263, "out=F.sigmoid(self.Linear(x))"),
                 (395, "], lr=0.00001)"), (397, "loss_func = torch.nn.MultiLabelSoftMarginLoss()"),
                 (437, "loss=loss_func(mix_speech,y_map)"), (443, "optimizer.zero_grad()"),
                 (444, "loss.backward()"), (445, "optimizer.step()")]:
        check(REL, n, t)
    ns = mr.base_namespace(mr.make_config(HIDDEN_UNITS=hidden_units, BATCH_SIZE=B))
    exec(mr.snippet_defs(REL, 235, 273, ["MIX_SPEECH_classifier"]), ns)
    exec(mr.snippet_defs(REL, 300, 351, ["count_multi_acc"]), ns)
    torch.manual_seed(seed)
    r = np.random.Generator(np.random.PCG64(seed))
    mix_feas = np.abs(r.normal(0.0, 1.0, size=(B, T, F))).astype(np.float32)
    y_spk = [sorted(r.choice(n_lab, size=2, replace=False).tolist()) for _ in range(B)]
    y_map = np.zeros((B, n_lab), np.float32)
    for b, line in enumerate(y_spk):
        y_map[b, line] = 1
    out = {}
    with mr.cpu_cuda():
        net = ns["MIX_SPEECH_classifier"](F, T, n_lab)
        for k, v in net.state_dict().items():
            out[f"weight/{k}"] = v.detach().numpy().copy()
        ns.update(mix_speech_class=net)
        exec(statements(REL, [(389, 397)]), ns)  # optimizer (Adam, lr 1e-5) and loss_func
        ns.update(mix_speech=net(torch.from_numpy(mix_feas)), y_map=torch.from_numpy(y_map))
        exec(statements(REL, [(437, 437), (443, 445)]), ns)  # loss, zero_grad, backward, step
    prob = ns["mix_speech"].detach().numpy()
    out.update({"in/mix_feas": mix_feas, "in/y_map": y_map, "in/y_spk": np.array(y_spk, np.int64),
                "out/prob": prob, "out/loss": np.float64(ns["loss"].item())})
    for k, p in net.named_parameters():
        out[f"grad/{k}"] = p.grad.detach().numpy().copy()
        out[f"param/{k}"] = p.detach().numpy().copy()
    import contextlib
    import io

    with contextlib.redirect_stdout(io.StringIO()):  # the function prints its top-k lists
        top2 = ns["count_multi_acc"](prob.copy(), [list(l) for l in y_spk], alpha=-0.1, top_k_num=2)
        thr = ns["count_multi_acc"](prob.copy(), [list(l) for l in y_spk], alpha=0.5, top_k_num=0)
    out["acc/top2"] = np.array(top2, np.float64)
    out["acc/thr"] = np.array(thr, np.float64)
    mr.meta(out, B=B, T=T, F=F, n_lab=n_lab, hidden=2 * hidden_units, layers=3, lr=1e-5, seed=seed,
            source=f"{REL}:235-273,300-351,389-397,437,443-445")
    path = os.path.join(HERE, "ref_cls_train.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; loss", out["out/loss"], "top2", top2, "thr", thr)


if __name__ == "__main__":
    main()
