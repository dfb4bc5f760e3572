"""Golden fixture of the reference's own Discriminator and its loss lines (run where the reference tree is
available: ``python tests/golden/make_ref_dis_fixture.py``; ``$DL4SS_REFERENCE``).

Like ``make_ref_classifier_fixture.py`` this reads the py2 file as text and translates it in memory with
``lib2to3``: the ``Discriminator`` class (TDAA_beta/main_run_sstune_dis.py:318-336) is taken out by AST with
its two ``print`` statements dropped, and the statements :615-616 (the two scores), :622-624 (loss_dis) and
:642 (the generator's "fake looks real" term) are run as they stand on torch-CPU fp32 at the reference's own
map size (bs, topk, len, fre) = (1, 2, 313, 129).  Inputs and weights come from the seeded numpy recipe
``disc_ref.fixture_recipe`` that the tests regenerate; they are not stored.  Nothing of the reference is
written into the repository: only data goes into ``tests/golden/ref_dis.npz``:

    score/true, score/false (2, 1); loss/dis_true, loss/dis_false, loss/dis, loss/adv;
    for each gradient -- of loss_dis by the eight parameters (``grad/<key>``) and by the predicted maps
    (``grad/dis_dpred``), of the :642 term by the predicted maps (``grad/adv_dpred``) -- its sum, its L2 norm
    and a seeded 512-element sample (``disc_ref.sample_index``)
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import disc_ref as R  # noqa: E402
import make_ref_classifier_fixture as mc  # noqa: E402
import make_ref_fixtures as mr  # noqa: E402

REL = "TDAA_beta/main_run_sstune_dis.py"


class _DropPrints(ast.NodeTransformer):
    def visit_Expr(self, node):
        return None if mr._is_logging(node) else node


def discriminator_class(ns):
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from lib2to3 import refactor

        tool = refactor.RefactoringTool(refactor.get_fixers_from_package("lib2to3.fixes"))
    with open(os.path.join(mr.REF, REL), encoding="utf-8") as f:
        lines = f.read().splitlines()[318 - 1:336]
    tree = ast.parse(str(tool.refactor_string("\n".join(lines) + "\n", REL)), REL)
    keep = [_DropPrints().visit(n) for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Discriminator"]
    assert len(keep) == 1
    exec(compile(ast.fix_missing_locations(ast.Module(body=keep, type_ignores=[])), os.path.join(mr.REF, REL), "exec"),
         ns)
    return ns["Discriminator"]


def stats(out, name, g):
    g = g.detach().numpy().astype(np.float64).reshape(-1)
    out[f"grad/{name}/sum"] = np.float64(g.sum())
    out[f"grad/{name}/norm"] = np.float64(np.linalg.norm(g))
    out[f"grad/{name}/sample"] = g[R.sample_index(name, g.size)].astype(np.float32)


def main():
    for n, t in [(324, "self.final=nn.Linear(36480,1)"), (615, "score_true=dis_layer(y_multi_map)"),
                 (616, "score_false=dis_layer(predict_multi_map)"),
                 (622, "loss_dis_true=loss_dis_class(score_true,"), (623, "loss_dis_false=loss_dis_class(score_false,"),
                 (624, "loss_dis=loss_dis_true+loss_dis_false"), (642, "loss_dis_false=loss_dis_class(score_false,")]:
        mc.check(REL, n, t)
    bs, topk, T, F = R.FIXTURE_SHAPE
    ns = mr.base_namespace(mr.make_config(BATCH_SIZE=bs))
    W, y_true, pred = R.fixture_recipe()
    out = {}
    with mr.cpu_cuda():
        dis = discriminator_class(ns)()
        dis.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
        predict = torch.from_numpy(pred).requires_grad_(True)
        ns.update(dis_layer=dis, y_multi_map=torch.from_numpy(y_true), predict_multi_map=predict, top_k_num=topk,
                  loss_dis_class=torch.nn.MSELoss())
        exec(mc.statements(REL, [(615, 616), (622, 624)]), ns)
        loss_dis, l_true, l_false = ns["loss_dis"], ns["loss_dis_true"], ns["loss_dis_false"]
        exec(mc.statements(REL, [(642, 642)]), ns)
        loss_adv = ns["loss_dis_false"]
    params = dict(dis.named_parameters())
    g = torch.autograd.grad(loss_dis, list(params.values()) + [predict], retain_graph=True)
    for k, v in zip(list(params) + ["dis_dpred"], g):
        stats(out, k, v)
    stats(out, "adv_dpred", torch.autograd.grad(loss_adv, predict)[0])
    out.update({"score/true": ns["score_true"].detach().numpy(), "score/false": ns["score_false"].detach().numpy(),
                "loss/dis_true": np.float64(l_true.item()), "loss/dis_false": np.float64(l_false.item()),
                "loss/dis": np.float64(loss_dis.item()), "loss/adv": np.float64(loss_adv.item())})
    mr.meta(out, shape=R.FIXTURE_SHAPE, seed=R.FIXTURE_SEED, source=f"{REL}:318-336,615-616,622-624,642")
    path = os.path.join(HERE, "ref_dis.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; scores", out["score/true"].ravel(), out["score/false"].ravel(),
          "losses", out["loss/dis"], out["loss/adv"])


if __name__ == "__main__":
    main()
