"""ATTENTION 'align' on the bf16 training steps (SepTrainer, precision "bf16" / "bf16s"), at the small bf16 step
shape of tests/test_step_gpu.py: BiLSTM-2L, B = 4, K = 2, N = 8000.

  * parity with the fp32 align step on the same weights and batch, label and pit, at the bounds
    tests/test_step_gpu.py::test_step_bilstm_bf16 applies to the small bf16 'dot' step: loss 1e-2 relative, masked
    magnitude 1e-2 rel-L2, every gradient within 5e-2 of its tensor's largest element (att.Linear_1/2/3.weight and
    the embedding rows included).  Every figure is printed before it is asserted.
  * the attention weights train; two trainers built alike agree bit for bit after three steps; step_graph() equals
    step() bit for bit; optimizer="nadam" with clipnorm; a world-size-1 RCCL group with the default buckets is
    bitwise the single-GPU step;
  * a 'dot' net in bf16 makes the library calls it made before 'align' reached the bf16 steps, and repeats bit for
    bit."""
import collections
import functools
import socket

import numpy as np
import pytest
import torch

from dl4ss_amd import _lib, engine, synth

pytestmark = pytest.mark.gpu
B, K, N, L = 4, 2, 8000, 2
ATT = ("att.Linear_1.weight", "att.Linear_2.weight", "att.Linear_3.weight")


@functools.lru_cache(maxsize=None)
def _batches(dev, n=3, seed=5):
    gen = synth.SyntheticMixtures(n_samples=N, k=K, seed=seed)
    out = []
    for _ in range(n):
        src, spk, u = gen.batch(B)
        out.append((torch.from_numpy(src.astype(np.float32)).to(dev),
                    torch.from_numpy(synth.gains_for(u, K).astype(np.float32)).to(dev),
                    torch.from_numpy(spk.astype(np.int32)).to(dev)))
    return tuple(out)


def _trainer(dev, precision, mode="pit", attention="align", **kw):
    net = engine.SepNet(cell="lstm", num_layers=L, device=dev, seed=7, attention=attention)
    return engine.SepTrainer(net, B, K, N, mode=mode, precision=precision, **kw)


@functools.lru_cache(maxsize=None)
def _grad_pass(dev, precision, mode, attention="align"):
    """Loss, masked magnitudes (the COST pass's predictions) and every gradient of one batch, on the host."""
    tr = _trainer(dev, precision, mode, attention)
    raw, gains, spk = _batches(dev)[0]
    tr.spk.copy_(spk)
    tr.features(raw, gains)
    tr.forward()
    pred = torch.empty(B, K, tr.T * tr.F, device=dev)
    tr.attn(0, pred_out=pred)
    loss = tr.loss_and_grad()
    tr.backward()
    tr.check()
    net = tr.net
    return dict(loss=float(loss[0]), pred=pred.double().cpu(), perm=tr.perm.cpu().clone(),
                grads={name: net.view(name, net.grad).double().cpu() for name, _ in net.specs})


def _errors(got, ref):
    errs = {"loss": abs(got["loss"] - ref["loss"]) / abs(ref["loss"]),
            "masked": float((got["pred"] - ref["pred"]).norm() / ref["pred"].norm())}
    for name, g in ref["grads"].items():
        errs[name] = float((got["grads"][name] - g).abs().max() / g.abs().max())
    return errs


@pytest.mark.parametrize("mode", ["label", "pit"])
@pytest.mark.parametrize("precision", ["bf16", "bf16s"])
def test_align_bf16_step_matches_the_fp32_align_step(dev, precision, mode):
    ref, got = _grad_pass(dev, "fp32", mode), _grad_pass(dev, precision, mode)
    errs = _errors(got, ref)
    print("align step", precision, mode, {k: f"{v:.3e}" for k, v in errs.items()})
    if mode == "pit":
        assert torch.equal(got["perm"], ref["perm"])
    assert set(ATT) | {"emb.layer.weight"} <= set(errs)
    assert all(float(ref["grads"][n].abs().max()) > 0 for n in ATT)
    assert errs["loss"] < 1e-2 and errs["masked"] < 1e-2, errs
    bad = {k: v for k, v in errs.items() if k not in ("loss", "masked") and not v <= 5e-2}
    assert not bad, (bad, errs)


def _state(tr):
    torch.cuda.synchronize()
    return dict(flat=tr.net.flat.clone(), m=tr.m.clone(), v=tr.v.clone(), grad=tr.net.grad_ext.clone(),
                loss=tr.loss.clone(), wb=[w.clone() for w in tr.wb_ih + [tr.wb_lin]])


def _steps(dev, precision, graph=False, n=3, **kw):
    """n steps (graph: the first eager, as capture() asks, the rest replayed); the trainer and its final state."""
    tr = _trainer(dev, precision, **kw)
    losses = []
    for i, b in enumerate(_batches(dev)[:n]):
        losses.append((tr.step_graph(*b) if (graph and i > 0) else tr.step(*b)).clone())
    tr.check()
    return tr, dict(_state(tr), losses=torch.stack(losses))


def _assert_same(a, b):
    for k in ("flat", "m", "v", "grad", "loss", "losses"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    for i, (x, y) in enumerate(zip(a["wb"], b["wb"])):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), i


@pytest.mark.parametrize("precision", ["bf16", "bf16s"])
def test_align_bf16_step_trains_repeats_and_replays(dev, precision):
    """After three steps the three attention weights have moved and the loss is finite; a second trainer built
    alike ends in the same bits; so does one that replays steps two and three from its captured graph."""
    init = _trainer(dev, precision).net
    tr, a = _steps(dev, precision)
    assert tr.fast and tr.zero_free and tr.align and tr.step_count == 3
    assert bool(torch.isfinite(a["losses"]).all())
    for name in ATT:
        assert not torch.equal(tr.net.view(name), init.view(name)), name
        g = tr.net.view(name, tr.net.grad)
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    _assert_same(a, _steps(dev, precision)[1])
    trg, g = _steps(dev, precision, graph=True)
    assert trg.graph is not None
    _assert_same(a, g)


def test_align_bf16_step_label_order_replays(dev):
    a, g = _steps(dev, "bf16", mode="label")[1], _steps(dev, "bf16", graph=True, mode="label")[1]
    _assert_same(a, g)


def test_align_bf16_step_with_nadam_and_clipnorm(dev):
    """Keras's optimizer on the align net's bf16 step: runs, repeats bit for bit, check() is clean, and the norm
    (over the whole flat gradient, the attention weights' included) is finite and was clipped or measured."""
    kw = dict(optimizer="nadam", clipnorm=200.0)
    tr, a = _steps(dev, "bf16", **kw)
    assert tr.skipped_nonfinite == 0 and tr.step_count == 3 and tr.status.tolist() == [0, 0]
    nrm, c = tr.grad_norm.tolist()
    assert np.isfinite(nrm) and nrm > 0 and 0 < c <= 1
    host = float(tr.net.grad.double().norm())
    assert abs(host - nrm) <= 1e-5 * host
    _assert_same(a, _steps(dev, "bf16", **kw)[1])
    _assert_same(a, _steps(dev, "bf16", graph=True, **kw)[1])
    plain = _steps(dev, "bf16")[1]
    assert not torch.equal(plain["flat"], a["flat"])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def pg(dev):
    import torch.distributed as dist

    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", device_id=dev, init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0,
                            world_size=1)
    yield dist.group.WORLD
    dist.destroy_process_group()


@pytest.mark.parametrize("precision", ["bf16", "bf16s"])
def test_align_bf16_step_data_parallel_world1_is_the_single_gpu_step(dev, pg, precision):
    """World 1 over RCCL (the all-reduce is an identity), the default buckets: the three attention weights leave
    with the Linear, the embedding and ADDJUST, in the range behind SepNet.bucket_split()."""
    single = _steps(dev, precision)[1]
    for graph in (False, True):
        tr, dp = _steps(dev, precision, graph=graph, process_group=pg)
        assert tr.buckets and tr.dp_layer is None
        assert all(4 + tr.net.offsets[n][0] >= tr.net.bucket_split() for n in ATT)
        _assert_same(single, dp)


# one step of a bf16 'dot' trainer at this shape (BiLSTM-2L, pit), by entry point: the calls the tree made before
# 'align' reached the bf16 steps
DOT_CALLS = {"dl4ss_mix_sources_rot": 1, "dl4ss_stft_fwd_ex": 1, "dl4ss_birnn_fwd_xw_ex": 2, "dl4ss_gemm_bf16_gl": 3,
             "dl4ss_query_fwd": 1, "dl4ss_mask_attn_loss_bf16v": 2, "dl4ss_pit_select": 1, "dl4ss_loss_finalize": 1,
             "dl4ss_query_bwd_ex": 1, "dl4ss_birnn_bwd_ex": 2, "dl4ss_birnn_bias_reduce_ex": 1,
             "dl4ss_gemm_bf16_gl_grouped_ex": 1, "dl4ss_gemm_bf16_gl_grouped": 1,
             "dl4ss_adam_guarded_dp_scaled_bf16": 1}  # 19 calls


def test_dot_bf16_step_is_unchanged(dev, monkeypatch):
    """A 'dot' net in bf16: no align entry point is called, the step makes the library calls it made before, and a
    second identical trainer ends in the same bits."""
    calls = collections.Counter()
    real = _lib.call

    def counting(name, *args, **kw):
        calls[name] += 1
        return real(name, *args, **kw)

    tr = _trainer(dev, "bf16", attention="dot")
    batches = _batches(dev)
    tr.step(*batches[0])  # (the first step also builds the grouped launches and converts the weights)
    monkeypatch.setattr(_lib, "call", counting)
    tr.step(*batches[1])
    monkeypatch.setattr(_lib, "call", real)
    tr.check()
    print("dot bf16 step calls", sum(calls.values()), sorted(calls.items()))
    assert not any("align" in name for name in calls)
    assert dict(calls) == DOT_CALLS, sorted(calls.items())
    a, b = _steps(dev, "bf16", attention="dot")[1], _steps(dev, "bf16", attention="dot")[1]
    _assert_same(a, b)
