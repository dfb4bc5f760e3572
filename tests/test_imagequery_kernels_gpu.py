"""The image-query encoder's kernels (csrc/imgq.hip) against the fp64 torch reference of tests/imagequery_ref.py.

Bar (imagequery_ref.case): the error of torch's own CPU fp32 run against the fp64 run on the same inputs, forward
and flat gradient each relative to the largest element, times 4, with a floor of one fp32 ulp of the largest
element.  Measured here at 28 x 28, E = 50: the fp32 run is off by 7e-8 .. 1.8e-7 (forward) and 4e-8 .. 1.1e-7
(gradient), so the bars are 2.8e-7 .. 7e-7 and 1.4e-7 .. 4.3e-7.

Inputs: synth.glyphs images (exact-zero background), conv biases non-zero and half positive, so every image has
tied positive windows and dead windows; seed 1 gives the same ReLU and pooling decisions in the fp32 and fp64
reference runs for every case (asserted before the GPU comparison)."""
import numpy as np
import pytest
import torch

import imagequery_ref as ir
from dl4ss_amd import ops
from dl4ss_amd.imagequery import ImageQueryEncoder, ImageQueryNet

pytestmark = pytest.mark.gpu
SEED = 1
SIZES = [(28, 28), (24, 24), (26, 37)]


def _net(case, size, E, dev):
    inet = ImageQueryNet(size, E, device=dev)
    for name, t in case["params"].items():
        assert tuple(inet.view(name).shape) == tuple(t.shape)
        inet.view(name).copy_(t)
    return inet


def _host_sum(dpart):
    """The documented order in fp32 (include/dl4ss_imgq.h, dl4ss_imgq_reduce): rows ascending, two sums of 2^l
    rows added (earlier + later) as soon as both exist, the rest folded from the latest rows back."""
    a = dpart.cpu().numpy()
    n, st = a.shape[0], {}
    for i in range(n):
        s, k, l = a[i], i + 1, 0
        while not k & 1:
            s = st.pop(l) + s
            k >>= 1
            l += 1
        st[l] = s
    total = None
    for l in sorted(st):
        total = st[l] if total is None else st[l] + total
    assert sorted(st) == [l for l in range(11) if (n >> l) & 1] and total.dtype == np.float32
    return torch.from_numpy(total)


@pytest.mark.parametrize("E", [50, 128])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n", [1, 3, 64, 65])
def test_forward_and_backward_against_fp64(dev, n, size, E):
    _check(dev, n, size, E)


@pytest.mark.parametrize("n, E", [(1, 128), (3, 50)])
def test_the_largest_image(dev, n, E):
    """48 x 48, the upper bound of the LDS plan: the launch with the largest dynamic LDS size (43 KB), and the
    only size here whose third stage has more than one pooled cell in both directions (16 x 4 x 4: D = 256), so
    that conv3's weight and data gradients walk several cells a channel.  The same checks and the same bar."""
    assert ir.stage_shapes(48, 48) == [(4, 22, 22), (8, 10, 10), (16, 4, 4)]
    _check(dev, n, (48, 48), E)


def _check(dev, n, size, E):
    c = ir.case(n, size, E, SEED)
    assert c["same_pattern"], "the fp32 and fp64 reference runs disagree on a ReLU sign or a pooling arg-max"
    dead = [float((~relu).float().mean()) for relu, _ in c["patterns"]]
    assert all(0.2 < d < 0.8 for d in dead), dead  # live and dead pre-activations in every stage
    inet = _net(c, size, E, dev)
    assert inet.num_params == ops.imgq_param_count(size[0], size[1], E)
    enc = ImageQueryEncoder(inet, n)
    images, dvec = c["images"].to(dev), c["dvec"].to(dev)
    nan = float("nan")
    enc.vec.fill_(nan)
    vec = enc.forward(images)
    assert not torch.isnan(vec).any()
    e_fwd = ir.rel_err(vec.cpu(), c["vec"])
    enc.dpart.fill_(nan)
    inet.grad.fill_(nan)
    g = enc.backward(dvec)
    assert g is inet.grad and not torch.isnan(g).any() and not torch.isnan(enc.dpart).any()
    assert (g[inet.num_params:] == 0).all() and (enc.dpart[:, inet.num_params:] == 0).all()  # the layout's padding
    got = torch.cat([inet.grad_view(k).reshape(-1) for k in ir.NAMES]).cpu()
    e_grad = ir.rel_err(got, c["flat_grad"])
    print(f"n={n} {size} E={E}: forward {e_fwd:.2e} (fp32 reference {c['err_fwd']:.2e}, bar {c['bar_fwd']:.2e}); "
          f"gradient {e_grad:.2e} (fp32 reference {c['err_grad']:.2e}, bar {c['bar_grad']:.2e})")
    assert e_fwd <= c["bar_fwd"]
    assert e_grad <= c["bar_grad"]
    # the same bits on a repeated call
    g1, d1 = g.clone(), enc.dpart.clone()
    inet.grad.fill_(nan)
    enc.dpart.fill_(nan)
    assert torch.equal(enc.backward(dvec), g1) and torch.equal(enc.dpart, d1)
    # the batch gradient is the fixed-order sum of the images' own rows, each as a single-image call gives it
    one = ImageQueryEncoder(inet, 1)
    rows = torch.empty_like(d1)
    for i in range(n):
        one.forward(images[i:i + 1])
        one.backward(dvec[i:i + 1])
        rows[i] = one.dpart[0]
        assert torch.equal(one.vec[0], vec[i])
    assert torch.equal(rows, d1)
    assert torch.equal(_host_sum(rows), g1.cpu())


def test_ties_and_dead_windows_follow_torch(dev):
    """Two flat images: every pre-activation of a window equals its neighbours', so every live window is a tie
    (gradient to element 0 of the window) and every other one is dead.  A wrong tie or ReLU rule moves whole
    gradient elements between filter taps (an error of the order of the elements themselves); rounding is below
    1e-6 of the largest element here (the cases above), so 1e-5 separates the two."""
    size, E, n = (28, 28), 50, 2
    c = ir.case(n, size, E, SEED)
    images = torch.zeros(n, *size)
    images[1] = 0.5
    v64, g64, _ = ir.run(images, c["params"], c["dvec"], torch.float64)
    inet = _net(c, size, E, dev)
    enc = ImageQueryEncoder(inet, n)
    vec = enc.forward(images.to(dev))
    enc.backward(c["dvec"].to(dev))
    got = torch.cat([inet.grad_view(k).reshape(-1) for k in ir.NAMES]).cpu()
    f64 = ir.flat(g64)
    assert float(f64[:1568].abs().max()) > 0  # the convolutions do get a gradient
    assert ir.rel_err(vec.cpu(), v64) <= 1e-5
    assert ir.rel_err(got, f64) <= 1e-5
    for k in ir.NAMES[:6]:  # and layer by layer, relative to the layer's own largest element
        assert ir.rel_err(inet.grad_view(k).cpu(), g64[k]) <= 1e-5, k


def test_wrappers_refuse_bad_arguments(dev):
    inet = ImageQueryNet((28, 28), 50, device=dev)
    with pytest.raises(ValueError):
        ImageQueryNet((23, 28), 50, device=dev)
    with pytest.raises(ValueError):
        ImageQueryNet((28, 49), 50, device=dev)
    with pytest.raises(ValueError):
        ImageQueryNet((28, 28), 129, device=dev)
    enc = ImageQueryEncoder(inet, 2)
    with pytest.raises(RuntimeError):
        enc.forward(torch.zeros(3, 28, 28, device=dev))
    with pytest.raises(RuntimeError):
        enc.backward(torch.zeros(2, 50, device=dev))  # no forward yet
    with pytest.raises(RuntimeError):
        ops.imgq_bwd(torch.zeros(2, 28, 28, device=dev), torch.zeros(2, 50, device=dev), inet.flat,
                     torch.zeros(2, 2000, device=dev))  # rows shorter than the parameter block
