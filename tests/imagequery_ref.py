"""Reference of the image-query encoder (dl4ss_amd/imagequery.py, csrc/imgq.hip): the network restated with
torch on the CPU (F.conv2d, relu, F.max_pool2d, F.linear; autograd for the gradients), run in fp64 as the
reference and in fp32 to measure what fp32 arithmetic alone costs on the same inputs.  Shared by
test_imagequery_ref_cpu.py and the GPU tests; the memory arithmetic is tests/voiceprint_ref.py's.

The bar of the kernel tests is not a constant: ``case()`` measures the error of the fp32 run against the fp64
run (each relative to the largest element of the fp64 result); the kernel is allowed 4x that (a different but
fixed summation order over dot products of at most 72 terms, and the n-row reduce), with a floor of one fp32 ulp
of the largest element.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from dl4ss_amd import synth

NAMES = ("img.conv1.weight", "img.conv1.bias", "img.conv2.weight", "img.conv2.bias", "img.conv3.weight",
         "img.conv3.bias", "img.dense.weight", "img.dense.bias")


def stage_shapes(h, w):
    """[(C, H, W)] after each of the three conv + pool stages."""
    out = []
    for c, k in ((4, 5), (8, 3), (16, 3)):
        h, w = (h - k + 1) // 2, (w - k + 1) // 2
        out.append((c, h, w))
    return out


def param_shapes(h, w, E):
    c3, h3, w3 = stage_shapes(h, w)[-1]
    return {"img.conv1.weight": (4, 1, 5, 5), "img.conv1.bias": (4,), "img.conv2.weight": (8, 4, 3, 3),
            "img.conv2.bias": (8,), "img.conv3.weight": (16, 8, 3, 3), "img.conv3.bias": (16,),
            "img.dense.weight": (E, c3 * h3 * w3), "img.dense.bias": (E,)}


def forward(images, params, keep=None):
    """images (n, h, w), params {name: tensor} -> vec (n, E).  ``keep`` (a list): gets each stage's
    (pre-activation, pooling indices)."""
    x = images[:, None]
    for i in (1, 2, 3):
        z = F.conv2d(x, params[f"img.conv{i}.weight"], params[f"img.conv{i}.bias"])
        x, idx = F.max_pool2d(F.relu(z), 2, return_indices=True)
        if keep is not None:
            keep.append((z.detach(), idx.detach()))
    return F.linear(x.flatten(1), params["img.dense.weight"], params["img.dense.bias"])


def run(images, params, dvec, dtype):
    """(vec, {name: gradient of sum(vec * dvec)}, [(relu sign pattern, pooling arg-max)] per stage) in ``dtype``."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    keep = []
    vec = forward(images.to(dtype), p, keep)
    (vec * dvec.to(dtype)).sum().backward()
    return vec.detach(), {k: v.grad for k, v in p.items()}, [(z > 0, idx) for z, idx in keep]


def flat(grads):
    return torch.cat([grads[k].reshape(-1) for k in NAMES])


def make_inputs(n, size, E, seed):
    """Glyph images (exact-zero flat background) of random classes, Glorot conv weights, conv biases non-zero
    with half of each layer's positive (flat regions then give tied positive windows and dead windows in the
    same image), dense N(0, 0.05), and an upstream gradient."""
    rng = np.random.default_rng(seed)
    gl = synth.glyphs(10, size, seed=seed)
    images = torch.from_numpy(gl.draw(rng.integers(0, 10, size=n), rng))
    g = torch.Generator().manual_seed(seed)
    params = {}
    for name, shape in param_shapes(size[0], size[1], E).items():
        if name.endswith("conv1.bias") or name.endswith("conv2.bias") or name.endswith("conv3.bias"):
            sign = torch.ones(shape[0])
            sign[torch.randperm(shape[0], generator=g)[:shape[0] // 2]] = -1.0
            t = sign * torch.empty(shape).uniform_(0.02, 0.1, generator=g)
        elif name == "img.dense.bias":
            t = torch.empty(shape).uniform_(-0.05, 0.05, generator=g)
        elif name == "img.dense.weight":
            t = torch.randn(shape, generator=g) * 0.05
        else:
            k = math.sqrt(6.0 / ((shape[0] + shape[1]) * shape[2] * shape[3]))
            t = torch.empty(shape).uniform_(-k, k, generator=g)
        params[name] = t
    dvec = torch.randn(n, E, generator=g)
    return images, params, dvec


def rel_err(a, ref):
    return float((a.double() - ref.double()).abs().max()) / float(ref.double().abs().max())


def ulp_floor(ref):
    """One fp32 ulp of the largest element, relative to it."""
    m = float(ref.double().abs().max())
    return float(np.spacing(np.float32(m))) / m


@functools.lru_cache(maxsize=None)
def case(n, size, E, seed):
    """Everything a kernel test needs for one case, computed once: inputs, the fp64 results, the fp32 run's
    errors against them, the two bars, and whether the fp32 and fp64 runs took the same ReLU and pooling
    decisions everywhere (``same_pattern``: without it a near-tie makes a gradient comparison meaningless)."""
    images, params, dvec = make_inputs(n, size, E, seed)
    v64, g64, p64 = run(images, params, dvec, torch.float64)
    v32, g32, p32 = run(images, params, dvec, torch.float32)
    same = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(p32, p64))
    f64 = flat(g64)
    e_fwd, e_grad = rel_err(v32, v64), rel_err(flat(g32), f64)
    return dict(images=images, params=params, dvec=dvec, vec=v64, grads=g64, flat_grad=f64, same_pattern=same,
                err_fwd=e_fwd, err_grad=e_grad, bar_fwd=max(4 * e_fwd, ulp_floor(v64)),
                bar_grad=max(4 * e_grad, ulp_floor(f64)), patterns=p64)


def idx_bytes(images_u8, labels_u8):
    """The IDX image and label files' bytes for (N, h, w) uint8 images and (N) uint8 labels."""
    n, h, w = images_u8.shape
    head = np.array([0x00000803, n, h, w], dtype=">u4").tobytes()
    lhead = np.array([0x00000801, labels_u8.shape[0]], dtype=">u4").tobytes()
    return head + images_u8.tobytes(), lhead + labels_u8.tobytes()
