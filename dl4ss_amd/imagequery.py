"""Image-query encoder on the HIP path: the target is named by a picture.

The third tree of the model this code base descends from (``Multi_modal/software/DL4SS_Keras``) is the separation
model with one change: a small CNN over a 28 x 28 image (``nnet.py:70-89``) produces the vector that goes into
``SpkLifeLongMemory`` (``nnet.py:93-94``), in place of the voiceprint BiLSTM + ``MeanPool``.  Memory, attention,
loss and the enrolment of unseen targets are the voiceprint path's (``voiceprint.SpeakerMemory``).

The network (``include/dl4ss_imgq.h`` has the layout; torch conventions: cross-correlation, NCHW flatten, floor
pooling): conv 4 x 5x5, conv 8 x 3x3, conv 16 x 3x3, each valid + bias + ReLU + 2x2 max-pool, then
Linear(16 h3 w3, E).  One fused kernel per direction, one workgroup per image (``csrc/imgq.hip``); the backward
recomputes the forward from the image and writes one gradient row per image, summed pairwise in a fixed order
(``ops.imgq_reduce``), so a repeated call gives the same bits.  fp32, single GPU, eager launches.
"""
import math

import torch

from . import _lib, ops
from .params import FlatParams
from .voiceprint import MemoryQueryStep


class ImageQueryNet(FlatParams):
    """Parameters of the image-query CNN, flat fp32 under ``img.conv{1,2,3}.{weight,bias}`` and
    ``img.dense.{weight,bias}`` in the kernels' layout; ``grad`` is the flat gradient of the same layout
    (ImageQueryEncoder.backward writes it)."""

    def __init__(self, image_size=(28, 28), emb=50, device="cuda", seed=1):
        h, w = (int(x) for x in image_size)
        c = _lib.CONSTANTS
        lo, hi = c["DL4SS_IMGQ_MIN_HW"], c["DL4SS_IMGQ_MAX_HW"]
        if not (lo <= h <= hi and lo <= w <= hi):
            raise ValueError(f"ImageQueryNet: images of {h} x {w}, expected {lo} <= h, w <= {hi}")
        if not 1 <= emb <= c["DL4SS_IMGQ_MAX_E"]:
            raise ValueError(f"ImageQueryNet: 1 <= emb <= {c['DL4SS_IMGQ_MAX_E']}")
        self.h, self.w, self.E = h, w, int(emb)
        self.image_size = (h, w)
        dims = [(h - 4) // 2, (w - 4) // 2]
        for _ in range(2):
            dims = [(x - 2) // 2 for x in dims]
        self.D = 16 * dims[0] * dims[1]  # the dense layer's inputs
        self._allocate([("img.conv1.weight", (4, 1, 5, 5)), ("img.conv1.bias", (4,)),
                        ("img.conv2.weight", (8, 4, 3, 3)), ("img.conv2.bias", (8,)),
                        ("img.conv3.weight", (16, 8, 3, 3)), ("img.conv3.bias", (16,)),
                        ("img.dense.weight", (self.E, self.D)), ("img.dense.bias", (self.E,))], device)
        self.num_params = sum(math.prod(shape) for _, shape in self.specs)
        # the flat layout is the kernels' parameter block (every tensor but the last is a multiple of 4 floats)
        off = dict(conv1=("W1", "B1"), conv2=("W2", "B2"), conv3=("W3", "B3"))
        for name, (kw, kb) in off.items():
            assert self.offsets[f"img.{name}.weight"][0] == c[f"DL4SS_IMGQ_OFF_{kw}"]
            assert self.offsets[f"img.{name}.bias"][0] == c[f"DL4SS_IMGQ_OFF_{kb}"]
        assert self.offsets["img.dense.weight"][0] == c["DL4SS_IMGQ_OFF_WD"]
        assert self.offsets["img.dense.bias"][0] == c["DL4SS_IMGQ_OFF_WD"] + self.E * self.D
        self.grad = torch.zeros_like(self.flat)
        self.reset_parameters(seed)

    def named_parameters(self):
        for name, _ in self.specs:
            yield name, self.view(name)

    def grad_view(self, name):
        return self.view(name, self.grad)

    def reset_parameters(self, seed=1):
        """Keras 1's defaults in torch's terms: Glorot-uniform conv weights (fan_in = C_in k k, fan_out =
        C_out k k), dense weights N(0, 0.05) (``init='normal'``), every bias zero."""
        g = torch.Generator().manual_seed(seed)
        for name, shape in self.specs:
            if name.endswith("bias"):
                t = torch.zeros(shape)
            elif name == "img.dense.weight":
                t = torch.randn(shape, generator=g) * 0.05
            else:
                k = math.sqrt(6.0 / ((shape[0] + shape[1]) * shape[2] * shape[3]))
                t = torch.empty(shape).uniform_(-k, k, generator=g)
            self.view(name).copy_(t)


class ImageQueryEncoder:
    """Buffers and launches of the encoder for n images: ``forward`` one launch, ``backward`` the per-image
    gradient rows ``dpart`` (n, numel) and their fixed-order pairwise column sum into ``net.grad``
    (``ops.imgq_reduce``; ``ops.vp_colsum`` would take n x numel too, but adds the rows serially: at n = 64 its
    rounding alone measured 2 - 4e-7 of the largest element, against 1e-7 for a single row)."""

    def __init__(self, inet, n):
        if not isinstance(inet, ImageQueryNet):
            raise ValueError("ImageQueryEncoder: expected an ImageQueryNet")
        n_max = _lib.CONSTANTS["DL4SS_IMGQ_MAX_N"]
        if not 1 <= n <= n_max:
            raise ValueError(f"ImageQueryEncoder: 1 <= n <= {n_max}")
        self.net, self.n = inet, int(n)
        f32 = dict(device=inet.device, dtype=torch.float32)
        self.vec = torch.empty(n, inet.E, **f32)
        self.dpart = torch.empty(n, inet.numel, **f32)
        self.images = None

    def forward(self, images):
        """images (n, h, w) -> vec (n, E) (a buffer the next call reuses).  The images are kept by reference for
        ``backward``, which recomputes the forward from them."""
        net = self.net
        if tuple(images.shape) != (self.n, net.h, net.w):
            raise RuntimeError(f"ImageQueryEncoder: images {tuple(images.shape)}, expected {(self.n, net.h, net.w)}")
        self.images = images
        return ops.imgq_fwd(images, net.flat, net.E, vec=self.vec)

    def backward(self, dvec):
        """dvec (n, E) -> net.grad, every element written (of the forward this follows)."""
        if self.images is None:
            raise RuntimeError("ImageQueryEncoder: backward() follows forward()")
        ops.imgq_bwd(self.images, dvec, self.net.flat, self.dpart)
        return ops.imgq_reduce(self.dpart, self.net.grad)

    def check(self):
        """(No recurrence, no hand-off: nothing can time out.)"""
        torch.cuda.synchronize()


class ImageQueryStep(MemoryQueryStep):
    """The image queries of a training step (SepTrainer(image_query=, memory=)): the encoder over the step's images
    (B, K, h, w), the memory, the encoder's guarded Adam and the memory refresh (voiceprint.MemoryQueryStep)."""

    def __init__(self, inet, memory, refresh, images, spk, q, dq, status, loss, lr, betas, eps, opt_kw=None):
        B, K, h, w = images.shape
        self.maps = images.view(B * K, h, w)
        super().__init__(inet, memory, refresh, ImageQueryEncoder(inet, B * K), spk, q, dq, status, loss, lr, betas,
                         eps, opt_kw)

    def encoder_input(self):
        return self.maps

    def guard(self):
        """Refuse a step whose loss is not finite (on device, in front of the first optimizer)."""
        ops.imgq_guard(self.opt.loss, self.status)
