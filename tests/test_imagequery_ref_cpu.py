"""The image-query reference of tests/imagequery_ref.py, checked without a GPU: its shapes at the three sizes the
kernel tests use, and the two gradient rules of torch the kernel copies -- pinned here, so that a torch that
changed them fails on the CPU and not as a kernel mismatch on the GPU."""
import pytest
import torch
import torch.nn.functional as F

import imagequery_ref as ir


@pytest.mark.parametrize("size, stages, dense_in", [
    ((28, 28), [(4, 12, 12), (8, 5, 5), (16, 1, 1)], 16),
    ((24, 24), [(4, 10, 10), (8, 4, 4), (16, 1, 1)], 16),  # the minimum: every stage keeps one cell
    ((26, 37), [(4, 11, 16), (8, 4, 7), (16, 1, 2)], 32),  # non-square, floor pooling drops a row and a column
])
def test_shapes(size, stages, dense_in):
    assert ir.stage_shapes(*size) == stages
    shapes = ir.param_shapes(size[0], size[1], 50)
    assert shapes["img.dense.weight"] == (50, dense_in)
    images, params, dvec = ir.make_inputs(3, size, 50, seed=1)
    assert images.shape == (3, *size) and images.dtype == torch.float32
    assert float(images.min()) == 0.0 and float(images.max()) <= 1.0 and float((images == 0).float().mean()) > 0.5
    keep = []
    vec = ir.forward(images.double(), {k: v.double() for k, v in params.items()}, keep)
    assert vec.shape == (3, 50)
    for (z, idx), (c, h, w), k in zip(keep, stages, (5, 3, 3)):
        assert idx.shape == (3, c, h, w)
    assert sum(t.numel() for t in params.values()) == 1568 + 50 * dense_in + 50
    for i in (1, 2, 3):  # biases non-zero, half of each layer's positive
        b = params[f"img.conv{i}.bias"]
        assert (b != 0).all() and int((b > 0).sum()) == b.numel() // 2


def test_parameter_count_at_the_default():
    assert sum(torch.Size(s).numel() for s in ir.param_shapes(28, 28, 50).values()) == 2418


def test_too_small_an_image_keeps_no_cell():
    assert ir.stage_shapes(23, 28)[-1][1] == 0 and ir.stage_shapes(24, 24)[-1][1:] == (1, 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_max_pool_sends_a_tie_to_the_first_element(dtype):
    x = torch.full((1, 1, 4, 4), 0.25, dtype=dtype, requires_grad=True)
    y = F.max_pool2d(x, 2)
    y.backward(torch.tensor([[[[1.0, 2.0], [3.0, 4.0]]]], dtype=dtype))
    want = torch.zeros(4, 4, dtype=dtype)
    want[0, 0], want[0, 2], want[2, 0], want[2, 2] = 1.0, 2.0, 3.0, 4.0  # element 0 of each all-equal window
    assert torch.equal(x.grad[0, 0], want)
    # a tie between elements 1 and 2 of a window goes to element 1 (row-major window order)
    x = torch.tensor([[[[0.0, 0.5], [0.5, 0.1]]]], dtype=dtype, requires_grad=True)
    F.max_pool2d(x, 2).sum().backward()
    assert x.grad.reshape(-1).tolist() == [0.0, 1.0, 0.0, 0.0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_relu_passes_no_gradient_at_zero(dtype):
    x = torch.tensor([-1.0, 0.0, -0.0, 1e-30, 2.0], dtype=dtype, requires_grad=True)
    F.relu(x).sum().backward()
    assert x.grad.tolist() == [0.0, 0.0, 0.0, 1.0, 1.0]


def test_floor_pooling_drops_the_trailing_row_and_column():
    x = torch.arange(15.0).reshape(1, 1, 3, 5).requires_grad_(True)
    y = F.max_pool2d(x, 2)
    assert y.shape == (1, 1, 1, 2) and y.reshape(-1).tolist() == [6.0, 8.0]
    y.sum().backward()
    assert float(x.grad[0, 0, 2].abs().sum()) == 0 and float(x.grad[0, 0, :, 4].abs().sum()) == 0


def test_the_kernel_cases_meet_their_input_condition():
    """Seed 1 (what test_imagequery_kernels_gpu.py uses): the fp32 and fp64 runs take the same ReLU and pooling
    decisions in every case, and every stage has live and dead pre-activations."""
    for size in ((28, 28), (24, 24), (26, 37)):
        for E in (50, 128):
            for n in (1, 3, 64, 65):
                c = ir.case(n, size, E, 1)
                assert c["same_pattern"], (n, size, E)
                assert c["bar_fwd"] < 2e-6 and c["bar_grad"] < 2e-6  # fp32 rounding, nothing coarser
                assert all(0.2 < float((~relu).float().mean()) < 0.8 for relu, _ in c["patterns"])
    for n, E in ((1, 128), (3, 50)):  # the largest image (test_the_largest_image)
        c = ir.case(n, (48, 48), E, 1)
        assert c["same_pattern"] and all(0.2 < float((~relu).float().mean()) < 0.8 for relu, _ in c["patterns"])


def test_flat_background_windows_are_exact_ties():
    """Over the exact-zero background every pre-activation of conv1 equals the bias bit for bit."""
    images, params, _ = ir.make_inputs(2, (28, 28), 50, seed=1)
    z = F.conv2d(images[:, None], params["img.conv1.weight"], params["img.conv1.bias"])
    flat = F.max_pool2d(images[:, None], 5, stride=1) == 0  # conv1's 5x5 window sees zeros only
    assert float(flat.float().mean()) > 0.2
    b = params["img.conv1.bias"].view(1, 4, 1, 1).expand_as(z)
    assert torch.equal(z[flat.expand_as(z)], b[flat.expand_as(z)])
