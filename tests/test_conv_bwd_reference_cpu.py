"""tests/conv_bwd_reference.py against float64 autograd (no GPU): conv2d with padding 1, the BatchNorm-backward map stated as
a plain affine function of g and y."""
import numpy as np
import pytest
import torch

import conv_bwd_reference as R


@pytest.mark.parametrize("B,H,W,CIN,N", [(2, 5, 4, 3, 2), (1, 3, 7, 2, 5), (3, 1, 1, 4, 4)])
def test_reference_matches_float64_autograd(B, H, W, CIN, N):
    rng = np.random.default_rng(B * 100 + H * 10 + W)
    inp = rng.standard_normal((B, H, W, CIN)).astype(np.float32)
    g = rng.standard_normal((B, H, W, N)).astype(np.float32)
    y = rng.standard_normal((B, H, W, N)).astype(np.float32)
    coef = rng.uniform(0.5, 1.5, (3, N)).astype(np.float32)
    mean = rng.standard_normal(N).astype(np.float32)
    w = rng.standard_normal((N, CIN, 3, 3)).astype(np.float32)
    dW, d_in, dy = R.conv_bwd(inp, g, y, coef, mean, w)
    c = torch.from_numpy(coef).double()
    dy_t = c[0] * torch.from_numpy(g).double() + c[1] * (torch.from_numpy(y).double() - torch.from_numpy(mean).double()) + c[2]
    np.testing.assert_allclose(dy, dy_t.numpy(), rtol=0, atol=1e-14)
    x_t = torch.from_numpy(inp).double().permute(0, 3, 1, 2).requires_grad_(True)
    w_t = torch.from_numpy(w).double().requires_grad_(True)
    out = torch.nn.functional.conv2d(x_t, w_t, padding=1)
    out.backward(dy_t.permute(0, 3, 1, 2))
    np.testing.assert_allclose(dW, w_t.grad.numpy(), rtol=0, atol=1e-12 * max(1.0, float(w_t.grad.abs().max())))
    np.testing.assert_allclose(d_in, x_t.grad.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12 * max(1.0, float(x_t.grad.abs().max())))


def test_the_ring_is_zero_padding_not_the_neighbouring_image():
    """an image's gradients read nothing of the images before and after it"""
    rng = np.random.default_rng(5)
    inp, g, y = (rng.standard_normal((3, 4, 4, c)) for c in (2, 3, 3))
    coef, mean, w = rng.standard_normal((3, 3)), rng.standard_normal(3), rng.standard_normal((3, 2, 3, 3))
    _, d_in, _ = R.conv_bwd(inp, g, y, coef, mean, w)
    _, d_one, _ = R.conv_bwd(inp[1:2], g[1:2], y[1:2], coef, mean, w)
    np.testing.assert_array_equal(d_in[1:2], d_one)
