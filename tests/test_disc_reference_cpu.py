"""tests/disc_reference.py checked on its own, in float64: a bar derived from it means something only where it states
the operation it claims to -- the reference's Clip_Discriminator layers in the project's transposed orientation, adjoint
pairs, the space-to-depth form, the head against autograd, and the keep rate of the restated dropout hash."""
import numpy as np
import pytest
import torch

import disc_reference as R
from oracle import crnn_oracle as co
from oracle import seeded


def _rng(seed):
    return np.random.default_rng(seed)


def _f32(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def test_conv_s2_layer_is_the_oracle_layer_on_the_permuted_image():
    """layers 1..5 of oracle Clip_Discriminator in float64, teacher-forced: conv_k + bn_k-apply + LeakyReLU of the
    (256 x T) image == conv_s2_layer on the (T x 256) image with the previous layer's (scale, shift) on the load"""
    N, T = 2, 67
    od = co.Clip_Discriminator()
    seeded.load_seeded(od, 3)
    od.double().train()
    x = torch.from_numpy(_f32(_rng(0), N, T, 256)).double()
    img = x.permute(0, 2, 1).unsqueeze(1)                     # (N,1,256,T), as the oracle's forward builds it
    y_prev, scale, shift = x.numpy()[..., None], None, None   # project layout (N,T,256,1)
    for k in range(1, 6):
        conv, bn = getattr(od, f"conv_{k}"), getattr(od, f"bn_{k}")
        y = conv(img)                                         # (N,co,F',T')
        mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
        sc = (bn.weight / torch.sqrt(var + bn.eps)).detach()
        sh = (bn.bias - mean * sc).detach()
        r = R.conv_s2_layer(y_prev, scale, shift, conv.weight.detach().numpy(), conv.bias.detach().numpy())
        want = y.detach().permute(0, 3, 2, 1).numpy()         # (N,T',F',co)
        assert r["out"].shape == want.shape, k
        assert np.abs(r["out"] - want).max() <= 1e-12 * np.abs(want).max(), k
        img = torch.nn.functional.leaky_relu(bn(y), 0.2)
        mine = R.act(r["out"], sc.numpy(), sh.numpy())
        assert np.abs(mine - img.detach().permute(0, 3, 2, 1).numpy()).max() <= 1e-11, k
        y_prev, scale, shift = r["out"], sc.numpy(), sh.numpy()


@pytest.mark.parametrize("Hi,Wi,C,CP", [(7, 9, 1, 1), (8, 7, 16, 32), (9, 10, 32, 32), (10, 8, 4, 4), (3, 3, 8, 8)])
def test_col2im_is_the_adjoint_of_im2col(Hi, Wi, C, CP):
    rng = _rng(Hi * 100 + Wi)
    N = 2
    x = _f32(rng, N, Hi, Wi, C)
    col = R.im2col_s2(x, CP=CP)
    d = _f32(rng, *col.shape)
    one = np.ones(C, np.float32)                                        # leaky'(y*1+1) == 1 for y = +1
    back = R.col2im_s2(d, np.ones_like(x), one, one, N, Hi, Wi, C, CP)["g"]
    lhs, rhs = float((col * d).sum()), float((x.astype(np.float64) * back).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


@pytest.mark.parametrize("Hi,Wi,Ha,Wa,C", [(7, 9, 7, 9, 4), (8, 7, 9, 9, 64), (10, 10, 11, 12, 16), (3, 3, 3, 3, 128)])
def test_s2d_bwd_is_the_adjoint_of_s2d_fwd(Hi, Wi, Ha, Wa, C):
    rng = _rng(Hi * 100 + Wi)
    N = 2
    x = _f32(rng, N, Ha, Wa, C)
    xp = R.s2d_fwd(x, None, None, Hi, Wi)
    d = _f32(rng, *xp.shape)
    one = np.ones(C, np.float32)
    back = R.s2d_bwd(d, np.ones_like(x), one, one, Hi, Wi)["g"]
    assert np.all(back[:, Hi:] == 0) and np.all(back[:, :, Wi:] == 0)
    lhs, rhs = float((xp * d).sum()), float((x.astype(np.float64) * back).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


@pytest.mark.parametrize("Hi,Wi", [(7, 9), (8, 7), (9, 10), (10, 8)])
def test_space_to_depth_form_equals_the_3x3_stride_2_form(Hi, Wi):
    """the 2x2 / stride-1 convolution over X' with the weight scattered by disc._S2D_SLOT == conv_s2_layer"""
    from bsed_amd.disc import _S2D_SLOT, TAPS2x2
    rng = _rng(Hi * 10 + Wi)
    N, cin, cout = 2, 4, 5
    x, w, b = _f32(rng, N, Hi, Wi, cin), _f32(rng, cout, cin, 3, 3), _f32(rng, cout)
    want = R.conv_s2_layer(x, None, None, w, b)["out"]
    xp = R.s2d_fwd(x, None, None, Hi, Wi)
    full = np.zeros((16, cin, cout))
    full[_S2D_SLOT] = w.astype(np.float64).transpose(2, 3, 1, 0).reshape(9, cin, cout)
    full = full.reshape(4, 4 * cin, cout)
    Ho, Wo = R.out_size(Hi), R.out_size(Wi)
    got = np.zeros((N, Ho, Wo, cout)) + b.astype(np.float64)
    for t, (dp, dq) in enumerate(TAPS2x2):
        got += xp[:, dp:dp + Ho, dq:dq + Wo, :] @ full[t]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("W5", [2, 3, 7, 8])
def test_disc_head_equals_autograd(W5):
    rng = _rng(W5)
    N, H5, Ns = 5, 3, 2
    y5 = _f32(rng, N, H5, W5, 8)
    scale, shift = (1 + 0.3 * _f32(rng, 8)), 0.2 * _f32(rng, 8)
    wl, bl = _f32(rng, 16), _f32(rng, 1)
    r = R.disc_head(y5, scale, shift, wl, bl, Ns)
    y = torch.from_numpy(y5).double()
    # g5 is the gradient on the BatchNorm output (the LeakyReLU's argument), which bn_bwd consumes: that is the leaf
    xn = (y * torch.from_numpy(scale).double() + torch.from_numpy(shift).double()).requires_grad_()
    lin = torch.nn.Linear(16, 1).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(wl).double().view(1, 16))
        lin.bias.copy_(torch.from_numpy(bl).double())
    a = torch.nn.functional.leaky_relu(xn, 0.2)
    img = a.permute(0, 3, 2, 1)                               # (N,8,features = W5,time = H5): the oracle's image
    pooled = torch.nn.AdaptiveAvgPool2d((2, 1))(img).flatten(1)
    d = torch.sigmoid(lin(pooled)).view(N)
    lab = (torch.arange(N) < Ns).double()
    loss = torch.nn.functional.binary_cross_entropy(d, lab)
    loss.backward()
    tol = 1e-12
    assert float((r["d"] - d.detach()).abs().max()) <= tol
    assert abs(float(r["loss"].sum() / N) - float(loss.detach())) <= tol
    assert float((r["g5"] - xn.grad).abs().max()) <= tol
    assert float((r["dwl"].sum(0) - lin.weight.grad.view(16)).abs().max()) <= tol
    assert abs(float(r["dbl"].sum()) - float(lin.bias.grad)) <= tol
    assert float((r["stats"][:, 0] - xn.grad.sum((1, 2))).abs().max()) <= tol
    assert float((r["stats"][:, 1] - (xn.grad * y).sum((1, 2))).abs().max()) <= tol


@pytest.mark.parametrize("p", [0.3, 0.5, 0.1])
def test_keep_mask_rate(p):
    n = 1_000_000
    keep = 1.0 - np.floor(float(np.float32(p)) * 2 ** 24) / 2 ** 24
    for stream, seed in ((401, 0), (402, 77), (7, (5 << 32) + 9)):
        rate = R.keep_mask(n, p, stream, seed).mean()
        assert abs(rate - keep) <= 5 * np.sqrt(keep * (1 - keep) / n), (p, stream, seed, rate)
    # a window of a longer mask is the mask of that window: the hash is of the element index alone
    assert np.array_equal(R.keep_mask(1000, p, 401, 3, start=500), R.keep_mask(1500, p, 401, 3)[500:])
