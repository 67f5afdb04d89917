"""float64 restatement of what include/bsed.h promises for bsed_conv_bwd3 (csrc/conv_bwd.hip): the backward of a 3 x 3 /
pad 1 convolution whose output feeds a train-mode BatchNorm.  Plain numpy, no kernel structure, no project code.  Not a
test module: tests/test_conv_bwd_reference_cpu.py pins it against float64 autograd, tests/test_conv_bwd_fused_gpu.py
compares the kernel with it.

Inputs, NHWC: inp (B,H,W,CIN), g = dL/d(BatchNorm output) and y = the convolution's output (B,H,W,N), coef (3,N) = the
[A|B|C] rows of bsed_bn_bwd, mean (N), w (N,CIN,3,3) = the nn.Conv2d weight.
    d_y[p][n]          = A[n] g[p][n] + B[n] (y[p][n] - mean[n]) + C[n]
    dW[n][k][kh][kw]   = sum_p inp[p + (kh-1, kw-1)][k] * d_y[p][n]            zero padding outside the image
    d_in[p][k]         = sum_{kh,kw,n} d_y[p - (kh-1, kw-1)][n] * w[n][k][kh][kw]
float32 inputs are taken at their float32 values (they are the operation's inputs)."""
import numpy as np


def d_y(g, y, coef, mean):
    coef, mean = np.asarray(coef, np.float64), np.asarray(mean, np.float64)
    return coef[0] * np.asarray(g, np.float64) + coef[1] * (np.asarray(y, np.float64) - mean) + coef[2]


def _shifted(a, dh, dw):
    """s[b][h][w] = a[b][h + dh][w + dw], zero where that falls outside the image"""
    B, H, W, C = a.shape
    pad = np.zeros((B, H + 2, W + 2, C), np.float64)
    pad[:, 1:H + 1, 1:W + 1] = a
    return pad[:, 1 + dh:1 + dh + H, 1 + dw:1 + dw + W]


def conv_bwd(inp, g, y, coef, mean, w):
    """-> (dW (N,CIN,3,3), d_in (B,H,W,CIN), d_y (B,H,W,N)), float64"""
    inp, w = np.asarray(inp, np.float64), np.asarray(w, np.float64)
    dy = d_y(g, y, coef, mean)
    N, CIN = w.shape[:2]
    dW = np.zeros((N, CIN, 3, 3), np.float64)
    d_in = np.zeros(inp.shape, np.float64)
    for kh in range(3):
        for kw in range(3):
            dW[:, :, kh, kw] = np.einsum("bhwk,bhwn->nk", _shifted(inp, kh - 1, kw - 1), dy)
            d_in += np.einsum("bhwn,nk->bhwk", _shifted(dy, 1 - kh, 1 - kw), w[:, :, kh, kw])
    return dW, d_in, dy
