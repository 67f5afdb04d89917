"""Plain float64 restatement of every operation in csrc/disc.hip and of one discriminator layer, for
tests/test_disc_kernels_gpu.py (checked on its own by tests/test_disc_reference_cpu.py).  Nothing here is shared with
bsed_amd/disc.py or the kernels: numpy slicing and loops, torch float64 autograd for the convolution.

Layout (the project's): images are (N, H = T, W = 256, C) -- the embedding's own memory order; the reference's
Conv2d sees the permuted (256 x T) image, so its kernel index kh runs over this W axis and kw over this H axis.
  column order of the gathered matrix   (dw*3 + dh)*CP + c       (== kh*3 + kw of the reference orientation)
  space-to-depth operand X'             [n][p][q][a*2 + b][c]  =  A[n][2p + a][2q + b][c]
Every function takes fp32 arrays, computes in float64 and returns float64.

LeakyReLU masks are exact, not approximate.  The kernels decide the branch on fmaf(y, scale, shift) > 0 with fp32 y,
scale, shift.  The product P = y*scale of two fp32 numbers has at most 48 significant bits and is exact in float64, so
float64 computes round64(P + shift) and fmaf computes round32(P + shift) of the SAME real number.  Round-to-nearest is
monotone and maps 0 to 0: it never moves a value across zero, and it takes a non-zero value to zero only by underflow.
A non-zero P + shift is a multiple of the smaller operand's last bit, which for the O(1) test data (|y|, |scale|,
|shift| in 2^-30..2^10) is above 2^-110, far from fp32's underflow at 2^-150.  Hence sign(float64 y*scale + shift) ==
sign(fmaf(y, scale, shift)) for every element: no element is ever excluded from a comparison, and the share of skipped
elements is 0 in every test that uses this file.
"""
import numpy as np
import torch

LEAKY = 0.2
CH = [1, 128, 64, 32, 16, 8]


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _pre(y, scale, shift):
    return y * _f64(scale) + _f64(shift)


def act(y, scale, shift):
    """leaky(y*scale + shift) per channel (last axis), identity without scale/shift"""
    y = _f64(y)
    if scale is None:
        return y
    v = _pre(y, scale, shift)
    return np.where(v > 0, v, LEAKY * v)


def dact(y, scale, shift):
    """leaky'(y*scale + shift): 1 where positive, 0.2 elsewhere (zero included, as `x > 0 ? 1 : 0.2`)"""
    return np.where(_pre(_f64(y), scale, shift) > 0, 1.0, LEAKY)


def out_size(n):
    return (n - 3) // 2 + 1


# ------------------------------------------------------------------------------------------------ gathers / scatters
def im2col_s2(a, scale=None, shift=None, CP=None):
    """a (N,Hi,Wi,C) -> col (N*Ho*Wo, K): K = 16 for C == 1 (9 taps, columns 9..15 zero), else 9*CP (pad channels zero)"""
    a = act(a, scale, shift)
    N, Hi, Wi, C = a.shape
    Ho, Wo = out_size(Hi), out_size(Wi)
    CPe = 1 if C == 1 else (CP or C)
    col = np.zeros((N, Ho, Wo, 16 if C == 1 else 9 * CPe))
    for dw in range(3):
        for dh in range(3):
            t = dw * 3 + dh
            for ho in range(Ho):
                for wo in range(Wo):
                    col[:, ho, wo, t * CPe:t * CPe + C] = a[:, 2 * ho + dh, 2 * wo + dw, :]
    return col.reshape(N * Ho * Wo, -1)


def scatter_s2(dcol, N, Hi, Wi, C, CP):
    Ho, Wo = out_size(Hi), out_size(Wi)
    CPe = 1 if C == 1 else CP
    d = _f64(dcol).reshape(N, Ho, Wo, -1)
    out = np.zeros((N, Hi, Wi, C))
    for dw in range(3):
        for dh in range(3):
            t = dw * 3 + dh
            for ho in range(Ho):
                for wo in range(Wo):
                    out[:, 2 * ho + dh, 2 * wo + dw, :] += d[:, ho, wo, t * CPe:t * CPe + C]
    return out


def block_partials(v, C):
    """sums per channel over consecutive groups of 256 float4 (= 1024 floats) of v in memory order: (blocks, C).
    1024 is a multiple of every admitted C, so every group starts at channel 0."""
    flat = _f64(v).reshape(-1)
    nb = -(-flat.size // 1024)
    pad = np.zeros(nb * 1024)
    pad[:flat.size] = flat
    return pad.reshape(nb, 1024 // C, C).sum(1)


def _bn_sums(g, y, C):
    y = _f64(y)
    return dict(g=g, sums=np.stack([g.reshape(-1, C).sum(0), (g * y).reshape(-1, C).sum(0)]),
                partials=np.stack([block_partials(g, C), block_partials(g * y, C)], 1))


def col2im_s2(dcol, y, scale, shift, N, Hi, Wi, C, CP=1, out_scale=1.0):
    """adjoint of im2col_s2.  C == 1: dict(g = scatter * out_scale).  C > 1: g = scatter * leaky'(y*scale+shift),
    sums (2,C) = (sum g, sum g*y), partials (blocks,2,C); abs_g / abs_partials are the same with |dcol| and |y| (the
    sum|terms| of the error bounds)."""
    a = scatter_s2(dcol, N, Hi, Wi, C, CP)
    if C == 1:
        return dict(g=a * float(out_scale), abs_g=scatter_s2(np.abs(_f64(dcol)), N, Hi, Wi, C, CP) * abs(float(out_scale)))
    m = dact(y, scale, shift)
    r = _bn_sums(a * m, y, C)
    ag = scatter_s2(np.abs(_f64(dcol)), N, Hi, Wi, C, CP) * m
    r.update(abs_g=ag, abs_partials=np.stack([block_partials(ag, C), block_partials(ag * np.abs(_f64(y)), C)], 1))
    return r


def s2d_fwd(y, scale, shift, Hi, Wi):
    """y (N,Ha,Wa,C) with valid extent (Hi,Wi) -> X' (N,Hp,Wp,4C), zero where 2p+a >= Hi or 2q+b >= Wi"""
    a = act(y, scale, shift)
    N, Ha, Wa, C = a.shape
    Hp, Wp = (Hi + 1) // 2, (Wi + 1) // 2
    xp = np.zeros((N, Hp, Wp, 4, C))
    for h in range(Hi):
        for w in range(Wi):
            xp[:, h // 2, w // 2, (h % 2) * 2 + (w % 2), :] = a[:, h, w, :]
    return xp.reshape(N, Hp, Wp, 4 * C)


def s2d_bwd(dxp, y, scale, shift, Hi, Wi):
    """adjoint of s2d_fwd on the allocated grid of y: g (zero outside the valid extent), sums, partials, abs_*.
    y is not read outside the valid extent (it may hold anything there)."""
    y = _f64(y).copy()
    y[:, Hi:], y[:, :, Wi:] = 0.0, 0.0
    N, Ha, Wa, C = y.shape
    Hp, Wp = (Hi + 1) // 2, (Wi + 1) // 2
    d = _f64(dxp).reshape(N, Hp, Wp, 4, C)
    a = np.zeros((N, Ha, Wa, C))
    for h in range(Hi):
        for w in range(Wi):
            a[:, h, w, :] = d[:, h // 2, w // 2, (h % 2) * 2 + (w % 2), :]
    m = dact(y, scale, shift)
    r = _bn_sums(a * m, y, C)
    ag = np.abs(a) * m
    r.update(abs_g=ag, abs_partials=np.stack([block_partials(ag, C), block_partials(ag * np.abs(y), C)], 1))
    return r


# ------------------------------------------------------------------------------------------------ clip head
def disc_head(y5, scale, shift, wl, bl, Ns, dtype=torch.float64):
    """BN-apply + LeakyReLU + AdaptiveAvgPool2d((2,1)) + Linear(16,1) + sigmoid + BCE(label = n < Ns), forward and
    backward in explicit formulas, per sample (nothing summed over N).  y5 (N,H5,W5,8); wl (16,) indexed c*2 + bin.
    PyTorch's bins over W5: [0, ceil(W5/2)) and [floor(W5/2), W5); BCE clamps the logs at -100 and its backward divides
    by max(d(1-d), 1e-12).  `dtype`: torch.float64 (the reference) or torch.float32 (the yardstick of the GPU test).
    Returns dict of d (N,), loss (N,), g5 (N,H5,W5,8), stats (N,2,8), dwl (N,16), dbl (N,)."""
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)
    y5, scale, shift, wl, bl = t(y5), t(scale), t(shift), t(wl).reshape(16), t(bl).reshape(())
    N, H5, W5, C = y5.shape
    bins = [(0, (W5 + 1) // 2), (W5 // 2, W5)]
    xn = y5 * scale + shift
    a = torch.where(xn > 0, xn, LEAKY * xn)
    pooled = torch.stack([a[:, :, s:e, :].sum((1, 2)) / (H5 * (e - s)) for s, e in bins], 2)    # (N,8,2)
    w2 = wl.view(8, 2)
    z = bl + (pooled * w2).sum((1, 2))
    d = 1 / (1 + torch.exp(-z))
    lab = (torch.arange(N) < Ns).to(dtype)
    loss = -(lab * torch.log(d).clamp(min=-100) + (1 - lab) * torch.log(1 - d).clamp(min=-100))
    dz = (d - lab) / ((1 - d) * d).clamp(min=1e-12) / N * d * (1 - d)
    dwl = dz[:, None, None] * pooled
    da = torch.zeros_like(y5)
    for i, (s, e) in enumerate(bins):
        da[:, :, s:e, :] += (dz[:, None] * w2[:, i] / (H5 * (e - s)))[:, None, None, :]
    g5 = da * torch.where(xn > 0, torch.ones_like(xn), torch.full_like(xn, LEAKY))
    stats = torch.stack([g5.sum((1, 2)), (g5 * y5).sum((1, 2))], 1)
    return dict(d=d, loss=loss, g5=g5, stats=stats, dwl=dwl.reshape(N, 16), dbl=dz)


# ------------------------------------------------------------------------------------------------ dropout mask
_M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def mix32(x):
    """lowbias32 of bsed_common.h on uint32 values held in uint64 arrays (every product masked back to 32 bits)"""
    x = _u32(x)
    x = x ^ (x >> np.uint64(16))
    x = _u32(x * np.uint64(0x7FEB352D))
    x = x ^ (x >> np.uint64(15))
    x = _u32(x * np.uint64(0x846CA68B))
    return x ^ (x >> np.uint64(16))


def drop_key(stream, seed):
    seed, stream = int(seed), int(stream)
    a = mix32((seed & 0xFFFFFFFF) ^ ((stream * 0x9E3779B9) & 0xFFFFFFFF))
    b = mix32(((seed >> 32) & 0xFFFFFFFF) ^ 0x85EBCA6B)
    return _u32(a + b)


def drop_threshold(p):
    """(uint32)(p * 16777216.0f) with p an fp32 number: floor(p * 2^24), the product being exact"""
    return int(np.float64(np.float32(p)) * 16777216.0)


def keep_mask(n, p, stream, seed, start=0):
    """keep-mask of elements start..start+n-1: a 24-bit threshold compare, (hash >> 8) >= floor(p * 2^24)"""
    e = np.arange(start, start + n, dtype=np.uint64)
    lo, hi = e & _M32, e >> np.uint64(32)
    h = mix32(_u32(lo * np.uint64(0x9E3779B1)) + drop_key(stream, seed) + _u32(hi * np.uint64(0x85EBCA6B)))
    return (h >> np.uint64(8)) >= np.uint64(drop_threshold(p))


def leaky_dropout(a, p, stream, seed, d_out=None, slope=LEAKY):
    """out = leaky(a) * mask / (1-p)  and, with d_out, d_a = d_out * leaky'(a) * mask / (1-p); mask over the flat index.
    Returns (out, d_a or None, mask)."""
    a = _f64(a)
    mask = keep_mask(a.size, p, stream, seed).reshape(a.shape) if p > 0 else np.ones(a.shape, bool)
    mul = mask / (1.0 - float(np.float32(p)))
    out = np.where(a > 0, a, slope * a) * mul
    d_a = None if d_out is None else _f64(d_out) * np.where(a > 0, 1.0, slope) * mul
    return out, d_a, mask


# ------------------------------------------------------------------------------------------------ frame head
def frame_head_fwd(x, w, b):
    return 1.0 / (1.0 + np.exp(-(_f64(x) @ _f64(w).reshape(-1) + float(np.asarray(b).reshape(-1)[0]))))


def frame_head_bwd(x, w, d, d_out):
    """dz = d_out * d (1-d);  dx = dz w;  dw = sum_m dz x;  db = sum_m dz;  abs_dw / abs_db = sum_m |terms|"""
    x, w, d, d_out = _f64(x), _f64(w).reshape(-1), _f64(d), _f64(d_out)
    dz = d_out * d * (1 - d)
    t = dz[:, None] * x
    return dict(dx=dz[:, None] * w[None, :], dw=t.sum(0), db=dz.sum(), abs_dw=np.abs(t).sum(0), abs_db=np.abs(dz).sum())


# ------------------------------------------------------------------------------------------------ one layer
def conv_s2_layer(y_prev, scale, shift, w, bias, dy=None):
    """3x3 / stride-2 convolution of the project's (N,H,W,C) image with the reference-orientation weight
    w (co,cin,kh,kw): out[n,i,j,o] = bias[o] + sum w[o,c,dw,dh] * A[n,2i+dh,2j+dw,c],  A = leaky(y_prev*scale+shift)
    (A = y_prev without scale/shift).  Forward and backward by float64 autograd.
    Returns dict(out (N,Ho,Wo,co)) and, with dy (N,Ho,Wo,co): dW (co,cin,3,3), dA = dL/dA, g_prev = dA * leaky'
    (None without scale/shift), sums (2,cin) = (sum g_prev, sum g_prev*y_prev), abs_sums = the same over |dA| leaky' and
    |y_prev|."""
    A = torch.from_numpy(act(y_prev, scale, shift)).requires_grad_()
    W = torch.from_numpy(_f64(w).copy()).requires_grad_()
    b = torch.from_numpy(_f64(bias).copy())
    out = torch.nn.functional.conv2d(A.permute(0, 3, 1, 2), W.transpose(2, 3), b, stride=2).permute(0, 2, 3, 1)
    r = dict(out=out.detach().numpy())
    if dy is None:
        return r
    out.backward(torch.from_numpy(_f64(dy).copy()))
    dA = A.grad.numpy()
    r.update(dW=W.grad.numpy(), dA=dA, g_prev=None, sums=None)
    if scale is not None:
        m, y = dact(y_prev, scale, shift), _f64(y_prev)
        g = dA * m
        C = y.shape[-1]
        ag = np.abs(dA) * m
        r.update(g_prev=g, sums=np.stack([g.reshape(-1, C).sum(0), (g * y).reshape(-1, C).sum(0)]),
                 abs_sums=np.stack([ag.reshape(-1, C).sum(0), (ag * np.abs(y)).reshape(-1, C).sum(0)]))
    return r
