"""Plain float64 restatement of one GLU stage (BatchNorm apply -> Linear -> sigmoid gate -> dropout -> avg-pool) and of
its backward, with the per-element error bound the kernel tests use.  Not a test module:
tests/test_glu_reference_cpu.py checks it against autograd, tests/test_glu_kernels_gpu.py compares the kernels of
csrc/glu3.hip, csrc/glu_bwd.hip, csrc/glu_small.hip and the GLU epilogues of csrc/igemm.hip with it.  It imports no
project code; the dropout keep-mask is an explicit 0/1 tensor that the caller obtains from the kernels themselves.

The math, as stated at the top of glu_bwd.hip and glu3.hip, on y (B,H,W,C), scale / shift / bias (C), w (C,C) = [n][c],
pool (ph,pw), mask (B,H,W,C), drop probability p, dpool (B,H//ph,W//pw,C):
    xn = y*scale + shift          lin = xn W^T + b          sig = sigmoid(xn)          res = lin*sig*mask/(1-p)
    pooled = average of res over the ph x pw windows of the floor extent: rows >= (H//ph)*ph and columns >= (W//pw)*pw
             feed nothing
    d_res = unpool(dpool)*mask/(1-p)/(ph*pw), zero outside the pooled extent
    d_lin = d_res*sig             db = sum d_lin            dW = d_lin^T xn  ([n][c])
    g     = d_lin W + d_res*lin*sig*(1-sig)                 st = (sum g, sum g*y) per channel

Error bound.  Every result comes with a COMPANION: the same expression with each product term replaced by its
absolute value (lin~ = |xn||W|^T + |b|, g~ = |d_lin||W| + |d_res|*sig*(1-sig)*lin~, dW~ = sum |d_lin||xn|, st~ =
(sum g~, sum g~|y|), ...) and with the term count K of the longest fp32 accumulation behind an element (C for lin,
pooled and g; the number of positions B*H*W for dW, db and st; 1 for d_lin).  A kernel that rounds each operand and
each product with relative error <= eps and accumulates K terms in fp32 (unit round-off 2^-24; the rounding errors of
a sum of K terms grow like sqrt(K) u times the sum of the absolute terms, with a constant of 4 for the order-dependent
part) stays within
    |got - ref| <= (eps + 2^-22 sqrt(K)) * companion
of the float64 value, element by element.  Where the companion is exactly 0 the bound is 0: every term of the
expression is an exact zero and the kernel must write an exact zero (g and d_lin on the rows and columns the floor
pooling leaves out, and wherever the mask drops every contribution).

eps per family of kernels:
    EPS_FP32  = 2^-18  exact-fp32 matrix-core kernels (glu16_*, glu_bwd_fused, the igemm epilogues): each element is a
                       chain of at most ~10 fp32 operations (fused multiply-add of the BatchNorm apply, exp and
                       reciprocal of sigmoid_fast at 2^-23 each, the products with the mask multiplier, the pooling
                       factor and 1 - sig), each 2^-24 .. 2^-23 relative: 64 units of 2^-24 cover the chain.
    EPS_SPLIT = 2^-14  split-bf16x3 kernels with fp32 activations: an operand is hi + lo with hi = bf16(x), lo =
                       bf16(x - hi), so the split residual is <= 2^-9 * 2^-9 = 2^-18 per operand and the dropped
                       lo*lo product is <= 2^-18 of the product: 2^-16 with both operands and the dropped term counted
                       (DESIGN.md section 5 states the same figure); x4 for sigmoid_fast and the fused multiply-adds
                       around the contractions, which the results pass through twice in the backward (lin, then g).
    EPS_BF16  = 2^-7   bf16-activation instances: xn, W, d_lin and the stored outputs are each rounded to bf16 at
                       2^-9 relative; four such roundings in a chain.  Their reference takes the bf16-rounded y and
                       dpool (what the kernel is given) as its inputs.
These figures are derived from the number formats, not tuned to what the kernels give.
"""
import math

import torch

EPS_FP32, EPS_SPLIT, EPS_BF16 = 2.0 ** -18, 2.0 ** -14, 2.0 ** -7
OUTPUTS = ("pooled", "g", "d_lin", "dW", "db", "st")


def avg_pool(x, pool):
    """(B,H,W,C) -> (B,H//ph,W//pw,C): mean over the windows of the floor extent"""
    ph, pw = pool
    B, H, W, C = x.shape
    Hp, Wp = H // ph, W // pw
    return x[:, :Hp * ph, :Wp * pw].reshape(B, Hp, ph, Wp, pw, C).mean(dim=(2, 4))


def unpool(d, pool, H, W):
    """(B,Hp,Wp,C) -> (B,H,W,C): every window position takes its window's value, zero outside the pooled extent"""
    ph, pw = pool
    B, Hp, Wp, C = d.shape
    out = torch.zeros(B, H, W, C, dtype=d.dtype)
    out[:, :Hp * ph, :Wp * pw] = d.repeat_interleave(ph, dim=1).repeat_interleave(pw, dim=2)
    return out


def glu_reference(y, scale, shift, w, bias, pool, mask, p, dpool=None):
    """float64 GLU stage.  Returns (ref, companion, K): three dicts keyed by OUTPUTS (only "pooled" without dpool).
    ref / companion hold float64 tensors of the kernels' shapes (dW (C,C) = [n][c], db (C), st (2,C)); K the term count
    of the bound."""
    y, scale, shift, w, bias, mask = (t.detach().cpu().double() for t in (y, scale, shift, w, bias, mask))
    B, H, W, C = y.shape
    ph, pw = pool
    assert mask.shape == y.shape and bool(((mask == 0) | (mask == 1)).all()) and 0.0 <= p < 1.0
    m = mask / (1.0 - p)
    xn = y * scale + shift
    wa = w.abs()
    lin = xn @ w.t() + bias
    lin_c = xn.abs() @ wa.t() + bias.abs()
    sig = torch.sigmoid(xn)
    ref = {"pooled": avg_pool(lin * sig * m, pool)}
    comp = {"pooled": avg_pool(lin_c * sig * m, pool)}
    K = {"pooled": C, "g": C, "d_lin": 1, "dW": B * H * W, "db": B * H * W, "st": B * H * W}
    if dpool is None:
        return ref, comp, {"pooled": C}
    dpool = dpool.detach().cpu().double()
    assert dpool.shape == (B, H // ph, W // pw, C)
    d_res = unpool(dpool, pool, H, W) * m / (ph * pw)
    d_lin = d_res * sig
    gate = sig * (1.0 - sig)
    g = d_lin @ w + d_res * lin * gate
    g_c = d_lin.abs() @ wa + d_res.abs() * gate * lin_c
    pos = (0, 1, 2)
    ref.update(g=g, d_lin=d_lin, db=d_lin.sum(pos), dW=torch.einsum("bhwn,bhwc->nc", d_lin, xn),
               st=torch.stack([g.sum(pos), (g * y).sum(pos)]))
    comp.update(g=g_c, d_lin=d_lin.abs(), db=d_lin.abs().sum(pos),
                dW=torch.einsum("bhwn,bhwc->nc", d_lin.abs(), xn.abs()),
                st=torch.stack([g_c.sum(pos), (g_c * y.abs()).sum(pos)]))
    return ref, comp, K


def bound(companion, K, eps):
    """the per-element bound (eps + 2^-22 sqrt(K)) * companion"""
    return (eps + 2.0 ** -22 * math.sqrt(K)) * companion


def err_over_bound(got, ref, companion, K, eps):
    """max over the elements of |got - ref| / bound; inf where the bound is 0 and the value is not an exact zero"""
    err = (got.detach().cpu().double() - ref).abs()
    b = bound(companion, K, eps)
    assert err.shape == b.shape, (err.shape, b.shape)
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf))
    ratio = torch.where(torch.isnan(err), torch.full_like(ratio, math.inf), ratio)
    return float(ratio.max()) if ratio.numel() else 0.0
