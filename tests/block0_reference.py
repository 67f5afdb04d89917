"""Plain float64 restatement of the first CNN block (conv3x3 1 -> CO with a zero halo, BatchNorm apply, GLU, dropout,
avg-pool) and of its backward down to conv0's weight gradient, with the per-element error bound the kernel tests use.
Not a test module: tests/test_block0_reference_cpu.py checks it against autograd, tests/test_block0_kernels_gpu.py
compares the kernels of csrc/block0.hip and the conv0 kernels of csrc/cnn_ops.hip with it.  It imports no project code,
only tests/glu_reference.py (the GLU stage and the bound); the dropout keep-mask is an explicit 0/1 tensor that the
caller obtains from the kernels themselves.

The math, on x (B,H,W), cw (CO,9) with tap t = 3 kh + kw, cb (CO), and the GLU arguments of glu_reference (CO = 16):
    x_t[b,h,w] = x[b, h + kh - 1, w + kw - 1], 0 outside the map            (conv_taps: THE statement of the halo)
    y[b,h,w,c] = cb[c] + sum_t cw[c][t] x_t                                 ycomp = |cb| + sum_t |cw[c][t]| |x_t|
    from x alone:  Sx[t] = sum_pos x_t,  R[t][u] = sum_pos x_t x_u  packed as [Sx (9) | R, t <= u, row by row (45)]
                   sy = (sum_pos y, sum_pos y^2) per channel
    GLU stage:     glu_reference(y, ...) -> pooled, g, d_lin, dW, db, st
    backward:      Gx[c][t] = sum_pos g x_t                                 companion sum_pos g~ |x_t|
                   d_y = A g + B (y - mean) + C,  coef = [A | B | C] (3,CO)
                   dW0[c][t] = sum_pos d_y x_t, evaluated DIRECTLY (not through R / Sx)
                   companion sum_pos (|A| g~ + |B| (ycomp + |mean|) + |C|) |x_t|

Error bound.  An output's bound is glu_reference.bound(companion, K, eps) + its PROPAGATED TERM.  K = positions =
B*H*W for every sum over positions, 16 for pooled and g, 1 for d_lin.  y itself is held to e_y alone (below), which is
tighter than bound(ycomp, 9, eps).  Where bound and term are both exactly 0 the kernel must write an exact 0.

The propagated term.  The fused kernels never store y: every kernel recomputes it with the chain of b0_conv1 / B0Conv::run
(csrc/block0.hip: the bias, then nine fused multiply-adds, one rounding of 2^-24 each), so everything downstream carries
the rounding of y,
    e_y = 10 * 2^-24 * ycomp,
which is not relative to the downstream companions (xn = y*scale + shift cancels).  Its first-order propagation:
    dxn = |scale| e_y                 dlin = dxn |W|^T                     dsig = sig (1 - sig) dxn
    dres = (dlin sig + |lin| dsig) m                                       -> pooled: its pooled average
    dd_lin = |d_res| dsig
    dg = dd_lin |W| + |d_res| (dlin gate + |lin| |gate'| dxn),  gate = sig (1 - sig), gate' = gate (1 - 2 sig)
    db: sum dd_lin     dW: sum dd_lin^T |xn| + |d_lin|^T dxn     st: (sum dg, sum dg |y| + |g| e_y)
    Gx: sum dg |x_t|   dW0: sum (|A| dg + |B| e_y) |x_t|
tests/test_block0_reference_cpu.py checks that it IS a bound (y + s e_y for random sign patterns s).

eps: EPS_FP32 for the fp32 instances (glu_reference places glu16_* there, and the fused kernels run the same GLU
arithmetic), EPS_BF16 for the ABF instances, whose reference takes x and cw rounded to bf16 and the bf16-rounded dpool
as its inputs: the conv products of bf16 operands are exact in fp32 and e_y keeps its form.

Further roundings, counted from the code:
  * sum y, sum y^2 (b0_stats_kernel, conv0_fwd_kernel) are sums of the ROUNDED y: y is off by <= 10 units of 2^-24 of
    ycomp and y^2 by <= 20 units of ycomp^2, inside the 64 units of EPS_FP32 against the companions sum ycomp and
    sum ycomp^2; no propagated term.
  * conv0_wgrad_kernel<CO, true> forms d_y in fp32 from the STORED y (an input, exact): fma(A, g, fma(B, y - mean, C)),
    three roundings relative to |A||g| + |B|(|y| + |mean|) + |C|, which is the companion (g~ = |g|, ycomp = |y| there).
  * the ABF backward kernel accumulates Gx with the fp32 window values of x (b0_bwd_kernel: x9[t] = win[...]), not the
    bf16-rounded ones its contractions see: 2^-9 relative to |x_t|, inside EPS_BF16 = 2^-7.
These figures are derived from the number formats and the code, not tuned to what the kernels give.
"""
import math

import torch

import glu_reference as G
from glu_reference import EPS_BF16, EPS_FP32, bound  # noqa: F401  (re-exported for the tests)

E_Y = 10.0 * 2.0 ** -24
NXR = 54
STAGE = ("pooled", "g", "d_lin", "dW", "db", "st", "Gx", "dW0")     # outputs behind y (they carry a propagated term)


def bf16(t):
    """round to bf16 (nearest even), back as float32"""
    return t.float().bfloat16().float()


def conv_taps(x):
    """(B,H,W) -> (9,B,H,W): the nine zero-padded shifts of x, t = 3 kh + kw"""
    x = x.detach().cpu().double()
    B, H, W = x.shape
    xp = torch.zeros(B, H + 2, W + 2, dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = x
    return torch.stack([xp[:, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3)])


def conv(xt, cw, cb):
    """y (B,H,W,CO) and its companion"""
    cw, cb = cw.detach().cpu().double().reshape(-1, 9), cb.detach().cpu().double()
    y = torch.einsum("tbhw,ct->bhwc", xt, cw) + cb
    return y, torch.einsum("tbhw,ct->bhwc", xt.abs(), cw.abs()) + cb.abs()


def pack_upper(r):
    """(9,9) -> the 45 entries t <= u, row by row"""
    return torch.stack([r[t, u] for t in range(9) for u in range(t, 9)])


def unpack_upper(v):
    """the 45 packed entries -> the symmetric (9,9) matrix"""
    r = torch.zeros(9, 9, dtype=v.dtype)
    k = 0
    for t in range(9):
        for u in range(t, 9):
            r[t, u] = r[u, t] = v[k]
            k += 1
    return r


def x_sums(xt):
    """[Sx | R packed] (54) and its companion"""
    f = xt.reshape(9, -1)
    a = f.abs()
    return torch.cat([f.sum(1), pack_upper(f @ f.t())]), torch.cat([a.sum(1), pack_upper(a @ a.t())])


def wgrad(xt, dy, dy_comp):
    """sum_pos dy x_t -> (CO,9) = [c][t], and its companion"""
    return torch.einsum("bhwc,tbhw->ct", dy, xt), torch.einsum("bhwc,tbhw->ct", dy_comp, xt.abs())


def bn_backward_map(g, g_comp, y, ycomp, coef, mean):
    """d_y = A g + B (y - mean) + C and its companion"""
    A, Bc, Cc = coef.detach().cpu().double()
    mean = mean.detach().cpu().double()
    return A * g + Bc * (y - mean) + Cc, A.abs() * g_comp + Bc.abs() * (ycomp + mean.abs()) + Cc.abs()


def conv0_wgrad_reference(x, dy, y=None, coef=None, mean=None):
    """bsed_conv0_wgrad: dy and the stored y are inputs.  Returns (ref, companion, K), (CO,9) each."""
    xt = conv_taps(x)
    dy = dy.detach().cpu().double()
    comp = dy.abs()
    if y is not None:
        y = y.detach().cpu().double()
        dy, comp = bn_backward_map(dy, comp, y, y.abs(), coef, mean)
    ref, c = wgrad(xt, dy, comp)
    return ref, c, x.numel()


class Block0Ref:
    """ref / comp / prop: dicts of float64 tensors keyed by output; K: term counts; y, ycomp, e_y, xt, res kept"""

    def bound(self, name, eps):
        if name == "y":
            return self.e_y
        return bound(self.comp[name], self.K[name], eps) + self.prop.get(name, 0.0)

    def err_over_bound(self, got, name, eps):
        """max over the elements of |got - ref| / bound; inf where the bound is 0 and the value is not an exact zero"""
        err = (got.detach().cpu().double() - self.ref[name]).abs()
        b = self.bound(name, eps)
        assert err.shape == b.shape, (name, err.shape, b.shape)
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf))
        ratio = torch.where(torch.isnan(err), torch.full_like(ratio, math.inf), ratio)
        return float(ratio.max()) if ratio.numel() else 0.0


def block0_reference(x, cw, cb, scale=None, shift=None, w=None, bias=None, pool=None, mask=None, p=0.0, dpool=None,
                     coef=None, mean=None, taps=conv_taps, y_offset=None):
    """float64 first block.  Without scale: y, xr and sy only (any CO).  With the GLU arguments: pooled as well; with
    dpool the backward (Gx included); with coef (3,CO) and mean also dW0.  taps: the halo rule (the tests pass wrong
    ones on purpose); y_offset: added to y before the stage (the tests pass s * e_y)."""
    r = Block0Ref()
    xt = taps(x)
    y, ycomp = conv(xt, cw, cb)
    n = x.numel()
    xr, xr_comp = x_sums(xt)
    pos = (0, 1, 2)
    r.xt, r.y, r.ycomp, r.e_y = xt, y, ycomp, E_Y * ycomp
    r.ref = {"y": y, "xr": xr, "sy": torch.stack([y.sum(pos), (y * y).sum(pos)])}
    r.comp = {"y": ycomp, "xr": xr_comp, "sy": torch.stack([ycomp.sum(pos), (ycomp * ycomp).sum(pos)])}
    r.K = {"y": 9, "xr": n, "sy": n}
    r.prop = {}
    if scale is None:
        return r
    if y_offset is not None:
        y = y + y_offset
    scale, shift, w, bias, mask = (t.detach().cpu().double() for t in (scale, shift, w, bias, mask))
    ref, comp, K = G.glu_reference(y, scale, shift, w, bias, pool, mask, p, dpool)
    r.ref.update(ref), r.comp.update(comp), r.K.update(K)
    # the stage's intermediates again, for the propagated term
    m = mask / (1.0 - p)
    ey = r.e_y
    xn = y * scale + shift
    wa = w.abs()
    lin = xn @ w.t() + bias
    sig = torch.sigmoid(xn)
    gate = sig * (1.0 - sig)
    dxn = scale.abs() * ey
    dlin = dxn @ wa.t()
    dsig = gate * dxn
    r.res = lin * sig * m
    r.prop["pooled"] = G.avg_pool((dlin * sig + lin.abs() * dsig) * m, pool)
    if dpool is None:
        return r
    ph, pw = pool
    B, H, W = x.shape
    d_res = (G.unpool(dpool.detach().cpu().double(), pool, H, W) * m / (ph * pw)).abs()
    dd_lin = d_res * dsig
    dg = dd_lin @ wa + d_res * (dlin * gate + lin.abs() * (gate * (1.0 - 2.0 * sig)).abs() * dxn)
    g, g_comp = r.ref["g"], r.comp["g"]
    r.prop.update(g=dg, d_lin=dd_lin, db=dd_lin.sum(pos),
                  dW=torch.einsum("bhwn,bhwc->nc", dd_lin, xn.abs()) + torch.einsum("bhwn,bhwc->nc", r.ref["d_lin"].abs(), dxn),
                  st=torch.stack([dg.sum(pos), (dg * y.abs() + g.abs() * ey).sum(pos)]))
    r.ref["Gx"], r.comp["Gx"] = wgrad(xt, g, g_comp)
    r.prop["Gx"] = wgrad(xt, g, dg)[1]
    r.K["Gx"] = n
    if coef is None:
        return r
    d_y, d_y_comp = bn_backward_map(g, g_comp, y, ycomp, coef, mean)
    r.ref["dW0"], r.comp["dW0"] = wgrad(xt, d_y, d_y_comp)
    ca = coef.detach().cpu().double().abs()
    r.prop["dW0"] = wgrad(xt, d_y, ca[0] * dg + ca[1] * ey)[1]
    r.K["dW0"] = n
    return r


def composed_dw0_bound(r, cw, cb, coef, mean, eps):
    """bound (1) of conv0's weight gradient as the kernels assemble it, dW0 = A Gx + B (Yx - mean Sx) + C Sx with
    Yx[c][t] = sum_u W[c][u] R[u][t] + cb[c] Sx[t]:
        |A| b(Gx) + |B| (sum_u |W[c][u]| b(R[u][t]) + (|cb| + |mean|) b(Sx[t])) + |C| b(Sx[t]) + 2^-24 |dW0|
    (the last term: one rounding of the fp32 result).  (CO,9)."""
    cw, cb, mean = (t.detach().cpu().double() for t in (cw.reshape(-1, 9), cb, mean))
    A, Bc, Cc = (t[:, None] for t in coef.detach().cpu().double().abs())
    bxr = r.bound("xr", eps)
    bsx, br = bxr[:9][None], unpack_upper(bxr[9:])
    return (A * r.bound("Gx", eps) + Bc * (cw.abs() @ br + (cb.abs() + mean.abs())[:, None] * bsx) + Cc * bsx
            + 2.0 ** -24 * r.ref["dW0"].abs())
