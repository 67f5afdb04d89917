"""float64 restatement of the contracts include/bsed.h gives for the BatchNorm-statistics, reduction and flat-arena
entry points (csrc/cnn_ops.hip, the slab reducers of csrc/reduce.hip, csrc/optim.hip).  Plain numpy, no kernel structure:
sums of partials are exactly rounded (math.fsum), so the reference carries no summation error of its own; everything
else is the header's formula evaluated in double.  float32 scalars (eps, momentum, lr, betas, ...) are taken at the
float32 value the ABI receives: they are the operation's inputs.  tests/test_stats_reference_cpu.py pins this module
against float64 autograd."""
import math
from fractions import Fraction

import numpy as np


def f32(x):
    """the float32 value a scalar argument of the C ABI arrives as, as a Python float"""
    return float(np.float32(x))


def exact_sum(a, axis0=True):
    """exactly rounded sum over the first axis: (n, ...) -> (...) float64, and the sum of magnitudes"""
    a = np.asarray(a, np.float64)
    flat = a.reshape(a.shape[0], -1)
    s = np.array([math.fsum(flat[:, j]) for j in range(flat.shape[1])], np.float64).reshape(a.shape[1:])
    sa = np.array([math.fsum(np.abs(flat[:, j])) for j in range(flat.shape[1])], np.float64).reshape(a.shape[1:])
    return s, sa


# ---------------------------------------------------------------------------------------------- BatchNorm
def bn_finalize(partial, count, eps, momentum, gamma, beta, running_mean=None, running_var=None, nbt=None):
    """partial (ntiles, 2, C) = per-tile (sum y, sum y^2) -> dict of float64 arrays (header: bsed_bn_finalize)"""
    s, sa = exact_sum(partial)
    eps, m, count = f32(eps), f32(momentum), float(count)
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    mean = s[0] / count
    var_raw = s[1] / count - mean * mean
    var = np.maximum(var_raw, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * invstd
    out = dict(s=s, abs_s=sa, mean=mean, var_raw=var_raw, var=var, invstd=invstd, scale=scale, shift=beta - mean * scale,
               abs_shift=np.abs(beta) + np.abs(mean * scale))
    if running_mean is not None:
        rm, rv = np.asarray(running_mean, np.float64), np.asarray(running_var, np.float64)
        unbiased = var * count / (count - 1) if count > 1 else var
        out.update(unbiased=unbiased, running_mean=(1 - m) * rm + m * mean, running_var=(1 - m) * rv + m * unbiased,
                   abs_running_mean=np.abs((1 - m) * rm) + np.abs(m * mean),
                   abs_running_var=np.abs((1 - m) * rv) + np.abs(m * unbiased))
    if nbt is not None:
        out["nbt"] = int(nbt) + 1
    return out


def bn_bwd(partial, count, gamma, mean, invstd):
    """partial (ntiles, 2, C) = per-tile (sum g, sum g*y); mean / invstd: the float32 values the kernel is handed, taken
    as exact.  -> dgamma, dbeta, coef (3, C) = [A | B | C] of d_y = A g + B (y - mean) + C (header: bsed_bn_bwd)"""
    s, sa = exact_sum(partial)
    count = float(count)
    gamma, mean, invstd = (np.asarray(v, np.float64) for v in (gamma, mean, invstd))
    dgamma = (s[1] - mean * s[0]) * invstd
    A = gamma * invstd
    coef = np.stack([A, -A * invstd * dgamma / count, -A * s[0] / count])
    return dict(s=s, abs_s=sa, dgamma=dgamma, dbeta=s[0].copy(), coef=coef)


def bn_bwd_apply(g, y, coef, mean):
    """(P, C) g, y -> d_y and the sum of the magnitudes of its three terms"""
    g, y, coef, mean = (np.asarray(v, np.float64) for v in (g, y, coef, mean))
    t = y - mean
    return coef[0] * g + coef[1] * t + coef[2], np.abs(coef[0] * g) + np.abs(coef[1] * t) + np.abs(coef[2])


def bn_eval(eps, gamma, beta, running_mean, running_var):
    """eval mode: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale"""
    gamma, beta, rm, rv = (np.asarray(v, np.float64) for v in (gamma, beta, running_mean, running_var))
    scale = gamma / np.sqrt(rv + f32(eps))
    return scale, beta - rm * scale, np.abs(beta) + np.abs(rm * scale)


# ---------------------------------------------------------------------------------------------- reductions
def colsum(inp, M, C, pitch, rows=None):
    """in: flat array of at least M * pitch elements -> sum_r in[r * pitch + c] for c < C (columns >= C never read),
    over rows = (r0, r1) if given; and the sum of magnitudes"""
    a = np.asarray(inp, np.float64).reshape(-1)[:M * pitch].reshape(M, pitch)[:, :C]
    if rows is not None:
        a = a[rows[0]:rows[1]]
    if a.shape[0] == 0:
        return np.zeros(C), np.zeros(C)
    return exact_sum(a)


def reduce_partials(part, K, N, dst, s_tap, s_k, s_n, accumulate, dst_offset=0):
    """part (G, ntaps, KP, NP); dst: flat array.  dst[off + tap*s_tap + k*s_k + n*s_n] (+)= sum_g part[g][tap][k][n] for
    k < K, n < N; the padding k >= K / n >= N is never read.  -> (new dst float64, sum of magnitudes per destination
    element, boolean mask of the addressed elements)"""
    part = np.asarray(part, np.float64)
    G, ntaps, KP, NP = part.shape
    s, sa = exact_sum(part[:, :, :K, :N])
    out = np.asarray(dst, np.float64).copy()
    mag = np.zeros_like(out)
    hit = np.zeros(out.shape, bool)
    tap, k, n = np.meshgrid(np.arange(ntaps), np.arange(K), np.arange(N), indexing="ij")
    idx = dst_offset + tap * s_tap + k * s_k + n * s_n
    assert len(np.unique(idx)) == idx.size, "the strides address one element twice"
    if accumulate:
        mag[idx] = np.abs(out[idx]) + sa
        out[idx] = out[idx] + s
    else:
        mag[idx] = sa
        out[idx] = s
    hit[idx] = True
    return out, mag, hit


# ---------------------------------------------------------------------------------------------- flat arena
def adam(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale):
    """torch.optim.Adam (L2 weight decay folded into the gradient), the scalars at their float32 values"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, gs = (f32(a) for a in (lr, b1, b2, eps, wd, grad_scale))
    gi = g * gs + wd * p
    m2 = b1 * m + (1 - b1) * gi
    v2 = b2 * v + (1 - b2) * gi * gi
    return dict(gi=gi, abs_gi=np.abs(g * gs) + np.abs(wd * p), m=m2, v=v2,
                update=adam_update(m2, v2, lr, b1, b2, eps, step))


def adam_update(m2, v2, lr, b1, b2, eps, step):
    """p' - p from the new moments: -(lr / (1 - b1^t)) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)"""
    lr, b1, b2, eps = (f32(a) for a in (lr, b1, b2, eps))
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return -(lr / bc1) * (np.asarray(m2, np.float64) / (np.sqrt(np.asarray(v2, np.float64)) / math.sqrt(bc2) + eps))


def sgd(p, g, buf, lr, momentum, wd, first, nesterov, grad_scale):
    """torch.optim.SGD(momentum, nesterov, weight_decay, dampening = 0).  -> new buffer (None when momentum == 0: the
    buffer is not touched), update p' - p, and the magnitude sums the rounding bounds are stated in"""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    lr, mom, wd, gs = (f32(a) for a in (lr, momentum, wd, grad_scale))
    gi = g * gs + wd * p
    G = np.abs(g * gs) + np.abs(wd * p)
    if mom == 0:
        return dict(buf=None, update=-lr * gi, abs_gi=G, abs_buf=None, abs_step=G)
    if first:
        b2, B = gi, G
    else:
        buf = np.asarray(buf, np.float64)
        b2, B = mom * buf + gi, np.abs(mom * buf) + G
    d, T = (gi + mom * b2, G + mom * B) if nesterov else (b2, B)
    return dict(buf=b2, update=-lr * d, abs_gi=G, abs_buf=B, abs_step=T)


def ema(ema_, p, alpha):
    e, p, a = np.asarray(ema_, np.float64), np.asarray(p, np.float64), f32(alpha)
    return e * a + p * (1 - a), np.abs(e * a) + np.abs(p * (1 - a))


def round_f32(x):
    """a Fraction rounded to the nearest float32 (ties to even), exactly; normal range only"""
    x = Fraction(x)
    if x == 0:
        return 0.0
    s, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1) and -126 <= e <= 127
    n = round(x / Fraction(2) ** (e - 23))          # Python rounds a Fraction half to even
    return s * float(n * Fraction(2) ** (e - 23))


def ema_i64(ema_, p, alpha):
    """int64 state entries: "float math, then truncation".  The float32 expression e*alpha + p*(1-alpha) has one value
    when every operation rounds, and one more for each product a fused multiply-add may leave unrounded: -> the set of
    admissible results per element (a list of sets of int)"""
    a = Fraction(f32(alpha))
    oma = Fraction(round_f32(1 - a))
    out = []
    for e, q in zip(np.asarray(ema_).reshape(-1).tolist(), np.asarray(p).reshape(-1).tolist()):
        fe, fq = Fraction(round_f32(e)), Fraction(round_f32(q))
        t1, t2 = fe * a, fq * oma
        vals = (round_f32(Fraction(round_f32(t1)) + Fraction(round_f32(t2))),     # every operation rounds
                round_f32(t1 + Fraction(round_f32(t2))),                          # fma(e, alpha, p*(1-alpha))
                round_f32(Fraction(round_f32(t1)) + t2))                          # fma(p, 1-alpha, e*alpha)
        out.append({int(math.trunc(x)) for x in vals})
    return out
