"""The flat-arena kernels of csrc/optim.hip -- bsed_adam_step, bsed_sgd_step, bsed_ema_update, bsed_ema_update_i64,
bsed_axpy, bsed_scale -- against the float64 evaluation (tests/stats_reference.py) of the formulas their header comments
and torch.optim give.  The scalars are taken at the float32 values the ABI receives.

Bounds.  u = 2^-24; every fp32 operation errs by at most u times its result, a fused multiply-add once for both.
Magnitudes are sums of |terms|, so cancellation inside an expression is carried.  G = |g gs| + |wd p|.

  gradient     gi = fma(wd, p, g * gs): two roundings, 2 u G; counted as 3 u G below, the third for second-order terms.
  Adam m'      fl(b1 m) + fl(fl(1 - b1) gi): u on the first term; u + u and the gradient's 2 u on the second; the sum u
               on both: 2 u |b1 m| + 5 u (1 - b1) G, held at 3 u |b1 m| + 6 u (1 - b1) G.
  Adam v'      fl(b2 v) + fl(fl(fl(1 - b2) gi) gi): u; three roundings and twice the gradient's 2 u; the sum:
               2 u b2 |v| + 8 u (1 - b2) G^2, held at 3 u b2 |v| + 9 u (1 - b2) G^2.
  Adam update  p' - p = -(lr / bc1) (m' / (sqrtf(v') / sqrtf(bc2) + eps)), evaluated by the reference from the kernel's
               own stored m' and v' (the values the kernel divides; they are checked on their own above).
               bc = 1 - powf(b, t) cancels: powf is within 1 ulp <= 2 u b^t, the subtraction adds u, so
               rel(bc1) <= 2 u b1^t / (1 - b1^t) + u and rel(sqrt bc2) <= u b2^t / (1 - b2^t) + u / 2 + u.  Then lr / bc1,
               sqrtf(v'), its quotient by sqrt bc2, + eps, m' / denom and the last product round once each: 6 u, held
               at 7.  The subtraction from p rounds once on the result: u (|p| + |update|).  In all
                 |err| <= (rel(bc1) + rel(sqrt bc2) + 7 u) |update| + u (|p| + |update|),
               which is the 2 u / (1 - b1^t) + u / (1 - b2^t) cancellation term plus the per-element roundings.
  SGD          buffer b' = gi (first step) or fl(mom b) + gi: E_b = 3 u G (+ 2 u (|mom b| + G) later).  Direction
               d = gi + mom b' (nesterov), b' (momentum) or gi: E_d = 3 u G + mom E_b + 2 u T, E_b or 3 u G, with T the
               magnitude sum of d.  update = -lr d: lr E_d + u lr T; the subtraction from p: u (|p| + lr T).
  EMA          fl(e a) + fl(p fl(1 - a)): 2 u on the first term, 3 u on the second, held at 3 u (1 + 4 u) sum|terms|.
               int64 entries: (long long)((float)e a + (float)p (1 - a)), each operation rounded, or either product
               left unrounded inside a fused multiply-add: the kernel must give one of those three integers.
  axpy, scale  one rounding: 0.5 ulp, held at 1 ulp of the reference.
Every case is launched twice on fresh buffers and must repeat its bits.  The launches cap their grid at 4096 workgroups
of 256: at n = 4096 * 256 + 257 the grid-stride loop wraps, 257 threads taking a second trip.  Parameters span five
decades of magnitude, so that for many elements the rounding of p' itself (u |p|) is far below the update."""
import itertools

import numpy as np
import pytest
import torch

import stats_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
SIZES = [1, 255, 4096 * 256 + 257]
LR, B1, B2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8
WORST = {}


def _mods():
    from bsed_amd import _lib as L
    from bsed_amd import ops
    return L, ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _within(got, ref, bound, key, what=None):
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    err = np.abs(got - ref)
    bad = ~(err <= bound)                               # NaN fails
    frac = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    assert not bad.any(), (key, what, int(bad.sum()), float(np.nanmax(frac)))
    WORST[key] = max(WORST.get(key, 0.0), float(frac.max()))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"worst error / bound  {k:28s} {WORST[k]:.3f}")


def _arena(n, seed):
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-2, 1, n)
    p = (10.0 ** rng.uniform(-5, 0, n) * rng.standard_normal(n)).astype(np.float32)
    g = (scale * rng.standard_normal(n)).astype(np.float32)
    m = (0.1 * scale * rng.standard_normal(n)).astype(np.float32)
    v = ((0.1 * scale * rng.standard_normal(n)) ** 2).astype(np.float32)
    return p, g, m, v


# ------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("n", SIZES)
def test_adam(n):
    L, ops = _mods()
    p, g, m, v = _arena(n, n)
    zero = np.arange(n) % 7 == 3                                    # elements with g = m = v = 0 (none at n = 1)
    g[zero], m[zero], v[zero] = 0, 0, 0
    b1, b2 = R.f32(B1), R.f32(B2)
    gd = _dev(g)
    for step, wd, gs in itertools.product((1, 2, 1000), (0.0, 1e-4), (1.0, 0.25)):
        def run():
            t = dict(p=_dev(p), m=_dev(m), v=_dev(v))
            ops.adam_step(t["p"], gd, t["m"], t["v"], LR, step, (B1, B2), ADAM_EPS, wd, gs)
            return t
        a, a2 = run(), run()
        assert all(torch.equal(a[k], a2[k]) for k in a), ("repeat", step, wd, gs)
        case = (n, step, wd, gs)
        r = R.adam(p, g, m, v, LR, B1, B2, ADAM_EPS, wd, step, gs)
        G = r["abs_gi"]
        m2, v2, p2 = _host(a["m"]), _host(a["v"]), _host(a["p"])
        _within(m2, r["m"], 3 * U * np.abs(b1 * m) + 6 * U * (1 - b1) * G, "adam m", case)
        _within(v2, r["v"], 3 * U * b2 * np.abs(v) + 9 * U * (1 - b2) * G * G, "adam v", case)
        x1, x2 = b1 ** step, b2 ** step
        rel = (2 * U * x1 / (1 - x1) + U) + (U * x2 / (1 - x2) + 1.5 * U) + 7 * U
        upd = R.adam_update(m2, v2, LR, B1, B2, ADAM_EPS, step)
        _within(p2 - p, upd, rel * np.abs(upd) + U * (np.abs(p) + np.abs(upd)), "adam update", case)
        assert np.all(np.isfinite(p2)) and np.all(np.isfinite(m2)) and np.all(np.isfinite(v2))
        if wd == 0:                                                  # (with weight decay the gradient is wd p, not 0)
            assert np.array_equal(p2[zero], p[zero].astype(np.float64)), "g = m = v = 0 stays put"
            assert np.all(m2[zero] == 0) and np.all(v2[zero] == 0)


def test_adam_all_zero_single_element():
    L, ops = _mods()
    for step in (1, 2, 1000):
        p, z = torch.tensor([0.75], device="cuda"), torch.zeros(1, device="cuda")
        m, v = z.clone(), z.clone()
        ops.adam_step(p, z, m, v, LR, step)
        assert float(p) == 0.75 and float(m) == 0 and float(v) == 0


def test_adam_against_double_precision_betas():
    """torch.optim.Adam keeps its betas in double; the ABI passes them as float32.  fl32(0.999) is 1.29e-5 (1 - b2) above
    0.999: v' and 1 - b2^t move by at most that, halved by the root: 1.29e-5; fl32(0.9) moves 1 - b1 by 2.4e-7 (twice:
    m' and 1 - b1^t); the fp32 roundings of three steps add ~2e-6.  Held at 2e-5 of the update; the figure is printed."""
    L, ops = _mods()
    n = 255
    rng = np.random.default_rng(4)
    p0 = np.zeros(n, np.float32)                                     # small parameters: p' - p resolves the update
    tp = torch.tensor(p0.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([tp], lr=LR, betas=(B1, B2), eps=ADAM_EPS)
    p, m, v = _dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    worst = 0.0
    for step in (1, 2, 3):
        g = rng.standard_normal(n).astype(np.float32)
        before, tbefore = _host(p), tp.detach().numpy().copy()
        tp.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        ops.adam_step(p, _dev(g), m, v, LR, step)
        want = tp.detach().numpy() - tbefore
        got = _host(p) - before
        rel = np.abs(got - want) / np.abs(want)
        keep = np.abs(want) > 0.1 * LR                              # where u |p| is below 1e-6 of the update
        worst = max(worst, float(rel[keep].max()))
        with torch.no_grad():
            tp.copy_(p.double().cpu())                               # the same parameters into the next step
    print(f"adam update, fp32 betas against torch.optim's double betas, steps 1-3: {worst:.2e} relative")
    assert worst <= 2e-5


# ------------------------------------------------------------------------------------------------ SGD
@pytest.mark.parametrize("n", SIZES)
def test_sgd(n):
    L, ops = _mods()
    p, g, buf, _ = _arena(n, n + 1)
    lr = 0.05
    gd = _dev(g)
    for first, nesterov, mom, wd, gs in itertools.product((1, 0), (0, 1), (0.0, 0.9), (0.0, 1e-4), (1.0, 0.25)):
        def run():
            t = dict(p=_dev(p), buf=_dev(buf))
            if first or mom == 0:
                t["buf"].fill_(NAN)                                  # never read: first step; never touched: no momentum
            ops.sgd_step(t["p"], gd, t["buf"], lr, mom, wd, bool(first), bool(nesterov), gs)
            return t
        a, a2 = run(), run()
        case = (n, first, nesterov, mom, wd, gs)
        assert torch.equal(a["p"], a2["p"]) and torch.equal(a["buf"].view(torch.int32), a2["buf"].view(torch.int32)), case
        r = R.sgd(p, g, buf, lr, mom, wd, first, nesterov, gs)
        G, T, lrf, momf = r["abs_gi"], r["abs_step"], R.f32(lr), R.f32(mom)
        e_g = 3 * U * G
        if mom == 0:
            assert bool(torch.isnan(a["buf"]).all()), ("momentum = 0 leaves the buffer alone", case)
            e_d = e_g
        else:
            e_b = e_g if first else e_g + 2 * U * r["abs_buf"]
            _within(_host(a["buf"]), r["buf"], e_b, "sgd buffer", case)
            e_d = e_g + momf * e_b + 2 * U * T if nesterov else e_b
        bound = lrf * e_d + U * lrf * T + U * (np.abs(p) + lrf * T)
        _within(_host(a["p"]) - p, r["update"], bound, "sgd update", case)


# ------------------------------------------------------------------------------------------------ EMA
@pytest.mark.parametrize("n", SIZES)
def test_ema_update(n):
    L, ops = _mods()
    p, e, _, _ = _arena(n, n + 2)
    pd = _dev(p)
    for alpha in (0.0, 0.5, 0.999):
        outs = []
        for _ in range(2):
            ed = _dev(e)
            ops.ema_update(ed, pd, alpha)
            outs.append(ed)
        assert torch.equal(outs[0], outs[1])
        ref, mag = R.ema(e, p, alpha)
        _within(_host(outs[0]), ref, 3 * U * (1 + 4 * U) * mag, "ema", (n, alpha))
        if alpha == 0:
            assert torch.equal(outs[0], pd), "alpha = 0 copies the student"


def test_ema_update_i64():
    L, ops = _mods()
    same = [0, 1, 7, 2999, 2 ** 24 + 1]
    e = same + [5, 100, 2999, 12345, 2 ** 24 + 1, 0, 7, 1]
    p = same + [9, 3, 0, 54321, 0, 2 ** 24 + 1, 1, 7]
    e, p = e * 5, p * 5                                              # 65 entries: a second workgroup of 64
    alphas = [0.0, 0.5, 0.999] + [min(1 - 1 / (k + 1), 0.999) for k in (1, 2, 6, 99, 998)]
    for alpha in alphas:
        outs = []
        for _ in range(2):
            ed, pd = torch.tensor(e, device="cuda"), torch.tensor(p, device="cuda")
            ops.ema_update_i64(ed, pd, alpha)
            assert pd.tolist() == p
            outs.append(ed.tolist())
        assert outs[0] == outs[1]
        for i, (got, ok) in enumerate(zip(outs[0], R.ema_i64(e, p, alpha))):
            assert got in ok, (alpha, e[i], p[i], got, ok)
            if e[i] == p[i] and e[i] < 3000:
                assert got == e[i], ("equal counters stay", alpha, e[i], got)


# ------------------------------------------------------------------------------------------------ axpy, scale
@pytest.mark.parametrize("n", SIZES)
def test_axpy_and_scale(n):
    L, ops = _mods()
    x, y, _, _ = _arena(n, n + 3)
    xd = _dev(x)
    for a in (1.0, -0.37):
        outs = []
        for _ in range(2):
            yd = _dev(y)
            assert ops.axpy(yd, xd, a) is yd
            outs.append(yd)
        assert torch.equal(outs[0], outs[1])
        ref = y.astype(np.float64) + R.f32(a) * x.astype(np.float64)
        _within(_host(outs[0]), ref, _ulp(ref), "axpy", (n, a))
    for s in (0.5, 1 / 3):
        outs = []
        for _ in range(2):
            yd = _dev(y)
            L.call("bsed_scale", L.ptr(yd), n, s, L.stream())
            outs.append(yd)
        assert torch.equal(outs[0], outs[1])
        ref = y.astype(np.float64) * R.f32(s)
        _within(_host(outs[0]), ref, _ulp(ref), "scale", (n, s))


def test_arena_argument_checks():
    L, ops = _mods()
    a, o = torch.ones(8, device="cuda"), torch.full((8,), NAN, device="cuda")
    i64 = torch.zeros(8, device="cuda", dtype=torch.int64)
    P, S = L.ptr, L.stream()
    bad = [
        ("bsed_adam_step", (P(o), P(a), P(o), P(o), 8, LR, B1, B2, ADAM_EPS, 0.0, 0, 1.0, S)),        # step < 1
        ("bsed_adam_step", (P(o), P(a), P(o), P(o), 0, LR, B1, B2, ADAM_EPS, 0.0, 1, 1.0, S)),        # n = 0
        ("bsed_adam_step", (P(o), P(a), None, P(o), 8, LR, B1, B2, ADAM_EPS, 0.0, 1, 1.0, S)),
        ("bsed_sgd_step", (P(o), P(a), None, 8, 0.1, 0.9, 0.0, 1, 1, 1.0, S)),
        ("bsed_sgd_step", (P(o), P(a), P(o), 0, 0.1, 0.9, 0.0, 1, 1, 1.0, S)),
        ("bsed_ema_update", (P(o), P(a), 0, 0.5, S)),
        ("bsed_ema_update_i64", (P(i64, torch.int64), None, 8, 0.5, S)),
        ("bsed_axpy", (P(o), None, 8, 1.0, S)),
        ("bsed_scale", (P(o), 0, 2.0, S)),
    ]
    for name, args in bad:
        with pytest.raises(L.BsedError):
            L.call(name, *args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and int(i64.abs().sum()) == 0
