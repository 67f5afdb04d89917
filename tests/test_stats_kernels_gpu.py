"""The BatchNorm-statistics kernels of csrc/cnn_ops.hip (stats_chunk + stats_finish behind bsed_bn_finalize, bsed_bn_bwd
and bsed_stats_to_grad; bn_bwd_apply, bn_eval, bn_eval_batch, colsum) and the three slab reducers of csrc/reduce.hip
against the float64 restatement in tests/stats_reference.py, whose sums are exactly rounded.

Bounds.  u = 2^-24 (fp32 unit roundoff; one correctly rounded operation errs by at most u |x| <= 1 ulp(x)),
ulp(x) = spacing of fp32 at |x|.  g(d) = d u / (1 - d u) bounds a sum in which no term passes through more than d
additions.

  statistics pair   The kernels add the fp32 partials in double: their sums differ from the exact ones by at most
                    ntiles 2^-53 sum|p|.  _fwd_condition / _bwd_condition push that (and the double roundings of the
                    formulas) through to every output and ASSERT it is below a quarter ulp of the output -- a condition
                    on the test's inputs, evaluated without the kernel.  A value within ulp/4 of the reference rounds to
                    within 0.75 ulp of it, so
      mean, invstd, coef, dgamma, dbeta, dst    1 ulp of the reference; with accumulate the add rounds once more:
                                                + 1 ulp of (old + reference)
      scale = gamma * (float)invstd             0.75 ulp(invstd) |gamma| <= 1.5 ulp(scale), + 0.5 for the product: 2 ulp
      shift = beta - (float)mean * scale        casts of mean and invstd 1.5 u each, gamma product 1, mean product 1
                                                (none under FMA contraction), the subtraction 1: 6 u, held at
                                                7 u (|beta| + |mean scale|), the seventh for the second-order terms
      running_mean = (1-m) rm + m (float)mean   fl(1-m) 1, its product 1, the cast 1.5, its product 1 (either product may
                                                fuse), the sum 1 over both terms: <= 3.5 u, held at 4 u sum|terms|
      running_var                               the same count with the cast at 1 u plus the propagated perturbation of
                                                the unbiased variance stated explicitly: 4 u sum|terms| + m d(unbiased)
  bn_bwd apply      d_y = fma(A, g, fma(B, fl(y - mean), C)) is three roundings, none passed through more than three
                    times: 4 u (|A g| + |B||y - mean| + |C|); the coefficients are within 1 ulp <= 2 u of the reference
                    ones: + 2 u of the same sum.  6 u in all.
  bn_eval           scale = gamma / sqrtf(rv + eps): the add u, halved by the root, the root u, the divide u: 2.5 u,
                    held at 3 ulp.  shift = beta - rm * scale: 2.5 u + 1 for the product on |rm scale|, 1 for the
                    subtraction on both terms: 4.5 u, held at 5 u (|beta| + |rm scale|).
  colsum            a thread adds every eighth row of its workgroup's r rows, four sums deep, then eight threads' sums
                    are added in order: no term passes more than r/8 + 2 + 8 additions; held at the looser
                    (r + 8) u sum|terms| per workgroup.  bsed_colsum finishes in double: + 1 ulp for the cast (+ 1 ulp
                    of the result with accumulate).  Queued (ops.deferred_reductions) the finish is an fp32 slab
                    reduction: + its bound below.
  slab reducers     plain kernel: slab g goes to running sum g mod 4 while four remain, the rest to sum 0; (s0 + s1) +
                    (s2 + s3): depth d = G // 4 + G % 4 + 2.  Split and batch kernels: wave w of S takes slabs w, w + S,
                    ...: n = ceil(G / S) of them at most, same four sums, then the S wave sums in order:
                    d = n // 4 + n % 4 + 2 + (S - 1).  Error <= g(d) sum|part|, + 1 ulp of the result with accumulate.
                    S follows the split rule of csrc/reduce.hip, reduce_shares (_split_s below).
  bitwise           every case is launched twice on fresh buffers and must repeat its bits; a batched or queued
                    reduction must give the bits of the immediate one; a NULL running-statistics call must give the
                    bits of the full one.
Output buffers are NaN before every launch: an element the kernel does not write fails its comparison."""
import numpy as np
import pytest
import torch

import stats_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
D = 2.0 ** -53
NAN = float("nan")
EPS, MOM = 1e-5, 0.1
TILE = 256
WORST = {}


def _mods():
    from bsed_amd import _lib as L
    from bsed_amd import ops
    return L, ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda", dtype=torch.float32)


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _gamma(d):
    return d * U / (1 - d * U)


def _within(got, ref, bound, key, what=None):
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    err = np.abs(got - ref)
    bad = ~(err <= bound)                               # NaN fails
    frac = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    assert not bad.any(), (key, what, int(bad.sum()), float(np.nanmax(frac)))
    WORST[key] = max(WORST.get(key, 0.0), float(frac.max()) if frac.size else 0.0)


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"worst error / bound  {k:28s} {WORST[k]:.3f}")


# ------------------------------------------------------------------------------------------------ inputs
def _fwd_partials(ntiles, C, seed):
    """(ntiles, 2, C) per-tile (sum y, sum y^2) of TILE positions each, with a per-channel scale.  Channel 0:
    mean^2 / var = 1e4.  Channel 1: all zero.  Channel 2: every tile holds TILE times 1.5, its second row four fp32
    steps below TILE * 2.25: s1 / count - mean^2 is slightly negative."""
    rng = np.random.default_rng(seed)
    sig = 10.0 ** rng.uniform(-1, 1, C)
    mu = 2 * sig * rng.standard_normal(C)
    zeta, chi = rng.standard_normal((ntiles, C)), rng.uniform(0.8, 1.2, (ntiles, C))
    if C >= 4:
        sig[0], mu[0] = 1.0, 100.0
        zeta[:, 0], chi[:, 0] = 0, 1
    m = mu + sig * zeta / 16
    p = np.stack([TILE * m, TILE * (sig * sig * chi + m * m)], 1).astype(np.float32)
    if C >= 4:
        p[:, :, 1] = 0
        low = np.float32(TILE * 2.25)
        for _ in range(4):
            low = np.nextafter(low, np.float32(0))
        p[:, 0, 2], p[:, 1, 2] = TILE * 1.5, low
    return p, float(ntiles * TILE)


def _bwd_partials(ntiles, C, seed, mean):
    """(ntiles, 2, C) per-tile (sum g, sum g*y) with y = mean + noise: the second row cancels against mean * first.
    Both rows carry a per-channel offset of either sign, three deviations wide: a sum of thousands of zero-mean tiles
    would cancel to where ntiles 2^-53 sum|p| no longer resolves a quarter ulp of it (_bwd_condition)."""
    rng = np.random.default_rng(seed + 1)
    sg = 10.0 ** rng.uniform(-1, 1, C)
    off = 3 * rng.choice([-1.0, 1.0], (2, C))
    p0 = (16 * sg * (rng.standard_normal((ntiles, C)) + off[0])).astype(np.float32)
    p1 = (np.asarray(mean, np.float64) * p0 + 16 * sg * (rng.standard_normal((ntiles, C)) + off[1])).astype(np.float32)
    p = np.stack([p0, p1], 1)
    if C >= 4:
        p[:, :, 1] = 0
    return p


def _quarter(delta, ref, what):
    assert np.all(delta <= 0.25 * _ulp(ref)), ("the inputs do not resolve this output to a quarter ulp", what,
                                               float(np.max(delta / _ulp(ref))))


def _fwd_condition(f, ntiles, count):
    """the propagated difference between sums that are off by ntiles 2^-53 sum|p| and the exact ones; returns the
    perturbation of the unbiased variance (used explicitly in the running_var bound)"""
    e0, e1 = ntiles * D * f["abs_s"][0], ntiles * D * f["abs_s"][1]
    mean = np.abs(f["mean"])
    d_mean = e0 / count + 2 * D * mean
    d_raw = e1 / count + 2 * mean * d_mean + 6 * D * (np.abs(f["s"][1]) / count + mean * mean)
    d_var = np.maximum(np.maximum(f["var_raw"] + d_raw, 0) - f["var"], f["var"] - np.maximum(f["var_raw"] - d_raw, 0))
    eps = R.f32(EPS)
    d_invstd = f["invstd"] * (0.5 * d_var / (np.maximum(f["var"] - d_var, 0) + eps) + 8 * D)
    _quarter(d_mean, f["mean"], "mean")
    _quarter(d_invstd, f["invstd"], "invstd")
    return d_var * (count / (count - 1) if count > 1 else 1.0) + 4 * D * f["var"]


def _bwd_condition(b, ntiles, count, gamma, mean, invstd):
    e0, e1 = ntiles * D * b["abs_s"][0], ntiles * D * b["abs_s"][1]
    m, is_ = np.abs(np.asarray(mean, np.float64)), np.asarray(invstd, np.float64)
    A = np.abs(b["coef"][0])
    d_dg = (e1 + m * e0 + 6 * D * (np.abs(b["s"][1]) + m * np.abs(b["s"][0]))) * is_
    _quarter(e0, b["dbeta"], "dbeta")
    _quarter(d_dg, b["dgamma"], "dgamma")
    _quarter(4 * D * A, b["coef"][0], "A")
    _quarter(A * is_ / count * d_dg + 8 * D * np.abs(b["coef"][1]), b["coef"][1], "B")
    _quarter(A / count * e0 + 8 * D * np.abs(b["coef"][2]), b["coef"][2], "C")


def _acc_bound(v, old):
    """1 ulp of the reference value, plus one rounding where accumulate adds"""
    return _ulp(v) + (0 if old is None else _ulp(old + v))


# ------------------------------------------------------------------------------------------------ statistics pair
def _finalize(L, ops, part, count, gamma, beta, rm, rv, nbt):
    C = part.shape[2]
    out = dict(mean=_nan(C), invstd=_nan(C), scale=_nan(C), shift=_nan(C))
    L.call("bsed_bn_finalize", L.ptr(part), part.shape[0], C, count, EPS, MOM, L.ptr(gamma), L.ptr(beta), L.ptr(rm),
           L.ptr(rv), L.ptr(nbt, torch.int64), *(L.ptr(out[k]) for k in ("mean", "invstd", "scale", "shift")),
           L.ptr(ops.stats_scratch(C, part.device), torch.float64), L.stream())
    return out


def _check_finalize(L, ops, p, count, seed):
    ntiles, _, C = p.shape
    rng = np.random.default_rng(seed + 2)
    gamma, beta = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32), (0.2 * rng.standard_normal(C)).astype(np.float32)
    rm0, rv0 = rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    f = R.bn_finalize(p, count, EPS, MOM, gamma, beta, rm0, rv0, 41)
    d_unb = _fwd_condition(f, ntiles, count)
    m = R.f32(MOM)
    pd, gd, bd = _dev(p), _dev(gamma), _dev(beta)

    def run():
        rm, rv, nbt = _dev(rm0), _dev(rv0), torch.tensor([41], device="cuda", dtype=torch.int64)
        full = _finalize(L, ops, pd, count, gd, bd, rm, rv, nbt)
        first = dict(full, running_mean=rm.clone(), running_var=rv.clone(), nbt=nbt.clone())
        bare = _finalize(L, ops, pd, count, gd, bd, None, None, None)
        _same(bare, full, "NULL running statistics change the batch statistics")
        assert torch.equal(rm, first["running_mean"]) and torch.equal(rv, first["running_var"]) and int(nbt) == 42
        again = _finalize(L, ops, pd, count, gd, bd, rm, rv, nbt)
        _same(again, full, "second call")
        return dict(first, running_mean2=rm, running_var2=rv, nbt2=nbt)

    a, b = run(), run()
    _same(a, b, "repeat")
    _within(_host(a["mean"]), f["mean"], _ulp(f["mean"]), "bn_finalize mean", (ntiles, C))
    _within(_host(a["invstd"]), f["invstd"], _ulp(f["invstd"]), "bn_finalize invstd", (ntiles, C))
    _within(_host(a["scale"]), f["scale"], 2 * _ulp(f["scale"]), "bn_finalize scale", (ntiles, C))
    _within(_host(a["shift"]), f["shift"], 7 * U * f["abs_shift"], "bn_finalize shift", (ntiles, C))
    _within(_host(a["running_mean"]), f["running_mean"], 4 * U * f["abs_running_mean"], "bn_finalize running_mean")
    _within(_host(a["running_var"]), f["running_var"], 4 * U * f["abs_running_var"] + m * d_unb,
            "bn_finalize running_var", (ntiles, C))
    assert int(a["nbt"]) == f["nbt"] == 42 and int(a["nbt2"]) == 43, "num_batches_tracked: + 1 per call"
    # the second update, from the kernel's own first one
    f2 = R.bn_finalize(p, count, EPS, MOM, gamma, beta, _host(a["running_mean"]), _host(a["running_var"]))
    _within(_host(a["running_mean2"]), f2["running_mean"], 4 * U * f2["abs_running_mean"], "bn_finalize running_mean")
    _within(_host(a["running_var2"]), f2["running_var"], 4 * U * f2["abs_running_var"] + m * d_unb,
            "bn_finalize running_var", (ntiles, C))
    if C >= 4 and count > 1:
        assert f["mean"][0] ** 2 / f["var"][0] == pytest.approx(1e4, rel=0.05)
        assert f["var_raw"][2] < 0 and f["var"][2] == 0 and float(a["invstd"][2]) == pytest.approx(EPS ** -0.5, rel=1e-6)
        assert float(a["mean"][1]) == 0 and float(a["shift"][1]) == float(beta[1])
    assert all(bool(torch.isfinite(a[k]).all()) for k in a)
    return f


def _check_bwd_coefficients(L, ops, ntiles, C, count, seed, f):
    rng = np.random.default_rng(seed + 3)
    gamma = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    mean, invstd = f["mean"].astype(np.float32), f["invstd"].astype(np.float32)
    p = _bwd_partials(ntiles, C, seed, mean)
    b = R.bn_bwd(p, count, gamma, mean, invstd)
    _bwd_condition(b, ntiles, count, gamma, mean, invstd)
    old = rng.standard_normal((2, C)).astype(np.float32)
    pd, gd, md, sd = _dev(p), _dev(gamma), _dev(mean), _dev(invstd)
    for acc in (0, 1):
        def run():
            dg, db = (_dev(old[0]), _dev(old[1])) if acc else (_nan(C), _nan(C))
            coef = _nan(3, C)
            L.call("bsed_bn_bwd", L.ptr(pd), ntiles, C, count, L.ptr(gd), L.ptr(md), L.ptr(sd), L.ptr(dg), L.ptr(db),
                   acc, None, None, C, L.ptr(coef), L.ptr(ops.stats_scratch(C, pd.device), torch.float64), L.stream())
            return dict(dgamma=dg, dbeta=db, coef=coef)
        a, a2 = run(), run()
        _same(a, a2, ("bn_bwd repeat", acc))
        o = old.astype(np.float64) if acc else (None, None)
        _within(_host(a["coef"]), b["coef"], _ulp(b["coef"]), "bn_bwd coef", (ntiles, C, acc))
        _within(_host(a["dgamma"]), b["dgamma"] + (o[0] if acc else 0), _acc_bound(b["dgamma"], o[0]),
                "bn_bwd dgamma", (ntiles, C, acc))
        _within(_host(a["dbeta"]), b["dbeta"] + (o[1] if acc else 0), _acc_bound(b["dbeta"], o[1]),
                "bn_bwd dbeta", (ntiles, C, acc))
    if C >= 4:
        assert float(a["dgamma"][1]) == float(old[0, 1]) and float(a["coef"][1, 1]) == 0      # the all-zero channel


def _check_to_grad(L, ops, p, seed):
    ntiles, _, C = p.shape
    s, sa = R.exact_sum(p)
    rng = np.random.default_rng(seed + 4)
    old = rng.standard_normal(C).astype(np.float32)
    pd = _dev(p)
    for which in (0, 1):
        _quarter(ntiles * D * sa[which], s[which], ("stats_to_grad", which))
        for acc in (0, 1):
            def run():
                dst = _dev(old) if acc else _nan(C)
                L.call("bsed_stats_to_grad", L.ptr(pd), ntiles, C, which, L.ptr(dst), acc,
                       L.ptr(ops.stats_scratch(C, pd.device), torch.float64), L.stream())
                return dst
            a, a2 = run(), run()
            assert torch.equal(a, a2), ("stats_to_grad repeat", which, acc)
            o = old.astype(np.float64) if acc else None
            _within(_host(a), s[which] + (o if acc else 0), _acc_bound(s[which], o), "stats_to_grad",
                    (ntiles, C, which, acc))
    if C >= 4:                                     # ops.stats_to_grad outside a deferred block: the same entry point
        dst = _dev(old)
        ops.stats_to_grad(pd, C, 1, dst)
        assert torch.equal(dst, a), "ops.stats_to_grad(which = 1)"


NTILES = [1, 7, 24, 25, 100, 128, 129, 255, 3973, 4229]


@pytest.mark.parametrize("ntiles", NTILES)
def test_statistics_pair(ntiles):
    """The launch has min(128, ntiles) chunks of ceil(ntiles / chunks) tiles; eight tile groups share a chunk, eight chunk
    groups the finish.  1: one tile, one chunk.  7, 24: one tile per chunk, the finish kernel's remainder loop alone.
    25, 100: its four-per-trip loop for some groups, a remainder for others.  128: every group takes four trips of
    four, no remainder.  129: 128 chunks of 2 tiles, chunks 65 .. 127 empty.  255: two tiles per chunk, the last chunk
    short.  3973: 32 tiles per chunk, the chunk kernel's four-per-trip loop without a remainder; 4229: 34 per chunk,
    with one."""
    L, ops = _mods()
    for C in (4, 16, 40, 64, 132):
        p, count = _fwd_partials(ntiles, C, 1000 * ntiles + C)
        f = _check_finalize(L, ops, p, count, 1000 * ntiles + C)
        _check_bwd_coefficients(L, ops, ntiles, C, count, 1000 * ntiles + C, f)
        _check_to_grad(L, ops, p, 1000 * ntiles + C)
    p, _ = _fwd_partials(ntiles, 1, ntiles)
    _check_to_grad(L, ops, p, ntiles)              # C = 1: the discriminator's dense bias


def test_finalize_count_one():
    """one position: s1 / count - mean^2 is the rounding of x^2, either sign; the unbiased variance must not divide by
    count - 1 = 0"""
    L, ops = _mods()
    x = np.array([1.7, -0.3, 0.0, 123.456], np.float32)
    p = np.stack([x, x * x])[None].astype(np.float32)
    f = _check_finalize(L, ops, p, 1.0, 77)           # every output finite, the running variance among them
    assert np.array_equal(f["unbiased"], f["var"])


def test_statistics_argument_checks():
    L, ops = _mods()
    a, o = torch.ones(64, device="cuda"), _nan(64)
    n64 = torch.zeros(1, device="cuda", dtype=torch.int64)
    P, S, sc = L.ptr, L.stream(), L.ptr(ops.stats_scratch(4, a.device), torch.float64)
    bad = [
        ("bsed_bn_finalize", (P(a), 0, 4, 8.0, EPS, MOM, P(a), P(a), None, None, None, P(o), P(o), P(o), P(o), sc, S)),
        ("bsed_bn_finalize", (P(a), 1, 4, 0.0, EPS, MOM, P(a), P(a), None, None, None, P(o), P(o), P(o), P(o), sc, S)),
        ("bsed_bn_finalize", (P(a), 1, 4, 8.0, EPS, MOM, P(a), P(a), None, None, P(n64, torch.int64), P(o), P(o), P(o),
                              None, sc, S)),
        ("bsed_bn_bwd", (P(a), 1, 6, 8.0, P(a), P(a), P(a), P(o), P(o), 0, None, None, 6, P(o), sc, S)),      # C % 4
        ("bsed_bn_bwd", (P(a), 1, 4, 8.0, P(a), P(a), P(a), P(o), P(o), 0, P(o), None, 4, P(o), sc, S)),      # g without y
        ("bsed_bn_bwd", (P(a), 1, 4, 8.0, P(a), P(a), P(a), P(o), P(o), 0, None, None, 6, P(o), sc, S)),      # n % C
        ("bsed_stats_to_grad", (P(a), 1, 4, 2, P(o), 0, sc, S)),                                            # which
        ("bsed_stats_to_grad", (P(a), 0, 4, 0, P(o), 0, sc, S)),
        ("bsed_colsum", (P(a), 4, 8, 7, P(o), 2, P(o), 0, sc, S)),                                          # pitch < C
        ("bsed_colsum_part", (P(a), 4, 8, 7, P(o), 2, S)),
        ("bsed_colsum_part", (P(a), 4, 4, 4, P(o), 5, S)),                                                  # G > M
        ("bsed_reduce_partials", (P(a), 1, 1, 2, 4, 3, 4, P(o), 0, 4, 1, 0, S)),                            # K > KP
        ("bsed_reduce_partials", (P(a), 0, 1, 4, 4, 4, 4, P(o), 0, 4, 1, 0, S)),                            # G = 0
    ]
    for name, args in bad:
        with pytest.raises(L.BsedError):
            L.call(name, *args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and int(n64) == 0


# ------------------------------------------------------------------------------------------------ bn_bwd with the apply pass
@pytest.mark.parametrize("P,C", [(1, 4), (3, 16), (257, 40), (524291, 16)])
def test_bn_bwd_apply(P, C):
    """(524291, 16): 2097164 float4 groups, past the 8192 x 256 the capped grid covers in one trip"""
    L, ops = _mods()
    if P > 10 ** 5:
        assert (P * C // 4 - 1) // 256 + 1 > 8192
    rng = np.random.default_rng(P + C)
    ntiles = -(-P // TILE)
    mean = rng.standard_normal(C).astype(np.float32)
    invstd = rng.uniform(0.5, 2, C).astype(np.float32)
    gamma = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    part = _bwd_partials(ntiles, C, P, mean)
    g = rng.standard_normal((P, C)).astype(np.float32)
    y = (mean + rng.standard_normal((P, C)) / invstd).astype(np.float32)
    b = R.bn_bwd(part, P, gamma, mean, invstd)
    _bwd_condition(b, ntiles, P, gamma, mean, invstd)
    ref, mag = R.bn_bwd_apply(g, y, b["coef"], mean)
    pd, gd, md, sd, yd = _dev(part), _dev(gamma), _dev(mean), _dev(invstd), _dev(y)
    y0 = yd.clone()

    def run():
        out = dict(g=_dev(g), dgamma=_nan(C), dbeta=_nan(C), coef=_nan(3, C))
        L.call("bsed_bn_bwd", L.ptr(pd), ntiles, C, float(P), L.ptr(gd), L.ptr(md), L.ptr(sd), L.ptr(out["dgamma"]),
               L.ptr(out["dbeta"]), 0, L.ptr(out["g"]), L.ptr(yd), P * C, L.ptr(out["coef"]),
               L.ptr(ops.stats_scratch(C, pd.device), torch.float64), L.stream())
        return out
    a, a2 = run(), run()
    _same(a, a2, "repeat")
    assert torch.equal(yd, y0), "y is an input"
    _within(_host(a["coef"]), b["coef"], _ulp(b["coef"]), "bn_bwd coef", (P, C))
    _within(_host(a["dgamma"]), b["dgamma"], _ulp(b["dgamma"]), "bn_bwd dgamma", (P, C))
    _within(_host(a["dbeta"]), b["dbeta"], _ulp(b["dbeta"]), "bn_bwd dbeta", (P, C))
    _within(_host(a["g"]), ref, 6 * U * mag, "bn_bwd apply", (P, C))
    # the wrapper: accumulate = 1 into the gradients, the same d_y bits
    old = rng.standard_normal((2, C)).astype(np.float32)
    dg, db, gw = _dev(old[0]), _dev(old[1]), _dev(g)
    coef = ops.bn_bwd(pd, C, float(P), gd, md, sd, dg, db, gw, yd)
    assert torch.equal(gw, a["g"]) and torch.equal(coef, a["coef"])
    _within(_host(dg), b["dgamma"] + old[0], _acc_bound(b["dgamma"], old[0].astype(np.float64)), "bn_bwd dgamma")
    _within(_host(db), b["dbeta"] + old[1], _acc_bound(b["dbeta"], old[1].astype(np.float64)), "bn_bwd dbeta")


# ------------------------------------------------------------------------------------------------ bn_eval
def _eval_inputs(C, seed):
    rng = np.random.default_rng(seed)
    gamma, beta = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32), (0.2 * rng.standard_normal(C)).astype(np.float32)
    rm, rv = rng.standard_normal(C).astype(np.float32), (10.0 ** rng.uniform(-3, 1, C)).astype(np.float32)
    rv[0] = 0.0                                                     # a channel that never varied
    return gamma, beta, rm, rv


def _eval_single(L, C, ins):
    scale, shift = _nan(C), _nan(C)
    L.call("bsed_bn_eval", C, EPS, *(L.ptr(t) for t in ins), L.ptr(scale), L.ptr(shift), L.stream())
    return scale, shift


@pytest.mark.parametrize("C", [1, 16, 128, 132])
def test_bn_eval(C):
    L, ops = _mods()
    host = _eval_inputs(C, C)
    ins = [_dev(v) for v in host]
    scale, shift = _eval_single(L, C, ins)
    again = _eval_single(L, C, ins)
    assert torch.equal(scale, again[0]) and torch.equal(shift, again[1])
    r_scale, r_shift, mag = R.bn_eval(EPS, *host)
    _within(_host(scale), r_scale, 3 * _ulp(r_scale), "bn_eval scale", C)
    _within(_host(shift), r_shift, 5 * U * mag, "bn_eval shift", C)
    w_scale, w_shift = ops.bn_eval(C, EPS, *ins)
    assert torch.equal(w_scale, scale) and torch.equal(w_shift, shift)


def _eval_jobs(L, ins, outs):
    arr = (L.STRUCTS["BsedBnEvalJob"] * max(len(ins), 1))()
    for a, (gamma, beta, rm, rv), (scale, shift) in zip(arr, ins, outs):
        a.gamma, a.beta, a.running_mean, a.running_var = (t.data_ptr() for t in (gamma, beta, rm, rv))
        a.scale, a.shift, a.C = scale.data_ptr(), shift.data_ptr(), gamma.numel()
    return arr


def test_bn_eval_batch():
    L, ops = _mods()
    assert ops.BN_EVAL_MAX_JOBS == 16
    widths = [1, 16, 128, 132, 132, 1, 128, 16, 40, 129, 127, 4, 1, 132, 64, 33, 16]
    ins = [[_dev(v) for v in _eval_inputs(C, 100 + i)] for i, C in enumerate(widths)]
    single = [_eval_single(L, C, t) for C, t in zip(widths, ins)]
    for _ in range(2):
        outs = [(_nan(C + 3), _nan(C + 3)) for C in widths]           # three more: nothing is written past C
        L.call("bsed_bn_eval_batch", _eval_jobs(L, ins[:16], outs[:16]), 16, EPS, L.stream())
        for C, (sc, sh), (s1, h1) in zip(widths[:16], outs, single):
            assert torch.equal(sc[:C], s1) and torch.equal(sh[:C], h1), C
            assert bool(torch.isnan(sc[C:]).all()) and bool(torch.isnan(sh[C:]).all())
    wrapped = ops.bn_eval_batch([(C, *t) for C, t in zip(widths[:16], ins)], EPS)
    for (sc, sh), (s1, h1) in zip(wrapped, single):
        assert torch.equal(sc, s1) and torch.equal(sh, h1)
    outs = [(_nan(C), _nan(C)) for C in widths]
    with pytest.raises(L.BsedError):
        L.call("bsed_bn_eval_batch", _eval_jobs(L, ins, outs), 17, EPS, L.stream())
    with pytest.raises(L.BsedError):
        L.call("bsed_bn_eval_batch", _eval_jobs(L, ins, outs), 0, EPS, L.stream())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for pair in outs for t in pair)


# ------------------------------------------------------------------------------------------------ colsum
def _pitched(M, C, pitch, seed):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((M, pitch)) * 10.0 ** rng.uniform(-1, 1, pitch)).astype(np.float32)
    a[:, C:] = np.nan                                               # a read past C shows
    return a


@pytest.mark.parametrize("M,C,pitch,G", [(1, 1, 1, 1), (5, 40, 48, 512), (200, 40, 48, 3), (257, 768, 768, 8),
                                         (1000, 20, 20, 512)])
def test_colsum(M, C, pitch, G):
    """(5, .., 512): G clamps to M.  (200, .., 3): 67 rows per workgroup, two four-per-trip rounds and a remainder.
    (1000, 20, 20, 512): two rows per workgroup, workgroups 500 .. 511 without rows write zeros."""
    L, ops = _mods()
    a = _pitched(M, C, pitch, M + C)
    ad = _dev(a)
    g = min(G, M)
    per = -(-M // g)
    s, sa = R.colsum(a, M, C, pitch)
    rng = np.random.default_rng(M)
    old = rng.standard_normal(C).astype(np.float32)
    scratch = L.ptr(ops.stats_scratch(C, ad.device), torch.float64)
    parts = []
    for acc in (0, 1):
        def run():
            part, dst = _nan(G, 2, C), (_dev(old) if acc else _nan(C))
            L.call("bsed_colsum", L.ptr(ad), M, C, pitch, L.ptr(part), G, L.ptr(dst), acc, scratch, L.stream())
            return dict(part=part, dst=dst)
        r, r2 = run(), run()
        assert torch.equal(r["dst"], r2["dst"]) and torch.equal(r["part"][:g], r2["part"][:g])
        o = old.astype(np.float64) if acc else None
        _within(_host(r["dst"]), s + (o if acc else 0), (per + 8) * U * sa + _acc_bound(s, o), "colsum", (M, C, acc))
        parts.append(r["part"])
    part = parts[0]
    assert torch.equal(parts[0][:g], parts[1][:g])
    assert bool(torch.isnan(part[g:]).all()), "only min(G, M) workgroups write"
    assert float(part[:g, 1].abs().max()) == 0.0
    ph = _host(part)
    for blk in range(g):
        bs, bsa = R.colsum(a, M, C, pitch, rows=(min(blk * per, M), min((blk + 1) * per, M)))
        _within(ph[blk, 0], bs, (per + 8) * U * bsa, "colsum_kernel part", (M, C, blk))
    alone = _nan(g, 2, C)
    L.call("bsed_colsum_part", L.ptr(ad), M, C, pitch, L.ptr(alone), g, L.stream())
    assert torch.equal(alone, part[:g]), "bsed_colsum_part: the first stage of bsed_colsum"
    # the wrapper, outside a deferred block: min(512, M) workgroups, float64 finish
    gw = min(512, M)
    dst = _dev(old)
    ops.colsum(ad, M, C, pitch, dst)
    _within(_host(dst), s + old, (-(-M // gw) + 8) * U * sa + _acc_bound(s, old.astype(np.float64)), "colsum", "ops")


# ------------------------------------------------------------------------------------------------ slab reducers
def _split_s(G, total):
    """the split rule of csrc/reduce.hip (reduce_shares): 0 = the plain kernel; else S waves share the slabs of 64 elements"""
    wgs = -(-total // 64)
    if not (wgs < 1024 and G >= 8):
        return 0
    S = 1
    while S < 16 and wgs * S < 1024 and 4 * S <= G:
        S *= 2
    return S


def _depth(G, S):
    n = -(-G // max(S, 1))
    return n // 4 + n % 4 + 2 + max(S, 1) - 1


def _reduce_cases():
    cases = []

    def add(G, ntaps, KP, NP, K, N, strides=None, off=0, size=None):
        strides = strides or (K * N, N, 1)
        size = size or ntaps * K * N
        for acc in (0, 1):
            cases.append(dict(G=G, ntaps=ntaps, KP=KP, NP=NP, K=K, N=N, strides=strides, off=off, size=size, acc=acc,
                              S=_split_s(G, ntaps * KP * NP), seed=len(cases)))
    for G in (1, 3, 7):
        add(G, 1, 16, 16, 16, 16)
    add(9, 9, 128, 64, 128, 64)
    for G in (8, 9, 31, 64, 129, 200):
        add(G, 1, 16, 16, 16, 16)
    add(9, 9, 64, 64, 64, 64)
    K, KP, N, NP = 10, 16, 20, 32
    for G in (5, 31):
        add(G, 9, KP, NP, K, N, (1, 9, 9 * K), off=7)               # the PyTorch (N, K, 3, 3) weight
        add(G, 1, KP, NP, K, N, (0, 1, K), off=3)                   # a Linear (N, K) weight
        add(G, 1, KP, NP, K, N, (0, N, 1), off=1)                   # its transpose
        add(G, 1, KP, NP, K, N, (0, N + 3, 1), off=2, size=K * (N + 3))   # rows with a pitch: gaps inside the pattern
    return cases


def _reduce_inputs(c):
    rng = np.random.default_rng(c["seed"])
    part = rng.standard_normal((c["G"], c["ntaps"], c["KP"], c["NP"])).astype(np.float32)
    part *= (10.0 ** rng.uniform(-1, 1, (c["ntaps"], c["KP"], c["NP"]))).astype(np.float32)
    part[:, :, c["K"]:], part[:, :, :, c["N"]:] = np.nan, np.nan    # the padding is never read
    dst = rng.standard_normal(c["off"] + c["size"] + 5).astype(np.float32)   # start values and sentinels
    return part, dst


def _reduce_now(L, c, pd, dst):
    L.call("bsed_reduce_partials", L.ptr(pd), c["G"], c["ntaps"], c["KP"], c["NP"], c["K"], c["N"],
           L.ptr(dst[c["off"]:]), *c["strides"], c["acc"], L.stream())


def _job_array(L, jobs):
    arr = (L.STRUCTS["BsedReduceJob"] * len(jobs))()
    for a, (c, pd, dst) in zip(arr, jobs):
        a.part, a.dst = pd.data_ptr(), dst[c["off"]:].data_ptr()
        a.G, a.ntaps, a.KP, a.NP, a.K, a.N, a.accumulate = c["G"], c["ntaps"], c["KP"], c["NP"], c["K"], c["N"], c["acc"]
        a.s_tap, a.s_k, a.s_n = c["strides"]
    return arr


def test_reduce_partials_immediate_and_batched():
    L, ops = _mods()
    cases = _reduce_cases()
    assert len(cases) <= ops.REDUCE_MAX_JOBS == 40
    # G = 1, 3, 7 and the 73728-element output: the plain kernel.  16 x 16 outputs, G = 8 .. 200: S = 4, 4, 8, 16, 16,
    # 16 waves (4 S <= G), 129 and 200 entering the eight-in-flight loop (G > 7 S).  36864 elements, G = 9: S = 2.
    assert [c["S"] for c in cases if c["acc"] == 0][:11] == [0, 0, 0, 0, 4, 4, 8, 16, 16, 16, 2]
    assert {c["S"] for c in cases[22:]} == {0, 8} and all(c["G"] > 7 * c["S"] for c in cases if c["G"] >= 129)
    jobs, now = [], []
    for c in cases:
        part, dst0 = _reduce_inputs(c)
        pd = _dev(part)
        ref, mag, hit = R.reduce_partials(part, c["K"], c["N"], dst0, *c["strides"], c["acc"], dst_offset=c["off"])
        outs = []
        for _ in range(2):
            dst = _dev(dst0)
            _reduce_now(L, c, pd, dst)
            outs.append(dst)
        assert torch.equal(outs[0], outs[1]), ("repeat", c)
        got = _host(outs[0])
        assert np.array_equal(got[~hit], dst0.astype(np.float64)[~hit]), ("a sentinel outside the pattern changed", c)
        bound = _gamma(_depth(c["G"], c["S"])) * mag + (_ulp(ref) if c["acc"] else 0)
        _within(got[hit], ref[hit], bound[hit], "reduce_partials " + ("plain" if c["S"] == 0 else "split"), c)
        now.append(outs[0])
        jobs.append((c, pd, dst0))
    for _ in range(2):
        batch = [(c, pd, _dev(dst0)) for c, pd, dst0 in jobs]
        L.call("bsed_reduce_partials_batch", _job_array(L, batch), len(batch), L.stream())
        for (c, _, dst), want in zip(batch, now):
            assert torch.equal(dst, want), ("a batched reduction differs from the immediate one", c)
    # refused before any launch: one job too many; two jobs with one destination
    c = dict(cases[0], acc=0)
    part, _ = _reduce_inputs(c)
    pd = _dev(part)
    many = [(c, pd, _nan(c["size"] + 5)) for _ in range(ops.REDUCE_MAX_JOBS + 1)]
    with pytest.raises(L.BsedError):
        L.call("bsed_reduce_partials_batch", _job_array(L, many), len(many), L.stream())
    twice = _nan(c["size"] + 5)
    with pytest.raises(L.BsedError):
        L.call("bsed_reduce_partials_batch", _job_array(L, [(c, pd, twice), many[0], (c, pd, twice)]), 3, L.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(twice).all()) and all(bool(torch.isnan(d).all()) for _, _, d in many)


def test_deferred_reductions_keep_order_and_bits():
    """two reductions into one destination inside ops.deferred_reductions() go to successive launches, in order"""
    L, ops = _mods()
    for G in (5, 31, 200):
        c = dict(G=G, ntaps=1, KP=16, NP=32, K=10, N=20, strides=(0, 20, 1), off=4, size=200, acc=0, seed=G)
        p1, dst0 = _reduce_inputs(c)
        p2, _ = _reduce_inputs(dict(c, seed=G + 1))
        other, _ = _reduce_inputs(dict(c, seed=G + 2))
        d1, d2, d3 = _dev(p1), _dev(p2), _dev(other)
        want, want3 = _dev(dst0), _dev(dst0)
        args = (G, 1, 16, 32, 10, 20)
        ops.reduce_partials(d1, *args, want, 0, 20, 1, accumulate=False, dst_offset=4)
        ops.reduce_partials(d2, *args, want, 0, 20, 1, accumulate=True, dst_offset=4)
        ops.reduce_partials(d3, *args, want3, 0, 20, 1, accumulate=True, dst_offset=4)
        got, got3 = _dev(dst0), _dev(dst0)
        with ops.deferred_reductions():
            ops.reduce_partials(d1, *args, got, 0, 20, 1, accumulate=False, dst_offset=4)
            ops.reduce_partials(d3, *args, got3, 0, 20, 1, accumulate=True, dst_offset=4)
            ops.reduce_partials(d2, *args, got, 0, 20, 1, accumulate=True, dst_offset=4)
            assert torch.equal(got, _dev(dst0)), "queued, not launched"
        assert torch.equal(got, want) and torch.equal(got3, want3), G
        now = _dev(dst0)
        with ops.deferred_reductions():
            ops.reduce_partials(d1, *args, now, 0, 20, 1, accumulate=False, dst_offset=4, defer=False)
            assert not torch.equal(now, _dev(dst0)), "defer = False runs inside the block"


@pytest.mark.parametrize("ntiles,C", [(7, 1), (129, 40), (4229, 132), (200, 16)])
def test_queued_stats_to_grad_and_colsum(ntiles, C):
    """inside ops.deferred_reductions() ops.stats_to_grad(which = 0) and ops.colsum finish in fp32 through the batch
    reducer; outside in double through bsed_stats_to_grad.  Each route at its own bound."""
    L, ops = _mods()
    p, _ = _fwd_partials(ntiles, C, ntiles + C)
    s, sa = R.exact_sum(p)
    rng = np.random.default_rng(ntiles)
    old = rng.standard_normal(C).astype(np.float32)
    o = old.astype(np.float64)
    pd = _dev(p)
    # immediate
    _quarter(ntiles * D * sa[0], s[0], "stats_to_grad")
    dst = _dev(old)
    ops.stats_to_grad(pd, C, 0, dst)
    _within(_host(dst), s[0] + o, _acc_bound(s[0], o), "stats_to_grad", (ntiles, C, "immediate"))
    # queued: a slab reduction of G = ntiles slabs of (KP = 2, NP = C), row 0 only
    S = _split_s(ntiles, 2 * C)
    outs = []
    for _ in range(2):
        q = _dev(old)
        with ops.deferred_reductions():
            ops.stats_to_grad(pd, C, 0, q)
            assert torch.equal(q, _dev(old))
        outs.append(q)
    assert torch.equal(outs[0], outs[1])
    bound_q = _gamma(_depth(ntiles, S)) * sa[0] + _ulp(s[0] + o)
    _within(_host(outs[0]), s[0] + o, bound_q, "stats_to_grad queued", (ntiles, C, S))
    # colsum of an (M, C) matrix, M = ntiles rows
    M, pitch = ntiles, C + 8
    a = _pitched(M, C, pitch, ntiles)
    ad = _dev(a)
    cs, csa = R.colsum(a, M, C, pitch)
    G = min(512, M)
    per = -(-M // G)
    for acc in (False, True):
        q = _dev(old) if acc else _nan(C)
        with ops.deferred_reductions():
            ops.colsum(ad, M, C, pitch, q, accumulate=acc)
        oo = o if acc else 0
        first = (per + 8) * U                           # the workgroup sums, then the slab reduction of those
        bound = (first + _gamma(_depth(G, _split_s(G, 2 * C))) * (1 + first)) * csa + (_ulp(cs + oo) if acc else 0)
        _within(_host(q), cs + oo, bound, "colsum queued", (M, C, acc))
