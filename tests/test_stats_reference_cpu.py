"""tests/stats_reference.py checked on its own in float64: the bounds of tests/test_stats_kernels_gpu.py and
tests/test_arena_kernels_gpu.py mean something only where the reference states the operation it claims to.  BatchNorm
forward, running statistics and backward against torch.nn.functional.batch_norm + autograd; the strided destination
addressing of reduce_partials against einsum + permute; Adam / SGD against torch.optim; the int64 EMA's fixed point."""
import numpy as np
import pytest
import torch

import stats_reference as R

P, C, TILE = 1000, 40, 128
EPS, MOM = 1e-5, 0.1
REL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = float(np.abs(got - want).max())
    assert err <= REL * float(np.abs(want).max()), (what, err)


def _tiles(*cols):
    """per-128-position partials in float64: (ntiles, len(cols), C)"""
    n = -(-P // TILE)
    return np.stack([np.stack([c[t * TILE:(t + 1) * TILE].sum(0) for c in cols]) for t in range(n)])


def _data(seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((P, C)) * (0.5 + rng.random(C)) + 3 * rng.standard_normal(C)
    return x, rng.standard_normal((P, C)), 1 + 0.3 * rng.standard_normal(C), 0.2 * rng.standard_normal(C)


def test_bn_train_forward_running_stats_and_backward_match_autograd():
    rm, rv, nbt = np.zeros(C), np.ones(C), 0
    t_rm, t_rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    for call in range(2):
        x, g, gamma, beta = _data(call)
        tx, tg, tb = (torch.tensor(a, requires_grad=True) for a in (x, gamma, beta))
        out = torch.nn.functional.batch_norm(tx, t_rm, t_rv, tg, tb, training=True, momentum=R.f32(MOM), eps=R.f32(EPS))
        out.backward(torch.from_numpy(g))
        part = _tiles(x, x * x)
        assert part.shape == (8, 2, C)
        f = R.bn_finalize(part, P, EPS, MOM, gamma, beta, rm, rv, nbt)
        _close(x * f["scale"] + f["shift"], out.detach().numpy(), "forward through scale / shift")
        rm, rv, nbt = f["running_mean"], f["running_var"], f["nbt"]
        _close(rm, t_rm.numpy(), ("running_mean", call))
        _close(rv, t_rv.numpy(), ("running_var", call))
        b = R.bn_bwd(_tiles(g, g * x), P, gamma, f["mean"], f["invstd"])
        d_y, mag = R.bn_bwd_apply(g, x, b["coef"], f["mean"])
        _close(d_y, tx.grad.numpy(), "d_x")
        _close(b["dgamma"], tg.grad.numpy(), "d_gamma")
        _close(b["dbeta"], tb.grad.numpy(), "d_beta")
        assert np.all(mag >= np.abs(d_y) * (1 - 1e-12))
    assert nbt == 2


def test_bn_finalize_edges():
    # count == 1: the unbiased variance is the plain one, nothing divides by zero
    f = R.bn_finalize(np.array([[[3.0], [9.0]]]), 1, EPS, MOM, [1.0], [0.0], [0.0], [1.0], 5)
    assert f["var"][0] == 0 and f["running_var"][0] == pytest.approx(1 - R.f32(MOM)) and f["nbt"] == 6
    # a slightly negative s1/count - mean^2 clamps to 0: invstd = 1/sqrt(eps)
    f = R.bn_finalize(np.array([[[4.0], [7.9999]]]), 2, EPS, MOM, [1.0], [0.0])
    assert f["var_raw"][0] < 0 and f["var"][0] == 0 and f["invstd"][0] == pytest.approx(R.f32(EPS) ** -0.5, rel=1e-15)
    assert "running_mean" not in f and "nbt" not in f


def test_bn_eval_matches_eval_mode_batch_norm():
    x, _, gamma, beta = _data(7)
    rng = np.random.default_rng(8)
    rm, rv = rng.standard_normal(C), 0.1 + rng.random(C)
    out = torch.nn.functional.batch_norm(*(torch.from_numpy(a) for a in (x, rm, rv, gamma, beta)), training=False,
                                         eps=R.f32(EPS))
    scale, shift, mag = R.bn_eval(EPS, gamma, beta, rm, rv)
    _close(x * scale + shift, out.numpy(), "eval forward")
    assert np.all(mag >= np.abs(shift))


def test_colsum_reads_c_columns_of_a_pitched_matrix():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((37, 48))
    a[:, 40:] = np.nan
    s, sa = R.colsum(a.reshape(-1), 37, 40, 48)
    _close(s, a[:, :40].sum(0), "colsum")
    _close(sa, np.abs(a[:, :40]).sum(0), "colsum magnitudes")
    s, _ = R.colsum(a.reshape(-1), 37, 40, 48, rows=(8, 16))
    _close(s, a[8:16, :40].sum(0), "colsum of a row range")


@pytest.mark.parametrize("accumulate", [0, 1])
def test_reduce_partials_addressing(accumulate):
    """the layouts the models use: (1, 9, 9K) is the PyTorch (N, K, 3, 3) conv weight, (0, 1, K) a Linear (N, K) weight,
    (0, N, 1) its transpose (K, N); padding K < KP, N < NP is never read; a dst_offset shifts the pattern"""
    rng = np.random.default_rng(5)
    G, K, KP, N, NP, off = 6, 10, 16, 20, 32, 7
    for ntaps, strides, shape, perm in ((9, (1, 9, 9 * K), (N, K, 9), "tkn->nkt"), (1, (0, 1, K), (N, K), "tkn->nk"),
                                        (1, (0, N, 1), (K, N), "tkn->kn")):
        part = rng.standard_normal((G, ntaps, KP, NP))
        part[:, :, K:], part[:, :, :, N:] = np.nan, np.nan
        size = int(np.prod(shape))
        dst = rng.standard_normal(off + size + 5)
        out, mag, hit = R.reduce_partials(part, K, N, dst, *strides, accumulate, dst_offset=off)
        want = torch.einsum("g" + perm, torch.from_numpy(part[:, :, :K, :N])).numpy().reshape(-1)
        body = out[off:off + size]
        _close(body, want + (dst[off:off + size] if accumulate else 0), (strides, "values"))
        assert np.array_equal(out[:off], dst[:off]) and np.array_equal(out[off + size:], dst[off + size:])
        assert hit[off:off + size].all() and hit.sum() == size
        assert np.all(mag[hit] >= np.abs(out[hit]) * (1 - 1e-12))


def _f32s(*a):
    return [R.f32(v) for v in a]


@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 0.25)])
def test_adam_matches_torch_optim(wd, gs):
    rng = np.random.default_rng(11)
    n = 50
    lr, b1, b2, eps, wdf = _f32s(1e-3, 0.9, 0.999, 1e-8, wd)
    p = rng.standard_normal(n)
    tp = torch.tensor(p, requires_grad=True)
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wdf)
    m, v = np.zeros(n), np.zeros(n)
    for step in (1, 2, 3):
        g = rng.standard_normal(n)
        tp.grad = torch.from_numpy(g * R.f32(gs))
        opt.step()
        r = R.adam(p, g, m, v, lr, b1, b2, eps, wd, step, gs)
        p, m, v = p + r["update"], r["m"], r["v"]
        _close(p, tp.detach().numpy(), ("adam", step))
        _close(R.adam_update(m, v, lr, b1, b2, eps, step), r["update"], "update from the moments")


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("nesterov", [0, 1])
@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 0.25)])
def test_sgd_matches_torch_optim(momentum, nesterov, wd, gs):
    if nesterov and momentum == 0:
        nesterov = 0                  # torch refuses the pair; the kernel ignores nesterov without momentum
    rng = np.random.default_rng(12)
    n = 50
    lr, mom, wdf = _f32s(0.05, momentum, wd)
    p = rng.standard_normal(n)
    tp = torch.tensor(p, requires_grad=True)
    opt = torch.optim.SGD([tp], lr=lr, momentum=mom, nesterov=bool(nesterov), weight_decay=wdf)
    buf = np.full(n, 123.0)           # never read on the first step
    for step in range(3):
        g = rng.standard_normal(n)
        tp.grad = torch.from_numpy(g * R.f32(gs))
        opt.step()
        r = R.sgd(p, g, buf, lr, momentum, wd, step == 0, nesterov, gs)
        p = p + r["update"]
        if momentum:
            buf = r["buf"]
        else:
            assert r["buf"] is None
        _close(p, tp.detach().numpy(), ("sgd", step))


def test_ema_and_round_f32():
    e, p = np.array([1.0, -2.0, 0.5]), np.array([3.0, 4.0, -1.0])
    out, mag = R.ema(e, p, 0.999)
    a = R.f32(0.999)
    _close(out, e * a + p * (1 - a), "ema")
    rng = np.random.default_rng(2)
    for x in np.concatenate([rng.standard_normal(200) * 10.0 ** rng.integers(-20, 20, 200), [2.0 ** 24 + 1, 1 - 2.0 ** -25]]):
        assert R.round_f32(x) == float(np.float32(x)), x
    assert R.round_f32(2 ** 24 + 1) == 2.0 ** 24 and R.round_f32(2 ** 24 + 3) == 2.0 ** 24 + 4      # ties to even


def test_ema_i64_leaves_equal_counters_unchanged():
    """update_ema_variables runs over num_batches_tracked too; teacher and student count the same batches, so the
    int64 form must map (c, c) to c for every alpha = min(1 - 1/(k+1), 0.999) the trainer uses.  In float32, every
    operation rounding: exhaustively for k < 1000 and c < 3000.  With one product left unrounded by a fused
    multiply-add (both choices): the same, the sum formed in float64, where it is exact before its one rounding to
    float32 (a 36-bit product plus a 24-bit term at most 2^12 below it)."""
    k = np.arange(1000, dtype=np.float64)
    alpha = np.minimum(1 - 1 / (k + 1), 0.999).astype(np.float32)[:, None]
    c = np.arange(3000, dtype=np.float32)[None, :]
    oma = np.float32(1) - alpha
    plain = (c * alpha + c * oma).astype(np.float32)
    assert np.array_equal(np.trunc(plain), np.broadcast_to(c, plain.shape))
    a64, o64, c64 = alpha.astype(np.float64), oma.astype(np.float64), c.astype(np.float64)
    fma1 = (c64 * a64 + (c * oma).astype(np.float64)).astype(np.float32)
    fma2 = ((c * alpha).astype(np.float64) + c64 * o64).astype(np.float32)
    assert np.array_equal(np.trunc(fma1), np.broadcast_to(c, plain.shape))
    assert np.array_equal(np.trunc(fma2), np.broadcast_to(c, plain.shape))
    # the reference's exact-rational form agrees on a sample, and follows "float math, then truncation" elsewhere
    for al in (0.0, 0.5, 0.999, float(alpha[7, 0])):
        vals = [0, 1, 7, 2999, 2 ** 24 + 1]
        assert R.ema_i64(vals, vals, al) == [{int(np.float32(x))} for x in vals], al
    assert R.ema_i64([10], [20], 0.5) == [{15}] and R.ema_i64([7], [0], 0.5) == [{3}]
    assert R.ema_i64([2 ** 24 + 1], [0], 0.0) == [{0}] and R.ema_i64([0], [2 ** 24 + 1], 0.0) == [{2 ** 24}]
