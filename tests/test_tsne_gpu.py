"""Exact t-SNE on the GPU (csrc/tsne.hip: bsed_tsne_affinities / bsed_tsne_gradient / bsed_tsne_update, and
bsed_amd.tsne) against the float64 restatement of tests/tsne_reference.py, which reads the SAME float32 inputs and is
pinned to sklearn in tests/test_tsne_reference_cpu.py.  Every output and workspace sits in a canary-guarded buffer.

The bounds are the DERIVED ones of tsne_reference.py's header (A - E), all teacher-forced: the affinities are checked at
the kernel's own beta, the gradient on the restatement's affinities, an iteration from the restatement's state.

MEASURED, with the restatement on the CPU, for the end-to-end case (two Gaussian blobs of 96 points, D = 16, centres
6 sigma apart, seed 12; perplexity 30, 500 iterations): the final float64 KL divergence of the restatement's own runs
from five random inits (1e-4 normal draws, seeds 100 .. 104) is 0.7216, 0.7056, 0.7035, 0.6963, 0.6983: mean 0.70507,
spread (largest - smallest) 0.02522; the 1-NN domain accuracy of all five maps is 1.0.  The GPU's map, which the float32
pair arithmetic sends to another optimum of the same landscape, must reach mean + 2 spread = 0.7555 or less."""
import ctypes

import numpy as np
import pytest
import torch

import tsne_reference as R
from test_domain_gap_gpu import _guarded, _intact, _place

pytestmark = pytest.mark.gpu

U = R.U
KL_MEAN, KL_SPREAD = 0.70507, 0.02522


def _check_canaries(bufs):
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view.numel()), f"{k}: written outside its {view.numel()} elements"


def launch_affinities(x, perplexity, misaligned=False):
    """bsed_tsne_affinities itself -> dict of numpy results (P (N, N) float32, beta (N) float32, sum_p float)"""
    from bsed_amd import _lib as L
    lib = L.lib()
    N, D = x.shape
    xg = _place(x, misaligned)
    nbytes = lib.bsed_tsne_affinities_workspace(N)
    assert nbytes > 0 and nbytes % 8 == 0
    bufs = {"P": _guarded(N * N, torch.float32), "beta": _guarded(N, torch.float32), "sum_p": _guarded(1, torch.float64),
            "ws": _guarded(nbytes // 8, torch.float64)}
    p = {k: ctypes.c_void_p(v[1].data_ptr()) for k, v in bufs.items()}
    rc = lib.bsed_tsne_affinities(ctypes.c_void_p(xg.data_ptr()), xg.stride(0), N, D, perplexity, p["P"], p["beta"],
                                  p["sum_p"], p["ws"], nbytes, L.stream())
    assert rc == 0, lib.bsed_last_error().decode()
    torch.cuda.synchronize()
    _check_canaries(bufs)
    return dict(P=bufs["P"][1].cpu().numpy().reshape(N, N).copy(), beta=bufs["beta"][1].cpu().numpy().copy(),
                sum_p=float(bufs["sum_p"][1].item()))


def launch_gradient(y, P, inv_sum_p, exaggeration=1.0, want_error=0, splits=0):
    """bsed_tsne_gradient itself -> (grad (N, 2) float32, stats (3) float64)"""
    from bsed_amd import _lib as L
    lib = L.lib()
    N = y.shape[0]
    yg, Pg = torch.from_numpy(np.ascontiguousarray(y, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(P, np.float32)).cuda()
    nbytes = lib.bsed_tsne_gradient_workspace(N, splits)
    assert nbytes > 0 and nbytes % 8 == 0
    bufs = {"grad": _guarded(2 * N, torch.float32), "stats": _guarded(3, torch.float64), "ws": _guarded(nbytes // 8, torch.float64)}
    p = {k: ctypes.c_void_p(v[1].data_ptr()) for k, v in bufs.items()}
    rc = lib.bsed_tsne_gradient(L.ptr(yg), L.ptr(Pg), N, inv_sum_p, exaggeration, want_error, splits, p["grad"], p["stats"],
                                p["ws"], nbytes, L.stream())
    assert rc == 0, lib.bsed_last_error().decode()
    torch.cuda.synchronize()
    _check_canaries(bufs)
    assert torch.equal(yg.cpu(), torch.from_numpy(np.ascontiguousarray(y, np.float32)))
    return bufs["grad"][1].cpu().numpy().reshape(N, 2).copy(), bufs["stats"][1].cpu().numpy().copy()


def launch_update(y, grad, update, gains, momentum, learning_rate, min_gain=0.01):
    """bsed_tsne_update itself on flat float32 arrays -> (y, update, gains) after the step"""
    from bsed_amd import _lib as L
    lib = L.lib()
    n = y.size
    bufs = {k: _guarded(n, torch.float32) for k in ("y", "grad", "update", "gains")}
    for k, a in (("y", y), ("grad", grad), ("update", update), ("gains", gains)):
        bufs[k][1].copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)))
    p = {k: ctypes.c_void_p(v[1].data_ptr()) for k, v in bufs.items()}
    rc = lib.bsed_tsne_update(p["y"], p["grad"], p["update"], p["gains"], n, momentum, learning_rate, min_gain, L.stream())
    assert rc == 0, lib.bsed_last_error().decode()
    torch.cuda.synchronize()
    _check_canaries(bufs)
    assert np.array_equal(bufs["grad"][1].cpu().numpy(), np.ascontiguousarray(grad, np.float32).reshape(-1))
    return tuple(bufs[k][1].cpu().numpy().reshape(np.shape(y)).copy() for k in ("y", "update", "gains"))


# ---- affinities ----
def make_points(kind, N, D, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D)).astype(np.float32)
    if kind == "lattice":                               # every d2 is an integer below 2^24: exact in float32
        x = rng.integers(-3, 4, size=(N, D)).astype(np.float32)
    elif kind == "duplicates":                          # pairs of coincident points, across a tile boundary too
        x[N - 1] = x[0]
        x[N // 2] = x[3]
    elif kind == "outlier":                             # one point far from all others: its beta runs down
        x[7] = 60.0
    elif kind == "cluster":                             # a tight cluster far from the origin: every beta runs up
        x = (5.0 + 1e-3 * x).astype(np.float32)
    return x


# (N, D, perplexity, kind, misaligned): N over one tile + 1, two tiles + 2, four tiles + 1; D = 1, below a load, a chunk
# + 1, eight chunks + 1; perplexity 5 and 30; the misaligned base with a pitch of D + 3 in a NaN-filled buffer
AFFINITY_CASES = [(65, 1, 5.0, "gaussian", False),
                  (65, 3, 30.0, "lattice", True),
                  (65, 33, 30.0, "cluster", True),
                  (130, 33, 5.0, "duplicates", False),
                  (130, 3, 30.0, "outlier", True),
                  (130, 257, 30.0, "lattice", False),
                  (257, 257, 30.0, "gaussian", True),
                  (257, 33, 5.0, "cluster", False),
                  (257, 3, 30.0, "duplicates", False)]


@pytest.mark.parametrize("N,D,perplexity,kind,misaligned", AFFINITY_CASES,
                         ids=[f"N{c[0]}-D{c[1]}-perp{int(c[2])}-{c[3]}" for c in AFFINITY_CASES])
def test_affinities_at_the_kernels_own_beta(N, D, perplexity, kind, misaligned):
    from bsed_amd import tsne as T
    x = make_points(kind, N, D, 1000 + N + D)
    got = launch_affinities(x, perplexity, misaligned)
    ref = R.affinities(x, perplexity)
    assert (ref["steps"] < R.STEPS).all()               # the inputs are built so that every search of the restatement ends
    d2, target = ref["d2"], np.log(float(np.float32(perplexity)))
    beta = got["beta"].astype(np.float64)
    assert np.isfinite(beta).all() and (beta > 0).all()
    if kind == "outlier":
        assert beta[7] < 0.25 * np.median(beta)
    if kind == "cluster":
        assert beta.min() > 1e3
    # the float64 entropy at the kernel's beta meets the stop rule up to the derived round-off (bound B)
    cond, H = R.conditional(d2, beta)
    eb = R.entropy_bound(d2, beta, D)
    excess = np.abs(H - target) - (R.TOL + eb)
    print(f"entropy: max |H - log perp| {np.abs(H - target).max():.3e}, round-off allowance up to {eb.max():.3e}")
    assert (excess <= 0).all(), (int(excess.argmax()), float(excess.max()))
    # against the restatement's beta: both meet the stop rule, so the entropies are within twice its allowance
    assert (np.abs(H - ref["H"]) <= 2 * R.TOL + 2 * eb).all()
    # the affinities are the float64 ones at that beta (bounds A and C), symmetric bit for bit, zero on the diagonal
    want = cond + cond.T
    bound = R.joint_bound(cond, R.cond_bound(d2, beta, D))
    err = np.abs(got["P"].astype(np.float64) - want)
    off = ~np.eye(N, dtype=bool)
    print(f"P: worst error / bound {float((err[off] / bound[off]).max()):.3f}")
    assert (err <= bound).all(), float((err[off] / bound[off]).max())
    assert np.array_equal(got["P"], got["P"].T) and (np.diag(got["P"]) == 0).all()
    total = float(got["P"].astype(np.float64).sum())
    assert abs(got["sum_p"] - total) <= 1e-12 * total and abs(total - 2.0 * N) <= 1e-3 * N
    # the same bits from a second launch, from the other load path and from the Python entry on a pitched view
    for again in (launch_affinities(x, perplexity, misaligned), launch_affinities(x, perplexity, not misaligned)):
        assert np.array_equal(again["P"], got["P"]) and np.array_equal(again["beta"], got["beta"])
        assert again["sum_p"] == got["sum_p"]
    aff = T.tsne_affinities_gpu(_place(x, misaligned), perplexity)
    assert aff.P.dtype == torch.float32 and aff.sum_p.dtype == torch.float64 and tuple(aff.beta.shape) == (N,)
    assert np.array_equal(aff.P.cpu().numpy(), got["P"]) and np.array_equal(aff.beta.cpu().numpy(), got["beta"])
    assert float(aff.sum_p) == got["sum_p"]


# ---- the shared references: computed once, never changed ----
def blobs():
    rng = np.random.default_rng(12)
    a = rng.standard_normal((96, 16)).astype(np.float32)
    b = rng.standard_normal((96, 16)).astype(np.float32)
    b[:, 0] += np.float32(6.0)
    return np.concatenate([a, b]), np.repeat([0, 1], 96)


@pytest.fixture(scope="module")
def blob_run():
    """the restatement's 500 iterations on the blobs from the fixed init, with every state kept"""
    x, labels = blobs()
    y0 = (1e-4 * np.random.default_rng(100).standard_normal((192, 2))).astype(np.float32)
    a = R.affinities(x, 30.0)
    P32 = a["P"].astype(np.float32)
    sum32 = float(P32.astype(np.float64).sum())
    trace = []
    lr = R.auto_learning_rate(192)
    run = R.run(P32.astype(np.float64), sum32, y0, lr, max_iter=500, trace=trace)
    for arr in (x, y0, P32, run["y"]):
        arr.setflags(write=False)
    return dict(x=x, labels=labels, y0=y0, aff=a, P32=P32, sum32=sum32, trace=trace, run=run, lr=lr)


@pytest.fixture(scope="module")
def gauss_aff():
    """the restatement's affinities of 257 Gaussian points in D = 3 (five column tiles, the last of one point)"""
    x = np.random.default_rng(31).standard_normal((257, 3)).astype(np.float32)
    P32 = R.affinities(x, 30.0)["P"].astype(np.float32)
    P32.setflags(write=False)
    return P32, float(P32.astype(np.float64).sum())


def check_gradient(y, P32, sum32, exaggeration, want_error, splits):
    grad, stats = launch_gradient(y, P32, 1.0 / sum32, exaggeration, want_error, splits)
    g = R.gradient(y, P32.astype(np.float64), 1.0 / sum32, exaggeration)
    b = R.grad_bound(g)
    err = np.abs(grad.astype(np.float64) - g["grad"])
    print(f"grad: worst error / bound {float((err / b).max()):.3f}; Z error {abs(stats[0] - g['Z']) / g['Z']:.2e}")
    assert (err <= b).all(), float((err / b).max())
    assert abs(stats[0] - g["Z"]) <= 9 * U * g["Z"]
    own = float((grad.astype(np.float64) ** 2).sum())
    assert abs(stats[1] - own) <= 1e-12 * own
    assert abs(stats[1] - float((g["grad"] ** 2).sum())) <= float((2 * np.abs(g["grad"]) * b + b * b).sum())
    if want_error:
        assert abs(stats[2] - g["kl"]) <= 9 * U * g["p_sum"] + 1e-11 * g["kl_abs"], (stats[2], g["kl"])
    else:
        assert np.isnan(stats[2])                       # as sklearn returns it when the error is not asked for
    grad2, stats2 = launch_gradient(y, P32, 1.0 / sum32, exaggeration, want_error, splits)
    assert np.array_equal(grad, grad2) and np.array_equal(stats, stats2, equal_nan=True)
    return grad, stats, g


@pytest.mark.parametrize("splits", [0, 1, 3])
@pytest.mark.parametrize("exaggeration,want_error", [(1.0, 1), (12.0, 0), (12.0, 1), (1.0, 0)])
def test_gradient_at_the_init_scale_with_coincident_points(gauss_aff, splits, exaggeration, want_error):
    """N = 257: five column tiles, which 3 splits share as 1 + 2 + 2; the last tile holds one point; N is odd, so the rows
    of P are not 16-byte aligned (the 4-byte load path)"""
    P32, sum32 = gauss_aff
    y = (1e-4 * np.random.default_rng(32).standard_normal((257, 2))).astype(np.float32)
    y[9] = y[5]
    y[200] = y[5]
    y[256] = y[64]
    grad, stats, g = check_gradient(y, P32, sum32, exaggeration, want_error, splits)
    one, _ = launch_gradient(y, P32, 1.0 / sum32, exaggeration, want_error, 1)
    # another split: float64 sums in another order, at most one float32 rounding apart
    assert (np.abs(grad.astype(np.float64) - one) <= 1e-12 * g["mag"] + 2 * U * np.abs(one) + R.TINY).all()


@pytest.mark.parametrize("splits", [0, 1, 3])
@pytest.mark.parametrize("exaggeration,want_error", [(1.0, 1), (12.0, 1), (1.0, 0)])
def test_gradient_at_a_converged_scale(blob_run, splits, exaggeration, want_error):
    """N = 192: rows of P 16-byte aligned (the 16-byte load path); y is the restatement's final map"""
    check_gradient(blob_run["run"]["y"], blob_run["P32"], blob_run["sum32"], exaggeration, want_error, splits)


def test_gradient_python_entry_gives_the_kernels_bits(blob_run):
    from bsed_amd import tsne as T
    y, P32, sum32 = blob_run["run"]["y"], blob_run["P32"], blob_run["sum32"]
    aff = T.TsneAffinities(torch.from_numpy(P32).cuda(), torch.tensor([sum32], dtype=torch.float64).cuda(),
                           torch.ones(192).cuda())
    want, stats = launch_gradient(y, P32, 1.0 / sum32, 12.0, 1, 3)
    grad, kl, norm, z = T.tsne_gradient_gpu(torch.from_numpy(y).cuda(), aff, 12.0, True, 3)
    assert np.array_equal(grad.cpu().numpy(), want) and (z, kl) == (stats[0], stats[2]) and norm == np.sqrt(stats[1])
    assert np.isnan(T.tsne_gradient_gpu(torch.from_numpy(y).cuda(), aff)[1])


# ---- update ----
def test_update_is_numpys_float32_step_bit_for_bit():
    """n = 1037 (four blocks and 13 elements): both signs of update * grad and a product of exactly 0, gains that the
    shrink takes below min_gain (clipped) and gains at the clip that grow, magnitudes over twelve decades"""
    rng = np.random.default_rng(41)
    n = 1037
    y = rng.standard_normal(n).astype(np.float32)
    grad = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 4, n)).astype(np.float32)
    update = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 4, n)).astype(np.float32)
    update[::7] = 0.0
    grad[3::11] = 0.0
    gains = rng.uniform(0.01, 3.0, n).astype(np.float32)
    gains[::5] = np.float32(0.01)
    gains[1::5] = np.float32(0.0124)                    # * 0.8 falls below the clip
    for momentum, lr in ((0.5, 50.0), (0.8, 416.6666666666667)):
        want = R.update_step(y, grad, update, gains, momentum, lr)
        prod = update * grad
        assert (prod < 0).sum() > 100 and (prod > 0).sum() > 100 and (prod == 0).sum() > 100
        assert (want[2] == np.float32(0.01)).sum() > 50
        got = launch_update(y, grad, update, gains, momentum, lr)
        for name, w, g in zip(("y", "update", "gains"), want, got):
            assert np.array_equal(w, g), (name, int((w != g).sum()))
    # 2 N elements of an (N, 2) map, N = 1
    got = launch_update(y[:2].reshape(1, 2), grad[:2], update[:2], gains[:2], 0.8, 50.0)
    assert np.array_equal(got[0].reshape(-1), R.update_step(y[:2], grad[:2], update[:2], gains[:2], 0.8, 50.0)[0])


# ---- iterations ----
def test_ten_teacher_forced_iterations_across_the_exaggeration_switch(blob_run):
    """iterations 245 .. 254: each starts from the restatement's state (map, velocity, gains) and is compared with the
    restatement's next map.  The step turns a gradient error b into lr * gains * b; where the gradient is within b of
    zero the sign of update * grad -- and with it the gain -- may differ: lr (|g| + b) |gain+ - gain-| more.  Rounding
    of the step itself: 4 u of its terms"""
    trace, P32, sum32, lr = blob_run["trace"], blob_run["P32"], blob_run["sum32"], blob_run["lr"]
    seen = set()
    for i in range(245, 255):
        k, y, grad_ref, update, gains, exaggeration, momentum = trace[i]
        assert k == i
        seen.add((exaggeration, momentum))
        if i == 250:
            assert (update == 0).all() and (gains == 1).all()          # the second phase starts afresh
        grad, _ = launch_gradient(y, P32, 1.0 / sum32, exaggeration, 0, 0)
        g = R.gradient(y, P32.astype(np.float64), 1.0 / sum32, exaggeration)
        b = R.grad_bound(g) + U * np.abs(g["grad"])                   # the restatement's gradient is rounded to float32
        assert (np.abs(grad.astype(np.float64) - grad_ref) <= b).all()
        y_gpu, update_gpu, gains_gpu = launch_update(y, grad, update, gains, momentum, lr)
        own = R.update_step(y, grad, update, gains, momentum, lr)       # the step itself: bit for bit on the GPU's gradient
        assert np.array_equal(y_gpu, own[0]) and np.array_equal(update_gpu, own[1]) and np.array_equal(gains_gpu, own[2])
        y_next = trace[i + 1][1].astype(np.float64)
        g64, gn = np.abs(grad_ref.astype(np.float64)), gains.astype(np.float64)
        up, down = np.maximum(gn + 0.2, 0.01), np.maximum(gn * 0.8, 0.01)
        tol = lr * np.maximum(up, down) * b + np.where(g64 <= b, lr * (g64 + b) * np.abs(up - down), 0.0)
        tol += 4 * U * (np.abs(momentum * update) + lr * g64 * np.maximum(up, down) + np.abs(y_next))
        assert (np.abs(y_gpu.astype(np.float64) - y_next) <= tol).all()
    assert seen == {(12.0, 0.5), (1.0, 0.8)}


def test_end_to_end_on_two_blobs(blob_run, tmp_path):
    from bsed_amd import domain_gap as DG
    from bsed_amd import tsne as T
    x, labels, y0 = blob_run["x"], blob_run["labels"], blob_run["y0"]
    # the restatement alone meets what is asked of the GPU's map
    assert blob_run["run"]["n_iter"] == 499 and R.nn_accuracy(blob_run["run"]["y"], labels) >= 0.99
    assert blob_run["run"]["kl"] <= KL_MEAN + 2 * KL_SPREAD
    xg = torch.from_numpy(x).cuda()
    kw = dict(perplexity=30.0, max_iter=500, init=y0)
    res = T.tsne(xg, **kw)
    again = T.tsne(xg, splits=0, **kw)
    emb = res.embedding.cpu().numpy()
    assert res.embedding.is_cuda and emb.dtype == np.float32 and emb.shape == (192, 2) and np.isfinite(emb).all()
    assert torch.equal(res.embedding, again.embedding) and res.kl_divergence == again.kl_divergence
    assert res.n_iter == again.n_iter == 499
    assert np.array_equal(y0, blob_run["y0"])                          # the init is copied, not stepped in place
    # the returned KL is the float64 one of the returned map on the GPU's own affinities (bound D's KL line)
    aff = T.tsne_affinities_gpu(xg, 30.0)
    g = R.gradient(emb, aff.P.cpu().numpy().astype(np.float64), 1.0 / float(aff.sum_p), 1.0)
    assert abs(res.kl_divergence - g["kl"]) <= 9 * U * g["p_sum"] + 1e-11 * g["kl_abs"], (res.kl_divergence, g["kl"])
    # quality, evaluated in float64 from the inputs: the domains are apart and the divergence is the restatement's level
    assert R.nn_accuracy(emb, labels) >= 0.99
    kl64 = R.gradient(emb, blob_run["aff"]["P"], 1.0 / blob_run["aff"]["sum_p"], 1.0)["kl"]
    print(f"float64 KL of the GPU's map {kl64:.5f} (the restatement's own runs: {KL_MEAN} +- {KL_SPREAD}); returned "
          f"{res.kl_divergence:.5f}")
    assert kl64 <= KL_MEAN + 2 * KL_SPREAD
    # the other inits, and what is not two components
    for init in ("pca", "random"):
        r = T.tsne(xg, perplexity=30.0, max_iter=250, init=init, seed=3)
        assert torch.equal(r.embedding, T.tsne(xg, perplexity=30.0, max_iter=250, init=init, seed=3).embedding)
        assert r.n_iter == 249 and np.isfinite(r.kl_divergence)
    for bad in (np.zeros((192, 3), np.float32), np.zeros((191, 2), np.float32), "spectral"):
        with pytest.raises(T.BsedError):
            T.tsne(xg, init=bad)
    # domain_map: the same map, the silhouette domain_gap takes of it, the file the reference writes
    dm = T.domain_map(x[:96], torch.from_numpy(x[96:]).cuda(), **kw)
    assert torch.equal(dm.embedding, res.embedding) and dm.labels.tolist() == labels.tolist()
    assert (dm.kl_divergence, dm.n_iter) == (res.kl_divergence, 499)
    assert dm.silhouette == DG.domain_gap(dm.embedding[:96], dm.embedding[96:]).silhouette and dm.silhouette > 0.3
    path = T.save_domain_map(dm, str(tmp_path))
    assert path.endswith("tsne(frame).npy") and np.array_equal(np.load(path), emb)


def test_domain_map_plot(blob_run, tmp_path):
    pytest.importorskip("matplotlib")
    import os
    from bsed_amd import tsne as T
    x = blob_run["x"]
    dm = T.domain_map(x[:96], x[96:], perplexity=30.0, max_iter=250, init=blob_run["y0"])
    T.save_domain_map(dm, str(tmp_path), plot=True)
    assert os.path.getsize(os.path.join(str(tmp_path), "syn vs real(frame).png")) > 1000


def test_domain_map_of_a_model_is_the_map_of_its_embeddings():
    from oracle import seeded
    from test_event_metrics_gpu import _seeded_models
    from bsed_amd import domain_gap as DG
    from bsed_amd import tsne as T
    crnn, pred = _seeded_models(51)

    def loader(seed, gain):
        x = seeded.db_like_input(seed, 4, 256) * gain
        return [(((torch.from_numpy(x[i:i + 2]), torch.from_numpy(x[i:i + 2])), None), [f"clip{j}" for j in (i, i + 1)])
                for i in (0, 2)]
    synth, real = loader(52, 1.0), loader(53, 0.5)
    kw = dict(perplexity=8.0, max_iter=250, init="random")
    got = T.domain_map_of(crnn, synth, real, pred, max_points=40, seed=5, **kw)
    s, r = (DG.embed(crnn, ld, pred, level="frame", max_points=40, seed=5) for ld in (synth, real))
    want = T.domain_map(s, r, seed=5, **kw)
    assert tuple(got.embedding.shape) == (s.shape[0] + r.shape[0], 2) and torch.equal(got.embedding, want.embedding)
    assert got.silhouette == want.silhouette and got.labels.tolist() == [0] * s.shape[0] + [1] * r.shape[0]


def test_refusals_on_the_gpu(monkeypatch):
    from bsed_amd import tsne as T
    x = torch.zeros((8, 3), device="cuda")
    for bad, kw in ((x.double(), {}), (x[0], {}), (x[:1], {}), (x, dict(perplexity=0.0)), (x, dict(perplexity=8.0))):
        with pytest.raises(T.BsedError):
            T.tsne_affinities_gpu(bad, **kw)
    aff = T.tsne_affinities_gpu(torch.randn((8, 3), device="cuda"), 3.0)
    for bad_y, kw in ((torch.zeros((7, 2), device="cuda"), {}), (torch.zeros((8, 3), device="cuda"), {}),
                      (torch.zeros((8, 2)), {}), (torch.zeros((8, 2), device="cuda"), dict(splits=-1))):
        with pytest.raises(T.BsedError):
            T.tsne_gradient_gpu(bad_y, aff, **kw)
    # affinities that do not fit the device: the bytes are named, nothing falls back to the host
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1 << 20, 1 << 30))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda device=None: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda device=None: 0)
    with pytest.raises(T.BsedError, match=str(4 * 1000 * 1000)):
        T.tsne_affinities_gpu(torch.zeros((1000, 3), device="cuda"))
