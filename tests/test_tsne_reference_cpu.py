"""The float64 restatement of exact t-SNE (tests/tsne_reference.py) pinned to sklearn's own functions, and everything of
bsed_amd.tsne / csrc/tsne.hip that can be checked without a GPU: the ABI, every refusal of the entry points and the
workspace queries (all before the first HIP call), the Python refusals and the schedule with a stub objective.

MEASURED tolerances (restatement against sklearn 1.7.2 on the fixture inputs below, on the CPU; two betas that both meet
the 1e-5 stop rule need not be equal and sklearn's inner loop divides before it sums, so these are not round-off bounds;
the allowance is twice the measured value):
  normalised P against ``_joint_probabilities``, both given the SAME float32 distances: measured 2.22e-16 absolute at
  perplexity 5 (sklearn clamps P from below at 2.2e-16, include/bsed.h leaves that out: the entries that differ are the
  clamped ones) and 1.1e-18 at perplexity 30 (P itself reaches 2e-3)                              -> allowed 4.5e-16;
  ``TSNE(method="exact")`` end to end at N = 192, 500 iterations, a fixed init, both given the same float32 distances
  (``metric="precomputed"``): ``n_iter_`` equal (499), ``kl_divergence_`` measured 7.9e-15 apart, the map measured equal
  bit for bit                                                  -> allowed 1.6e-14 for the divergence, equal bits for the map.
  With sklearn's own distances instead (it forms them from the Gram matrix, the restatement by direct differences: they
  differ near 1e-7 relative) the 500 iterations amplify the difference into another local optimum: measured 1.4e-3 in
  the divergence (0.7547 against 0.7561) and 0.67 of the largest coordinate in the map on one such pair of blobs.  Nothing can be pinned there
  but the iteration count, the separation of the blobs and the level of the divergence (within 5 % of each other).
Everything else is compared at float64 round-off (1e-12 relative) or bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import tsne_reference as R
from bsed_amd import _lib as L
from bsed_amd import tsne as T

P_ALLOWED = 4.5e-16
KL_ALLOWED = 1.6e-14


def _blobs(seed=0, n=96, D=16, sep=6.0):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, D)).astype(np.float32)
    b = rng.standard_normal((n, D)).astype(np.float32)
    b[:, 0] += np.float32(sep)
    return np.concatenate([a, b]), np.concatenate([np.zeros(n, np.int64), np.ones(n, np.int64)])


FIXTURES = {"gaussian-30": (lambda: np.random.default_rng(1).standard_normal((96, 8)).astype(np.float32), 30.0),
            "gaussian-5": (lambda: np.random.default_rng(2).standard_normal((70, 3)).astype(np.float32), 5.0),
            "blobs-30": (lambda: _blobs(3, 48)[0], 30.0)}


@pytest.mark.parametrize("name", list(FIXTURES))
def test_affinities_are_sklearns_joint_probabilities(name):
    sk = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    make, perplexity = FIXTURES[name]
    d32 = R.d2_matrix(make()).astype(np.float32)
    want = squareform(sk._joint_probabilities(d32.astype(np.float64), perplexity, 0))
    beta, steps = R.search(d32.astype(np.float64), perplexity)
    assert (steps < R.STEPS).all()
    cond, H = R.conditional(d32.astype(np.float64), beta)
    assert np.abs(H - np.log(float(np.float32(perplexity)))).max() <= R.TOL
    assert np.abs(cond.sum(axis=1) - 1.0).max() <= 1e-12
    P, sum_p = R.joint(cond)
    got = P / sum_p
    err = float(np.abs(got - np.where(np.eye(len(got), dtype=bool), 0.0, want)).max())
    print(f"{name}: max |P - sklearn| = {err:.3e} (P max {want.max():.3e})")
    assert err <= P_ALLOWED
    assert abs(sum_p - 2.0 * len(got)) <= 1e-9                      # every row of the conditionals sums to 1


@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
@pytest.mark.parametrize("scale", [1e-4, 5.0])
def test_gradient_and_error_are_sklearns_kl_divergence(exaggeration, scale):
    sk = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    x, _ = _blobs(4, 30, 6)
    a = R.affinities(x, 10.0)
    y = (scale * np.random.default_rng(5).standard_normal((60, 2))).astype(np.float32)
    y[7] = y[3]                                                      # coincident points
    p_sk = squareform(a["P"] / a["sum_p"], checks=False) * exaggeration
    kl, grad = sk._kl_divergence(y.ravel(), p_sk, 1, 60, 2)          # a float32 map, as TSNE hands it over
    g = R.gradient(y, a["P"], 1.0 / a["sum_p"], exaggeration, clamp_q=True)
    # sklearn returns the gradient in the map's float32; mag = 4 SUM_j |terms| per element
    assert grad.dtype == np.float32
    assert (np.abs(g["grad"] - grad.reshape(60, 2)) <= R.U * np.abs(g["grad"]) + 1e-11 * g["mag"] + R.TINY).all()
    assert abs(g["kl"] - kl) <= 1e-11 * g["kl_abs"]
    free = R.gradient(y, a["P"], 1.0 / a["sum_p"], exaggeration)     # without the clamp of q: what the kernel computes
    assert (np.abs(free["grad"] - g["grad"]) <= R.clamp_bound(g) + 1e-12 * g["mag"]).all()
    assert free["kl"] == g["kl"] and free["Z"] == g["Z"]


def test_update_step_is_sklearns_gradient_descent_bit_for_bit():
    """a quadratic bowl (the sign of update * grad changes now and then) and a gradient whose sign alternates from call to
    call on most elements (their gains shrink to the min_gain clip; the others' grow)"""
    sk = pytest.importorskip("sklearn.manifold._t_sne")
    rng = np.random.default_rng(6)
    p0 = rng.standard_normal(37).astype(np.float32)
    centre = rng.standard_normal(37).astype(np.float32)
    amplitude = rng.uniform(0.1, 1.0, 37).astype(np.float32)
    calls = [0]

    def bowl(p, compute_error=True):
        return 0.0, ((p - centre) * np.float32(0.9)).astype(np.float32)

    def alternating(p, compute_error=True):
        calls[0] += 1
        sign = np.where(np.arange(37) < 30, np.float32(1 if calls[0] % 2 else -1), np.float32(1))
        return 0.0, (sign * amplitude).astype(np.float32)
    for objective, momentum, lr, iters in ((bowl, 0.5, 3.0, 1), (bowl, 0.8, 3.0, 40), (alternating, 0.8, 0.7, 40)):
        calls[0] = 0
        want, _, _ = sk._gradient_descent(objective, p0.copy(), 0, iters, momentum=momentum, learning_rate=lr,
                                          min_grad_norm=0.0)
        calls[0] = 0
        y, update, gains = p0.copy(), np.zeros_like(p0), np.ones_like(p0)
        for _ in range(iters):
            y, update, gains = R.update_step(y, objective(y)[1], update, gains, momentum, lr)
        assert want.dtype == np.float32 and np.array_equal(want, y)
        if objective is alternating:
            assert (gains[:30] == np.float32(0.01)).sum() >= 20 and (gains[30:] > 1).all()


def test_restatement_end_to_end_against_sklearn_exact():
    manifold = pytest.importorskip("sklearn.manifold")
    x, labels = _blobs(12, 96, 16)
    N = x.shape[0]
    y0 = (1e-4 * np.random.default_rng(8).standard_normal((N, 2))).astype(np.float32)
    lr = R.auto_learning_rate(N)
    kw = dict(method="exact", init=y0.copy(), perplexity=30.0, max_iter=500, learning_rate=lr)
    # the same float32 distances to both: sklearn squares what it is given (exact for the root of a float32 value)
    d32 = R.d2_matrix(x).astype(np.float32).astype(np.float64)
    sk = manifold.TSNE(metric="precomputed", **kw)
    want = sk.fit_transform(np.sqrt(d32))
    beta, _ = R.search(d32, 30.0)
    P, sum_p = R.joint(R.conditional(d32, beta)[0])
    got = R.run(P, sum_p, y0, lr, max_iter=500)
    kl_gap = abs(got["kl_last"] - sk.kl_divergence_)
    print(f"n_iter {got['n_iter']} / {sk.n_iter_}; kl {got['kl_last']:.9f} / {sk.kl_divergence_:.9f} (gap {kl_gap:.3e}); "
          f"map gap {np.abs(got['y'] - want).max():.3e}")
    assert got["n_iter"] == sk.n_iter_ == 499
    assert kl_gap <= KL_ALLOWED and np.array_equal(got["y"], want)
    assert abs(got["kl"] - got["kl_last"]) <= 1e-3                      # the returned map against the one a step before
    # sklearn on its own distances: another optimum of the same quality (the header)
    own = manifold.TSNE(**kw)
    own_map = own.fit_transform(x)
    assert own.n_iter_ == 499 and abs(own.kl_divergence_ - got["kl_last"]) <= 0.05 * got["kl_last"]
    assert R.nn_accuracy(got["y"], labels) >= 0.99 and R.nn_accuracy(own_map, labels) >= 0.99


def test_pca_init_is_the_principal_components_at_1e_4():
    rng = np.random.default_rng(9)
    for N, D in ((40, 5), (12, 30), (9, 1)):
        x = (rng.standard_normal((N, D)) * np.linspace(3.0, 0.5, D)).astype(np.float32)
        want, got = R.pca_init(x), T.pca_init(torch.from_numpy(x)).numpy()
        assert got.dtype == np.float32 and got.shape == (N, 2)
        assert np.abs(got - want).max() <= 1e-6 * 1e-4 + 1e-12
        assert abs(float(got[:, 0].astype(np.float64).std()) - 1e-4) <= 1e-10
        assert (got[np.abs(got).argmax(axis=0), [0, 1]] >= 0).all()
        if D == 1:
            assert (got[:, 1] == 0).all()
    with pytest.raises(L.BsedError):
        T.pca_init(torch.ones((5, 3)))


# ---- the C entry points: every check runs before the first HIP call ----
_AFF = dict(x=0x1000, x_pitch=8, N=100, D=8, perplexity=30.0, P=0x1000, beta=0x1000, sum_p=0x1000, workspace=0x1000,
            workspace_bytes=1 << 20, stream=None)
_AFF_DEFECTS = {
    "null x": dict(x=None), "null P": dict(P=None), "null beta": dict(beta=None), "null sum_p": dict(sum_p=None),
    "null workspace": dict(workspace=None), "N = 1": dict(N=1), "N above the cap": dict(N=65537), "D = 0": dict(D=0),
    "x_pitch < D": dict(x_pitch=7), "perplexity = 0": dict(perplexity=0.0), "perplexity < 0": dict(perplexity=-1.0),
    "perplexity = N": dict(perplexity=100.0), "perplexity NaN": dict(perplexity=float("nan")),
    "workspace one byte short": dict(workspace_bytes=2 * 2 * 8 - 1), "workspace misaligned": dict(workspace=0x1004),
    "x misaligned": dict(x=0x1002),
}
_GRAD = dict(y=0x1000, P=0x1000, N=100, inv_sum_p=0.005, exaggeration=1.0, want_error=0, splits=0, grad=0x1000,
             stats=0x1000, workspace=0x1000, workspace_bytes=1 << 20, stream=None)
_GRAD_DEFECTS = {
    "null y": dict(y=None), "null P": dict(P=None), "null grad": dict(grad=None), "null stats": dict(stats=None),
    "null workspace": dict(workspace=None), "N = 1": dict(N=1), "N above the cap": dict(N=65537),
    "inv_sum_p = 0": dict(inv_sum_p=0.0), "inv_sum_p NaN": dict(inv_sum_p=float("nan")),
    "exaggeration = 0": dict(exaggeration=0.0), "exaggeration inf": dict(exaggeration=float("inf")),
    "want_error = 2": dict(want_error=2), "splits < 0": dict(splits=-1), "splits above 65535": dict(splits=65536),
    "workspace one byte short": dict(splits=2, workspace_bytes=8 * (2 * 100 * 5 + 100 * 5 + 2 * 2) - 1),
    "workspace short for the automatic split": dict(workspace_bytes=64), "workspace misaligned": dict(workspace=0x1004),
    "stats misaligned": dict(stats=0x1004),
}
_UPD = dict(y=0x1000, grad=0x1000, update=0x1000, gains=0x1000, n=200, momentum=0.5, learning_rate=50.0, min_gain=0.01,
            stream=None)
_UPD_DEFECTS = {"null y": dict(y=None), "null grad": dict(grad=None), "null update": dict(update=None),
                "null gains": dict(gains=None), "n = 0": dict(n=0), "n above the cap": dict(n=2 * 65536 + 1),
                "misaligned": dict(gains=0x1002)}
_ENTRIES = [(name, ok, defect, change) for name, ok, defects in (("bsed_tsne_affinities", _AFF, _AFF_DEFECTS),
                                                                 ("bsed_tsne_gradient", _GRAD, _GRAD_DEFECTS),
                                                                 ("bsed_tsne_update", _UPD, _UPD_DEFECTS))
            for defect, change in defects.items()]


@pytest.mark.parametrize("entry,ok,defect,change", _ENTRIES, ids=[f"{e[0]}-{e[2]}" for e in _ENTRIES])
def test_every_argument_defect_is_refused_before_any_hip_call(entry, ok, defect, change):
    lib = L.lib()
    assert lib.bsed_abi_version() >= 19
    rc = getattr(lib, entry)(*dict(ok, **change).values())
    msg = lib.bsed_last_error().decode()
    assert rc == -1, (entry, defect, rc, msg)                          # BSED_ERR_ARG
    assert msg.startswith(entry + ":"), (entry, defect, msg)


def test_workspace_queries():
    lib = L.lib()
    assert L.CONSTANTS["BSED_TSNE_MAX_POINTS"] == 65536 == T.TSNE_MAX_POINTS
    aff, grad, splits = lib.bsed_tsne_affinities_workspace, lib.bsed_tsne_gradient_workspace, lib.bsed_tsne_gradient_splits
    assert L.FUNCTIONS["bsed_tsne_affinities_workspace"][0] is ctypes.c_size_t
    assert L.FUNCTIONS["bsed_tsne_gradient_workspace"][0] is ctypes.c_size_t
    assert aff(100) == 2 * 2 * 8 and aff(64) == 8 and aff(65) == 32 and aff(65536) == 1024 * 1024 * 8
    assert aff(1) == 0 and aff(65537) == 0 and aff(-5) == 0
    assert grad(100, 2) == 8 * (2 * 100 * 5 + 100 * 5 + 2 * 2) and grad(101, 2) > grad(100, 2) and grad(100, 3) > grad(100, 2)
    for bad in ((1, 1), (65537, 1), (100, -1), (100, 65536)):
        assert grad(*bad) == 0, bad
    for N in (2, 64, 257, 2000, 20000, 65536):
        auto = splits(N)
        assert 1 <= auto <= (N + 63) // 64 and grad(N, 0) == grad(N, auto)
    assert splits(0) >= 1


def test_python_refusals_without_a_gpu(tmp_path):
    x = torch.zeros((8, 3))
    with pytest.raises(L.BsedError):
        T.tsne_affinities_gpu(x)                                       # a CPU tensor
    with pytest.raises(L.BsedError):
        T.tsne_affinities_gpu(x.numpy())
    with pytest.raises(L.BsedError):
        T.tsne(x)
    with pytest.raises(L.BsedError):
        T.tsne_gradient_gpu(torch.zeros((8, 2)), "not affinities")
    with pytest.raises(L.BsedError):
        T.tsne_gradient_gpu(torch.zeros((8, 2)), T.TsneAffinities(torch.zeros((8, 8)), torch.ones(1), torch.ones(8)))
    with pytest.raises(L.BsedError):
        T.save_domain_map("not a map", str(tmp_path))
    with pytest.raises(L.BsedError):
        T.run_schedule(None, None, None, max_iter=249)
    assert T.affinity_bytes(20000) == 1_600_000_000
    if not torch.cuda.is_available():
        with pytest.raises(L.BsedError):
            T.domain_map(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32))


def test_save_domain_map_round_trips_without_a_gpu(tmp_path):
    emb = np.random.default_rng(3).standard_normal((7, 2)).astype(np.float32)
    res = T.DomainMap(torch.from_numpy(emb), np.array([0, 0, 0, 1, 1, 1, 1]), 0.5, 1.0, 499)
    path = T.save_domain_map(res, str(tmp_path / "out"))
    assert path.endswith("tsne(frame).npy") and np.array_equal(np.load(path), emb)
    assert T.save_domain_map(res, str(tmp_path / "out"), level="clip").endswith("tsne(clip).npy")


# ---- the schedule with a stub objective ----
class _Stub:
    """records what the schedule asks for; ``errors(i)`` / ``norms(i)`` give what a check of iteration i measures"""

    def __init__(self, errors=lambda i: 1.0 / (i + 1), norms=lambda i: 1.0):
        self.calls, self.steps, self.measured, self.i = [], [], [], -1
        self.errors, self.norms = errors, norms

    def objective(self, exaggeration, want_error):
        self.i += 1
        self.calls.append((self.i, exaggeration, want_error))
        return (self.i, want_error)

    def update(self, handle, momentum, restart):
        assert handle[0] == self.i
        self.steps.append((self.i, momentum, restart))

    def measure(self, handle):
        assert handle == (self.i, True)                                # only evaluations made with want_error are read
        self.measured.append(self.i)
        return self.errors(self.i), self.norms(self.i)


def _run(stub, **kw):
    return T.run_schedule(stub.objective, stub.update, stub.measure, **kw)


def test_schedule_phases_and_checks():
    s = _Stub()
    error, n_iter = _run(s, max_iter=500)
    assert n_iter == 499 and error == 1.0 / 500
    assert [c[0] for c in s.calls] == list(range(500))
    assert all(ex == 12.0 for i, ex, _ in s.calls if i < 250) and all(ex == 1.0 for i, ex, _ in s.calls if i >= 250)
    assert all(m == 0.5 for i, m, _ in s.steps if i < 250) and all(m == 0.8 for i, m, _ in s.steps if i >= 250)
    assert [i for i, _, restart in s.steps if restart] == [0, 250]     # velocity and gains start afresh in each phase
    assert [i for i, _, e in s.calls if e] == list(range(49, 500, 50)) == s.measured
    # a last iteration that is no check still evaluates the error
    s = _Stub()
    error, n_iter = _run(s, max_iter=275, early_exaggeration=4.0)
    assert n_iter == 274 and s.measured == [49, 99, 149, 199, 249, 274] and error == 1.0 / 275
    assert s.calls[0][1] == 4.0


def test_schedule_stops():
    # no progress: the error stops improving after iteration 299; with a patience of 100 the check at 449 ends the run
    # (449 - 299 = 150 > 100; at 399 the distance is exactly 100, which is not more)
    s = _Stub(errors=lambda i: 1.0 / (min(i, 299) + 1))
    error, n_iter = _run(s, max_iter=1000, n_iter_without_progress=100)
    assert n_iter == 449 and s.measured[-1] == 449
    # gradient norm: phase 1 ends at its first check below the threshold, phase 2 starts right after it and ends likewise
    s = _Stub(norms=lambda i: 1e-8 if i in (99, 349) else 1.0)
    error, n_iter = _run(s, max_iter=1000)
    assert n_iter == 349 and [i for i, _, r in s.steps if r] == [0, 100]
    assert all(ex == 12.0 for i, ex, _ in s.calls if i < 100) and all(ex == 1.0 for i, ex, _ in s.calls if i >= 100)
    assert _run(_Stub(norms=lambda i: 1e-7), max_iter=1000)[1] == 99   # at most min_grad_norm: the phases end at 49 and 99
    # phase 1 never tests progress beyond its own 250 iterations: a flat error does not end it early
    s = _Stub(errors=lambda i: 1.0)
    assert _run(s, max_iter=300, n_iter_without_progress=50)[1] == 299
