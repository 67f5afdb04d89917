"""The float64 restatement of the domain classifier (tests/svc_reference.py) pinned to sklearn's ``SVC`` and
``cross_val_score``, and everything of bsed_amd.svc / csrc/svc.hip that can be checked without a GPU: the ABI, every
refusal of the three entry points (all before the first HIP call), the workspace query, the Python refusals and the draw
of ``svm_classification``.

MEASURED tolerances (restatement against sklearn 1.7.2 on the five fixtures of ``svc_reference.fixture``, on the CPU).
They are not round-off bounds: sklearn's kernel values are float64 from the Gram form, the restatement's float32 from
direct differences (about 1e-7 apart), and two solvers that both meet a stop rule ``gap < tol`` need not agree closer than
``tol`` allows.  The allowance is twice the measured value:
  held-out decision values, restatement at tol = 1e-6 against ``SVC(tol=1e-10)``: measured 8.03e-7 (the largest of the
  five fixtures, on "uneven")                                                                     -> allowed 1.7e-6;
  the same at tol = 1e-3 (the default): measured 5.49e-4 ("uneven"); sklearn's own ``SVC()`` at tol = 1e-3 is 4.92e-4
  from ``SVC(tol=1e-10)`` there                                                                   -> allowed 1.1e-3.
The folds, gamma (1e-12 relative: float64 round-off of a variance) and the per-fold scores are compared exactly: on these
fixtures no held-out point lies close enough to zero for the difference above to turn a prediction."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import svc_reference as R
from bsed_amd import _lib as L
from bsed_amd import svc as S

DEC_ALLOWED = {1e-6: 1.7e-6, 1e-3: 1.1e-3}


@functools.lru_cache(maxsize=None)
def _restated(name, tol):
    X, t = R.fixture(name)
    return R.cross_validate(X, t, tol=tol)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_folds_gamma_and_scores_are_sklearns(name):
    ms = pytest.importorskip("sklearn.model_selection")
    svm = pytest.importorskip("sklearn.svm")
    X, t = R.fixture(name)
    got = _restated(name, 1e-3)
    for f, (tr, te) in enumerate(ms.StratifiedKFold(5).split(X, t)):
        assert np.array_equal(te, np.nonzero(got["fold"] == f)[0]) and np.array_equal(tr, np.nonzero(got["fold"] != f)[0])
        want = svm.SVC().fit(X[tr], t[tr])._gamma
        assert abs(R.scale_gamma(X[tr]) - want) <= 1e-12 * want
        assert got["gamma"][f] == float(np.float32(R.scale_gamma(X[tr])))
    assert np.array_equal(S.stratified_folds(t), got["fold"])         # the product's folds are the same rule
    want = ms.cross_val_score(svm.SVC(), X, t, cv=5)
    print(f"{name}: scores {got['scores'].tolist()} sklearn {want.tolist()} iterations {got['iterations']}")
    assert np.array_equal(got["scores"], want)
    assert got["status"] == [R.CONVERGED] * 5


@pytest.mark.parametrize("tol", [1e-6, 1e-3])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_decision_values_against_sklearn_at_a_tight_tolerance(name, tol):
    svm = pytest.importorskip("sklearn.svm")
    X, t = R.fixture(name)
    got = _restated(name, tol)
    worst = 0.0
    for f in range(5):
        tr, te = got["fold"] != f, got["fold"] == f
        want = svm.SVC(tol=1e-10).fit(X[tr], t[tr]).decision_function(X[te])
        worst = max(worst, float(np.abs(got["decision"][te] - want).max()))
    print(f"{name}: tol {tol:g}: max |decision - SVC(tol=1e-10)| = {worst:.3e} (allowed {DEC_ALLOWED[tol]:.1e})")
    assert worst <= DEC_ALLOWED[tol]


def test_unshuffled_stratified_folds_on_other_label_orders():
    ms = pytest.importorskip("sklearn.model_selection")
    rng = np.random.default_rng(3)
    for y in (rng.integers(0, 2, 57), np.array([0] * 13 + [1] * 7), np.array([1, 0] * 11 + [1] * 5),
              rng.integers(0, 3, 40)):
        for k in (2, 5):
            want = np.empty(len(y), np.int64)
            for f, (_tr, te) in enumerate(ms.StratifiedKFold(k).split(np.zeros((len(y), 1)), y)):
                want[te] = f
            assert np.array_equal(R.stratified_folds(y, k), want) and np.array_equal(S.stratified_folds(y, k), want)


@pytest.mark.parametrize("C", [0.5, 1.0, 3.0, 100.0])
def test_two_point_problem_has_the_closed_form(C):
    """one point per class: alpha_1 = alpha_2 = min(C, 1 / (1 - K)) and rho = 0; K = 0.5 clips below C = 2"""
    K = np.array([[1.0, 0.5], [0.5, 1.0]], np.float32)
    fit = R.solve(K, np.array([1.0, -1.0]), C=C, tol=1e-9)
    want = min(C, 1.0 / (1.0 - 0.5))
    assert fit["status"] == R.CONVERGED and fit["iterations"] == 1
    assert np.allclose(fit["alpha"], [want, want], rtol=1e-15, atol=0) and abs(fit["rho"]) <= 1e-15
    assert R.kkt_gap(fit["alpha"], [1.0, -1.0], K, C) <= 1e-9
    dec = R.decision(fit["alpha"], [1.0, -1.0], fit["rho"], K)
    assert dec[0] > 0 > dec[1] and abs(dec[0] + dec[1]) <= 1e-15


def test_scale_gamma_of_the_product():
    x = np.random.default_rng(5).standard_normal((40, 9)).astype(np.float32) * 3 + 2
    assert S.scale_gamma(x) == float(np.float32(R.scale_gamma(x))) == S.scale_gamma(torch.from_numpy(x))
    assert S.scale_gamma(np.full((4, 3), 2.5, np.float32)) == 1.0
    with pytest.raises(L.BsedError):
        S.scale_gamma(np.zeros(5))


# ---- the C entry points: every check runs before the first HIP call ----
_GAMMA = (ctypes.c_float * 5)(*[0.05] * 5)


def _gamma(*values):
    return (ctypes.c_float * len(values))(*values)


_D2 = dict(x=0x1000, x_pitch=8, N=100, D=8, d2=0x1000, stream=None)
_D2_DEFECTS = {"null x": dict(x=None), "null d2": dict(d2=None), "N = 0": dict(N=0), "N above the cap": dict(N=16385),
               "D = 0": dict(D=0), "x_pitch < D": dict(x_pitch=7), "x misaligned": dict(x=0x1002),
               "d2 misaligned": dict(d2=0x1001)}
_SOLVE = dict(d2=0x1000, N=100, y=0x1000, train_offsets=0x1000, train_index=0x1000, P=5, total_train=400, max_train=80,
              gamma=_GAMMA, C=1.0, tol=1e-3, max_iter=1000, alpha=0x1000, rho=0x1000, gap=0x1000, info=0x1000,
              workspace=0x1000, workspace_bytes=1 << 20, stream=None)
_SOLVE_DEFECTS = {
    "null d2": dict(d2=None), "null y": dict(y=None), "null train_offsets": dict(train_offsets=None),
    "null train_index": dict(train_index=None), "null gamma": dict(gamma=None), "null alpha": dict(alpha=None),
    "null rho": dict(rho=None), "null gap": dict(gap=None), "null info": dict(info=None),
    "null workspace": dict(workspace=None), "N = 1": dict(N=1), "N above the cap": dict(N=16385), "P = 0": dict(P=0),
    "P above the cap": dict(P=65, gamma=_gamma(*[0.05] * 65)), "total_train = 0": dict(total_train=0),
    "total_train above P * cap": dict(total_train=5 * 16384 + 1), "max_train = 0": dict(max_train=0),
    "max_train above the cap": dict(max_train=16385), "C = 0": dict(C=0.0), "C NaN": dict(C=float("nan")),
    "C inf": dict(C=float("inf")), "tol = 0": dict(tol=0.0), "tol < 0": dict(tol=-1e-3), "tol inf": dict(tol=float("inf")),
    "gamma = 0": dict(gamma=_gamma(0.05, 0.05, 0.0, 0.05, 0.05)),
    "gamma < 0": dict(gamma=_gamma(-0.05, 0.05, 0.05, 0.05, 0.05)),
    "gamma NaN": dict(gamma=_gamma(0.05, 0.05, 0.05, 0.05, float("nan"))),
    "gamma inf": dict(gamma=_gamma(0.05, float("inf"), 0.05, 0.05, 0.05)),
    "max_iter = 0": dict(max_iter=0), "max_iter above the cap": dict(max_iter=10_000_001),
    "d2 misaligned": dict(d2=0x1002), "y misaligned": dict(y=0x1001), "train_index misaligned": dict(train_index=0x1002),
    "info misaligned": dict(info=0x1002), "alpha misaligned": dict(alpha=0x1004), "rho misaligned": dict(rho=0x1004),
    "gap misaligned": dict(gap=0x1004), "workspace misaligned": dict(workspace=0x1004),
    "workspace one byte short": dict(workspace_bytes=400 * 12 - 1),
}
_DEC = dict(d2=0x1000, N=100, y=0x1000, train_offsets=0x1000, train_index=0x1000, test_offsets=0x1000, test_index=0x1000,
            P=5, total_train=400, total_test=100, gamma=_GAMMA, alpha=0x1000, rho=0x1000, info=0x1000, dec=0x1000,
            stream=None)
_DEC_DEFECTS = {
    "null d2": dict(d2=None), "null y": dict(y=None), "null train_offsets": dict(train_offsets=None),
    "null train_index": dict(train_index=None), "null test_offsets": dict(test_offsets=None),
    "null test_index": dict(test_index=None), "null gamma": dict(gamma=None), "null alpha": dict(alpha=None),
    "null rho": dict(rho=None), "null info": dict(info=None), "null dec": dict(dec=None), "N = 1": dict(N=1),
    "N above the cap": dict(N=16385), "P = 0": dict(P=0), "P above the cap": dict(P=65, gamma=_gamma(*[0.05] * 65)),
    "total_train = 0": dict(total_train=0), "total_test = 0": dict(total_test=0),
    "total_test above P * cap": dict(total_test=5 * 16384 + 1), "gamma = 0": dict(gamma=_gamma(0.0, 1.0, 1.0, 1.0, 1.0)),
    "gamma NaN": dict(gamma=_gamma(1.0, 1.0, 1.0, float("nan"), 1.0)), "test_index misaligned": dict(test_index=0x1002),
    "alpha misaligned": dict(alpha=0x1004), "dec misaligned": dict(dec=0x1004), "info misaligned": dict(info=0x1001),
}
_ENTRIES = [(name, ok, defect, change) for name, ok, defects in (("bsed_svc_d2", _D2, _D2_DEFECTS),
                                                                 ("bsed_svc_solve", _SOLVE, _SOLVE_DEFECTS),
                                                                 ("bsed_svc_decision", _DEC, _DEC_DEFECTS))
            for defect, change in defects.items()]


@pytest.mark.parametrize("entry,ok,defect,change", _ENTRIES, ids=[f"{e[0]}-{e[2]}" for e in _ENTRIES])
def test_every_argument_defect_is_refused_before_any_hip_call(entry, ok, defect, change):
    lib = L.lib()
    rc = getattr(lib, entry)(*dict(ok, **change).values())
    msg = lib.bsed_last_error().decode()
    assert rc == -1, (entry, defect, rc, msg)                          # BSED_ERR_ARG
    assert msg.startswith(entry + ":"), (entry, defect, msg)


def test_abi_constants_and_workspace_query():
    lib = L.lib()
    assert lib.bsed_abi_version() >= 20
    assert L.CONSTANTS["BSED_SVC_MAX_POINTS"] == 16384 == S.SVC_MAX_POINTS
    assert L.CONSTANTS["BSED_SVC_MAX_PROBLEMS"] >= 16 and S.SVC_MAX_PROBLEMS == L.CONSTANTS["BSED_SVC_MAX_PROBLEMS"]
    assert L.CONSTANTS["BSED_SVC_MAX_ITER"] == 10_000_000
    assert [L.CONSTANTS["BSED_SVC_" + k] for k in ("CONVERGED", "NOT_CONVERGED", "BAD_INDEX", "BAD_LABEL", "ONE_CLASS",
                                                    "BAD_OFFSETS")] == [0, 1, 2, 3, 4, 5]
    ws = lib.bsed_svc_solve_workspace
    assert L.FUNCTIONS["bsed_svc_solve_workspace"][0] is ctypes.c_size_t
    # a float64 and an int32 per training point, a multiple of 8 bytes
    assert ws(5, 400) == 400 * 12 and ws(1, 7) == 7 * 8 + 8 * 4 and ws(1, 1) == 16
    assert ws(64, 64 * 16384) == 64 * 16384 * 12
    for bad in ((0, 10), (65, 10), (5, 0), (5, -3), (5, 5 * 16384 + 1)):
        assert ws(*bad) == 0, bad
    for name in ("bsed_svc_d2", "bsed_svc_solve", "bsed_svc_decision"):
        assert name in L.header_symbols()


def test_python_refusals_without_a_gpu():
    x = torch.zeros((8, 3))
    y = torch.ones(8, dtype=torch.int32)
    with pytest.raises(L.BsedError):
        S.svc_d2_gpu(x)                                                # a CPU tensor
    with pytest.raises(L.BsedError):
        S.svc_d2_gpu(x.numpy())
    with pytest.raises(L.BsedError):
        S.svc_solve_gpu(torch.zeros((8, 8)), y, [0, 8], np.arange(8), 0.5)
    with pytest.raises(L.BsedError):
        S.svc_decision_gpu(torch.zeros((8, 8)), y, [0, 8], np.arange(8), [0, 8], np.arange(8), 0.5, None)
    with pytest.raises(L.BsedError):
        S.stratified_folds(np.array([0, 0, 0, 1, 1]), 5)               # a class of 2 points for 5 folds
    with pytest.raises(L.BsedError):
        S.stratified_folds(np.zeros((3, 2)))
    with pytest.raises(L.BsedError):
        S.sample_indices(0, 5)
    with pytest.raises(L.BsedError):
        S.svm_classification(np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((5, 3)), np.zeros((4, 3)))
    assert S.svm_classfication is S.svm_classification                # the reference's spelling
    assert S.default_max_iter(10) == 10_000 and S.default_max_iter(1600) == 160_000
    assert S.default_max_iter(10 ** 7) == 10_000_000
    if not torch.cuda.is_available():
        with pytest.raises(L.BsedError):
            S.domain_svc(np.zeros((10, 3), np.float32), np.ones((10, 3), np.float32))


def test_the_draw_of_svm_classification(monkeypatch):
    """the same rows for both models' features, with replacement, reproducible by seed"""
    si, ri = S.sample_indices(50, 30, 200, seed=4)
    assert si.shape == ri.shape == (200,) and si.min() >= 0 and si.max() < 50 and ri.min() >= 0 and ri.max() < 30
    assert len(np.unique(si)) < 200                                    # with replacement: duplicates
    again = S.sample_indices(50, 30, 200, seed=4)
    assert np.array_equal(si, again[0]) and np.array_equal(ri, again[1])
    assert not np.array_equal(si, S.sample_indices(50, 30, 200, seed=5)[0])
    rng = np.random.default_rng(4)
    assert np.array_equal(si, rng.integers(0, 50, 200)) and np.array_equal(ri, rng.integers(0, 30, 200))
    # svm_classification hands the SAME rows of both feature sets to domain_svc
    rows = np.arange(50, dtype=np.float32)[:, None]
    sets = (rows + 0.0, rows[:30] + 100.0, rows + 1000.0, rows[:30] + 1100.0)
    seen = []
    monkeypatch.setattr(S, "domain_svc", lambda s, r, **kw: seen.append((s.numpy().ravel(), r.numpy().ravel(), kw)))
    S.svm_classification(*sets, sample_num=200, seed=4, C=2.0)
    (a_s, a_r, kw), (n_s, n_r, _) = seen
    assert np.array_equal(a_s, si) and np.array_equal(a_r, ri + 100) and kw == dict(C=2.0)
    assert np.array_equal(n_s, si + 1000) and np.array_equal(n_r, ri + 1100)
