"""The domain classifier on the GPU (csrc/svc.hip: bsed_svc_d2 / bsed_svc_solve / bsed_svc_decision, and bsed_amd.svc)
against the float64 restatement of tests/svc_reference.py, which tests/test_svc_reference_cpu.py pins to sklearn.  The
restatement is always given the GPU's OWN float32 kernel values (read back through the decision kernel: a problem that
trains on the single point j with alpha = 1 and rho = 0 returns K(t, j)), so what is compared is the solver.

Bounds, u = 2^-24:
1. d2: per element (D + 3) u d2_64, the bound tests/test_domain_gap_gpu.py derives for this chain (bound 1 there).
2. Kernel values: within 2 float32 ulp of exp of the float32 argument -(gamma * d2) formed from the GPU's d2 (the product
   of two float32 values rounds the same way everywhere).  HIP documents expf at 1 ulp; the second covers the rounding of
   the float64 reference value to the float32 grid.
3. Box and equality constraint: 0 <= alpha <= C exactly (the update clips to the bounds themselves);
   |SUM y alpha| <= n C 2^-50: every pair update moves the sum by a few roundings of values <= C (2^-53 C each).
4. Stop rule: the float64 gap recomputed from the returned alpha on the GPU's kernel values is <= tol + 1e-9 and equals the
   returned one within 1e-9: the 1e-9 covers the incremental float64 gradient over at most 1e5 updates (1e5 * n * 2^-53 C).
5. Decision values at tol = 1e-6 against the restatement at tol = 1e-10: 4 times the restatement's own spread between
   tol = 1e-6 and tol = 1e-10 on the same problem, MEASURED on the CPU (numpy's float32 kernel values) and listed in SPREAD
   below, plus 1e-12 for the float64 round-off of the sums (n terms <= C, 2^-53 each) where the spread is 0 because both
   runs make the same updates (two points; C = 0.01, where every alpha ends at C).
6. domain_svc at the defaults (tol = 1e-3): predictions equal the restatement's at tol = 1e-10 except where its decision
   value is within 2e-3 of zero, at most two such points per fixture (the restatement finds at most one).  The decision
   values themselves: 4 times the restatement's own spread between tol = 1e-3 and 1e-10 on the fixtures, measured on the
   CPU at 5.49e-4 ("uneven") -> 2.2e-3.  At another tolerance (1e-4 below) the allowance is 2 tol: the measured spread is
   between 0.06 and 0.9 of tol on every case of SPREAD and at tol = 1e-3 alike."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import svc_reference as R
from test_domain_gap_gpu import _guarded, _intact, _place

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# max |decision(tol = 1e-6) - decision(tol = 1e-10)| of the restatement on solver_case(name), measured on the CPU
SPREAD = {"n2": 0.0, "n63": 5.111e-07, "n64": 5.304e-07, "n65": 4.649e-07, "n255": 5.964e-07, "n256": 5.293e-07,
          "n257": 7.004e-07, "fold160": 3.068e-07, "fold96": 5.533e-08, "fold108": 6.865e-07, "C0.01": 0.0,
          "C100": 1.063e-06, "duplicates": 4.597e-07}


def _S():
    from bsed_amd import svc as S
    return S


def _gpu(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def gpu_kernel_matrix(d2, gamma):
    """the kernel's own K(t, j) of all points, float64 numpy (N, N), through bsed_svc_decision: problem j trains on the
    point j alone with alpha = 1, y = +1, rho = 0 and evaluates every point"""
    S = _S()
    N = d2.shape[0]
    ones = torch.ones(N, device="cuda", dtype=torch.int32)
    every = np.arange(N)
    out = np.empty((N, N))
    for j0 in range(0, N, S.SVC_MAX_PROBLEMS):
        P = min(S.SVC_MAX_PROBLEMS, N - j0)
        fit = S.SvcFit(torch.ones(P, device="cuda", dtype=torch.float64), torch.zeros(P, device="cuda", dtype=torch.float64),
                       torch.zeros(P, device="cuda", dtype=torch.float64), torch.zeros((P, 2), device="cuda", dtype=torch.int32))
        dec = S.svc_decision_gpu(d2, ones, np.arange(P + 1), np.arange(j0, j0 + P), np.arange(P + 1) * N, np.tile(every, P),
                                 float(gamma), fit)
        out[:, j0:j0 + P] = dec.cpu().numpy().reshape(P, N).T
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """solver_case(name) on the GPU: its d2, the GPU's kernel values and the restatement at tol = 1e-10 on them"""
    S = _S()
    c = R.solver_case(name)
    d2 = S.svc_d2_gpu(_gpu(c["x"], torch.float32))
    K = gpu_kernel_matrix(d2, c["gamma"])
    tr, te = c["train"], c["test"]
    ref = R.solve(K[np.ix_(tr, tr)].astype(np.float32), c["y"][tr], c["C"], 1e-10)
    ref_dec = R.decision(ref["alpha"], c["y"][tr], ref["rho"], K[np.ix_(te, tr)].astype(np.float32))
    return dict(c, d2=d2, K=K, ref=ref, ref_dec=ref_dec, y_gpu=_gpu(c["y"], torch.int32))


def _solve_case(c, tol, max_iter=1_000_000):
    S = _S()
    tr, te = c["train"], c["test"]
    fit = S.svc_solve_gpu(c["d2"], c["y_gpu"], [0, len(tr)], tr, float(c["gamma"]), c["C"], tol, max_iter)
    dec = S.svc_decision_gpu(c["d2"], c["y_gpu"], [0, len(tr)], tr, [0, len(te)], te, float(c["gamma"]), fit)
    info = fit.info.cpu().numpy()
    return dict(alpha=fit.alpha.cpu().numpy(), rho=float(fit.rho[0]), gap=float(fit.gap[0]), iterations=int(info[0, 0]),
                status=int(info[0, 1]), dec=dec.cpu().numpy(), fit=fit)


def _check_feasible(alpha, y, C):
    assert (alpha >= 0).all() and (alpha <= C).all()
    assert abs(float((y * alpha).sum())) <= len(alpha) * C * 2.0 ** -50


# ------------------------------------------------------------------------------------------------ d2
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("N,D", [(65, 1), (130, 67), (200, 6)])
def test_d2_is_the_direct_difference_matrix(N, D, misaligned):
    from bsed_amd import _lib as L
    x = np.random.default_rng(N + D).standard_normal((N, D)).astype(np.float32)
    x[N - 1] = x[0]                                                   # a duplicated row: d2 = 0 off the diagonal
    xg = _place(x, misaligned)
    buf, out = _guarded(N * N, torch.float32)
    rc = L.lib().bsed_svc_d2(ctypes.c_void_p(xg.data_ptr()), xg.stride(0), N, D, ctypes.c_void_p(out.data_ptr()), L.stream())
    assert rc == 0, L.lib().bsed_last_error().decode()
    torch.cuda.synchronize()
    assert _intact(buf, N * N)
    got = out.cpu().numpy().reshape(N, N)
    want = R.d2_matrix(x)
    assert np.array_equal(got.view(np.uint32), got.T.view(np.uint32)) and (np.diag(got) == 0).all()
    assert got[0, N - 1] == 0 and not np.isnan(got).any()
    assert (np.abs(got - want) <= (D + 3) * U * want).all()
    # the wrapper hands out the same bits, whatever the pitch
    assert np.array_equal(_S().svc_d2_gpu(xg).cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------ the solver
@pytest.mark.parametrize("name", R.SOLVER_CASES)
def test_solver_meets_the_optimality_conditions(name):
    c = _case(name)
    tr, te, C = c["train"], c["test"], c["C"]
    y = c["y"][tr].astype(np.float64)
    Ktr = c["K"][np.ix_(tr, tr)]
    # (d) the kernel values
    arg = -(np.float32(c["gamma"]) * c["d2"].cpu().numpy())
    assert arg.dtype == np.float32
    want_k = np.exp(arg.astype(np.float64))
    assert (np.abs(c["K"] - want_k) <= 2 * np.spacing(want_k.astype(np.float32)).astype(np.float64)).all()
    assert (np.diag(c["K"]) == 1).all() and np.array_equal(c["K"], c["K"].T)
    for tol in (1e-3, 1e-6):
        got = _solve_case(c, tol)
        assert got["status"] == R.CONVERGED and 1 <= got["iterations"] < 100_000
        _check_feasible(got["alpha"], y, C)                                                        # (a), (b)
        kkt = R.kkt_gap(got["alpha"], y, Ktr.astype(np.float32), C)                              # (c)
        print(f"{name}: tol {tol:g}: {got['iterations']} updates, gap {got['gap']:.3e}, recomputed {kkt:.3e}, "
              f"restatement at 1e-10: {c['ref']['iterations']}")
        assert kkt <= tol + 1e-9 and abs(kkt - got["gap"]) <= 1e-9 and got["gap"] < tol
    err = float(np.abs(got["dec"] - c["ref_dec"]).max())                                           # (e), at tol = 1e-6
    print(f"{name}: max |decision - restatement(1e-10)| = {err:.3e} (allowed {4 * SPREAD[name] + 1e-12:.3e})")
    assert err <= 4 * SPREAD[name] + 1e-12
    if name == "n2":                                                   # the closed form of two points
        k = Ktr[0, 1]
        assert np.allclose(got["alpha"], min(C, 1.0 / (1.0 - k)), rtol=1e-15, atol=0) and abs(got["rho"]) <= 1e-15
    if name == "C0.01":                                                # everything bounded: rho = (ub + lb) / 2
        assert (got["alpha"] == C).all() and abs(got["rho"] - c["ref"]["rho"]) <= 1e-12
    if name == "duplicates":                                           # TAU: pairs of training points with K = 1 exactly
        assert int((Ktr == 1).sum()) - len(tr) >= 8


# ------------------------------------------------------------------------------------------------ batches
def _batch(P):
    """P problems of unequal sizes over the 200 points of a fixture: unsorted lists with gaps -> (c, lists, gammas)"""
    c = _case("fold160")
    rng = np.random.default_rng(40 + P)
    N = c["d2"].shape[0]
    lists = [rng.permutation(N)[:int(n)] for n in rng.integers(20, 150, P)]
    gammas = [float(np.float32(g)) for g in rng.uniform(0.02, 0.2, P)]
    return c, lists, gammas


def _launch(c, lists, gammas, tol=1e-3, max_iter=100_000):
    S = _S()
    off = np.concatenate([[0], np.cumsum([len(t) for t in lists])])
    return S.svc_solve_gpu(c["d2"], c["y_gpu"], off, np.concatenate(lists), gammas, 1.0, tol, max_iter), off


@pytest.mark.parametrize("P", [1, 5, 64])
def test_a_batch_gives_every_problem_the_bits_it_gets_alone(P):
    S = _S()
    assert S.SVC_MAX_PROBLEMS == 64
    c, lists, gammas = _batch(P)
    fit, off = _launch(c, lists, gammas)
    again, _ = _launch(c, lists, gammas)
    for a, b in zip(fit, again):
        assert torch.equal(a, b)                                       # two launches: the same bits
    assert (fit.info[:, 1] == S.CONVERGED).all()
    N = c["d2"].shape[0]
    test_off = np.arange(P + 1) * N
    dec = S.svc_decision_gpu(c["d2"], c["y_gpu"], off, np.concatenate(lists), test_off, np.tile(np.arange(N), P), gammas, fit)
    for p in range(0, P, max(1, P // 5)):
        alone, _ = _launch(c, [lists[p]], [gammas[p]])
        assert torch.equal(alone.alpha, fit.alpha[off[p]:off[p + 1]]) and torch.equal(alone.rho[0], fit.rho[p])
        assert torch.equal(alone.gap[0], fit.gap[p]) and torch.equal(alone.info[0], fit.info[p])
        dec1 = S.svc_decision_gpu(c["d2"], c["y_gpu"], [0, len(lists[p])], lists[p], [0, N], np.arange(N), gammas[p], alone)
        assert torch.equal(dec1, dec[p * N:(p + 1) * N])
        _check_feasible(alone.alpha.cpu().numpy(), c["y"][lists[p]].astype(np.float64), 1.0)


def test_state_in_global_memory_gives_the_same_bits():
    """max_train above BSED_SVC_LDS_POINTS moves alpha, G and the packed words from LDS to global memory; the arithmetic
    and so the bits stay (the problems themselves are small: the placement follows the argument)"""
    from bsed_amd import _lib as L
    S = _S()
    c, lists, gammas = _batch(5)
    fit, off = _launch(c, lists, gammas)
    lib = L.lib()
    P, total, N = 5, int(off[-1]), c["d2"].shape[0]
    ws_bytes = lib.bsed_svc_solve_workspace(P, total)
    ws_buf, ws = _guarded(ws_bytes // 8, torch.float64)
    alpha_buf, alpha = _guarded(total, torch.float64)
    rho, gap = torch.empty(P, device="cuda", dtype=torch.float64), torch.empty(P, device="cuda", dtype=torch.float64)
    info = torch.empty((P, 2), device="cuda", dtype=torch.int32)
    og, ig = _gpu(off, torch.int32), _gpu(np.concatenate(lists), torch.int32)
    max_train = L.CONSTANTS["BSED_SVC_LDS_POINTS"] + 1
    rc = lib.bsed_svc_solve(L.ptr(c["d2"]), N, L.ptr(c["y_gpu"], torch.int32), L.ptr(og, torch.int32), L.ptr(ig, torch.int32), P,
                            total, max_train, (ctypes.c_float * P)(*gammas), 1.0, 1e-3, 100_000,
                            ctypes.c_void_p(alpha.data_ptr()), L.ptr(rho, torch.float64), L.ptr(gap, torch.float64),
                            L.ptr(info, torch.int32), ctypes.c_void_p(ws.data_ptr()), ws_bytes, L.stream())
    assert rc == 0, lib.bsed_last_error().decode()
    torch.cuda.synchronize()
    assert _intact(ws_buf, ws_bytes // 8) and _intact(alpha_buf, total)
    assert torch.equal(alpha, fit.alpha) and torch.equal(rho, fit.rho) and torch.equal(gap, fit.gap)
    assert torch.equal(info, fit.info)


def test_a_bad_problem_among_good_ones():
    """an index of -1, an index of N, a label of 0, one class only, offsets that run backwards: the status, a NaN rho, an
    untouched alpha and gap; the neighbours' results are those of a launch without the bad problems"""
    from bsed_amd import _lib as L
    S = _S()
    c, lists, gammas = _batch(5)
    N = c["d2"].shape[0]
    y = c["y"].copy()
    zero_label = 7
    lists = [t[t != zero_label] for t in lists]                        # a point no good problem trains on
    y[zero_label] = 0
    good = [0, 2, 4]
    bad = {1: np.concatenate([lists[1][:7], [-1], lists[1][7:]]), 3: np.concatenate([lists[3][:3], [N]]),
           5: np.concatenate([lists[1][:9], [zero_label]]), 6: np.nonzero(y == 1)[0][:30]}
    problems = [lists[0], bad[1], lists[2], bad[3], lists[4], bad[5], bad[6], lists[1][:11]]
    want_status = [0, S.L.CONSTANTS["BSED_SVC_BAD_INDEX"], 0, S.L.CONSTANTS["BSED_SVC_BAD_INDEX"], 0,
                   S.L.CONSTANTS["BSED_SVC_BAD_LABEL"], S.L.CONSTANTS["BSED_SVC_ONE_CLASS"],
                   S.L.CONSTANTS["BSED_SVC_BAD_OFFSETS"]]
    P = len(problems)
    g = gammas + [0.05, 0.05, 0.05]
    off = np.concatenate([[0], np.cumsum([len(t) for t in problems])]).astype(np.int32)
    off[P] = off[P - 1] - 4                                           # the last problem's list ends before it begins
    total = int(off[P - 1])
    index = np.concatenate(problems)[:total].astype(np.int32)
    lib = L.lib()
    bufs = {"alpha": _guarded(total, torch.float64), "rho": _guarded(P, torch.float64), "gap": _guarded(P, torch.float64),
            "info": _guarded(2 * P, torch.int32)}
    for k in ("alpha", "gap"):
        bufs[k][1].fill_(-3.5)
    bufs["info"][1].fill_(-9)
    ws_bytes = lib.bsed_svc_solve_workspace(P, total)
    ws = torch.empty(ws_bytes // 8, device="cuda", dtype=torch.float64)
    yg, og, ig = _gpu(y, torch.int32), _gpu(off, torch.int32), _gpu(index, torch.int32)
    rc = lib.bsed_svc_solve(L.ptr(c["d2"]), N, L.ptr(yg, torch.int32), L.ptr(og, torch.int32), L.ptr(ig, torch.int32), P, total,
                            150, (ctypes.c_float * P)(*g), 1.0, 1e-3, 100_000, *(ctypes.c_void_p(bufs[k][1].data_ptr())
                                                                                 for k in ("alpha", "rho", "gap", "info")),
                            L.ptr(ws, torch.float64), ws_bytes, L.stream())
    assert rc == 0, lib.bsed_last_error().decode()
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view.numel()), k
    alpha, rho, gap = (bufs[k][1].cpu().numpy() for k in ("alpha", "rho", "gap"))
    info = bufs["info"][1].cpu().numpy().reshape(P, 2)
    assert info[:, 1].tolist() == want_status
    ref, ref_off = _launch(c, [lists[p] for p in good], [gammas[p] for p in good])
    for k, p in enumerate(good):                                       # the neighbours: as if the bad ones were not there
        assert np.array_equal(alpha[off[p]:off[p + 1]], ref.alpha[ref_off[k]:ref_off[k + 1]].cpu().numpy())
        assert rho[p] == float(ref.rho[k]) and gap[p] == float(ref.gap[k]) and info[p].tolist() == ref.info[k].tolist()
    for p in (1, 3, 5, 6, 7):
        assert np.isnan(rho[p]) and gap[p] == -3.5 and info[p, 0] == 0
        if p < 7:
            assert (alpha[off[p]:off[p + 1]] == -3.5).all()
    # the decision values of a bad problem are NaN, and so is a test index out of range; the others are untouched by it
    S_fit = S.SvcFit(bufs["alpha"][1], bufs["rho"][1], bufs["gap"][1], bufs["info"][1].view(P, 2))
    off[P] = off[P - 1]                                                # the wrapper wants offsets that rise
    tests = [np.array([0, 5, N, 7, -1, 9])] * P
    dec = S.svc_decision_gpu(c["d2"], yg, off, index, np.arange(P + 1) * 6, np.concatenate(tests), g, S_fit).cpu().numpy()
    dec = dec.reshape(P, 6)
    assert np.isnan(dec[[1, 3, 5, 6, 7]]).all() and np.isnan(dec[:, [2, 4]]).all()
    assert np.isfinite(dec[good][:, [0, 1, 3, 5]]).all()


def test_max_iter_3_stops_unconverged_and_domain_svc_warns():
    S = _S()
    c = _case("fold160")
    got = _solve_case(c, 1e-3, max_iter=3)
    assert got["status"] == S.NOT_CONVERGED and got["iterations"] == 3 and got["gap"] >= 1e-3
    _check_feasible(got["alpha"], c["y"][c["train"]].astype(np.float64), c["C"])
    assert 2 <= int((got["alpha"] > 0).sum()) <= 6
    X, t = R.fixture("overlap")
    with pytest.warns(S.SvcConvergenceWarning, match=r"fold 0 stopped at max_iter=3 with a gap of \d"):
        res = S.domain_svc(X[t == 1], X[t == 0], max_iter=3)
    assert res.scores.shape == (5,) and not res.converged.any() and res.iterations.tolist() == [3] * 5
    assert ((0 <= res.scores) & (res.scores <= 1)).all() and np.isfinite(res.decision).all()


# ------------------------------------------------------------------------------------------------ domain_svc
@pytest.mark.parametrize("name", R.FIXTURES)
def test_domain_svc_predicts_what_the_restatement_predicts(name):
    S = _S()
    from bsed_amd import domain_gap as DG
    X, t = R.fixture(name)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = S.domain_svc(X[t == 1], X[t == 0])
    N = len(t)
    assert np.array_equal(res.fold, R.stratified_folds(t, 5)) and res.converged.all() and (res.iterations > 0).all()
    d2 = S.svc_d2_gpu(_gpu(X, torch.float32))
    y = np.where(t == 1, 1.0, -1.0)
    want_dec = np.empty(N)
    for f in range(5):
        tr, te = np.nonzero(res.fold != f)[0], np.nonzero(res.fold == f)[0]
        want_gamma = np.float32(R.scale_gamma(X[tr]))
        assert abs(res.gamma[f] - float(want_gamma)) <= float(np.spacing(want_gamma))           # one float32 ulp
        K = gpu_kernel_matrix(d2, res.gamma[f]).astype(np.float32)
        fit = R.solve(K[np.ix_(tr, tr)], y[tr], 1.0, 1e-10)
        want_dec[te] = R.decision(fit["alpha"], y[tr], fit["rho"], K[np.ix_(te, tr)])
        assert 2 <= res.n_support[f] <= len(tr)
    near = np.abs(want_dec) <= 2e-3
    err = float(np.abs(res.decision - want_dec).max())
    print(f"{name}: {int(near.sum())} points within 2e-3 of zero; max |decision - restatement(1e-10)| = {err:.3e}; "
          f"scores {res.scores.tolist()}; iterations {res.iterations.tolist()}")
    assert near.sum() <= 2 and err <= 2.2e-3
    assert np.array_equal((res.decision > 0)[~near], (want_dec > 0)[~near])
    want_scores = np.array([((want_dec > 0) == (y > 0))[res.fold == f].mean() for f in range(5)])
    sizes = np.array([(res.fold == f).sum() for f in range(5)])
    assert (np.abs(res.scores - want_scores) * sizes <= near.sum() + 1e-9).all()
    assert res.accuracy == float(res.scores.mean()) and res.proxy_a_distance == DG.proxy_a_distance(res.accuracy)
    if name == "apart":
        assert res.accuracy >= 0.95
    if name == "same":
        assert res.accuracy <= 0.65


def test_domain_svc_takes_a_fixed_gamma_and_another_fold_count():
    S = _S()
    X, t = R.fixture("uneven")
    res = S.domain_svc(torch.from_numpy(X[t == 1]).cuda(), X[t == 0], cv=3, C=2.0, gamma=0.07, tol=1e-4)
    assert res.scores.shape == (3,) and res.gamma.tolist() == [float(np.float32(0.07))] * 3
    assert np.array_equal(res.fold, R.stratified_folds(t, 3)) and res.converged.all()
    ref = R.cross_validate(X, t, cv=3, C=2.0, tol=1e-10, d2_32=S.svc_d2_gpu(_gpu(X, torch.float32)).cpu().numpy(),
                           kernel=lambda d2, g: gpu_kernel_matrix(_gpu(d2, torch.float32), 0.07).astype(np.float32))
    assert np.abs(res.decision - ref["decision"]).max() <= 2 * 1e-4      # 2 tol (the header, 6)


def test_domain_svc_of_a_model_is_the_classifier_of_its_embeddings():
    from oracle import seeded
    from test_event_metrics_gpu import _seeded_models
    from bsed_amd import domain_gap as DG
    S = _S()
    crnn, pred = _seeded_models(51)

    def loader(seed, gain):
        x = seeded.db_like_input(seed, 4, 256) * gain
        return [(((torch.from_numpy(x[i:i + 2]), torch.from_numpy(x[i:i + 2])), None), [f"clip{j}" for j in (i, i + 1)])
                for i in (0, 2)]
    synth, real = loader(52, 1.0), loader(53, 0.5)
    got = S.domain_svc_of(crnn, synth, real, pred, level="frame", max_points=40, seed=5, C=2.0)
    s, r = (DG.embed(crnn, ld, pred, level="frame", max_points=40, seed=5) for ld in (synth, real))
    want = S.domain_svc(s, r, C=2.0)
    assert got.decision.shape == (s.shape[0] + r.shape[0],) and np.array_equal(got.decision, want.decision)
    assert np.array_equal(got.scores, want.scores) and np.array_equal(got.gamma, want.gamma)


def test_svm_classification_end_to_end():
    """the reference's function: with replacement, so the sample holds duplicated points (the TAU rule)"""
    S = _S()
    rng = np.random.default_rng(9)
    synth = rng.normal(0, 1, (60, 12)).astype(np.float32)
    real_far, real_near = synth[:50] + np.float32(1.5), (synth[:50] + rng.normal(0, 1, (50, 12))).astype(np.float32)
    ada, no_ada = S.svm_classfication(synth, real_near, synth * 2, real_far * 2, sample_num=80, seed=3)
    si, ri = S.sample_indices(60, 50, 80, seed=3)
    assert len(np.unique(si)) < 80
    for res, (a, b) in ((ada, (synth, real_near)), (no_ada, (synth * 2, real_far * 2))):
        want = S.domain_svc(a[si], b[ri])
        assert np.array_equal(res.decision, want.decision) and res.converged.all() and res.scores.shape == (5,)
    assert no_ada.accuracy > ada.accuracy and no_ada.proxy_a_distance > ada.proxy_a_distance


def test_a_non_default_stream_gives_the_same_bits():
    S = _S()
    c, lists, gammas = _batch(5)
    x = _gpu(R.solver_case("fold160")["x"], torch.float32)
    fit, off = _launch(c, lists, gammas)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d2 = S.svc_d2_gpu(x)
        c2 = dict(c, d2=d2)
        fit2, _ = _launch(c2, lists, gammas)
        dec2 = S.svc_decision_gpu(d2, c["y_gpu"], off, np.concatenate(lists), [0] * 5 + [3], [1, 2, 3], gammas, fit2)
    stream.synchronize()
    dec = S.svc_decision_gpu(c["d2"], c["y_gpu"], off, np.concatenate(lists), [0] * 5 + [3], [1, 2, 3], gammas, fit)
    assert torch.equal(d2, c["d2"]) and torch.equal(dec, dec2)
    for a, b in zip(fit, fit2):
        assert torch.equal(a, b)


def test_refusals_on_the_gpu(monkeypatch):
    S = _S()
    x = torch.zeros((8, 3), device="cuda")
    for bad in (x.double(), x[0], torch.zeros((0, 3), device="cuda")):
        with pytest.raises(S.BsedError):
            S.svc_d2_gpu(bad)
    d2 = S.svc_d2_gpu(torch.randn((8, 3), device="cuda"))
    y = torch.tensor([1, -1] * 4, device="cuda", dtype=torch.int32)
    ok = dict(d2=d2, y=y, train_offsets=[0, 8], train_index=np.arange(8), gamma=0.5)
    for change in (dict(d2=d2[:, :7]), dict(d2=d2.double()), dict(y=y.long()), dict(y=y[:7]), dict(y=y.cpu()),
                   dict(train_offsets=[0, 7]), dict(train_offsets=[1, 8]), dict(train_offsets=[0, 9, 8]),
                   dict(train_offsets=torch.tensor([0, 8], device="cuda")), dict(train_index=np.arange(8.0)),
                   dict(gamma=0.0), dict(gamma=float("nan")), dict(gamma=[0.5, 0.5]), dict(gamma=1e-60), dict(C=0.0),
                   dict(tol=float("inf")), dict(max_iter=0), dict(max_iter=10_000_001),
                   dict(train_offsets=np.arange(66) * 0 + 8 * (np.arange(66) > 0))):
        with pytest.raises(S.BsedError):
            S.svc_solve_gpu(**dict(ok, **change))
    fit = S.svc_solve_gpu(**ok)
    assert int(fit.info[0, 1]) == S.CONVERGED
    for change in (dict(fit=None), dict(fit=fit._replace(alpha=fit.alpha[:7])), dict(test_offsets=[0, 2]),
                   dict(test_offsets=[0, 1, 3]), dict(fit=fit._replace(info=fit.info.long()))):
        with pytest.raises(S.BsedError):
            S.svc_decision_gpu(**dict(dict(ok, test_offsets=[0, 3], test_index=[0, 1, 2], fit=fit), **change))
    for bad in (dict(cv=1), dict(cv=65), dict(gamma="auto"), dict(cv=5, real=np.zeros((4, 3), np.float32)),
                dict(real=np.zeros((9, 4), np.float32))):
        with pytest.raises(S.BsedError):
            S.domain_svc(**dict(dict(synth=np.ones((9, 3), np.float32), real=np.zeros((9, 3), np.float32)), **bad))
    # distances that do not fit the device: the bytes are named, nothing falls back to the host
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1 << 20, 1 << 30))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda device=None: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda device=None: 0)
    with pytest.raises(S.BsedError, match=str(4 * 1000 * 1000)):
        S.svc_d2_gpu(torch.zeros((1000, 3), device="cuda"))
