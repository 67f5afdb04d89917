"""The domain classifier of the reference's analysis script (src/visualize.py, ``svm_classfication``:
``cross_val_score(SVC(), features, target, cv=5)`` on the synthetic and the real embeddings, with and without adversarial
training), made on the GPU: the accuracy of a trained domain classifier and the proxy A-distance made from it.

It is sklearn's ``SVC()`` -- libsvm's C-SVC with an RBF kernel at ``gamma="scale"`` -- under sklearn's unshuffled
``StratifiedKFold``: ``svc_d2_gpu`` makes the squared distances of all points once, ``svc_solve_gpu`` solves the duals of
all folds in ONE launch (one workgroup per fold) and ``svc_decision_gpu`` evaluates every held-out point in one more
(csrc/svc.hip; the rules are stated in include/bsed.h and restated in float64 by tests/svc_reference.py, which is pinned
to sklearn).  What is pinned: the folds, gamma, the optimum the solver converges to (so the decision values to the
solver's tolerance, and the per-fold scores except for held-out points whose decision value is within that tolerance of
zero).  What is not: libsvm's path to the optimum (its shrinking heuristic and its tie rule are left out), its float64
kernel values (they are float32 here, from the direct-difference distances), and the reference's draw of the sample,
which comes from numpy's global state.  Nothing falls back to the host."""
import ctypes
import warnings
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from ._lib import BsedError
from ._points import check_dense_fits, embed_two, gpu_points, two_domains
from ._points import gpu_tensor as _gpu_tensor
from .domain_gap import proxy_a_distance

SVC_MAX_POINTS = L.CONSTANTS["BSED_SVC_MAX_POINTS"]
SVC_MAX_PROBLEMS = L.CONSTANTS["BSED_SVC_MAX_PROBLEMS"]
SVC_MAX_ITER = L.CONSTANTS["BSED_SVC_MAX_ITER"]
CONVERGED, NOT_CONVERGED = L.CONSTANTS["BSED_SVC_CONVERGED"], L.CONSTANTS["BSED_SVC_NOT_CONVERGED"]
STATUS_NAMES = {L.CONSTANTS[k]: k[len("BSED_SVC_"):].lower().replace("_", " ") for k in (
    "BSED_SVC_CONVERGED", "BSED_SVC_NOT_CONVERGED", "BSED_SVC_BAD_INDEX", "BSED_SVC_BAD_LABEL", "BSED_SVC_ONE_CLASS",
    "BSED_SVC_BAD_OFFSETS")}

SvcFit = namedtuple("SvcFit", ["alpha", "rho", "gap", "info"])
DomainSvcResult = namedtuple("DomainSvcResult", ["scores", "accuracy", "proxy_a_distance", "decision", "fold", "n_support",
                                                 "iterations", "converged", "gamma"])


class SvcConvergenceWarning(UserWarning):
    """a fold's solver stopped at ``max_iter`` (what sklearn reports as a ``ConvergenceWarning``)"""


def svc_d2_gpu(x):
    """``x`` (N, D) float32 GPU tensor (unit stride along D, any row pitch >= D) -> ``d2`` (N, N) float32: the squared
    distances as ``bsed_pair_stats`` defines them, symmetric bit for bit with a zero diagonal.  One HIP launch, no host
    sync (include/bsed.h: ``bsed_svc_d2``)."""
    who = "svc_d2_gpu"
    x, pitch = gpu_points(x, who, 1, SVC_MAX_POINTS)
    N, D = x.shape
    check_dense_fits(N, x.device, who, "distances")
    d2 = torch.empty((N, N), device=x.device, dtype=torch.float32)
    L.call("bsed_svc_d2", ctypes.c_void_p(x.data_ptr()), pitch, N, D, L.ptr(d2), L.stream())
    return d2


def _d2_and_labels(d2, y, who):
    d2 = _gpu_tensor(d2, who, "d2", torch.float32, 2)
    N = d2.shape[0]
    if d2.shape[1] != N or not d2.is_contiguous() or not 2 <= N <= SVC_MAX_POINTS:
        raise BsedError(f"{who}: d2 must be a contiguous (N, N) matrix with 2 <= N <= {SVC_MAX_POINTS}, got "
                        f"{tuple(d2.shape)}")
    y = _gpu_tensor(y, who, "y", torch.int32, 1)
    if y.shape[0] != N or not y.is_contiguous():
        raise BsedError(f"{who}: y must be ({N},) contiguous int32 labels +1 / -1, got {tuple(y.shape)}")
    return d2, y, N


def _lists(offsets, index, device, who, name):
    """host offsets (P + 1) and the concatenated indices -> (offsets numpy int64, offsets on the GPU, indices on the GPU)"""
    if isinstance(offsets, torch.Tensor):
        if offsets.is_cuda:
            raise BsedError(f"{who}: {name}_offsets must live on the host (they size the launch)")
        offsets = offsets.numpy()
    off = np.asarray(offsets)
    if off.ndim != 1 or off.shape[0] < 2 or not np.issubdtype(off.dtype, np.integer):
        raise BsedError(f"{who}: {name}_offsets must be (P + 1,) integers, got {off.shape} {off.dtype}")
    off = off.astype(np.int64)
    index = torch.as_tensor(index)
    if index.dim() != 1 or index.dtype not in (torch.int32, torch.int64):
        raise BsedError(f"{who}: {name}_index must be a flat int32 or int64 list, got {tuple(index.shape)} {index.dtype}")
    total = index.shape[0]
    if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != total or total < 1:
        raise BsedError(f"{who}: {name}_offsets must rise from 0 to the {total} entries of {name}_index, got "
                        f"{off.tolist()}")
    index = index.to(device=device, dtype=torch.int32).contiguous()
    return off, torch.from_numpy(off.astype(np.int32)).to(device), index


def _gammas(gamma, P, who):
    g = np.asarray(gamma, np.float64).reshape(-1)
    if g.shape[0] == 1:
        g = np.repeat(g, P)
    if g.shape[0] != P or not (np.isfinite(g).all() and (g > 0).all()):
        raise BsedError(f"{who}: gamma must be one positive finite value or one per problem ({P}), got {g.tolist()}")
    g32 = g.astype(np.float32)
    if not (np.isfinite(g32).all() and (g32 > 0).all()):
        raise BsedError(f"{who}: gamma must be a positive finite float32, got {g.tolist()}")
    return (ctypes.c_float * P)(*g32.tolist())


def svc_solve_gpu(d2, y, train_offsets, train_index, gamma, C=1.0, tol=1e-3, max_iter=SVC_MAX_ITER):
    """The C-SVC duals of ``P`` problems in one launch (include/bsed.h: ``bsed_svc_solve``).  ``d2`` (N, N) float32 of
    ``svc_d2_gpu``, ``y`` (N) int32 GPU labels +1 / -1, ``train_offsets`` (P + 1) HOST integers into ``train_index``, the
    concatenated training points of the problems (any order), ``gamma`` one value or one per problem (host) ->
    ``SvcFit`` of GPU tensors: ``alpha`` float64 in the order of ``train_index``, ``rho`` (P), ``gap`` (P) float64,
    ``info`` (P, 2) int32 = (pair updates made, status: ``STATUS_NAMES``).  A problem with an index outside [0, N), a label
    that is not +1 / -1 or one class only gets its status, a NaN ``rho`` and a NaN-filled ``alpha``.  No host sync."""
    who = "svc_solve_gpu"
    d2, y, N = _d2_and_labels(d2, y, who)
    off, off_gpu, index = _lists(train_offsets, train_index, d2.device, who, "train")
    P = off.shape[0] - 1
    if not 1 <= P <= SVC_MAX_PROBLEMS:
        raise BsedError(f"{who}: 1 to {SVC_MAX_PROBLEMS} problems, got {P}")
    sizes = np.diff(off)
    if sizes.max() > SVC_MAX_POINTS:
        raise BsedError(f"{who}: at most {SVC_MAX_POINTS} training points per problem, got {int(sizes.max())}")
    C, tol, max_iter = float(C), float(tol), int(max_iter)
    if not (np.isfinite(C) and C > 0 and np.isfinite(tol) and tol > 0):
        raise BsedError(f"{who}: C and tol must be positive and finite, got {C} and {tol}")
    if not 1 <= max_iter <= SVC_MAX_ITER:
        raise BsedError(f"{who}: max_iter must lie in 1..{SVC_MAX_ITER}, got {max_iter}")
    gammas = _gammas(gamma, P, who)
    total = int(off[-1])
    ws_bytes = L.lib().bsed_svc_solve_workspace(P, total)
    if ws_bytes == 0:
        raise BsedError(f"{who}: no workspace for P={P}, total_train={total}")
    dev = d2.device
    ws = torch.empty(ws_bytes // 8, device=dev, dtype=torch.float64)
    alpha = torch.full((total,), float("nan"), device=dev, dtype=torch.float64)
    rho = torch.full((P,), float("nan"), device=dev, dtype=torch.float64)
    gap = torch.full((P,), float("nan"), device=dev, dtype=torch.float64)
    info = torch.zeros((P, 2), device=dev, dtype=torch.int32)
    L.call("bsed_svc_solve", L.ptr(d2), N, L.ptr(y, torch.int32), L.ptr(off_gpu, torch.int32), L.ptr(index, torch.int32), P,
           total, int(max(sizes.max(), 1)), gammas, C, tol, max_iter, L.ptr(alpha, torch.float64),
           L.ptr(rho, torch.float64), L.ptr(gap, torch.float64), L.ptr(info, torch.int32), L.ptr(ws, torch.float64),
           ws_bytes, L.stream())
    return SvcFit(alpha, rho, gap, info)


def svc_decision_gpu(d2, y, train_offsets, train_index, test_offsets, test_index, gamma, fit):
    """The decision values ``SUM_j alpha_j y_j K(t, j) - rho`` of every entry of ``test_index`` under its problem's
    ``fit`` (the ``SvcFit`` of ``svc_solve_gpu`` on the same training lists and ``gamma``) -> (len(test_index)) float64
    GPU tensor, NaN for the entries of a problem that the solver marked bad.  One launch for all problems, no host
    sync (include/bsed.h: ``bsed_svc_decision``)."""
    who = "svc_decision_gpu"
    d2, y, N = _d2_and_labels(d2, y, who)
    off, off_gpu, index = _lists(train_offsets, train_index, d2.device, who, "train")
    toff, toff_gpu, tindex = _lists(test_offsets, test_index, d2.device, who, "test")
    P = off.shape[0] - 1
    if not 1 <= P <= SVC_MAX_PROBLEMS or toff.shape[0] != P + 1:
        raise BsedError(f"{who}: 1 to {SVC_MAX_PROBLEMS} problems with P + 1 train and test offsets, got {off.shape[0]} "
                        f"and {toff.shape[0]} offsets")
    if not isinstance(fit, SvcFit):
        raise BsedError(f"{who}: fit must be the SvcFit of svc_solve_gpu")
    total, total_test = int(off[-1]), int(toff[-1])
    alpha = _gpu_tensor(fit.alpha, who, "fit.alpha", torch.float64, 1)
    rho = _gpu_tensor(fit.rho, who, "fit.rho", torch.float64, 1)
    info = _gpu_tensor(fit.info, who, "fit.info", torch.int32, 2)
    if alpha.shape[0] != total or rho.shape[0] != P or tuple(info.shape) != (P, 2):
        raise BsedError(f"{who}: fit does not belong to these {P} problems of {total} training points: alpha "
                        f"{tuple(alpha.shape)}, rho {tuple(rho.shape)}, info {tuple(info.shape)}")
    if max(total, total_test) > P * SVC_MAX_POINTS:
        raise BsedError(f"{who}: at most {P * SVC_MAX_POINTS} entries per list, got {total} and {total_test}")
    gammas = _gammas(gamma, P, who)
    dec = torch.empty(total_test, device=d2.device, dtype=torch.float64)
    L.call("bsed_svc_decision", L.ptr(d2), N, L.ptr(y, torch.int32), L.ptr(off_gpu, torch.int32),
           L.ptr(index, torch.int32), L.ptr(toff_gpu, torch.int32), L.ptr(tindex, torch.int32), P, total, total_test,
           gammas, L.ptr(alpha, torch.float64), L.ptr(rho, torch.float64), L.ptr(info, torch.int32),
           L.ptr(dec, torch.float64), L.stream())
    return dec


def scale_gamma(x_train):
    """sklearn's ``gamma="scale"`` of a training set (n, D), array or tensor: ``1 / (D * x.var())``, the variance taken
    over ALL elements in float64 where ``x`` lives; 1.0 when the variance is 0.  Rounded to float32, which is what the
    kernel takes -> a Python float."""
    x = torch.as_tensor(x_train)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise BsedError(f"scale_gamma: x_train must be (n, D), got {tuple(x.shape)}")
    var = float(x.double().var(unbiased=False))
    return float(np.float32(1.0 / (x.shape[1] * var) if var != 0 else 1.0))


def stratified_folds(y, k=5):
    """(N) labels -> (N) int64 numpy: the test fold of every point under sklearn's unshuffled ``StratifiedKFold(k)``,
    which is what ``cross_val_score`` uses for a classifier.  The classes are numbered by first appearance; their sorted
    numbers are dealt round-robin to the k folds, which fixes how many points of each class a fold tests; each class
    then hands its points out in order, fold 0's share first.  Raises when a class has fewer than ``k`` points (sklearn
    warns there unless every class has)."""
    y = np.asarray(y.detach().cpu() if isinstance(y, torch.Tensor) else y)
    k = int(k)
    if y.ndim != 1 or y.shape[0] < 2 or k < 2:
        raise BsedError(f"stratified_folds: (N,) labels with N >= 2 and k >= 2, got {y.shape} and k={k}")
    classes, first, counts = np.unique(y, return_index=True, return_counts=True)
    if counts.min() < k:
        raise BsedError(f"stratified_folds: every class needs at least k={k} points, got counts {counts.tolist()}")
    rank = np.empty(len(classes), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(classes))
    enc = rank[np.searchsorted(classes, y)]
    dealt = np.sort(enc)
    fold = np.empty(y.shape[0], np.int64)
    for c in range(len(classes)):
        share = [int(np.count_nonzero(dealt[f::k] == c)) for f in range(k)]
        fold[enc == c] = np.repeat(np.arange(k), share)
    return fold


def _centred_moments(x, rows=4096):
    """(N, D) float32 GPU tensor -> (s1, s2) (N) float64: per row the sums of (x - m) and (x - m)^2, m = the float64 mean
    of all elements; the variance of any subset of rows follows from them without another pass over x"""
    total = torch.zeros((), device=x.device, dtype=torch.float64)
    for r in range(0, x.shape[0], rows):
        total += x[r:r + rows].double().sum()
    mean = total / x.numel()
    s1, s2 = [], []
    for r in range(0, x.shape[0], rows):
        c = x[r:r + rows].double() - mean
        s1.append(c.sum(dim=1))
        s2.append((c * c).sum(dim=1))
    return torch.cat(s1), torch.cat(s2)


def default_max_iter(n_train):
    """the iteration bound ``domain_svc`` uses when none is given: 100 pair updates per training point, at least 10 000
    and at most the library's cap.  Measured (the float64 restatement of the solver, tol = 1e-3, C = 1): between 0.5 n
    and 1.2 n updates on the test fixtures (n = 96 .. 160: 72 .. 189) and 2 037 at n = 2 000, D = 256 -- a bound a
    hundred times what a fold needs never ends a healthy run, and still ends one that cycles."""
    return int(min(max(10_000, 100 * int(n_train)), SVC_MAX_ITER))


def domain_svc(synth, real, cv=5, C=1.0, gamma="scale", tol=1e-3, max_iter=None):
    """Two (n, D) sets of points (arrays or tensors) -> ``DomainSvcResult``: sklearn's ``cross_val_score(SVC(C=C,
    gamma=gamma, tol=tol), X, target, cv=cv)`` of the domain labelling, X = synth then real, target 1 = synth (y = +1)
    and 0 = real (y = -1).  ``scores`` (cv) float64 numpy = the accuracy on each held-out fold, ``accuracy`` their mean,
    ``proxy_a_distance`` = ``domain_gap.proxy_a_distance`` of it, ``decision`` (N) float64 numpy = the held-out decision
    value of every point (above 0 predicts synth; exactly 0 predicts real -- parity with sklearn on that measure-zero case
    is not pinned), ``fold`` (N) = ``stratified_folds``, ``n_support`` (cv) = the support vectors of each fold's fit,
    ``iterations`` (cv) the pair updates made, ``converged`` (cv) bool, ``gamma`` (cv) the float32 value of each fold:
    ``"scale"`` = ``scale_gamma`` of that fold's training rows, as sklearn fits it, or one number for all.
    One ``svc_d2_gpu`` over all points, one solve launch (the folds side by side) and one decision launch.  A fold that
    stops at ``max_iter`` (default ``default_max_iter`` of the largest training set) raises a ``SvcConvergenceWarning``
    naming the fold and its gap; the scores are still returned."""
    who = "domain_svc"
    x, ns, nr = two_domains(synth, real, who)
    cv = int(cv)
    N = ns + nr
    if not 2 <= cv <= SVC_MAX_PROBLEMS or N > SVC_MAX_POINTS:
        raise BsedError(f"{who}: 2 to {SVC_MAX_PROBLEMS} folds and at most {SVC_MAX_POINTS} points, got cv={cv}, N={N}")
    target = np.concatenate([np.ones(ns, np.int64), np.zeros(nr, np.int64)])
    fold = stratified_folds(target, cv)
    y = torch.from_numpy(np.where(target == 1, 1, -1).astype(np.int32)).to(x.device)
    train = [np.nonzero(fold != f)[0] for f in range(cv)]
    test = [np.nonzero(fold == f)[0] for f in range(cv)]
    train_offsets = np.concatenate([[0], np.cumsum([len(t) for t in train])])
    test_offsets = np.concatenate([[0], np.cumsum([len(t) for t in test])])
    train_index, test_index = np.concatenate(train), np.concatenate(test)
    if isinstance(gamma, str):
        if gamma != "scale":
            raise BsedError(f"{who}: gamma must be 'scale' or a positive number, got {gamma!r}")
        s1, s2 = _centred_moments(x)
        keep = torch.from_numpy(np.stack([fold != f for f in range(cv)])).to(x.device).double()      # (cv, N)
        m = keep.sum(dim=1) * x.shape[1]
        var = (keep @ s2) / m - ((keep @ s1) / m) ** 2
        gammas = [float(np.float32(1.0 / (x.shape[1] * v) if v != 0 else 1.0)) for v in var.tolist()]
    else:
        gammas = [float(np.float32(gamma))] * cv
    if max_iter is None:
        max_iter = default_max_iter(max(len(t) for t in train))
    d2 = svc_d2_gpu(x)
    fit = svc_solve_gpu(d2, y, train_offsets, train_index, gammas, C, tol, max_iter)
    dec = svc_decision_gpu(d2, y, train_offsets, train_index, test_offsets, test_index, gammas, fit)
    decision = np.empty(N)
    decision[test_index] = dec.cpu().numpy()
    info, gaps, alpha = fit.info.cpu().numpy(), fit.gap.cpu().numpy(), fit.alpha.cpu().numpy()
    for f in range(cv):
        if info[f, 1] not in (CONVERGED, NOT_CONVERGED):
            raise BsedError(f"{who}: fold {f}: {STATUS_NAMES.get(int(info[f, 1]), info[f, 1])}")
        if info[f, 1] == NOT_CONVERGED:
            warnings.warn(f"{who}: fold {f} stopped at max_iter={int(max_iter)} with a gap of {gaps[f]:.3e} (tol={tol}): "
                          "its score comes from a solution that has not converged; raise max_iter or scale the features",
                          SvcConvergenceWarning)
    scores = np.array([float(((decision[t] > 0) == (target[t] == 1)).mean()) for t in test])
    n_support = np.array([int((alpha[train_offsets[f]:train_offsets[f + 1]] > 0).sum()) for f in range(cv)])
    acc = float(scores.mean())
    return DomainSvcResult(scores, acc, proxy_a_distance(acc), decision, fold, n_support, info[:, 0].astype(np.int64),
                           info[:, 1] == CONVERGED, np.asarray(gammas))


def domain_svc_of(model, synth_loader, real_loader, predictor, fpn=False, level="clip", max_points=None, seed=0, **kw):
    """``domain_svc`` of the embeddings ``domain_gap.embed`` makes of the two loaders with ``model`` and ``predictor``
    (the reference classifies clips: ``level="clip"``)"""
    synth, real = embed_two(model, synth_loader, real_loader, predictor, fpn, level, max_points, seed)
    return domain_svc(synth, real, **kw)


def sample_indices(n_synth, n_real, sample_num=1000, seed=0):
    """the rows ``svm_classification`` draws: ``sample_num`` indices WITH replacement per domain from
    ``numpy.random.default_rng(seed)``, the synthetic ones first -> (synth_index, real_index)"""
    n_synth, n_real, sample_num = int(n_synth), int(n_real), int(sample_num)
    if min(n_synth, n_real, sample_num) < 1:
        raise BsedError(f"sample_indices: nothing to draw from: n_synth={n_synth}, n_real={n_real}, "
                        f"sample_num={sample_num}")
    rng = np.random.default_rng(int(seed))
    return rng.integers(0, n_synth, sample_num), rng.integers(0, n_real, sample_num)


def svm_classification(ada_synth, ada_real, no_ada_synth, no_ada_real, sample_num=1000, seed=0, **kw):
    """The reference's ``svm_classfication``: ``sample_num`` points per domain drawn with replacement, the SAME rows for
    the features of the model trained with adversarial adaptation (``ada_*``) and of the one without (``no_ada_*``), and
    ``domain_svc`` of each -> ``(ada, no_ada)``, two ``DomainSvcResult``; the reference prints their ``accuracy``.  The
    draw is this project's own stream (``sample_indices``: a numpy ``Generator`` seeded with ``seed``); the reference
    draws from numpy's global state, which nothing can reproduce.  Drawing with replacement puts duplicated points into
    the sample; the solver's TAU rule takes them.  ``kw`` goes to ``domain_svc``."""
    who = "svm_classification"
    sets = [torch.as_tensor(v) for v in (ada_synth, ada_real, no_ada_synth, no_ada_real)]
    if any(v.dim() != 2 for v in sets) or sets[0].shape[0] != sets[2].shape[0] or sets[1].shape[0] != sets[3].shape[0]:
        raise BsedError(f"{who}: four (n, D) sets, the two synthetic ones of the same n and the two real ones likewise (the "
                        f"same rows are drawn from both models' features), got {[tuple(v.shape) for v in sets]}")
    si, ri = sample_indices(sets[0].shape[0], sets[1].shape[0], sample_num, seed)
    pick = lambda v, idx: v[torch.from_numpy(idx).to(v.device)]
    ada = domain_svc(pick(sets[0], si), pick(sets[1], ri), **kw)
    no_ada = domain_svc(pick(sets[2], si), pick(sets[3], ri), **kw)
    return ada, no_ada


svm_classfication = svm_classification     # the reference's spelling
