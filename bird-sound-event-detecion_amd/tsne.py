"""The t-SNE map of the embedding: the picture and the number of the reference's analysis script (src/visualize.py:
``TSNE(n_components=2, perplexity=30).fit_transform`` of the synthetic and the real embeddings together, saved as
``tsne(frame).npy``, scattered, and scored with the silhouette of the two domains ON THE MAP), made on the GPU.

It is exact t-SNE -- sklearn's ``TSNE(method="exact")``, the algorithm that the reference's default Barnes-Hut method
approximates -- as an all-pairs problem: ``tsne_affinities_gpu`` makes the dense symmetric affinities with sklearn's
perplexity search, ``tsne_gradient_gpu`` the gradient of the KL divergence (one pass over the N x N affinities) and
``tsne`` runs sklearn's schedule on them (csrc/tsne.hip; the rules are stated in include/bsed.h and restated in float64
by tests/tsne_reference.py, which is pinned to sklearn's own functions).  ``domain_map`` / ``domain_map_of`` make the
reference's map of two domains with the silhouette ``domain_gap`` takes on it, ``save_domain_map`` writes the file and
the scatter plot.  What is not reproduced: the Barnes-Hut tree, and the reference's own printed number, which depends
on the draw of its random initialisation.  Nothing falls back to the host: a point count whose affinities do not fit
the device raises."""
import ctypes
import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from . import domain_gap as DG
from ._lib import BsedError
from ._points import check_dense_fits, embed_two, gpu_matrix, gpu_points, two_domains

TSNE_MAX_POINTS = L.CONSTANTS["BSED_TSNE_MAX_POINTS"]
EXPLORATION_ITER = 250                 # sklearn's TSNE._EXPLORATION_MAX_ITER
N_ITER_CHECK = 50                      # sklearn's TSNE._N_ITER_CHECK
EXPLORATION_MOMENTUM, FINAL_MOMENTUM, MIN_GAIN = 0.5, 0.8, 0.01

TsneAffinities = namedtuple("TsneAffinities", ["P", "sum_p", "beta"])
TsneResult = namedtuple("TsneResult", ["embedding", "kl_divergence", "n_iter"])
DomainMap = namedtuple("DomainMap", ["embedding", "labels", "silhouette", "kl_divergence", "n_iter"])


def affinity_bytes(n):
    """the bytes of the dense (n, n) float32 affinities"""
    return 4 * int(n) * int(n)


def tsne_affinities_gpu(x, perplexity=30.0):
    """``x`` (N, D) float32 GPU tensor (unit stride along D, any row pitch >= D) -> ``TsneAffinities``: ``P`` (N, N)
    float32 = p(j|i) + p(i|j), symmetric bit for bit with a zero diagonal and NOT divided by its sum, ``sum_p`` (1)
    float64 = that sum, ``beta`` (N) float32 = the precision sklearn's perplexity search ends at for each row.  Four HIP
    launches, no host sync; the definitions are include/bsed.h's (``bsed_tsne_affinities``)."""
    who = "tsne_affinities_gpu"
    x, pitch = gpu_points(x, who, 2, TSNE_MAX_POINTS)
    N, D = x.shape
    perplexity = float(perplexity)
    if not 0.0 < perplexity < N:
        raise BsedError(f"{who}: the perplexity must lie in (0, N={N}), got {perplexity}")
    check_dense_fits(N, x.device, who, "affinities")
    lib = L.lib()
    ws_bytes = lib.bsed_tsne_affinities_workspace(N)
    ws = torch.empty(ws_bytes // 8, device=x.device, dtype=torch.float64)
    P = torch.empty((N, N), device=x.device, dtype=torch.float32)
    beta = torch.empty(N, device=x.device, dtype=torch.float32)
    sum_p = torch.empty(1, device=x.device, dtype=torch.float64)
    L.call("bsed_tsne_affinities", ctypes.c_void_p(x.data_ptr()), pitch, N, D, perplexity, L.ptr(P), L.ptr(beta),
           L.ptr(sum_p, torch.float64), L.ptr(ws, torch.float64), ws_bytes, L.stream())
    return TsneAffinities(P, sum_p, beta)


class _Gradient:
    """the buffers of ``bsed_tsne_gradient`` for one set of affinities, allocated once; ``launch`` reads nothing back"""

    def __init__(self, aff, splits, who):
        if not isinstance(aff, TsneAffinities):
            raise BsedError(f"{who}: aff must be the TsneAffinities of tsne_affinities_gpu")
        self.P = gpu_matrix(aff.P, who, "aff.P", 2, TSNE_MAX_POINTS)
        self.N = self.P.shape[0]
        if self.P.shape[1] != self.N or not self.P.is_contiguous():
            raise BsedError(f"{who}: aff.P must be a contiguous (N, N) matrix, got {tuple(self.P.shape)}")
        self.splits = int(splits)
        if self.splits < 0:
            raise BsedError(f"{who}: splits must be 0 (the library's choice) or positive, got {splits}")
        sum_p = float(aff.sum_p)                                     # one host sync, once per set of affinities
        if not (np.isfinite(sum_p) and sum_p > 0.0):
            raise BsedError(f"{who}: the affinities sum to {sum_p}")
        self.inv_sum_p = 1.0 / sum_p
        self.ws_bytes = L.lib().bsed_tsne_gradient_workspace(self.N, self.splits)
        if self.ws_bytes == 0:
            raise BsedError(f"{who}: no workspace for N={self.N}, splits={self.splits}")
        dev = self.P.device
        self.ws = torch.empty(self.ws_bytes // 8, device=dev, dtype=torch.float64)
        self.grad = torch.empty((self.N, 2), device=dev, dtype=torch.float32)
        self.stats = torch.empty(3, device=dev, dtype=torch.float64)

    def launch(self, y, exaggeration, error):
        L.call("bsed_tsne_gradient", L.ptr(y), L.ptr(self.P), self.N, self.inv_sum_p, float(exaggeration), int(bool(error)),
               self.splits, L.ptr(self.grad), L.ptr(self.stats, torch.float64), L.ptr(self.ws, torch.float64),
               self.ws_bytes, L.stream())


def _map_tensor(y, n, who):
    y = gpu_matrix(y, who, "y", 2, TSNE_MAX_POINTS, cols=2)
    if y.shape[0] != n:
        raise BsedError(f"{who}: y must be ({n}, 2), got {tuple(y.shape)}")
    return y.contiguous()


def tsne_gradient_gpu(y, aff, exaggeration=1.0, error=False, splits=0):
    """``y`` (N, 2) float32 GPU tensor, ``aff`` of ``tsne_affinities_gpu`` -> ``(grad, kl, grad_norm, z)``: the gradient
    (N, 2) float32 of the KL divergence between the affinities (times ``exaggeration``) and the Student-t similarities
    of the map, as sklearn's ``_kl_divergence`` forms it; ``kl`` the divergence itself with ``error=True``, NaN
    otherwise; ``grad_norm`` = the Euclidean norm of ``grad``; ``z`` = the sum of 1 / (1 + |y_i - y_j|^2) over i != j.
    The three scalars are read back (one host sync); ``tsne`` reads them at its convergence checks only."""
    who = "tsne_gradient_gpu"
    g = _Gradient(aff, splits, who)
    g.launch(_map_tensor(y, g.N, who), exaggeration, error)
    z, g2, kl = g.stats.tolist()
    return g.grad, kl, float(np.sqrt(g2)), z


def run_schedule(objective, update, measure, max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7,
                 early_exaggeration=12.0):
    """sklearn's t-SNE schedule (``TSNE._tsne`` over two calls of ``_gradient_descent``) with the arithmetic left to
    three callables, so it runs anywhere: ``objective(exaggeration, want_error)`` evaluates the gradient at the current
    map and returns a handle to it; ``update(handle, momentum, restart)`` takes the step (``restart``: first zero the
    velocity and set the gains to 1, which sklearn does at the start of each phase); ``measure(handle)`` ->
    ``(error, grad_norm)`` of an evaluation made with ``want_error`` and stepped from -- the only place a value is read.
    Phase 1: iterations 0 .. 249 at momentum 0.5 with the affinities times ``early_exaggeration``, no progress allowed
    for 250 iterations; phase 2: up to ``max_iter`` at momentum 0.8 without exaggeration, ``n_iter_without_progress``.
    Every 50th iteration is a check: the error is measured; the phase ends when the error has not improved for more than
    the allowed number of iterations (not tested on a check that improves it) or when the gradient norm is at most
    ``min_grad_norm``.  The last iteration of a phase evaluates the error too.  -> ``(error, n_iter)``: the error of the
    last evaluation (made BEFORE the last step, as sklearn's ``kl_divergence_`` is) and the index of the last iteration
    (sklearn's ``n_iter_``: ``max_iter - 1`` when nothing stops it)."""
    max_iter = int(max_iter)
    if max_iter < EXPLORATION_ITER:
        raise BsedError(f"run_schedule: max_iter must be at least {EXPLORATION_ITER} (sklearn's rule), got {max_iter}")

    def descend(it, last, momentum, exaggeration, patience):
        error = best_error = np.finfo(float).max
        best_iter = i = it
        for i in range(it, last):
            check = (i + 1) % N_ITER_CHECK == 0
            want_error = check or i == last - 1
            handle = objective(exaggeration, want_error)
            update(handle, momentum, i == it)
            if check:
                error, grad_norm = measure(handle)
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > patience:
                    break
                if grad_norm <= min_grad_norm:
                    break
            elif want_error:
                error = measure(handle)[0]
        return error, i

    error, it = descend(0, EXPLORATION_ITER, EXPLORATION_MOMENTUM, float(early_exaggeration), EXPLORATION_ITER)
    if it < EXPLORATION_ITER - 1 or max_iter > EXPLORATION_ITER:
        error, it = descend(it + 1, max_iter, FINAL_MOMENTUM, 1.0, int(n_iter_without_progress))
    return float(error), it


def pca_init(x):
    """(N, D) tensor -> (N, 2) float32 on the same device: the scores of the two leading principal components, in
    float64, from the eigenvectors of the smaller of the covariance (D x D) and the Gram (N x N) matrix of the centred
    points, scaled so that the first column has standard deviation 1e-4 (sklearn's rule).  Sign: each column is oriented
    so that its entry of largest magnitude is positive -- this project's convention; sklearn's randomized PCA has its
    own, and neither the sign nor the solver is pinned.  A second component that does not exist (D = 1) is zero."""
    x = torch.as_tensor(x).double()
    if x.dim() != 2 or x.shape[0] < 2:
        raise BsedError(f"pca_init: x must be (N, D) with N >= 2, got {tuple(x.shape)}")
    N, D = x.shape
    c = x - x.mean(dim=0, keepdim=True)
    k = min(2, N, D)
    if D <= N:
        _, vec = torch.linalg.eigh(c.T @ c)
        y = c @ vec[:, -k:].flip(1)
    else:
        val, vec = torch.linalg.eigh(c @ c.T)
        y = vec[:, -k:].flip(1) * val[-k:].flip(0).clamp_min(0).sqrt()
    rows = y.abs().argmax(dim=0)
    y = y * torch.where(y[rows, torch.arange(k, device=y.device)] < 0, -1.0, 1.0)
    if k < 2:
        y = torch.cat([y, torch.zeros((N, 2 - k), dtype=y.dtype, device=y.device)], dim=1)
    std = y[:, 0].std(unbiased=False)
    if not (torch.isfinite(std) and std > 0):
        raise BsedError("pca_init: the points do not vary: there is no principal component to start from")
    return (y / std * 1e-4).float()


def _initial_map(x, init, seed, who):
    N = x.shape[0]
    if isinstance(init, str):
        if init == "pca":
            return pca_init(x).contiguous()
        if init == "random":
            gen = torch.Generator().manual_seed(int(seed))
            return (1e-4 * torch.randn((N, 2), generator=gen, dtype=torch.float32)).to(x.device)
        raise BsedError(f"{who}: init must be 'pca', 'random' or an (N, 2) array, got {init!r}")
    y = torch.as_tensor(init)
    if y.dim() != 2 or y.shape[0] != N or y.shape[1] != 2:
        raise BsedError(f"{who}: two components only: init must be ({N}, 2), got {tuple(y.shape)}")
    return y.to(device=x.device, dtype=torch.float32).clone().contiguous()


def tsne(x, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, n_iter_without_progress=300,
         min_grad_norm=1e-7, init="pca", seed=0, splits=0):
    """``x`` (N, D) float32 GPU tensor -> ``TsneResult(embedding (N, 2) float32 GPU tensor, kl_divergence, n_iter)``:
    sklearn's ``TSNE(n_components=2, method="exact")`` with these parameters (``run_schedule``; ``learning_rate="auto"``
    = max(N / early_exaggeration / 4, 50)).  ``init``: ``"pca"`` (``pca_init``), ``"random"`` (1e-4 times normal draws of
    a torch generator seeded with ``seed``) or an (N, 2) array.  An iteration is a gradient (three launches) and an update
    (one); the host reads three scalars at every 50th iteration, where the gradient norm it tests is, as in sklearn, the
    one of the gradient times the gains.  ``kl_divergence`` is the divergence of the RETURNED map (one more evaluation;
    sklearn's ``kl_divergence_`` is the one of the map before its last step), ``n_iter`` sklearn's ``n_iter_``."""
    who = "tsne"
    x = gpu_matrix(x, who, "x", 2, TSNE_MAX_POINTS)        # checked before the init is made; the affinities take any pitch
    N = x.shape[0]
    y = _initial_map(x, init, seed, who)
    if learning_rate == "auto":
        learning_rate = max(N / float(early_exaggeration) / 4.0, 50.0)
    learning_rate = float(learning_rate)
    if not (learning_rate > 0 and float(early_exaggeration) >= 1.0):
        raise BsedError(f"{who}: learning_rate must be positive and early_exaggeration at least 1, got {learning_rate} and "
                        f"{early_exaggeration}")
    if int(max_iter) < EXPLORATION_ITER:
        raise BsedError(f"{who}: max_iter must be at least {EXPLORATION_ITER} (sklearn's rule), got {max_iter}")
    aff = tsne_affinities_gpu(x, perplexity)
    g = _Gradient(aff, splits, who)
    velocity, gains = torch.zeros_like(y), torch.ones_like(y)

    def objective(exaggeration, want_error):
        g.launch(y, exaggeration, want_error)
        return g

    def update(_handle, momentum, restart):
        if restart:
            velocity.zero_()
            gains.fill_(1.0)
        L.call("bsed_tsne_update", L.ptr(y), L.ptr(g.grad), L.ptr(velocity), L.ptr(gains), 2 * N, momentum, learning_rate,
               MIN_GAIN, L.stream())

    def measure(_handle):
        norm = torch.linalg.vector_norm((g.grad * gains).double())    # sklearn tests the norm of grad * gains
        return float(g.stats[2]), float(norm)

    _, n_iter = run_schedule(objective, update, measure, max_iter, n_iter_without_progress, min_grad_norm,
                             early_exaggeration)
    g.launch(y, 1.0, True)
    return TsneResult(y, float(g.stats[2]), n_iter)


def domain_map(synth, real, **tsne_kw):
    """Two (n, D) sets of points (arrays or tensors) -> ``DomainMap``: ``embedding`` (n_synth + n_real, 2) float32 GPU
    tensor, the ``tsne`` map of the two sets together (synth first), ``labels`` (0 = synth, 1 = real, int64 numpy),
    ``silhouette`` = ``domain_gap``'s silhouette of the two domains taken ON THE MAP -- the number src/visualize.py
    prints --, ``kl_divergence`` and ``n_iter`` of the run."""
    x, ns, nr = two_domains(synth, real, "domain_map")
    res = tsne(x, **tsne_kw)
    labels = np.concatenate([np.zeros(ns, np.int64), np.ones(nr, np.int64)])
    gap = DG.domain_gap(res.embedding[:ns], res.embedding[ns:])
    return DomainMap(res.embedding, labels, gap.silhouette, res.kl_divergence, res.n_iter)


def domain_map_of(model, synth_loader, real_loader, predictor, fpn=False, level="frame", max_points=None, seed=0,
                  **tsne_kw):
    """``domain_map`` of the embeddings ``domain_gap.embed`` makes of the two loaders (the reference maps frames:
    ``level="frame"``, with ``max_points`` drawn per domain -- it samples 1000 of each)"""
    synth, real = embed_two(model, synth_loader, real_loader, predictor, fpn, level, max_points, seed)
    return domain_map(synth, real, seed=seed, **tsne_kw)


def save_domain_map(result, folder, plot=False, level="frame"):
    """writes the map as ``tsne(<level>).npy`` into ``folder`` (the reference's file name; float32, synth rows first) and
    returns its path.  ``plot=True`` also writes the reference's scatter ``syn vs real(<level>).png``: synth as x
    markers, real in red, a legend, no axes; it needs matplotlib and raises without it."""
    if not isinstance(result, DomainMap):
        raise BsedError("save_domain_map: result must be the DomainMap of domain_map")
    emb = result.embedding.detach().cpu().numpy() if isinstance(result.embedding, torch.Tensor) else np.asarray(result.embedding)
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, f"tsne({level}).npy")
    np.save(path, emb.astype(np.float32))
    if plot:
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError as e:
            raise BsedError(f"save_domain_map: plot=True needs matplotlib ({e})")
        labels = np.asarray(result.labels)
        fig = plt.figure()
        plt.scatter(emb[labels == 0, 0], emb[labels == 0, 1], alpha=0.6, s=10, marker="x", label="synth")
        plt.scatter(emb[labels == 1, 0], emb[labels == 1, 1], alpha=0.3, s=10, c="r", label="real")
        plt.legend()
        plt.axis("off")
        fig.savefig(os.path.join(folder, f"syn vs real({level}).png"))
        plt.close(fig)
    return path
