"""The synthetic-to-real domain gap of the embedding: what the reference's analysis script measures after adversarial
training (src/visualize.py: ``visualization`` prints sklearn's ``silhouette_score`` of the synth / real labelling,
``svm_classfication`` cross-validates a domain classifier), computed on the GPU from one all-pairs pass over the
embeddings (``pair_stats_gpu``; the sums as include/bsed.h states them, ``bsed_pair_stats``):

- the silhouette of the two domains (``silhouette_samples`` / ``silhouette_score``, sklearn's rules);
- the leave-one-out nearest-neighbour domain accuracy (``nn_accuracy``) -- the cheap measure that needs no training; the
  reference's SVC cross-validation itself is ``bsed_amd.svc`` -- and the proxy A-distance made from it
  (``proxy_a_distance``);
- the multi-kernel MMD^2 of the domain-adaptation literature (``mmd_scales``, ``mk_mmd2``).

The arithmetic on the sums is float64 numpy on the host and works on arrays without a GPU.  ``embed`` collects the
embeddings of a loader on the GPU, ``load_embedded_features`` reads the dumps of ``get_predictions(saved_feature_dir=
...)``, ``domain_gap`` scores two sets and ``domain_gap_of`` composes the two.  The silhouette here is taken on the
embedding itself; the reference takes it on a t-SNE map of the two domains, which ``bsed_amd.tsne`` makes
(``tsne.domain_map`` scores its map with this module's silhouette: ``domain_gap`` takes any ``(n, D)``).  ``embed``,
``load_embedded_features`` and the checks of the point matrix are ``_points``'s, shared with ``tsne`` and ``svc``."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from ._lib import BsedError
from ._points import embed, load_embedded_features  # noqa: F401  (public names of this module)
from ._points import embed_two, gpu_points, two_domains

PAIR_MAX_GROUPS = L.CONSTANTS["BSED_PAIR_MAX_GROUPS"]
PAIR_MAX_SCALES = L.CONSTANTS["BSED_PAIR_MAX_SCALES"]
DAN_MULTIPLIERS = (0.25, 0.5, 1.0, 2.0, 4.0)

PairStats = namedtuple("PairStats", ["dist_sum", "kern_sum", "nn_d2", "nn_index", "counts"])
DomainGapResult = namedtuple("DomainGapResult", ["silhouette", "silhouette_samples", "nn_accuracy", "proxy_a_distance",
                                                 "mmd2", "mk_mmd2", "mean_sq_distance", "counts"])


def pair_stats_gpu(x, groups, n_groups=None, scales=(), splits=0):
    """``x`` (N, D) float32 GPU tensor (unit stride along D, any row pitch >= D), ``groups`` (N) integer labels ->
    ``PairStats`` of GPU tensors: ``dist_sum`` (N, G) float64 = per point and group the sum of the distances to the other
    points of that group, ``kern_sum`` (N, G, S) float64 = the same sums of ``exp(-d2 * scales[s])``, ``nn_d2`` (N)
    float32 / ``nn_index`` (N) int32 = the nearest other point (smallest index on a tie; inf / -1 when there is none),
    ``counts`` (G) int64 = the points per group.  A label outside ``[0, n_groups)`` masks its point: it is summed into
    nothing, is nobody's neighbour and is not counted; its own row is still produced.  ``n_groups`` defaults to the
    largest label + 1 (one host sync).  ``splits``: the column splits of the launch, 0 = the library's choice; any value
    gives the same sums to float64 round-off.  Two HIP launches; the definitions are include/bsed.h's.  ``counts`` comes from
    ``torch.bincount`` over the unmasked labels, which reads a size back: the one host sync besides ``n_groups=None``."""
    who = "pair_stats_gpu"
    x, pitch = gpu_points(x, who)
    N, D = x.shape
    groups = torch.as_tensor(groups)
    if groups.dtype not in (torch.int32, torch.int64) or tuple(groups.shape) != (N,):
        raise BsedError(f"{who}: groups must be ({N},) int32 or int64 labels, got {tuple(groups.shape)} {groups.dtype}")
    groups = groups.to(device=x.device, dtype=torch.int32).contiguous()
    G = int(groups.max()) + 1 if n_groups is None else int(n_groups)
    if not 1 <= G <= PAIR_MAX_GROUPS:
        raise BsedError(f"{who}: 1 to {PAIR_MAX_GROUPS} groups, got {G}")
    scales = torch.as_tensor(scales, dtype=torch.float32).reshape(-1).to(x.device)
    S = scales.numel()
    if S > PAIR_MAX_SCALES:
        raise BsedError(f"{who}: at most {PAIR_MAX_SCALES} scales, got {S}")
    splits = int(splits)
    if splits < 0:
        raise BsedError(f"{who}: splits must be 0 (the library's choice) or positive, got {splits}")
    lib = L.lib()
    ws_bytes = lib.bsed_pair_stats_workspace(N, G, S, splits)
    if ws_bytes == 0:
        raise BsedError(f"{who}: no workspace for N={N}, G={G}, S={S}, splits={splits}")
    ws = torch.empty(ws_bytes // 8, device=x.device, dtype=torch.float64)
    dist_sum = torch.empty((N, G), device=x.device, dtype=torch.float64)
    kern_sum = torch.empty((N, G, S), device=x.device, dtype=torch.float64)
    nn_d2 = torch.empty(N, device=x.device, dtype=torch.float32)
    nn_index = torch.empty(N, device=x.device, dtype=torch.int32)
    L.call("bsed_pair_stats", ctypes.c_void_p(x.data_ptr()), pitch, N, D, L.ptr(groups, torch.int32), G,
           L.ptr(scales, torch.float32) if S else None, S, splits, L.ptr(dist_sum, torch.float64),
           L.ptr(kern_sum, torch.float64) if S else None, L.ptr(nn_d2), L.ptr(nn_index, torch.int32),
           L.ptr(ws, torch.float64), ws_bytes, L.stream())
    valid = (groups >= 0) & (groups < G)
    counts = torch.bincount(groups[valid].long(), minlength=G)
    return PairStats(dist_sum, kern_sum, nn_d2, nn_index, counts)


def _host(a, dtype=None):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a if dtype is None else a.astype(dtype)


def _labels(groups, counts, who):
    groups, counts = _host(groups, np.int64), _host(counts, np.int64)
    if groups.ndim != 1 or counts.ndim != 1:
        raise BsedError(f"{who}: groups must be (N,) and counts (G,), got {groups.shape} and {counts.shape}")
    return groups, counts, (groups >= 0) & (groups < counts.shape[0])


def silhouette_samples(dist_sum, groups, counts):
    """(N, G) distance sums of ``pair_stats_gpu``, (N) labels, (G) points per group -> (N) float64 silhouette
    coefficients by sklearn's rules: a = the sum to the own group / (n_own - 1), b = the smallest mean distance to
    another non-empty group, s = (b - a) / max(a, b); a point alone in its group scores 0, and so does 0 / 0.  A masked
    point (label outside [0, G)) scores NaN.  Fewer than 2 non-empty groups raise."""
    who = "silhouette_samples"
    d = _host(dist_sum, np.float64)
    groups, counts, valid = _labels(groups, counts, who)
    N, G = groups.shape[0], counts.shape[0]
    if d.shape != (N, G):
        raise BsedError(f"{who}: dist_sum must be ({N}, {G}), got {d.shape}")
    if int((counts > 0).sum()) < 2:
        raise BsedError(f"{who}: the silhouette needs at least 2 non-empty groups, got counts {counts.tolist()}")
    own = np.where(valid, groups, 0)
    rows = np.arange(N)
    n_own = counts[own]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = d[rows, own] / (n_own - 1)
        mean = d / counts[None, :]
        mean[:, counts == 0] = np.inf
        mean[rows, own] = np.inf
        b = mean.min(axis=1)
        s = (b - a) / np.maximum(a, b)
    s = np.where(np.isnan(s) | (n_own == 1), 0.0, s)
    return np.where(valid, s, np.nan)


def silhouette_score(dist_sum, groups, counts):
    """the mean of ``silhouette_samples`` over the unmasked points (sklearn's ``silhouette_score``)"""
    s = silhouette_samples(dist_sum, groups, counts)
    return float(s[~np.isnan(s)].mean())


def nn_accuracy(nn_index, groups):
    """(N) nearest-neighbour indices of ``pair_stats_gpu``, (N) labels -> the share of the points with a neighbour
    (index >= 0) whose neighbour has their label: the leave-one-out 1-NN accuracy of the domain labelling, 0.5 for two
    domains that cannot be told apart, 1 for separated ones.  NaN when no point has a neighbour."""
    nn, groups = _host(nn_index, np.int64), _host(groups, np.int64)
    if nn.shape != groups.shape or nn.ndim != 1:
        raise BsedError(f"nn_accuracy: nn_index {nn.shape} and groups {groups.shape} must both be (N,)")
    has = nn >= 0
    if not has.any():
        return float("nan")
    return float((groups[nn[has]] == groups[has]).mean())


def proxy_a_distance(acc):
    """the proxy A-distance 2 (1 - 2 err) = 2 (2 acc - 1) of a domain classifier of accuracy ``acc``"""
    return 2.0 * (2.0 * float(acc) - 1.0)


def mean_sq_distance(x):
    """(N, D) array or tensor -> the mean of the squared distance over the pairs i != j, from the centred second
    moment in float64 (sum_{i != j} |x_i - x_j|^2 = 2 N sum_i |x_i - mean|^2): O(N D), no kernel; runs where ``x``
    lives"""
    x = torch.as_tensor(x)
    if x.dim() != 2 or x.shape[0] < 2:
        raise BsedError(f"mean_sq_distance: x must be (N, D) with N >= 2, got {tuple(x.shape)}")
    x = x.double()
    c = x - x.mean(dim=0, keepdim=True)
    return float(2.0 * (c * c).sum() / (x.shape[0] - 1))


def mmd_scales(mean_d2, multipliers=DAN_MULTIPLIERS):
    """the scales 1 / (2 alpha mean_d2) of DAN's Gaussian kernels exp(-d2 / (2 alpha mean_d2)), one per multiplier
    alpha, as float32 (what ``pair_stats_gpu`` takes)"""
    m = np.asarray(multipliers, np.float64).reshape(-1)
    if not (np.isfinite(mean_d2) and mean_d2 > 0) or not (m > 0).all():
        raise BsedError(f"mmd_scales: the mean squared distance and the multipliers must be positive, got {mean_d2!r}, "
                        f"{m.tolist()}")
    return (1.0 / (2.0 * m * float(mean_d2))).astype(np.float32)


def mk_mmd2(kern_sum, groups, counts, a=0, b=1, unbiased=False):
    """(N, G, S) kernel sums of ``pair_stats_gpu`` -> ``(per_scale (S) float64, their sum)``: the squared maximum mean
    discrepancy between groups ``a`` and ``b``.  Biased (the V-statistic): (K_aa + n_a) / n_a^2 + (K_bb + n_b) / n_b^2 -
    2 K_ab / (n_a n_b), the diagonal's k = 1 terms added here; unbiased (the U-statistic): K_aa / (n_a (n_a - 1)) +
    K_bb / (n_b (n_b - 1)) - 2 K_ab / (n_a n_b).  K_uv = the sum of ``kern_sum[i][v]`` over the points i of group u."""
    who = "mk_mmd2"
    k = _host(kern_sum, np.float64)
    groups, counts, _ = _labels(groups, counts, who)
    if k.ndim != 3 or k.shape[:2] != (groups.shape[0], counts.shape[0]):
        raise BsedError(f"{who}: kern_sum must be ({groups.shape[0]}, {counts.shape[0]}, S), got {k.shape}")
    if a == b or not (0 <= a < counts.shape[0] and 0 <= b < counts.shape[0]):
        raise BsedError(f"{who}: a and b must be two different groups below {counts.shape[0]}, got {a} and {b}")
    na, nb = int(counts[a]), int(counts[b])
    if min(na, nb) < (2 if unbiased else 1):
        raise BsedError(f"{who}: groups of {na} and {nb} points are too small")
    kaa, kbb = k[groups == a, a, :].sum(axis=0), k[groups == b, b, :].sum(axis=0)
    kab = k[groups == a, b, :].sum(axis=0)
    if unbiased:
        per = kaa / (na * (na - 1)) + kbb / (nb * (nb - 1)) - 2.0 * kab / (na * nb)
    else:
        per = (kaa + na) / (na * na) + (kbb + nb) / (nb * nb) - 2.0 * kab / (na * nb)
    return per, float(per.sum())


def domain_gap(synth, real, multipliers=DAN_MULTIPLIERS, splits=0):
    """Two (n, D) sets of points (arrays or tensors; group 0 = ``synth``, group 1 = ``real``) -> ``DomainGapResult``:
    ``silhouette`` of the two-domain labelling and its ``silhouette_samples`` (synth first), ``nn_accuracy`` and the
    ``proxy_a_distance`` made from it, ``mmd2`` per multiplier (biased, Gaussian kernels at ``mmd_scales`` of the pooled
    ``mean_sq_distance``) and their sum ``mk_mmd2``, ``counts``.  One all-pairs pass on the GPU (``pair_stats_gpu``),
    float64 arithmetic on its sums on the host."""
    x, ns, nr = two_domains(synth, real, "domain_gap")
    groups = torch.cat([torch.zeros(ns, dtype=torch.int32), torch.ones(nr, dtype=torch.int32)])
    mean_d2 = mean_sq_distance(x)
    scales = mmd_scales(mean_d2, multipliers)
    stats = pair_stats_gpu(x, groups.to(x.device), 2, scales, splits)
    counts = stats.counts.cpu().numpy()
    samples = silhouette_samples(stats.dist_sum, groups, counts)
    acc = nn_accuracy(stats.nn_index, groups)
    per, total = mk_mmd2(stats.kern_sum, groups, counts)
    return DomainGapResult(float(samples.mean()), samples, acc, proxy_a_distance(acc), per, total, mean_d2, counts)


def domain_gap_of(model, synth_loader, real_loader, predictor, fpn=False, level="clip", max_points=None, seed=0,
                  multipliers=DAN_MULTIPLIERS, splits=0):
    """``domain_gap`` of the embeddings ``embed`` makes of the two loaders with ``model`` and ``predictor``"""
    synth, real = embed_two(model, synth_loader, real_loader, predictor, fpn, level, max_points, seed)
    return domain_gap(synth, real, multipliers, splits)
