"""Float64 restatement of the all-pairs statistics behind the domain gap (include/bsed.h, ``bsed_pair_stats``) and of
the measures made from them (bsed_amd/domain_gap.py), in plain numpy with direct differences, from the SAME float32
inputs the kernel reads.  Nothing here is shared with the product: the product's host functions are compared with
these, and these with sklearn (tests/test_domain_gap_reference_cpu.py)."""
import numpy as np

from d2_reference import U, d2_matrix  # noqa: F401  (the tests read them as R.U and R.d2_matrix)


def valid_mask(groups, G):
    groups = np.asarray(groups, np.int64)
    return (groups >= 0) & (groups < G)


def pair_stats_np(x, groups, G, scales=(), roots=None):
    """-> dict: ``d2`` (N,N), ``dist_sum`` (N,G), ``kern_sum`` (N,G,S), ``nn_d2`` (N), ``nn_index`` (N) (smallest j on
    a tie, -1 / inf without a candidate), ``counts`` (G), ``pairs`` (N,G) = the number of pairs summed.  ``scales`` are
    taken as float32 values (what the kernel reads).  ``roots``: a function applied to d2 in place of the float64
    square root (the exact-lattice tests pass the float32-rounded root)."""
    groups = np.asarray(groups, np.int64)
    N = groups.shape[0]
    d2 = d2_matrix(x)
    d = np.sqrt(d2) if roots is None else roots(d2)
    scales = np.asarray(scales, np.float32).astype(np.float64).reshape(-1)
    valid = valid_mask(groups, G)
    dist_sum, kern_sum = np.zeros((N, G)), np.zeros((N, G, scales.shape[0]))
    pairs = np.zeros((N, G), np.int64)
    nn_d2, nn_index = np.full(N, np.inf), np.full(N, -1, np.int64)
    for i in range(N):
        for g in range(G):
            sel = (groups == g) & valid
            sel[i] = False
            pairs[i, g] = sel.sum()
            dist_sum[i, g] = d[i, sel].sum()
            for s, c in enumerate(scales):
                kern_sum[i, g, s] = np.exp(-(d2[i, sel] * c)).sum()
        cand = valid.copy()
        cand[i] = False
        if cand.any():
            j = np.flatnonzero(cand)
            k = j[np.argmin(d2[i, j])]                  # argmin takes the first of equal values: the smallest j
            nn_d2[i], nn_index[i] = d2[i, k], k
    counts = np.bincount(groups[valid], minlength=G)
    return dict(d2=d2, dist_sum=dist_sum, kern_sum=kern_sum, nn_d2=nn_d2, nn_index=nn_index, counts=counts, pairs=pairs)


def silhouette_samples_np(d, groups, G):
    """(N,N) distances -> (N) silhouette coefficients, point by point as the definition reads: a = the mean distance to
    the other points of the own group, b = the smallest mean distance to the points of another non-empty group,
    (b - a) / max(a, b); 0 for a point alone in its group and for 0 / 0"""
    groups = np.asarray(groups, np.int64)
    N = groups.shape[0]
    present = [g for g in range(G) if (groups == g).any()]
    if len(present) < 2:
        raise ValueError("fewer than 2 non-empty groups")
    out = np.zeros(N)
    for i in range(N):
        own = groups == groups[i]
        own[i] = False
        if not own.any():
            continue
        a = d[i, own].mean()
        b = min(d[i, groups == g].mean() for g in present if g != groups[i])
        out[i] = 0.0 if max(a, b) == 0 else (b - a) / max(a, b)
    return out


def nn_accuracy_np(nn_index, groups):
    groups = np.asarray(groups, np.int64)
    hits = [groups[j] == groups[i] for i, j in enumerate(nn_index) if j >= 0]
    return float(np.mean(hits)) if hits else float("nan")


def mean_sq_distance_np(x):
    d2 = d2_matrix(x)
    n = d2.shape[0]
    return float((d2.sum() - np.trace(d2)) / (n * (n - 1)))


def mmd_scales_np(mean_d2, multipliers=(0.25, 0.5, 1, 2, 4)):
    return (1.0 / (2.0 * np.asarray(multipliers, np.float64) * mean_d2)).astype(np.float32)


def mk_mmd2_np(x, groups, scales, a=0, b=1, unbiased=False):
    """per scale, from the full kernel matrix: biased = the mean of k over ALL pairs of a (the diagonal included) + the
    same for b - 2 * the mean over the pairs (a, b); unbiased: the means within a and within b leave the diagonal out"""
    groups = np.asarray(groups, np.int64)
    d2 = d2_matrix(x)
    ia, ib = np.flatnonzero(groups == a), np.flatnonzero(groups == b)
    per = []
    for c in np.asarray(scales, np.float32).astype(np.float64).reshape(-1):
        k = np.exp(-(d2 * c))
        kaa, kbb, kab = k[np.ix_(ia, ia)], k[np.ix_(ib, ib)], k[np.ix_(ia, ib)]
        if unbiased:
            na, nb = len(ia), len(ib)
            per.append((kaa.sum() - np.trace(kaa)) / (na * (na - 1)) + (kbb.sum() - np.trace(kbb)) / (nb * (nb - 1))
                       - 2.0 * kab.mean())
        else:
            per.append(kaa.mean() + kbb.mean() - 2.0 * kab.mean())
    per = np.asarray(per)
    return per, float(per.sum())


def domain_gap_np(synth, real, multipliers=(0.25, 0.5, 1, 2, 4)):
    """the float64 counterpart of ``bsed_amd.domain_gap.domain_gap``"""
    x = np.concatenate([np.asarray(synth, np.float32), np.asarray(real, np.float32)])
    groups = np.concatenate([np.zeros(len(synth), np.int64), np.ones(len(real), np.int64)])
    mean_d2 = mean_sq_distance_np(x)
    scales = mmd_scales_np(mean_d2, multipliers)
    st = pair_stats_np(x, groups, 2, scales)
    samples = silhouette_samples_np(np.sqrt(st["d2"]), groups, 2)
    acc = nn_accuracy_np(st["nn_index"], groups)
    per, total = mk_mmd2_np(x, groups, scales)
    return dict(silhouette=float(samples.mean()), silhouette_samples=samples, nn_accuracy=acc,
                proxy_a_distance=2.0 * (2.0 * acc - 1.0), mmd2=per, mk_mmd2=total, mean_sq_distance=mean_d2,
                counts=st["counts"])


def lattice_points(rng, N, D):
    """(N, D) float32 with entries in {-3..3}: every d2 is an integer below 2^24, exact in float32 in any order"""
    return rng.integers(-3, 4, size=(N, D)).astype(np.float32)


def float32_roots(d2):
    """the correctly rounded float32 square root of exactly representable d2, as float64"""
    return np.sqrt(d2.astype(np.float32)).astype(np.float64)
