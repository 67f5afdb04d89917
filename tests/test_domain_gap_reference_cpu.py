"""The float64 restatement of tests/domain_gap_reference.py against sklearn and against hand-worked cases, so that the
GPU tests compare the kernel with something that has itself been checked."""
import numpy as np
import pytest

import domain_gap_reference as R


def _case(name):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((23, 7)).astype(np.float32)
    if name == "two groups":
        g = (np.arange(23) % 2).astype(np.int64)
    elif name == "singleton and empty group id":
        g = (np.arange(23) % 2).astype(np.int64)        # group 2 is empty, group 3 holds one point
        g[5] = 3
    else:                                               # a duplicated row in the same group and one in the other
        g = (np.arange(23) % 3).astype(np.int64)
        x[9] = x[3]
        x[10] = x[4]
    return x, g, int(g.max()) + 1


@pytest.mark.parametrize("name", ["two groups", "singleton and empty group id", "duplicated row"])
def test_silhouette_samples_equal_sklearn_on_the_precomputed_route(name):
    """sklearn's own Euclidean route forms the distances by the Gram form and differs by about 1e-9; with the distance
    matrix handed over (metric="precomputed") only the silhouette arithmetic is compared"""
    metrics = pytest.importorskip("sklearn.metrics")
    x, g, G = _case(name)
    d = np.sqrt(R.d2_matrix(x))
    assert (np.diag(d) == 0).all()
    want = metrics.silhouette_samples(d, g, metric="precomputed")
    got = R.silhouette_samples_np(d, g, G)
    assert np.abs(got - want).max() <= 1e-12
    if name == "singleton and empty group id":
        assert got[5] == 0.0 and want[5] == 0.0
    # the sums the kernel makes carry the same information: the product's rule applied to them gives the same values
    st = R.pair_stats_np(x, g, G)
    assert st["counts"].tolist() == np.bincount(g, minlength=G).tolist()
    assert np.allclose(st["dist_sum"].sum(axis=1), d.sum(axis=1), rtol=1e-13)


def test_all_points_equal_score_zero():
    x = np.ones((6, 3), np.float32)
    g = np.asarray([0, 0, 0, 1, 1, 1])
    assert (R.silhouette_samples_np(np.sqrt(R.d2_matrix(x)), g, 2) == 0).all()
    with pytest.raises(ValueError):
        R.silhouette_samples_np(np.zeros((3, 3)), np.zeros(3, np.int64), 2)


def test_hand_worked_mmd_of_two_points_per_group():
    """a = {0, 1}, b = {3, 4} on a line, scale c: d2 within a group is 1, across 9, 16, 4, 9.  With e(t) = exp(-c t):
    biased   = (2 + 2 e(1)) / 4 + (2 + 2 e(1)) / 4 - 2 (e(9) + e(16) + e(4) + e(9)) / 4
    unbiased = e(1) + e(1) - (2 e(9) + e(16) + e(4)) / 2"""
    x = np.asarray([[0.0], [1.0], [3.0], [4.0]], np.float32)
    g = np.asarray([0, 0, 1, 1])
    c = np.float32(0.125)                               # exact in float32

    def e(t):
        return np.exp(-0.125 * t)
    per, total = R.mk_mmd2_np(x, g, [c])
    want = 1.0 + e(1) - (2 * e(9) + e(16) + e(4)) / 2
    assert abs(per[0] - want) <= 1e-15 and total == per[0]
    per_u, _ = R.mk_mmd2_np(x, g, [c], unbiased=True)
    assert abs(per_u[0] - (2 * e(1) - (2 * e(9) + e(16) + e(4)) / 2)) <= 1e-15
    # two scales are summed; the kernel sums of the all-pairs pass hold the same numbers
    per2, total2 = R.mk_mmd2_np(x, g, [c, np.float32(0.5)])
    assert per2[0] == per[0] and total2 == per2.sum()
    st = R.pair_stats_np(x, g, 2, [c])
    assert abs(st["kern_sum"][0, 0, 0] - e(1)) <= 1e-16 and abs(st["kern_sum"][0, 1, 0] - (e(9) + e(16))) <= 1e-16
    assert st["pairs"].tolist() == [[1, 2], [1, 2], [2, 1], [2, 1]]


def test_nearest_neighbour_takes_the_smallest_index_on_a_tie_and_skips_masked_points():
    # point 2 lies exactly between 0 and 4 (and 1 and 3 coincide with 0 and 4 but are masked / come later)
    x = np.asarray([[0.0], [0.0], [1.0], [2.0], [2.0]], np.float32)
    g = np.asarray([0, -1, 1, 7, 0])                    # 1 and 3 are masked (labels outside [0, 2))
    st = R.pair_stats_np(x, g, 2)
    assert st["nn_index"].tolist() == [2, 0, 0, 4, 2] and st["nn_d2"].tolist() == [1.0, 0.0, 1.0, 0.0, 1.0]
    assert st["counts"].tolist() == [2, 1]
    assert st["dist_sum"][1].tolist() == [2.0, 1.0]     # a masked point's own row is still produced
    assert st["dist_sum"][2].tolist() == [2.0, 0.0]     # and nobody sums a masked point
    # a duplicate: distance 0 to the first copy wins over everything, ties among copies go to the smallest index
    x = np.asarray([[5.0], [1.0], [5.0], [5.0]], np.float32)
    st = R.pair_stats_np(x, np.zeros(4, np.int64), 1)
    assert st["nn_index"].tolist() == [2, 0, 0, 0] and st["nn_d2"].tolist() == [0.0, 16.0, 0.0, 0.0]
    # nobody to be near to
    st = R.pair_stats_np(np.zeros((1, 4), np.float32), np.zeros(1, np.int64), 2)
    assert st["nn_index"].tolist() == [-1] and np.isinf(st["nn_d2"][0]) and st["dist_sum"].tolist() == [[0.0, 0.0]]
    assert R.nn_accuracy_np([2, 0, 0, 0], [0, 1, 0, 1]) == 0.5


def test_mean_squared_distance_and_scales():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((9, 4)).astype(np.float32)
    m = R.mean_sq_distance_np(x)
    c = x.astype(np.float64) - x.astype(np.float64).mean(axis=0)
    assert abs(m - 2.0 * (c * c).sum() / 8) <= 1e-13 * m
    s = R.mmd_scales_np(m)
    assert s.dtype == np.float32 and np.allclose(s, 1.0 / (2 * np.asarray([0.25, 0.5, 1, 2, 4]) * m), rtol=1e-7)
