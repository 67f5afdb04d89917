"""bsed_amd.domain_gap without a GPU: the host arithmetic on the sums of the float64 restatement
(tests/domain_gap_reference.py), the argument checks of bsed_pair_stats (all before the first HIP call), the workspace
query, the order in which the feature dumps are read, and the errors raised when there is no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import domain_gap_reference as R
from bsed_amd import _lib as L
from bsed_amd import domain_gap as DG


def _cloud(seed=3, n=(9, 7, 1), D=5):
    """three groups (the last a singleton) under group ids 0, 1, 3 (2 is empty), one duplicated row, one masked point"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((sum(n), D)).astype(np.float32)
    g = np.concatenate([np.full(n[0], 0), np.full(n[1], 1), np.full(n[2], 3)]).astype(np.int64)
    x[4] = x[2]
    return x, g


def test_host_functions_on_the_restatements_sums_give_the_restatements_results():
    x, g = _cloud()
    G = 4
    m = R.mean_sq_distance_np(x)
    assert abs(DG.mean_sq_distance(x) - m) <= 1e-12 * m
    assert abs(DG.mean_sq_distance(torch.from_numpy(x)) - m) <= 1e-12 * m
    scales = DG.mmd_scales(m)
    assert scales.dtype == np.float32 and np.array_equal(scales, R.mmd_scales_np(m))
    st = R.pair_stats_np(x, g, G, scales)
    want = R.silhouette_samples_np(np.sqrt(st["d2"]), g, G)
    got = DG.silhouette_samples(st["dist_sum"], g, st["counts"])
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12
    assert got[-1] == 0.0                                              # the singleton
    assert abs(DG.silhouette_score(st["dist_sum"], g, st["counts"]) - want.mean()) <= 1e-12
    # tensors are taken as well as arrays
    assert np.array_equal(DG.silhouette_samples(torch.from_numpy(st["dist_sum"]), torch.from_numpy(g),
                                                torch.from_numpy(st["counts"])), got)
    assert DG.nn_accuracy(st["nn_index"], g) == R.nn_accuracy_np(st["nn_index"], g)
    for unbiased in (False, True):
        per, total = DG.mk_mmd2(st["kern_sum"], g, st["counts"], unbiased=unbiased)
        wper, wtotal = R.mk_mmd2_np(x, g, scales, unbiased=unbiased)
        assert per.shape == (5,) and np.abs(per - wper).max() <= 1e-12 and abs(total - wtotal) <= 1e-12
    per, _ = DG.mk_mmd2(st["kern_sum"], g, st["counts"], a=1, b=0)
    assert np.abs(per - R.mk_mmd2_np(x, g, scales)[0]).max() <= 1e-12  # symmetric in the two groups
    assert DG.proxy_a_distance(1.0) == 2.0 and DG.proxy_a_distance(0.5) == 0.0 and DG.proxy_a_distance(0.75) == 1.0


def test_silhouette_rules_masked_points_all_equal_points_and_too_few_groups():
    x, g = _cloud()
    g = g.copy()
    g[0] = -1                                                          # masked: scores NaN, is nobody's neighbour
    st = R.pair_stats_np(x, g, 4)
    got = DG.silhouette_samples(st["dist_sum"], g, st["counts"])
    keep = g >= 0
    want = R.silhouette_samples_np(np.sqrt(st["d2"])[np.ix_(keep, keep)], g[keep], 4)
    assert np.isnan(got[0]) and np.abs(got[keep] - want).max() <= 1e-12
    assert abs(DG.silhouette_score(st["dist_sum"], g, st["counts"]) - want.mean()) <= 1e-12
    st = R.pair_stats_np(np.ones((6, 3), np.float32), [0, 0, 0, 1, 1, 1], 2)
    assert (DG.silhouette_samples(st["dist_sum"], [0, 0, 0, 1, 1, 1], st["counts"]) == 0).all()      # 0 / 0 scores 0
    with pytest.raises(L.BsedError):
        DG.silhouette_samples(np.zeros((3, 2)), [0, 0, 0], [3, 0])
    with pytest.raises(L.BsedError):
        DG.silhouette_samples(np.zeros((3, 3)), [0, 0, 1], [2, 1])                                   # shapes disagree
    with pytest.raises(L.BsedError):
        DG.mk_mmd2(np.zeros((3, 2, 1)), [0, 0, 1], [2, 1], unbiased=True)                            # n_b - 1 = 0
    with pytest.raises(L.BsedError):
        DG.mmd_scales(0.0)
    assert np.isnan(DG.nn_accuracy([-1], [0]))


# ---- the C entry point: every check runs before the first HIP call ----
_OK = dict(x=0x1000, x_pitch=8, N=4, D=8, group=0x1000, G=2, scale=0x1000, S=2, splits=0, dist_sum=0x1000,
           kern_sum=0x1000, nn_d2=0x1000, nn_index=0x1000, workspace=0x1000, workspace_bytes=1 << 20, stream=None)
_DEFECTS = {
    "null x": dict(x=None), "null group": dict(group=None), "null dist_sum": dict(dist_sum=None),
    "null nn_d2": dict(nn_d2=None), "null nn_index": dict(nn_index=None), "null workspace": dict(workspace=None),
    "null scale with S > 0": dict(scale=None), "null kern_sum with S > 0": dict(kern_sum=None),
    "N = 0": dict(N=0), "D = 0": dict(D=0), "G = 0": dict(G=0), "G = 9": dict(G=9), "S = -1": dict(S=-1),
    "S = 9": dict(S=9), "x_pitch < D": dict(x_pitch=7), "splits < 0": dict(splits=-1),
    "workspace one byte short": dict(splits=3, workspace_bytes=3 * 4 * (8 * 2 * 3 + 8) - 1),
    "workspace short for the automatic split": dict(workspace_bytes=8),
}


@pytest.mark.parametrize("defect", list(_DEFECTS))
def test_every_argument_defect_is_refused_before_any_hip_call(defect):
    lib = L.lib()
    assert lib.bsed_abi_version() >= 17
    args = dict(_OK, **_DEFECTS[defect])
    rc = lib.bsed_pair_stats(*args.values())
    msg = lib.bsed_last_error().decode()
    assert rc == -1, (defect, rc, msg)                                 # BSED_ERR_ARG
    assert msg.startswith("bsed_pair_stats:"), (defect, msg)


def test_null_scale_and_kern_sum_pass_the_checks_only_with_no_scale():
    """with S = 0 the two may be NULL: the call is then refused by a LATER check (the workspace), not by the null check"""
    lib = L.lib()
    args = dict(_OK, S=0, scale=None, kern_sum=None, workspace_bytes=8)
    assert lib.bsed_pair_stats(*args.values()) == -1
    assert b"workspace" in lib.bsed_last_error()


def test_workspace_query_grows_with_each_argument_and_refuses_bad_ones():
    lib = L.lib()
    ws = lib.bsed_pair_stats_workspace
    base = ws(100, 2, 5, 3)
    assert base == 3 * 100 * (8 * 2 * 6 + 8)                           # float64 sums + float32 d2 + int32 index per split
    assert ws(101, 2, 5, 3) > base and ws(100, 3, 5, 3) > base and ws(100, 2, 6, 3) > base and ws(100, 2, 5, 4) > base
    assert ws(100, 2, 0, 1) == 100 * (8 * 2 + 8)
    for bad in ((0, 2, 5, 3), (100, 0, 5, 3), (100, 9, 5, 3), (100, 2, -1, 3), (100, 2, 9, 3), (100, 2, 5, -1)):
        assert ws(*bad) == 0, bad
    # splits = 0 sizes it for the automatic choice
    for N, D in ((1, 4), (64, 2), (257, 515), (4096, 256), (100000, 8)):
        auto = lib.bsed_pair_stats_splits(N, D)
        assert 1 <= auto <= (N + 63) // 64
        assert ws(N, 2, 5, 0) == ws(N, 2, 5, auto)
    assert lib.bsed_pair_stats_splits(0, 0) >= 1
    assert L.FUNCTIONS["bsed_pair_stats_workspace"][0] is ctypes.c_size_t
    assert L.CONSTANTS["BSED_PAIR_MAX_GROUPS"] == 8 and L.CONSTANTS["BSED_PAIR_MAX_SCALES"] == 8


def test_feature_dumps_are_read_in_numeric_order(tmp_path):
    for i, n in ((0, 2), (2, 1), (10, 3)):                             # batches of n clips, (T', F) = (3, 4)
        np.save(tmp_path / f"{i}", np.full((n, 3, 4), float(i), np.float32))
    np.save(tmp_path / "labels", np.zeros(3))                          # not a batch
    clips = DG.load_embedded_features(str(tmp_path))
    assert clips.shape == (6, 12) and clips.dtype == np.float32
    assert clips[:, 0].tolist() == [0, 0, 2, 10, 10, 10]               # 0, 2, 10 -- not the string order 0, 10, 2
    frames = DG.load_embedded_features(str(tmp_path), level="frame")
    assert frames.shape == (18, 4) and frames[:, 0].tolist() == [0] * 6 + [2] * 3 + [10] * 9
    with pytest.raises(L.BsedError):
        DG.load_embedded_features(str(tmp_path), level="class")
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(L.BsedError):
        DG.load_embedded_features(str(empty))


def test_no_cpu_fallback():
    """a CPU tensor is refused everywhere; without a GPU, so is an array"""
    x = torch.zeros((4, 3))
    with pytest.raises(L.BsedError):
        DG.pair_stats_gpu(x, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(L.BsedError):
        DG.pair_stats_gpu(x.numpy(), np.zeros(4, np.int32))
    if not torch.cuda.is_available():
        with pytest.raises(L.BsedError):
            DG.domain_gap(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32))
