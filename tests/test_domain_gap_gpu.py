"""The all-pairs kernel of the domain gap (csrc/pair_stats.hip, bsed_pair_stats) and bsed_amd.domain_gap on the GPU
against the float64 restatement of tests/domain_gap_reference.py, which reads the SAME float32 inputs.

Derived bounds, with u = 2^-24 (the unit round-off of float32) and d2_64 / ref the restatement's float64 values:

1. Squared distance.  Each difference is rounded once (relative error <= u), its square once more, and a float32 sum of
   D non-negative terms in any order adds at most (D - 1) u: together <= (D + 3) u relative, to first order, FMA or not.
   So  |nn_d2[i] - d2_64(i, nn_index[i])| <= (D + 3) u d2_64,  and the neighbour the kernel picks by ITS d2 is within
   twice that of the true minimum:  d2_64(i, nn_index[i]) <= (1 + 2 (D + 3) u) min_j d2_64(i, j).
2. Distance sums.  The square root halves the relative error and adds one rounding; every term is non-negative, so the
   bound of a term is the bound of the sum:  |dist_sum - ref| <= ((D + 3) / 2 + 2) u ref.  The float64 additions add
   less than 1e-12 relative and are covered by the slack of the "+ 2".
3. Kernel sums.  The argument d2 * scale has relative error <= (D + 4) u (one more rounding for the product);
   |d exp(-a)| = exp(-a) a |da / a| and a exp(-a) <= 1 / e, so a term moves by at most (D + 4) u / e; expf itself is
   documented by HIP with a maximum error of 1 ulp = 2 u of a value <= 1, the bound allots 4 u to it and the conversion.
   With n pairs summed:  |kern_sum - ref| <= n ((D + 4) u / e + 4 u).

On integer lattices (entries in -3..3) every d2 is an integer below 2^24, exact in float32 in any order: there nn_d2 and
nn_index are compared with == and dist_sum is within 1e-12 relative of the float64 sum of the float32-rounded roots."""
import ctypes
import math

import numpy as np
import pytest
import torch

import domain_gap_reference as R

pytestmark = pytest.mark.gpu

U = R.U
CANARY = -7777.25
PAD = 64
MULTIPLIERS = {0: (), 1: (1.0,), 5: (0.25, 0.5, 1.0, 2.0, 4.0), 8: (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)}


def _guarded(n, dtype):
    """n elements inside a canary-filled buffer -> (buffer, the view of the n elements)"""
    buf = torch.full((n + 2 * PAD,), CANARY, device="cuda", dtype=torch.float64).to(dtype)
    return buf, buf[PAD:PAD + n]


def _intact(buf, n):
    want = torch.tensor(CANARY, dtype=torch.float64).to(buf.dtype).item()
    return bool((buf[:PAD] == want).all()) and bool((buf[PAD + n:] == want).all())


def _place(x, misaligned):
    """the (N, D) float32 array on the GPU.  ``misaligned``: rows D + 3 elements apart in a NaN-filled buffer, the base
    one float past the allocation's start -- the 4-byte path, and whatever is read outside a row poisons the result"""
    N, D = x.shape
    if not misaligned:
        return torch.from_numpy(x).cuda()
    pitch = D + 3
    buf = torch.full((1 + N * pitch,), float("nan"), device="cuda", dtype=torch.float32)
    view = buf[1:].view(N, pitch)[:, :D]
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.stride() == (pitch, 1)
    return view


def launch(x, groups, G, scales, splits=0, misaligned=False, stream=None):
    """bsed_pair_stats itself, every output and the workspace inside canary-filled buffers that must be intact
    afterwards -> dict of numpy results"""
    from bsed_amd import _lib as L
    lib = L.lib()
    N, D = x.shape
    S = len(scales)
    xg = _place(x, misaligned)
    gg = torch.from_numpy(np.asarray(groups, np.int32)).cuda()
    sg = torch.from_numpy(np.asarray(scales, np.float32)).cuda() if S else None
    nbytes = lib.bsed_pair_stats_workspace(N, G, S, splits)
    assert nbytes > 0 and nbytes % 8 == 0
    bufs = {"dist_sum": _guarded(N * G, torch.float64), "kern_sum": _guarded(N * G * S, torch.float64),
            "nn_d2": _guarded(N, torch.float32), "nn_index": _guarded(N, torch.int32),
            "ws": _guarded(nbytes // 8, torch.float64)}
    p = {k: ctypes.c_void_p(v[1].data_ptr()) for k, v in bufs.items()}

    def go():
        rc = lib.bsed_pair_stats(ctypes.c_void_p(xg.data_ptr()), xg.stride(0), N, D, L.ptr(gg, torch.int32), G,
                                 L.ptr(sg) if S else None, S, splits, p["dist_sum"], p["kern_sum"] if S else None,
                                 p["nn_d2"], p["nn_index"], p["ws"], nbytes, L.stream())
        assert rc == 0, lib.bsed_last_error().decode()
    if stream is None:
        go()
    else:
        with torch.cuda.stream(stream):
            go()
        stream.synchronize()
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view.numel()), f"{k}: written outside its {view.numel()} elements"
    return dict(dist_sum=bufs["dist_sum"][1].cpu().numpy().reshape(N, G).copy(),
                kern_sum=bufs["kern_sum"][1].cpu().numpy().reshape(N, G, S).copy(),
                nn_d2=bufs["nn_d2"][1].cpu().numpy().copy(), nn_index=bufs["nn_index"][1].cpu().numpy().copy())


def make_case(N, D, G, seed, close=False):
    """float32 points, labels, the edges N allows: G = 2: alternating labels; G = 3: group 1 a singleton, group 2 empty;
    from N >= 4 on one masked point (label G) and one duplicated row in the other tile / the same group"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D)).astype(np.float32)
    if close:                                           # an embedding's points: close together, far from the origin
        x = (5.0 + 0.05 * x).astype(np.float32)
    g = (np.arange(N) % 2) if G == 2 else np.zeros(N, np.int64)
    g = g.astype(np.int64)
    if G == 3 and N > 1:
        g[N // 2] = 1
    if N >= 4:
        g[1] = G                                        # masked
        x[N - 1] = x[0]                                 # duplicated: d2 = 0 exactly
    return x, g


def check_bounds(got, x, g, G, scales):
    N, D = x.shape
    ref = R.pair_stats_np(x, g, G, scales)
    valid = R.valid_mask(g, G)
    # 1. the nearest neighbour
    for i in range(N):
        cand = valid.copy()
        cand[i] = False
        j = int(got["nn_index"][i])
        if not cand.any():
            assert j == -1 and got["nn_d2"][i] == np.inf
            continue
        assert 0 <= j < N and cand[j], (i, j)
        d64 = ref["d2"][i, j]
        assert abs(float(got["nn_d2"][i]) - d64) <= (D + 3) * U * d64, (i, j, got["nn_d2"][i], d64)
        assert d64 <= (1 + 2 * (D + 3) * U) * ref["d2"][i, cand].min(), (i, j)
    # 2. the distance sums
    err = np.abs(got["dist_sum"] - ref["dist_sum"])
    bound = ((D + 3) / 2 + 2) * U * ref["dist_sum"]
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert (got["dist_sum"][ref["pairs"] == 0] == 0).all()
    # 3. the kernel sums
    if len(scales):
        err = np.abs(got["kern_sum"] - ref["kern_sum"])
        bound = ref["pairs"][:, :, None] * ((D + 4) * U / math.e + 4 * U)
        assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    return ref


# (N, D, G, S, splits, misaligned, own stream, close together): the smallest shapes that reach every edge -- one point,
# D = 1, a partial second tile, exactly one tile, D no multiple of 4 or 32, a chunked D, five tiles with a one-row tail,
# a long D; 3 and 7 splits do not divide the tile count
CASES = [(1, 4, 2, 1, 0, False, False, False),
         (2, 1, 2, 0, 7, False, False, False),
         (70, 1, 3, 5, 3, True, False, False),
         (64, 2, 2, 8, 1, False, False, False),
         (130, 67, 3, 5, 7, True, False, False),
         (97, 256, 2, 5, 0, False, True, True),
         (257, 515, 2, 1, 3, False, False, False),
         (40, 5000, 2, 5, 0, True, False, True)]


@pytest.mark.parametrize("N,D,G,S,splits,misaligned,own_stream,close", CASES,
                         ids=[f"N{c[0]}-D{c[1]}-G{c[2]}-S{c[3]}-splits{c[4]}" for c in CASES])
def test_sums_and_neighbours_within_the_derived_bounds(N, D, G, S, splits, misaligned, own_stream, close):
    from bsed_amd import domain_gap as DG
    x, g = make_case(N, D, G, 100 + N, close)
    mean_d2 = R.mean_sq_distance_np(x) if N > 1 else 1.0
    scales = R.mmd_scales_np(mean_d2, MULTIPLIERS[S]) if S else np.zeros(0, np.float32)
    stream = torch.cuda.Stream() if own_stream else None
    got = launch(x, g, G, scales, splits, misaligned, stream)
    ref = check_bounds(got, x, g, G, scales)
    # repeatability: the same bits from three launches
    for _ in range(2):
        again = launch(x, g, G, scales, splits, misaligned, stream)
        assert all(np.array_equal(got[k], again[k]) for k in got)
    # the Python entry gives the kernel's bits, on a non-contiguous row pitch too, and counts the unmasked points
    st = DG.pair_stats_gpu(_place(x, misaligned), torch.from_numpy(g), G, scales, splits)
    assert st.dist_sum.dtype == torch.float64 and st.kern_sum.shape == (N, G, S) and st.nn_index.dtype == torch.int32
    assert np.array_equal(st.dist_sum.cpu().numpy(), got["dist_sum"])
    assert np.array_equal(st.kern_sum.cpu().numpy(), got["kern_sum"])
    assert np.array_equal(st.nn_d2.cpu().numpy(), got["nn_d2"]) and np.array_equal(st.nn_index.cpu().numpy(), got["nn_index"])
    assert st.counts.cpu().tolist() == ref["counts"].tolist()
    # the measures made from the kernel's sums are the restatement's, to what the bounds above leave
    if (ref["counts"] > 0).sum() >= 2:
        want = R.silhouette_samples_np(np.sqrt(ref["d2"])[np.ix_(g < G, g < G)], g[g < G], G)
        sil = DG.silhouette_samples(st.dist_sum, g, st.counts)
        assert np.abs(sil[g < G] - want).max() <= 4 * ((D + 3) / 2 + 2) * U


@pytest.mark.parametrize("splits,S", [(0, 5), (1, 8), (3, 0), (7, 1)])
def test_every_split_count_and_scale_count_on_one_shape(splits, S):
    """(130, 67): three tiles, the last of two rows; D = 67 leaves a tail of 3 in the third chunk.  Results for
    different splits are within 1e-12 relative of each other (float64 sums in another order; d2 itself has the same
    bits), and the neighbour is the same"""
    x, g = make_case(130, 67, 2, 5)
    all_scales = R.mmd_scales_np(R.mean_sq_distance_np(x), MULTIPLIERS[8])
    got = launch(x, g, 2, all_scales[:S], splits)
    check_bounds(got, x, g, 2, all_scales[:S])
    one = launch(x, g, 2, all_scales[:S], 1, misaligned=True)          # the other load path, one split
    assert np.array_equal(got["nn_d2"], one["nn_d2"]) and np.array_equal(got["nn_index"], one["nn_index"])
    assert np.allclose(got["dist_sum"], one["dist_sum"], rtol=1e-12, atol=0)
    assert np.allclose(got["kern_sum"], one["kern_sum"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("splits", [1, 3, 0])
def test_integer_lattice_is_exact_and_ties_go_to_the_smallest_index(splits):
    """200 points with entries in -3..3 in D = 6: four column tiles (the last of 8), with 3 splits the ranges are tile 0,
    tile 1, tiles 2-3.  Points 3, 67 and 130 coincide: every row that is nearest to them must name 3 -- a tie across a
    tile boundary with one split, across both split boundaries with three -- and the three name each other by the same
    rule.  The lattice is dense enough that dozens of other rows have a tie for the nearest neighbour too."""
    N, D = 200, 6
    rng = np.random.default_rng(17)
    x = R.lattice_points(rng, N, D)
    x[67] = x[3]
    x[130] = x[3]
    g = (rng.integers(0, 2, N)).astype(np.int64)
    g[5] = 2                                            # masked
    scales = np.asarray([0.125, 0.03125], np.float32)
    ref = R.pair_stats_np(x, g, 2, scales, roots=R.float32_roots)
    off_diagonal = ref["d2"] + np.diag(np.full(N, np.inf))
    ties = int(((off_diagonal[:, R.valid_mask(g, 2)] == ref["nn_d2"][:, None]).sum(axis=1) > 1).sum())
    assert ties > 20 and ref["nn_index"][3] == 67 and ref["nn_index"][67] == 3 and ref["nn_index"][130] == 3
    got = launch(x, g, 2, scales, splits)
    assert np.array_equal(got["nn_d2"].astype(np.float64), ref["nn_d2"])
    assert np.array_equal(got["nn_index"], ref["nn_index"])
    assert np.allclose(got["dist_sum"], ref["dist_sum"], rtol=1e-12, atol=0)
    bound = ref["pairs"][:, :, None] * (1 * U / math.e + 4 * U)        # d2 is exact: only the product's rounding is left
    assert (np.abs(got["kern_sum"] - ref["kern_sum"]) <= bound).all()
    # a long exact row: D = 5000, d2 up to 180000, still below 2^24
    x = R.lattice_points(rng, 40, 5000)
    g = (np.arange(40) % 2).astype(np.int64)
    ref = R.pair_stats_np(x, g, 2, roots=R.float32_roots)
    got = launch(x, g, 2, np.zeros(0, np.float32), splits, misaligned=True)
    assert np.array_equal(got["nn_d2"].astype(np.float64), ref["nn_d2"]) and np.array_equal(got["nn_index"], ref["nn_index"])
    assert np.allclose(got["dist_sum"], ref["dist_sum"], rtol=1e-12, atol=0)


def test_a_masked_point_contributes_nothing_and_wild_labels_are_never_used_as_an_index():
    """the masked points' features are NaN: had any of them been summed into a row or taken for a neighbour, that row
    would show it.  Their labels are far outside [0, G) on both sides."""
    N, D, G = 150, 9, 2
    rng = np.random.default_rng(23)
    x = rng.standard_normal((N, D)).astype(np.float32)
    g = (np.arange(N) % 2).astype(np.int64)
    masked = [0, 63, 64, 149]
    for i, label in zip(masked, (-1, 2 ** 31 - 1, -2 ** 31, G)):
        g[i] = label
        x[i] = np.nan
    scales = R.mmd_scales_np(2.0 * D, (0.5, 2.0))
    got = launch(x, g.astype(np.int32), G, scales, 3)
    keep = np.setdiff1d(np.arange(N), masked)
    assert np.isfinite(got["dist_sum"][keep]).all() and np.isfinite(got["kern_sum"][keep]).all()
    assert np.isfinite(got["nn_d2"][keep]).all() and not np.isin(got["nn_index"][keep], masked).any()
    # the rest equals the run without the masked points (their rows taken out; indices shifted accordingly)
    sub = launch(x[keep], g[keep].astype(np.int32), G, scales, 3)
    assert np.allclose(got["dist_sum"][keep], sub["dist_sum"], rtol=1e-12, atol=0)
    assert np.allclose(got["kern_sum"][keep], sub["kern_sum"], rtol=1e-12, atol=0)
    assert np.array_equal(got["nn_d2"][keep], sub["nn_d2"]) and np.array_equal(got["nn_index"][keep], keep[sub["nn_index"]])
    check_bounds(sub, x[keep], g[keep], G, scales)


def test_wrong_dtype_device_and_sizes_raise():
    from bsed_amd import domain_gap as DG
    from bsed_amd._lib import BsedError
    x = torch.zeros((4, 3), device="cuda")
    g = torch.zeros(4, dtype=torch.int32, device="cuda")
    for bad_x, bad_g, kw in ((x.double(), g, {}), (x.cpu(), g, {}), (x, g.float(), {}), (x, g[:3], {}), (x[0], g, {}),
                             (x, g, dict(n_groups=9)), (x, g, dict(scales=[1.0] * 9)), (x, g, dict(splits=-1))):
        with pytest.raises(BsedError):
            DG.pair_stats_gpu(bad_x, bad_g, **kw)
    st = DG.pair_stats_gpu(x, g.long())                                # int64 labels are converted; n_groups from them
    assert st.dist_sum.shape == (4, 1) and st.kern_sum.shape == (4, 1, 0) and st.nn_index.tolist() == [1, 0, 0, 0]
    assert st.counts.tolist() == [4] and (st.dist_sum == 0).all()


def test_separated_clouds_and_one_cloud_split_at_random():
    """thresholds on constructed inputs; the seed is chosen so that the float64 restatement alone meets them, which is
    asserted first"""
    from bsed_amd import domain_gap as DG
    rng = np.random.default_rng(7)
    a = rng.standard_normal((70, 16)).astype(np.float32)
    b = (rng.standard_normal((58, 16)) + 4).astype(np.float32)
    c = rng.standard_normal((128, 16)).astype(np.float32)
    p = rng.permutation(128)
    want_sep, want_one = R.domain_gap_np(a, b), R.domain_gap_np(c[p[:70]], c[p[70:]])
    assert want_sep["silhouette"] > 0.5 and want_sep["nn_accuracy"] == 1.0
    assert abs(want_one["silhouette"]) < 0.1 and want_one["mk_mmd2"] < want_sep["mk_mmd2"]
    sep, one = DG.domain_gap(a, torch.from_numpy(b).cuda()), DG.domain_gap(c[p[:70]], c[p[70:]], splits=2)
    assert sep.silhouette > 0.5 and sep.nn_accuracy == 1.0 and sep.proxy_a_distance == 2.0
    assert abs(one.silhouette) < 0.1 and one.mk_mmd2 < sep.mk_mmd2
    D = 16
    for got, want in ((sep, want_sep), (one, want_one)):
        assert got.counts.tolist() == [70, 58] and got.silhouette_samples.shape == (128,)
        assert abs(got.mean_sq_distance - want["mean_sq_distance"]) <= 1e-12 * want["mean_sq_distance"]
        assert np.abs(got.silhouette_samples - want["silhouette_samples"]).max() <= 4 * ((D + 3) / 2 + 2) * U
        assert abs(got.silhouette - want["silhouette"]) <= 4 * ((D + 3) / 2 + 2) * U
        assert got.nn_accuracy == want["nn_accuracy"] and got.proxy_a_distance == want["proxy_a_distance"]
        # per multiplier: three means of kernel values, each within the per-term bound of the kernel sums
        assert np.abs(got.mmd2 - want["mmd2"]).max() <= 4 * ((D + 4) * U / math.e + 4 * U)
        assert abs(got.mk_mmd2 - want["mk_mmd2"]) <= 5 * 4 * ((D + 4) * U / math.e + 4 * U)


def test_domain_gap_of_a_model_equals_domain_gap_of_its_features():
    """a tiny CRNN + Predictor on two loaders of two small batches: ``domain_gap_of`` = ``embed`` + ``domain_gap``, and
    ``embed`` hands out what ``_forward(features=True)`` returns, per clip flattened or per frame"""
    from oracle import seeded
    from test_event_metrics_gpu import _seeded_models
    from bsed_amd import domain_gap as DG
    from bsed_amd.evaluation._common import _eval_mode, _forward
    crnn, pred = _seeded_models(51)
    T = 256

    def loader(seed, gain):
        x = seeded.db_like_input(seed, 4, T) * gain
        return [(((torch.from_numpy(x[i:i + 2]), torch.from_numpy(x[i:i + 2])), None), [f"clip{j}" for j in (i, i + 1)])
                for i in (0, 2)]
    synth, real = loader(52, 1.0), loader(53, 0.5)
    feats = []
    with _eval_mode(crnn, pred):
        for ld in (synth, real):
            feats.append(torch.cat([_forward(crnn, pred, False, torch.as_tensor(b[0][0][0]).float().cuda(), features=True)[2]
                                    for b in ld]))
    assert feats[0].dim() == 3 and feats[0].shape[0] == 4
    Tp, F = feats[0].shape[1:]
    for level, shape in (("clip", (4, Tp * F)), ("frame", (4 * Tp, F))):
        e = DG.embed(crnn, synth, pred, level=level)
        assert e.is_cuda and e.dtype == torch.float32 and tuple(e.shape) == shape
        assert torch.equal(e, feats[0].reshape(shape))
        got = DG.domain_gap_of(crnn, synth, real, pred, level=level)
        want = DG.domain_gap(feats[0].reshape(shape), feats[1].reshape(shape))
        assert got.silhouette == want.silhouette and np.array_equal(got.silhouette_samples, want.silhouette_samples)
        assert got.nn_accuracy == want.nn_accuracy and np.array_equal(got.mmd2, want.mmd2)
        assert got.mean_sq_distance == want.mean_sq_distance and got.counts.tolist() == [shape[0]] * 2
    # a seeded sample of the frames, without replacement and in order
    some = DG.embed(crnn, synth, pred, level="frame", max_points=10, seed=3)
    keep = torch.randperm(4 * Tp, generator=torch.Generator().manual_seed(3))[:10].sort().values
    assert torch.equal(some, feats[0].reshape(4 * Tp, F)[keep.cuda()])
    assert torch.equal(some, DG.embed(crnn, synth, pred, level="frame", max_points=10, seed=3))
    assert crnn.training and pred.training


def _svc_d2(xg):
    """bsed_svc_d2 of a placed point matrix into a canary-guarded buffer -> (N, N) float32 numpy"""
    from bsed_amd import _lib as L
    N, D = xg.shape
    buf, out = _guarded(N * N, torch.float32)
    rc = L.lib().bsed_svc_d2(ctypes.c_void_p(xg.data_ptr()), xg.stride(0), N, D, ctypes.c_void_p(out.data_ptr()), L.stream())
    assert rc == 0, L.lib().bsed_last_error().decode()
    torch.cuda.synchronize()
    assert _intact(buf, N * N), "d2: written outside its N * N elements"
    return out.cpu().numpy().reshape(N, N).copy()


SHARED_CORE_D = (1, 3, 32, 33, 37, 100)


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("N", [63, 64, 65, 130])
def test_the_shared_tile_core_gives_pair_stats_and_svc_d2_the_same_bits(N, misaligned):
    """pair_stats_kernel and d2_tile_kernel run one device function (csrc/d2_tile.h: d2_tile_acc), so the nearest
    neighbour that bsed_pair_stats reports is, bit for bit, the smallest off-diagonal entry of the row of bsed_svc_d2,
    at the smallest column that holds it.  Seeded normal points with one duplicated row (an exact 0 and a tie), every
    label 0 (G = 1, S = 0); N around one tile and three tiles with a tail of two rows; D = 1, below a load of four, a
    whole chunk, one and five past it (a second chunk that is almost all zero fill), four chunks with a tail of four;
    both load paths; the automatic split, one split and three (more splits than column tiles at N <= 128)."""
    for D in SHARED_CORE_D:
        rng = np.random.default_rng(1000 * N + D)
        x = rng.standard_normal((N, D)).astype(np.float32)
        x[N - 1] = x[0]
        d2 = _svc_d2(_place(x, misaligned))
        assert np.array_equal(d2, d2.T) and (np.diag(d2) == 0).all() and d2[0, N - 1] == 0
        off = d2.copy()
        np.fill_diagonal(off, np.inf)
        want_j = off.argmin(axis=1)                                   # the first, so the smallest, column of the minimum
        want_d2 = off[np.arange(N), want_j]
        for splits in (0, 1, 3):
            got = launch(x, np.zeros(N, np.int32), 1, np.zeros(0, np.float32), splits, misaligned)
            assert np.array_equal(got["nn_d2"].view(np.uint32), want_d2.view(np.uint32)), (D, splits)
            assert np.array_equal(got["nn_index"], want_j), (D, splits)


def test_the_shared_tile_core_with_one_point():
    """N = 1: the only entry of d2 is the diagonal's exact 0, and the point has no neighbour: inf / -1"""
    for D in SHARED_CORE_D:
        x = np.random.default_rng(D).standard_normal((1, D)).astype(np.float32)
        for misaligned in (False, True):
            assert _svc_d2(_place(x, misaligned)).tolist() == [[0.0]]
            for splits in (0, 1, 3):
                got = launch(x, np.zeros(1, np.int32), 1, np.zeros(0, np.float32), splits, misaligned)
                assert got["nn_d2"].tolist() == [np.inf] and got["nn_index"].tolist() == [-1], (D, misaligned, splits)
