"""Clip-level tagging on the GPU: ``bsed_tag_counts`` / ``bsed_tag_masks`` against the numpy restatement of
tests/tagging_reference.py (integer counts from float compares: equal means exactly equal), accumulation, repeatability,
and the passes built on them -- ``validate_weak``, ``get_f_measure_by_class``, ``pseudo_label``,
``validate(tagging_thresholds=...)`` -- on a small model, both sides reading the ONE weak tensor the pass produced."""
import numpy as np
import pytest
import torch

import tagging_reference as R
from oracle import crnn_oracle as co
from oracle import seeded

pytestmark = pytest.mark.gpu


def thresholds_for(rng, S, C, per_class):
    """(S) or (S,C) float32-representable thresholds as nested lists"""
    if per_class:
        return rng.uniform(0.02, 0.98, (S, C)).astype(np.float32).astype(np.float64).tolist()
    return [float(v) for v in np.linspace(0.02, 0.98, S).astype(np.float32)] if S > 1 else [0.5]


def weak_scores(rng, B, T, C, thresholds):
    """(B,C) for T == 0, else (B,T,C) whose maximum over time is a given (B,C) array: uniform values, about 10 % of them
    EXACTLY equal to a threshold (of their class), a few NaN.  In the 3-D form every (clip, class) column holds its
    maximum once, at a random frame, and smaller values elsewhere."""
    thr = np.asarray(thresholds, np.float32)
    top = rng.random((B, C)).astype(np.float32)
    hit = rng.random((B, C)) < 0.1
    pick = rng.integers(0, len(thr), (B, C))
    top[hit] = (thr[pick, np.arange(C)[None, :].repeat(B, 0)] if thr.ndim == 2 else thr[pick])[hit]
    if T == 0:
        top[rng.random((B, C)) < 0.02] = np.nan
        top[B // 2, C // 2] = np.nan
        return top
    x = top[:, None, :] * rng.random((B, T, C)).astype(np.float32)
    at = rng.integers(0, T, (B, C))
    np.put_along_axis(x, at[:, None, :], top[:, None, :], 1)
    x[rng.random((B, T, C)) < 0.02 / T] = np.nan                     # the maximum of such a column is NaN
    x[B // 2, T // 2, C // 2] = np.nan
    return x


def weak_targets(rng, B, T, C):
    """(B,C) of 0 / 1 with some rows of -1 (encode_weak("empty")), or (B,T,C) frame labels: columns that are silent, hold
    a run of ones, or only reach 0.5 (which `> 0.5` leaves off), and some clips of -1"""
    if T == 0:
        y = (rng.random((B, C)) < 0.4).astype(np.float32)
        y[rng.random(B) < 0.15] = -1.0
        y[B - 1] = -1.0 if B > 2 else y[B - 1]
        return y
    y = np.zeros((B, T, C), np.float32)
    kind = rng.random((B, C))
    at = rng.integers(0, T, (B, C))
    np.put_along_axis(y, at[:, None, :], np.where(kind < 0.4, 1.0, np.where(kind < 0.6, 0.5, 0.0)).astype(np.float32)[:, None, :], 1)
    y[rng.random(B) < 0.15] = -1.0
    y[B - 1] = -1.0 if B > 2 else y[B - 1]
    return y


FORMS = [(0, 0), (0, 3), (1, 0), (1, 1), (2, 313), (2, 0), (313, 0), (313, 313)]      # (T of the scores, T of the targets)
SWEEPS = [(1, False), (7, False), (50, False), (1, True), (7, True), (50, True)]


@pytest.mark.parametrize("B", [1, 3, 65, 257])
@pytest.mark.parametrize("C", [1, 20, 33, 64])
def test_counts_equal_the_restatement(C, B):
    from bsed_amd.evaluation import tag_counts_gpu
    rng = np.random.default_rng(1000 * C + B)
    saw_equal = saw_nan = saw_empty = False
    for Ts, Tt in FORMS:
        sweeps = [(S, pc, thresholds_for(rng, S, C, pc)) for S, pc in SWEEPS]
        # the entries equal to a threshold are drawn from the 50-row per-class sweep and the 50 global values
        pool = np.concatenate([np.asarray(sweeps[5][2], np.float32), np.asarray(sweeps[2][2], np.float32)[:, None].repeat(C, 1)])
        x, y = weak_scores(rng, B, Ts, C, pool), weak_targets(rng, B, Tt, C)
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        top = x if Ts == 0 else np.max(x, 1)
        saw_nan |= bool(np.isnan(top).any())
        saw_empty |= bool((y == -1).any())
        for S, pc, thr in sweeps:
            got = tag_counts_gpu(xd, yd, thr)
            assert got.dtype == torch.int64 and tuple(got.shape) == (S, C, 4) and got.is_cuda
            want = R.counts_np([(x, y)], thr)
            assert np.array_equal(got.cpu().numpy(), want), (Ts, Tt, S, pc)
            assert (want.sum(-1) == B).all()            # targets of -1 / 0 / 1: every clip is in exactly one count
            t32 = np.asarray(thr, np.float32)
            saw_equal |= bool((top[None] == (t32[:, None, :] if pc else t32[:, None, None])).any())
    if B * C >= 60:
        assert saw_equal and saw_nan and saw_empty      # the edges were in the data


def test_counts_beyond_the_lds_tile_take_the_unstaged_path():
    """C = 8200: one clip's two rows (65.6 KB) exceed the 64 KB tile, the thresholds read global memory"""
    from bsed_amd.evaluation import tag_counts_gpu
    rng = np.random.default_rng(5)
    B, C = 5, 8200
    for Ts, Tt in ((0, 0), (2, 3)):
        thr = thresholds_for(rng, 3, C, False)
        x, y = weak_scores(rng, B, Ts, C, thr), weak_targets(rng, B, Tt, C)
        got = tag_counts_gpu(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), thr)
        assert np.array_equal(got.cpu().numpy(), R.counts_np([(x, y)], thr))
        pc = thresholds_for(rng, 2, C, True)
        got = tag_counts_gpu(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), pc)
        assert np.array_equal(got.cpu().numpy(), R.counts_np([(x, y)], pc))


def test_hand_worked_counts_and_soft_targets_on_the_gpu():
    from bsed_amd.evaluation import tag_counts_gpu
    got = tag_counts_gpu(torch.from_numpy(R.HAND_SCORES).cuda(), torch.from_numpy(R.HAND_TARGETS).cuda(),
                         [[0.5] * 3, R.HAND_CLASS_THRESHOLDS])
    assert got.cpu().numpy().tolist() == [R.HAND_COUNTS, R.HAND_CLASS_COUNTS]
    # 2-D targets are used as given: 2 counts as the arithmetic says, 0.3 and NaN fall out of all four counts; the
    # float32 neighbour of 1 is NOT 1 (the compares run in float64, as numpy's do on est (float64) + labels (float32))
    below_one = np.nextafter(np.float32(1), np.float32(0))
    x = np.asarray([[0.9, 0.1]] * 5, np.float32)
    y = np.asarray([[2, 2], [0.3, 0.3], [np.nan, np.nan], [below_one, below_one], [1, 1]], np.float32)
    got = tag_counts_gpu(x, y, [0.5]).cpu().numpy()
    assert np.array_equal(got, R.counts_np([(x, y)], [0.5]))
    assert got[0].tolist() == [[1, 0, 1, 0], [1, 0, 1, 0]]       # est 1: ref 2 -> fn, ref 1 -> tp;  est 0: ref 2 -> tp, ref 1 -> fn


def test_non_contiguous_inputs_and_host_targets():
    from bsed_amd.evaluation import tag_counts_gpu
    rng = np.random.default_rng(9)
    B, T, C = 7, 5, 20
    thr = thresholds_for(rng, 7, C, False)
    x, y = weak_scores(rng, B, T, 2 * C, thr), weak_targets(rng, B, 0, 2 * C)
    xd = torch.from_numpy(x).cuda()[:, :, ::2]
    xt = torch.from_numpy(np.ascontiguousarray(x[:, :, ::2].transpose(1, 0, 2))).cuda().transpose(0, 1)
    yd = torch.from_numpy(y).cuda()[:, ::2]
    assert not xd.is_contiguous() and not xt.is_contiguous() and not yd.is_contiguous()
    want = R.counts_np([(x[:, :, ::2], y[:, ::2])], thr)
    assert np.array_equal(tag_counts_gpu(xd, yd, thr).cpu().numpy(), want)
    assert np.array_equal(tag_counts_gpu(xt, yd, thr).cpu().numpy(), want)
    # the loader's y is a host tensor (the reference calls y.numpy()), possibly float64
    assert np.array_equal(tag_counts_gpu(xd, torch.from_numpy(y[:, ::2].astype(np.float64)), thr).cpu().numpy(), want)


def test_accumulation_empty_batches_and_repeatability():
    from bsed_amd._lib import BsedError
    from bsed_amd.evaluation import TagThresholds, tag_counts_gpu
    rng = np.random.default_rng(11)
    B, T, C, S = 150, 4, 20, 7
    thr = thresholds_for(rng, S, C, True)
    x, y = weak_scores(rng, B, T, C, thr), weak_targets(rng, B, 0, C)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    whole = tag_counts_gpu(xd, yd, thr)
    out = tag_counts_gpu(xd[:70], yd[:70], thr)
    assert tag_counts_gpu(xd[70:], yd[70:], thr, out=out) is out
    assert torch.equal(out, whole) and (whole.sum(-1) == B).all()
    before = out.clone()
    tag_counts_gpu(xd[:0], yd[:0], thr, out=out)                     # B == 0 leaves the accumulator untouched
    assert torch.equal(out, before)
    fresh = tag_counts_gpu(xd[:0], yd[:0], thr)
    assert tuple(fresh.shape) == (S, C, 4) and int(fresh.abs().sum()) == 0
    for _ in range(3):                                               # two runs give the same bits
        assert torch.equal(tag_counts_gpu(xd, yd, TagThresholds(thr)), whole)
    with pytest.raises(BsedError):
        tag_counts_gpu(xd, yd, thr, out=torch.zeros((S, C, 3), device="cuda", dtype=torch.int64))
    with pytest.raises(BsedError):
        tag_counts_gpu(xd, yd[:, :5], thr)
    with pytest.raises(BsedError):
        tag_counts_gpu(xd, yd, thresholds_for(rng, S, C + 1, True))
    with pytest.raises(BsedError):
        tag_counts_gpu(xd[:, :0], yd, [0.5])                         # a 3-D score without a frame has no maximum


@pytest.mark.parametrize("C", [1, 20, 64])
def test_masks_equal_the_host_threshold(C):
    from bsed_amd.evaluation import tag_masks_gpu
    rng = np.random.default_rng(20 + C)
    for B, T in ((1, 0), (3, 2), (65, 0), (257, 0), (70, 313), (5, 1)):
        cls = thresholds_for(rng, 1, C, True)[0]
        x = weak_scores(rng, B, T, C, [cls, [0.5] * C])
        xd = torch.from_numpy(x).cuda()
        masks, n = tag_masks_gpu(xd, 0.5)
        got = masks.cpu().numpy().view(np.uint64)
        want = R.masks_np(x, 0.5)
        assert masks.dtype == torch.int64 and np.array_equal(got, want), (B, T)
        assert int(n) == int(np.count_nonzero(want))
        masks, n = tag_masks_gpu(xd, class_thresholds=cls)
        want = R.masks_np(x, class_thresholds=cls)
        assert np.array_equal(masks.cpu().numpy().view(np.uint64), want) and int(n) == int(np.count_nonzero(want))
    # the first and the last bit by hand
    x = np.zeros((2, C), np.float32)
    x[0, 0] = x[1, C - 1] = 0.75
    masks, n = tag_masks_gpu(x, 0.5)
    assert masks.cpu().numpy().view(np.uint64).tolist() == [1, 1 << (C - 1)] and int(n) == 2
    assert (masks.cpu().numpy()[1] < 0) == (C == 64)                 # bit 63 is the sign bit of the int64 storage


def test_masks_row_offset_counter_and_the_class_limit():
    from bsed_amd._lib import BsedError
    from bsed_amd.evaluation import tag_masks_gpu
    rng = np.random.default_rng(31)
    C = 20
    a, b = weak_scores(rng, 70, 0, C, [0.5]), weak_scores(rng, 33, 3, C, [0.5])
    buf = torch.full((110,), -1, device="cuda", dtype=torch.int64)
    count = torch.full((1,), 1000, device="cuda", dtype=torch.int64)
    tag_masks_gpu(a, 0.5, out=buf, row_offset=0, nonempty=count)
    tag_masks_gpu(b, 0.5, out=buf, row_offset=70, nonempty=count)
    want = np.concatenate([R.masks_np(a), R.masks_np(b)])
    got = buf.cpu().numpy()
    assert np.array_equal(got[:103].view(np.uint64), want) and (got[103:] == -1).all()       # rows behind stay intact
    assert int(count) == 1000 + int(np.count_nonzero(want)) and 0 < np.count_nonzero(want)
    tag_masks_gpu(a[:0], 0.5, out=buf, row_offset=110, nonempty=count)                       # an empty batch at the end
    assert np.array_equal(buf.cpu().numpy(), got)
    with pytest.raises(BsedError, match="inside the buffer"):
        tag_masks_gpu(b, 0.5, out=buf, row_offset=78, nonempty=count)
    with pytest.raises(BsedError, match="at most 64 classes"):
        tag_masks_gpu(np.zeros((2, 65), np.float32))
    with pytest.raises(BsedError):
        tag_masks_gpu(a, class_thresholds=[0.5] * 19)
    assert np.array_equal(buf.cpu().numpy(), got) and int(count) == 1000 + int(np.count_nonzero(want))


# ---------------------------------------------------------------------------------------------------------------------
# End to end on a small model
# ---------------------------------------------------------------------------------------------------------------------
class Tap(torch.nn.Module):
    """wraps a predictor (or a whole tagger) and keeps the weak tensor of every call, so that the test scores the very
    tensor the pass scored"""

    def __init__(self, inner, take=1):
        super().__init__()
        self.inner, self.take, self.seen = inner, take, []

    def forward(self, x, **kw):
        out = self.inner(x, **kw)
        self.seen.append(out[self.take] if self.take is not None else out)
        return out

    def weak(self):
        got, self.seen = [w.detach().cpu().numpy() for w in self.seen], []
        return got


def _seeded_models(seed):
    from bsed_amd.models import CRNN, Predictor
    ocrnn, opred = co.CRNN(**co.CRNN_KWARGS), co.Predictor(**co.PREDICTOR_KWARGS)
    seeded.load_seeded(ocrnn, seed); seeded.load_seeded(opred, seed + 1)
    crnn, pred = CRNN(**co.CRNN_KWARGS), Predictor(**co.PREDICTOR_KWARGS)
    crnn.load_state_dict(ocrnn.state_dict()); pred.load_state_dict(opred.state_dict())
    return crnn, pred


@pytest.fixture(scope="module")
def small_pass(tmp_path_factory):
    """two batches of (4, 3) clips, a tapped predictor, targets made from a first look at the weak output: about half
    of them agree with it at the per-class median, one row is -1"""
    from bsed_amd.evaluation import validate_weak
    seed, B, T = 51, 7, 256
    crnn, pred = _seeded_models(seed)
    tap = Tap(pred)
    x = seeded.db_like_input(seed + 2, B, T)
    root = tmp_path_factory.mktemp("weak")
    paths = [str(root / "wav" / f"clip{j}.npy") for j in range(B)]
    cuts = [(0, 4), (4, 7)]

    def loader(y):
        return [(((torch.from_numpy(x[a:b]), torch.from_numpy(x[a:b])), None if y is None else torch.from_numpy(y[a:b])),
                 paths[a:b]) for a, b in cuts]

    validate_weak(crnn, loader(np.zeros((B, 20), np.float32)), predictor=tap)
    weak = np.concatenate(tap.weak())
    median = np.median(weak, 0)
    rng = np.random.default_rng(seed)
    y = ((weak > median) ^ (rng.random(weak.shape) < 0.3)).astype(np.float32)
    y[5] = -1.0
    return dict(crnn=crnn, pred=pred, tap=tap, loader=loader, y=y, cuts=cuts, paths=paths, weak=weak,
                median=[float(v) for v in median.astype(np.float32)])


def test_get_f_measure_by_class_equals_the_restatement_on_the_same_tensor(small_pass):
    from bsed_amd.evaluation import TaggingResult, get_f_measure_by_class, validate_weak
    p = small_pass
    crnn, tap, y = p["crnn"], p["tap"], p["y"]
    crnn.train(); tap.eval()
    for thresholds_ in (None, p["median"]):
        f = get_f_measure_by_class(crnn, 20, p["loader"](y), thresholds_=thresholds_, predictor=tap)
        weak = tap.weak()
        assert [w.shape for w in weak] == [(4, 20), (3, 20)]
        want = R.counts_np([(w, y[a:b]) for w, (a, b) in zip(weak, p["cuts"])], [0.5 if thresholds_ is None else thresholds_])
        assert f.dtype == np.float64 and f.shape == (20,) and f.tolist() == R.f_measure_np(want[0]).tolist()
        assert crnn.training and not tap.training and not p["pred"].training         # flags restored
    assert 0 < f.mean() < 1                                          # targets that agree with the output in part
    # the sweep: one pass, all thresholds, the per-class choice handed back as the reference's thresholds_
    sweep = [0.3, 0.4, 0.5, 0.6] + sorted(set(p["median"]))[:3]
    res = validate_weak(crnn, p["loader"](y), predictor=tap, thresholds=sweep)
    weak = tap.weak()
    want = R.counts_np([(w, y[a:b]) for w, (a, b) in zip(weak, p["cuts"])], sweep)
    assert isinstance(res, TaggingResult) and res.counts.dtype == np.int64 and np.array_equal(res.counts, want)
    assert res.thresholds == sweep and (res.counts.sum(-1) == 7).all()
    assert res.class_f1.tolist() == [R.f_measure_np(c).tolist() for c in want]
    assert all(t in sweep for t in res.class_thresholds)
    again = get_f_measure_by_class(crnn, 20, p["loader"](y), thresholds_=res.class_thresholds, predictor=tap)
    tap.weak()
    assert again.tolist() == [res.class_f1[s, c] for c, s in enumerate(res.class_best_index)]
    assert again.mean() >= res.best_macro_f1
    with pytest.raises(NotImplementedError, match="seg_index"):
        get_f_measure_by_class(crnn, 20, p["loader"](y))
    from bsed_amd._lib import BsedError
    with pytest.raises(BsedError):
        get_f_measure_by_class(crnn, 19, p["loader"](y), predictor=tap)
    with pytest.raises(BsedError):
        get_f_measure_by_class(crnn, 20, p["loader"](None), predictor=tap)
    tap.weak()


def test_pseudo_label_rows_equal_the_host_threshold_of_the_same_tensor(small_pass, tmp_path):
    from bsed_amd._lib import BsedError
    from bsed_amd.evaluation import pseudo_label, pseudo_label_frame
    from bsed_amd.labels import BIRD_LIST, ManyHotEncoder
    p = small_pass
    crnn, tap = p["crnn"], p["tap"]
    enc = ManyHotEncoder(BIRD_LIST)
    # a threshold that leaves about half of the clips without a label, then the per-class medians
    high = float(np.sort(p["weak"].max(1))[3])
    out = tmp_path / "sub" / "pseudo.tsv"
    for kw in (dict(threshold=high), dict(class_thresholds=p["median"]), dict()):
        df = pseudo_label(crnn, p["loader"](None), enc.decode_weak, predictor=tap, save_path=str(out), **kw)
        weak = np.concatenate(tap.weak())
        want = pseudo_label_frame(R.masks_np(weak, **kw), p["paths"], BIRD_LIST)
        assert list(df.columns) == ["filename", "event_labels"] and df.equals(want)
        assert open(out).read().splitlines() == ["filename\tevent_labels"] + [f"{r.filename}\t{r.event_labels}" for r in want.itertuples()]
    df = pseudo_label(crnn, p["loader"](None), enc.decode_weak, predictor=tap, threshold=high)
    weak = np.concatenate(tap.weak())
    assert 0 < len(df) < 7 and df.filename.tolist() == [f for f, w in zip(p["paths"], weak) if (w > np.float32(high)).any()]
    with pytest.raises(BsedError, match="decode_weak"):
        pseudo_label(crnn, p["loader"](None), enc.decode_strong, predictor=tap)
    with pytest.raises(NotImplementedError, match="seg_index"):
        pseudo_label(crnn, p["loader"](None), enc.decode_weak)


def test_validate_with_tagging_thresholds_equals_validate_weak_and_changes_nothing_without(small_pass):
    from bsed_amd.evaluation import validate, validate_weak
    from bsed_amd.labels import BIRD_LIST, ManyHotEncoder
    p = small_pass
    crnn, pred, y = p["crnn"], p["pred"], p["y"]
    enc = ManyHotEncoder(BIRD_LIST, n_frames=64)
    sweep = [0.2, 0.5, 0.8]
    kw = dict(pooling_time_ratio=4, thresholds=[0.4, 0.5], predictor=pred, median_window=5)
    weak = validate_weak(crnn, p["loader"](y), predictor=pred, thresholds=sweep)
    both = validate(crnn, p["loader"](y), enc.decode_strong, tagging_thresholds=sweep, **kw)
    assert both.tagging is not None and np.array_equal(both.tagging.counts, weak.counts)
    assert both.tagging.thresholds == sweep and both.tagging.labels == BIRD_LIST
    assert both.tagging.class_thresholds == weak.class_thresholds and both.tagging.best_index == weak.best_index
    plain, second = validate(crnn, p["loader"](y), enc.decode_strong, **kw), validate(crnn, p["loader"](None), enc.decode_strong, **kw)
    assert plain.tagging is None and second.tagging is None
    assert np.array_equal(plain.counts, second.counts) and np.array_equal(plain.counts, both.counts)


class StrongOnly(torch.nn.Module):
    def __init__(self, tagger):
        super().__init__()
        self.tagger = tagger

    def forward(self, x):
        return self.tagger(x)[0]


def _tagger():
    from bsed_amd.models import CRNN_pred
    kw = dict(co.CRNN_KWARGS)
    kw.update(nclass=128, n_RNN_cell=64, dropout=0.0)
    torch.manual_seed(3)
    return CRNN_pred(**kw)


def test_trained_form_with_the_cnn_tagger_and_strong_only_models():
    from bsed_amd.evaluation import get_f_measure_by_class, validate_weak
    B, T = 5, 256
    x = seeded.db_like_input(77, B, T)
    tagger = Tap(_tagger())                              # returns (strong, weak): the weak part is scored
    rng = np.random.default_rng(7)
    y = (rng.random((B, 128)) < 0.5).astype(np.float32)
    loader = [(((torch.from_numpy(x[a:b]), None), torch.from_numpy(y[a:b])), [f"c{j}" for j in range(a, b)]) for a, b in ((0, 2), (2, 5))]
    tagger.train()
    f = get_f_measure_by_class(tagger, 128, loader, trained=True)
    weak = tagger.weak()
    assert [w.shape for w in weak] == [(2, 128), (3, 128)] and tagger.training
    want = R.counts_np([(weak[0], y[:2]), (weak[1], y[2:])], [0.5])
    assert f.tolist() == R.f_measure_np(want[0]).tolist()
    # a model that only predicts strong outputs: (B,T,C), reduced by its maximum over time; strong targets too
    strong_only = Tap(StrongOnly(tagger.inner), take=None)
    ys = (rng.random((B, 64, 128)) < 0.01).astype(np.float32)
    loader = [(((torch.from_numpy(x), None), torch.from_numpy(ys)), [f"c{j}" for j in range(B)])]
    res = validate_weak(strong_only, loader, trained=True, thresholds=[0.5, 0.9])
    strong = strong_only.weak()
    assert strong[0].ndim == 3 and np.array_equal(res.counts, R.counts_np([(strong[0], ys)], [0.5, 0.9]))
    assert (res.counts.sum(-1) == B).all()


def test_training_flags_are_restored_after_an_exception_inside_the_loader(small_pass):
    from bsed_amd.evaluation import pseudo_label, validate, validate_weak
    from bsed_amd.labels import BIRD_LIST, ManyHotEncoder
    p = small_pass
    crnn, pred, y = p["crnn"], p["pred"], p["y"]
    enc = ManyHotEncoder(BIRD_LIST, n_frames=64)

    def broken():
        yield p["loader"](y)[0]
        raise RuntimeError("the disk went away")

    for call in (lambda: validate_weak(crnn, broken(), predictor=pred),
                 lambda: pseudo_label(crnn, broken(), enc.decode_weak, predictor=pred),
                 lambda: validate(crnn, broken(), enc.decode_strong, predictor=pred, tagging_thresholds=[0.5])):
        crnn.train(); pred.eval()
        with pytest.raises(RuntimeError, match="disk went away"):
            call()
        assert crnn.training and not pred.training
        crnn.eval(); pred.train()
        with pytest.raises(RuntimeError, match="disk went away"):
            call()
        assert not crnn.training and pred.training
