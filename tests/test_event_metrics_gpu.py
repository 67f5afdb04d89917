"""Validation on the GPU (csrc/metrics.hip, evaluation.sweep_events_gpu / event_counts_gpu / validate / score_recording):
the one-launch threshold sweep against the per-threshold route (binarize_median_gpu -> decode_regions_gpu), and the event
counts against the float64 restatement of tests/event_metrics_reference.py.  Everything here is integer counts and
float64 seconds from exact operations: equal means exactly equal."""
import numpy as np
import pandas as pd
import pytest
import torch

import event_metrics_reference as R
from oracle import crnn_oracle as co
from oracle import seeded

pytestmark = pytest.mark.gpu

SCALE = 4 / (32000 / 255)


def thresholds_for(S):
    return [float(v) for v in np.linspace(0.02, 0.98, S).astype(np.float32)] if S > 1 else [0.5]


def old_route(strong, thresholds, median_window=1, classwise=None, max_len=10.0):
    """the parent route, one threshold at a time -> (counts (S,B,C), frames (E,2), seconds (E,2))"""
    from bsed_amd.evaluation import binarize_median_classwise_gpu, binarize_median_gpu, decode_regions_gpu
    B, T, C = strong.shape
    counts, frames, seconds = [], [], []
    for t in thresholds:
        mask = (binarize_median_classwise_gpu(strong, t, list(classwise)) if classwise is not None
                else binarize_median_gpu(strong, t, median_window))
        ev_clip, ev_class, ev_frames, ev_sec = decode_regions_gpu(mask, SCALE, max_len)
        counts.append(np.bincount(ev_clip.astype(np.int64) * C + ev_class, minlength=B * C).reshape(B, C))
        assert np.all(np.diff(ev_clip.astype(np.int64) * C + ev_class) >= 0)         # clip, then class
        frames.append(ev_frames); seconds.append(ev_sec)
    return np.asarray(counts), np.concatenate(frames), np.concatenate(seconds)


def assert_same_lists(events, want, what):
    counts, frames, seconds = events.host()
    assert counts.shape == want[0].shape and np.array_equal(counts, want[0]), what
    assert frames.dtype == np.int32 and np.array_equal(frames, want[1]), what
    assert seconds.dtype == np.float64 and np.array_equal(seconds, want[2]), what
    assert events.total == len(want[1])


def probabilities(seed, B, T, C, thresholds):
    """smooth-ish random probabilities (runs of on frames, not salt and pepper) with entries EQUAL to thresholds"""
    rng = np.random.default_rng(seed)
    x = rng.random((B, T, C)).astype(np.float32)
    if T >= 8:
        k = np.ones(5) / 5
        x = (0.5 * x + 0.5 * np.apply_along_axis(lambda v: np.convolve(v, k, "same"), 1, rng.random((B, T, C)) ** 0.5 * 1.3)
             ).astype(np.float32).clip(0, 1)
    thr = np.asarray(thresholds, np.float32)
    hit = rng.random((B, T, C)) < 0.1
    x[hit] = thr[rng.integers(0, len(thr), int(hit.sum()))]
    return x


@pytest.mark.parametrize("T", [1, 2, 13, 216, 313])
def test_sweep_equals_the_per_threshold_route(T):
    from bsed_amd.evaluation import sweep_events_gpu
    B, C, S = 3, 20, 7
    thresholds = thresholds_for(S)
    x = torch.from_numpy(probabilities(T, B, T, C, thresholds)).cuda()
    for win in (1, 14, 84, T + 5, 2 * T + 3, 5 * T + 1, 4 * T):
        events = sweep_events_gpu(x, thresholds, median_window=win, scale=SCALE, max_len_seconds=10.0)
        want = old_route(x, thresholds, win)
        assert_same_lists(events, want, (T, win))
        if T >= 13 and win == 1:
            assert events.total > 0
    # max_len clips the late events: the same clip as the decode kernel
    events = sweep_events_gpu(x, thresholds, median_window=3, scale=SCALE, max_len_seconds=0.4 * T * SCALE)
    assert_same_lists(events, old_route(x, thresholds, 3, max_len=0.4 * T * SCALE), (T, "max_len"))


@pytest.mark.parametrize("S", [1, 7, 50])
def test_sweep_threshold_counts_classwise_windows_and_constant_inputs(S):
    from bsed_amd.evaluation import classwise_median_windows, sweep_events_gpu
    B, T, C = 4, 313, 20
    thresholds = thresholds_for(S)
    x = torch.from_numpy(probabilities(100 + S, B, T, C, thresholds)).cuda()
    for win in (14, 84):
        assert_same_lists(sweep_events_gpu(x, thresholds, median_window=win, scale=SCALE), old_route(x, thresholds, win), (S, win))
    windows = classwise_median_windows(32000, 255, 4)                # 10 windows for 20 classes: classes 10.. are dropped
    events = sweep_events_gpu(x, thresholds, classwise_median_window=windows, scale=SCALE)
    assert_same_lists(events, old_route(x, thresholds, classwise=windows), (S, "classwise"))
    counts = events.host()[0]
    assert counts[:, :, :10].sum() > 0 and counts[:, :, 10:].sum() == 0
    for value in (0.0, 1.0):
        const = torch.full((B, T, C), value, device="cuda")
        for t_list in (thresholds, [0.0, 1.0]):
            assert_same_lists(sweep_events_gpu(const, t_list, median_window=14, scale=SCALE), old_route(const, t_list, 14),
                              (S, value))
    # every probability equal to a threshold: `>` is false at it and true below it
    eq = torch.full((B, T, C), thresholds[0], device="cuda")
    ev = sweep_events_gpu(eq, [thresholds[0], float(np.nextafter(np.float32(thresholds[0]), np.float32(-1)))], scale=SCALE)
    assert ev.host()[0][0].sum() == 0 and (ev.host()[0][1] == 1).all()
    assert_same_lists(ev, old_route(eq, [thresholds[0], float(np.nextafter(np.float32(thresholds[0]), np.float32(-1)))]), "eq")


def test_sweep_against_the_scipy_restatement_and_a_tile_beyond_lds():
    from bsed_amd.evaluation import sweep_events_gpu
    thresholds = thresholds_for(5)
    for B, T, C, windows in ((2, 313, 20, [14] * 10 + [84] * 5 + [0] * 5), (1, 2100, 20, [7] * 20)):     # 2100 * 20 * 4 B = 168 KB
        x = probabilities(T + C, B, T, C, thresholds)
        events = sweep_events_gpu(torch.from_numpy(x).cuda(), thresholds, classwise_median_window=[w for w in windows if w],
                                  scale=SCALE, max_len_seconds=1e9)
        assert_same_lists(events, R.flatten(R.sweep_events_np(x, thresholds, windows, SCALE, 1e9)), (B, T, C))
        assert events.total > 0


def test_sweep_frames_equal_get_predictions_frames_and_empty_batches():
    from bsed_amd.evaluation import EventLists, sweep_events_gpu
    from bsed_amd.labels import BIRD_LIST
    thresholds = thresholds_for(3)
    x = torch.from_numpy(probabilities(9, 3, 64, 20, thresholds)).cuda()
    names = ["a", "b", "c"]
    events = sweep_events_gpu(x, thresholds, median_window=5, scale=SCALE)
    assert isinstance(events, EventLists) and (events.S, events.B, events.C) == (3, 3, 20)
    dfs = events.frames(BIRD_LIST, names)
    _, _, want_sec = old_route(x, thresholds, 5)
    assert len(dfs) == 3 and sum(len(d) for d in dfs) == len(want_sec) > 0
    from bsed_amd.evaluation import binarize_median_gpu, decode_regions_gpu
    for t, df in zip(thresholds, dfs):
        ev_clip, ev_class, _, ev_sec = decode_regions_gpu(binarize_median_gpu(x, t, 5), SCALE, 10.0)
        want = pd.DataFrame({"event_label": np.asarray(BIRD_LIST, dtype=object)[ev_class], "onset": ev_sec[:, 0],
                             "offset": ev_sec[:, 1], "filename": np.asarray(names, dtype=object)[ev_clip]})
        assert list(df.columns) == list(want.columns) and (df.dtypes == want.dtypes).all() and df.equals(want)
    empty = sweep_events_gpu(torch.zeros((0, 64, 20), device="cuda"), thresholds)
    assert empty.total == 0 and all(len(d) == 0 for d in empty.frames(BIRD_LIST, []))


def soup(seed, S, B, C, max_ref=6, max_est=9, span=10.0):
    """random reference and estimated lists with overlaps: est[s][b][c], ref[b][c]"""
    rng = np.random.default_rng(seed)

    def events(n, around=None):
        on = rng.uniform(0, span, n) if around is None or not len(around) else \
            around[rng.integers(0, len(around), n), 0] + rng.uniform(-0.3, 0.3, n)
        a = np.stack([on, on + rng.uniform(0.05, 4.0, n)], 1).reshape(-1, 2)
        if around is not None and len(around) and n:        # half of them with an offset near a reference offset
            k = rng.integers(0, len(around), n)
            near = rng.random(n) < 0.5
            a[near, 1] = around[k[near], 1] + rng.uniform(-0.5, 0.5, int(near.sum()))
        return a[np.lexsort((a[:, 1], a[:, 0]))]
    ref = [[events(int(rng.integers(0, max_ref + 1))) if rng.random() < 0.6 else np.zeros((0, 2)) for _ in range(C)] for _ in range(B)]
    est = [[[events(int(rng.integers(0, max_est + 1)), ref[b][c]) if rng.random() < 0.7 else np.zeros((0, 2)) for c in range(C)]
            for b in range(B)] for _ in range(S)]
    return est, ref


def to_gpu(est, ref):
    from bsed_amd.evaluation import EventLists, EventReference
    S, B, C = len(est), len(ref), len(ref[0])
    counts = np.asarray([[[len(est[s][b][c]) for c in range(C)] for b in range(B)] for s in range(S)])
    flat = [est[s][b][c] for s in range(S) for b in range(B) for c in range(C)]
    rcounts = np.asarray([[len(ref[b][c]) for c in range(C)] for b in range(B)])
    rflat = [ref[b][c] for b in range(B) for c in range(C)]
    return (EventLists.from_host(counts, np.concatenate(flat).reshape(-1, 2)),
            EventReference(rcounts, np.concatenate(rflat).reshape(-1, 2), [f"clip{b}" for b in range(B)], [f"class{c}" for c in range(C)]))


@pytest.mark.parametrize("name,ref,est,ntp", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
def test_hand_worked_counts_on_the_gpu(name, ref, est, ntp):
    from bsed_amd.evaluation import event_counts_gpu
    ref, est = np.asarray(ref, np.float64).reshape(-1, 2), np.asarray(est, np.float64).reshape(-1, 2)
    got = event_counts_gpu(*to_gpu([[[est]]], [[ref]]))
    assert got.dtype == torch.int64 and got.cpu().numpy().tolist() == [[[ntp, len(est), len(ref)]]]


def test_pinned_first_fit_case_needs_the_maximum_matching():
    from bsed_amd.evaluation import event_counts_gpu
    ref, est, greedy, best = R.FIRST_FIT_CASE
    ref, est = np.asarray(ref), np.asarray(est)
    assert R.first_fit_ntp(R.hit_matrix(ref, est)) == greedy < best
    assert event_counts_gpu(*to_gpu([[[est]]], [[ref]])).cpu().numpy().tolist() == [[[best, 2, 2]]]
    # the same problem in the middle of a batch, and with the estimates the other way round
    est3 = [[[est, est[::-1].copy()], [np.zeros((0, 2)), est]]]
    ref3 = [[ref, ref], [ref, np.zeros((0, 2))]]
    assert event_counts_gpu(*to_gpu(est3, ref3)).cpu().numpy().tolist() == [[[2, 2, 4], [2, 4, 2]]]


@pytest.mark.parametrize("S,B,C", [(1, 1, 1), (3, 5, 4), (7, 11, 20), (50, 17, 3)])
def test_counts_equal_the_restatement_on_random_event_soups(S, B, C):
    from bsed_amd.evaluation import event_counts_gpu
    est, ref = soup(S * 100 + B, S, B, C)
    want = R.event_counts_np(est, ref)
    got = event_counts_gpu(*to_gpu(est, ref))
    assert np.array_equal(got.cpu().numpy(), want)
    assert want[:, :, 0].sum() > 0 or S * B * C == 1
    # other collars
    for collar, pct in ((0.05, 0.0), (0.5, 1.0), (0.0, 0.2)):
        assert np.array_equal(event_counts_gpu(*to_gpu(est, ref), collar, pct).cpu().numpy(), R.event_counts_np(est, ref, collar, pct))


def test_groups_at_the_cap_and_above_it():
    from bsed_amd._lib import BsedError
    from bsed_amd.evaluation import MATCH_MAX_REF, event_counts_gpu
    rng = np.random.default_rng(11)
    assert MATCH_MAX_REF == 64

    def dense(n, jitter):
        on = np.sort(0.05 * np.arange(n) + rng.uniform(-jitter, jitter, n))      # every event hits a dozen neighbours
        return np.stack([on, on + 1.0 + rng.uniform(-0.15, 0.15, n)], 1)
    ref = [[dense(64, 0.02), dense(63, 0.02), np.zeros((0, 2))], [dense(1, 0.0), dense(64, 0.1), dense(64, 0.0)]]
    est = [[[dense(100, 0.1), dense(64, 0.2), dense(5, 0.1)], [dense(70, 0.1), dense(3, 0.1), dense(64, 0.0)]],
           [[dense(20, 0.3), np.zeros((0, 2)), dense(5, 0.1)], [dense(64, 0.1)[::-1].copy(), dense(200, 0.4), dense(1, 0.0)]]]
    want = R.event_counts_np(est, ref)
    assert want[0, 0, 0] >= 64 and want[0, 2, 0] == 64
    assert np.array_equal(event_counts_gpu(*to_gpu(est, ref)).cpu().numpy(), want)
    ref[1][0] = dense(65, 0.02)
    events, reference = to_gpu(est, ref)
    with pytest.raises(BsedError, match=r"at most 64.*'clip1'.*65.*'class0'"):
        event_counts_gpu(events, reference)


def test_accumulation_over_batches_equals_one_batch_and_two_runs_give_the_same_bits():
    from bsed_amd.evaluation import event_counts_gpu
    S, B, C = 6, 24, 20
    est, ref = soup(77, S, B, C)
    whole = event_counts_gpu(*to_gpu(est, ref))
    again = event_counts_gpu(*to_gpu(est, ref))
    assert torch.equal(whole, again) and np.array_equal(whole.cpu().numpy(), R.event_counts_np(est, ref))
    acc = None
    for lo_, hi in ((0, 7), (7, 8), (8, 24)):
        part = to_gpu([[e[lo_:hi] for e in est][s] for s in range(S)], ref[lo_:hi])
        out = event_counts_gpu(*part, out=acc)
        assert acc is None or out is acc
        acc = out
    assert torch.equal(acc, whole)


def test_clips_outside_the_ground_truth_are_not_scored():
    from bsed_amd.evaluation import event_counts_gpu
    est, ref = soup(5, 2, 6, 3)
    evaluated = np.asarray([True, False, True, True, False, True])
    for b in np.nonzero(~evaluated)[0]:
        ref[b] = [np.zeros((0, 2))] * 3
    events, reference = to_gpu(est, ref)
    reference.evaluated = evaluated
    assert np.array_equal(event_counts_gpu(events, reference).cpu().numpy(), R.event_counts_np(est, ref, evaluated=evaluated))


def test_sentinels_behind_every_output_stay_intact():
    from bsed_amd import _lib as L
    S, B, T, C, PAD = 5, 3, 313, 20, 16
    thresholds = thresholds_for(S)
    x = torch.from_numpy(probabilities(3, B, T, C, thresholds)).cuda()
    thr = torch.tensor(thresholds, dtype=torch.float32).cuda()
    win = torch.full((C,), 5, dtype=torch.int32).cuda()
    n = S * B * C
    counts = torch.full((n + PAD,), -7, dtype=torch.int32, device="cuda")
    L.call("bsed_sweep_count", L.ptr(x), L.ptr(thr), L.ptr(win, torch.int32), S, B, T, C, L.ptr(counts, torch.int32), L.stream())
    assert (counts[n:] == -7).all() and (counts[:n] >= 0).all()
    offsets = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    offsets[1:] = torch.cumsum(counts[:n], 0)
    E = int(offsets[-1])
    assert E > 0
    frames = torch.full((E + PAD, 2), -7, dtype=torch.int32, device="cuda")
    seconds = torch.full((E + PAD, 2), -7.0, dtype=torch.float64, device="cuda")
    L.call("bsed_sweep_write", L.ptr(x), L.ptr(thr), L.ptr(win, torch.int32), L.ptr(offsets, torch.int32), S, B, T, C, SCALE, 10.0,
           L.ptr(frames, torch.int32), L.ptr(seconds, torch.float64), L.stream())
    assert (frames[E:] == -7).all() and (seconds[E:] == -7.0).all()
    assert (frames[:E] >= 0).all() and (seconds[:E] >= 0).all()
    want = old_route(x, thresholds, 5)
    assert np.array_equal(frames[:E].cpu().numpy(), want[1]) and np.array_equal(seconds[:E].cpu().numpy(), want[2])
    # the accumulator: (S, C, 3) counts in front of a padded tail
    _, ref = soup(8, 1, B, C)
    ref_counts = np.asarray([[len(ref[b][c]) for c in range(C)] for b in range(B)])
    ref_off = torch.from_numpy(np.concatenate([[0], np.cumsum(ref_counts.ravel())]).astype(np.int32)).cuda()
    ref_sec = torch.from_numpy(np.concatenate([ref[b][c] for b in range(B) for c in range(C)]).reshape(-1, 2)).cuda()
    acc = torch.full((S * C * 3 + PAD,), -7, dtype=torch.int64, device="cuda")
    acc[:S * C * 3] = 0
    L.call("bsed_event_match", L.ptr(offsets, torch.int32), L.ptr(seconds, torch.float64), L.ptr(ref_off, torch.int32),
           L.ptr(ref_sec, torch.float64), S, B, C, 0.2, 0.2, L.ptr(acc, torch.int64), L.stream())
    assert (acc[S * C * 3:] == -7).all()
    got = acc[:S * C * 3].reshape(S, C, 3).cpu().numpy()
    assert np.array_equal(got[:, :, 1], np.diff(offsets.cpu().numpy()).reshape(S, B, C).sum(1))
    assert np.array_equal(got[:, :, 2], np.broadcast_to(ref_counts.sum(0), (S, C)))


def _seeded_models(seed):
    from bsed_amd.models import CRNN, Predictor
    ocrnn, opred = co.CRNN(**co.CRNN_KWARGS), co.Predictor(**co.PREDICTOR_KWARGS)
    seeded.load_seeded(ocrnn, seed); seeded.load_seeded(opred, seed + 1)
    with torch.no_grad():
        opred.dense.bias += 1.0                          # push some classes over the thresholds
    crnn, pred = CRNN(**co.CRNN_KWARGS), Predictor(**co.PREDICTOR_KWARGS)
    crnn.load_state_dict(ocrnn.state_dict()); pred.load_state_dict(opred.state_dict())
    return crnn, pred


@pytest.mark.parametrize("learned_post", [False, True])
def test_validate_equals_get_predictions_followed_by_the_host_restatement(tmp_path, learned_post):
    from bsed_amd.evaluation import ValidationResult, event_f1, get_predictions, validate
    from bsed_amd.labels import BIRD_LIST, ManyHotEncoder
    seed, B, T = 41, 6, 256
    crnn, pred = _seeded_models(seed)
    x = seeded.db_like_input(seed + 2, B, T)
    root = tmp_path / "d"
    (root / "wav").mkdir(parents=True); (root / "annotation").mkdir()
    # two batches of three clips
    loader = [(((torch.from_numpy(x[i:i + 3]), torch.from_numpy(x[i:i + 3])), None),
               [str(root / "wav" / f"clip{j}.npy") for j in range(i, i + 3)]) for i in (0, 3)]
    enc = ManyHotEncoder(BIRD_LIST, n_frames=T // 4)
    thresholds = [0.3, 0.5, 0.6, 0.7]
    kw = dict(pooling_time_ratio=4, thresholds=thresholds, predictor=pred, learned_post=learned_post, median_window=5)
    first, _, _ = get_predictions(crnn, loader, enc.decode_strong, **kw)
    assert all(len(df) > 0 for df in first[:2])
    # ground truth made from the events of threshold 0.5, moved about so that some hit and some miss; clip4 is an empty
    # clip in DESED's form (one row of NaN), clip5 has no annotation file
    rng = np.random.default_rng(seed)
    for j in range(5):
        rows = first[1][first[1].filename == f"clip{j}"]
        with open(root / "annotation" / f"clip{j}.txt", "w") as f:
            f.write("onset\toffset\tevent_label\n")
            if j == 4:
                f.write("\t\t\n")
                continue
            for r in rows.itertuples():
                if rng.random() < 0.8:
                    f.write(f"{max(r.onset + rng.uniform(-0.3, 0.3), 0.0)}\t{r.offset + rng.uniform(-0.4, 0.4)}\t{r.event_label}\n")
            f.write("1.0\t2.0\tBAWW\n")
    preds, gt_df, _ = get_predictions(crnn, loader, enc.decode_strong, **kw)
    names = [f"clip{j}" for j in range(B)]
    est, ref, evaluated = R.frames_to_lists(preds, gt_df, BIRD_LIST, names)
    assert evaluated.tolist() == [True] * 5 + [False]
    want = R.event_counts_np(est, ref, evaluated=evaluated)
    crnn.train(); pred.eval()
    res = validate(crnn, loader, enc.decode_strong, return_predictions=True, **kw)
    assert isinstance(res, ValidationResult) and crnn.training and not pred.training        # flags restored
    assert res.counts.dtype == np.int64 and res.counts.shape == (4, 20, 3) and np.array_equal(res.counts, want)
    assert want[:, :, 0].sum() > 0 and want[:, :, 0].sum() < want[:, :, 2].sum()
    cls, macro, micro = R.f1_np(want)
    assert np.array_equal(res.class_f1, cls, equal_nan=True) and np.array_equal(res.macro_f1, macro, equal_nan=True)
    assert np.array_equal(res.micro_f1, micro, equal_nan=True)
    best = max(range(4), key=lambda i: (macro[i], -thresholds[i]))
    assert res.best_index == best and res.best_threshold == thresholds[best] and res.best_macro_f1 == macro[best]
    assert res.thresholds == thresholds and res.labels == BIRD_LIST
    for a, b in zip(res.predictions, preds):
        assert list(a.columns) == list(b.columns) and (a.dtypes == b.dtypes).all() and a.equals(b)
    assert res.groundtruth_df.equals(gt_df)
    quiet = validate(crnn, loader, enc.decode_strong, **kw)
    assert quiet.predictions is None and np.array_equal(quiet.counts, want)
    assert event_f1(quiet.counts)["macro"].tolist() == res.macro_f1.tolist()
    with pytest.raises(FileNotFoundError):
        validate(crnn, loader, enc.decode_strong, require_annotations=True, **kw)


def test_score_recording_equals_the_restatement_on_a_long_list():
    from bsed_amd.evaluation import score_recording
    labels = ["EATO", "WOTH", "BCCH"]
    rng = np.random.default_rng(13)
    ron = np.sort(rng.uniform(0, 3600, 900))                        # 300 events a class in an hour: far above 64 a list
    gt = pd.DataFrame({"onset": ron, "offset": ron + rng.uniform(0.1, 3, 900), "event_label": [labels[i] for i in rng.integers(0, 3, 900)]})
    dfs = []
    for s in range(3):
        eon = ron[rng.integers(0, 900, 1200)] + rng.uniform(-0.4, 0.4, 1200)
        dfs.append(pd.DataFrame({"event_label": [labels[i] for i in rng.integers(0, 3, 1200)], "onset": eon,
                                 "offset": eon + rng.uniform(0.1, 3, 1200), "filename": "rec"}))
    est, ref, _ = R.frames_to_lists(dfs, gt.assign(filename="rec"), labels, ["rec"])
    want = R.event_counts_np(est, ref)
    got = score_recording(dfs, gt, labels)
    assert got.dtype == np.int64 and np.array_equal(got, want) and want[:, :, 0].min() > 5
    assert np.array_equal(score_recording(dfs[1], gt, labels), want[1:2])
