"""Intersection-based counts on the GPU (csrc/intersect.hip, evaluation.intersection_counts_gpu / validate(intersection=...) /
compute_metrics / compute_psds_from_operating_points) against the plain-loop restatement of
tests/intersection_reference.py.  The sums of both sides run in the same order with one correctly rounded division per
pair, so the integer counts are compared with ==: there is no tolerance anywhere in this file."""
import numpy as np
import pandas as pd
import pytest
import torch

import intersection_reference as R
from oracle import seeded
from test_event_metrics_gpu import SCALE, _seeded_models, probabilities, thresholds_for

pytestmark = pytest.mark.gpu

GRID = 0.031875                                         # seconds per output frame at 32 kHz / hop 255 / pooling 4


def to_gpu(est, ref, evaluated=None):
    from bsed_amd.evaluation import EventLists, EventReference
    S, B, C = len(est), len(ref), len(ref[0])
    counts = np.asarray([[[len(est[s][b][c]) for c in range(C)] for b in range(B)] for s in range(S)])
    flat = [np.asarray(est[s][b][c], np.float64).reshape(-1, 2) for s in range(S) for b in range(B) for c in range(C)]
    rcounts = np.asarray([[len(ref[b][c]) for c in range(C)] for b in range(B)])
    rflat = [np.asarray(ref[b][c], np.float64).reshape(-1, 2) for b in range(B) for c in range(C)]
    return (EventLists.from_host(counts, np.concatenate(flat).reshape(-1, 2)),
            EventReference(rcounts, np.concatenate(rflat).reshape(-1, 2), [f"clip{b}" for b in range(B)],
                           [f"class{c}" for c in range(C)], evaluated))


def assert_counts(got, want, what=None):
    acc, ct = got
    assert acc.dtype == torch.int64 and ct.dtype == torch.int64
    assert np.array_equal(acc.cpu().numpy(), want[0]), what
    assert np.array_equal(ct.cpu().numpy(), want[1]), what


@pytest.mark.parametrize("name,ref,est,counts,cts", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
def test_hand_cases_on_the_gpu(name, ref, est, counts, cts):
    from bsed_amd.evaluation import intersection_counts_gpu
    assert_counts(intersection_counts_gpu(*to_gpu(*R.hand_lists(ref, est))), R.hand_expected(counts, cts), name)


@pytest.mark.parametrize("S,B,C", [(1, 1, 1), (3, 5, 4), (7, 11, 20), (5, 3, 64)])
def test_counts_equal_the_restatement_on_random_event_soups(S, B, C):
    from bsed_amd.evaluation import intersection_counts_gpu
    est, ref = R.soup(S * 100 + B, S, B, C)
    if S * B * C == 1:                                  # the one list of the smallest problem is not left to chance
        ref[0][0] = np.asarray([[1.0, 2.0], [1.5, 4.0]]) // GRID * GRID
        est[0][0][0] = np.asarray([[0.9, 2.2], [3.0, 9.0], [3.5, 3.9]]) // GRID * GRID
    want = R.intersection_counts_np(est, ref)
    assert_counts(intersection_counts_gpu(*to_gpu(est, ref)), want, (S, B, C))
    assert 0 < want[0][:, :, 0].sum() < want[0][:, :, 3].sum() and want[0][:, :, 1].sum() > 0
    assert want[1].sum() > 0 or C == 1
    assert np.diagonal(want[1], axis1=1, axis2=2).sum() == 0
    # every list on the frame grid, clipped to 10 s; some clips are all empty
    every = np.concatenate([np.concatenate(r).reshape(-1, 2) for r in ref])
    assert np.array_equal(every, np.clip(np.rint(every / GRID) * GRID, 0, 10.0))
    assert B < 5 or any(all(len(a) == 0 for a in r) for r in ref)
    # other criteria: strict ones, lax ones, 1.0 (only a full cover passes)
    for crit in ((0.7, 0.7, 0.5), (0.1, 0.2, 0.05), (1.0, 1.0, 1.0)):
        assert_counts(intersection_counts_gpu(*to_gpu(est, ref), *crit), R.intersection_counts_np(est, ref, *crit), crit)


def test_long_lists_in_one_group_and_more_than_a_wave_on_one_side():
    from bsed_amd.evaluation import intersection_counts_gpu
    rng = np.random.default_rng(5)

    def dense(n, longest):
        on = rng.integers(0, 300, n)
        a = np.stack([on * GRID, (on + rng.integers(1, longest, n)) * GRID], 1).clip(0, 10.0)
        return a[np.lexsort((a[:, 1], a[:, 0]))]
    none = np.zeros((0, 2))
    # clip 0: 200 estimated and 150 reference events in class 1; clip 1: 70 reference events against 2 detections in
    # class 0, 130 detections against 1 reference event in class 2 (more than a wave on one side only)
    ref = [[dense(3, 40), dense(150, 12), none], [dense(70, 6), none, np.asarray([[2.0, 8.0]]) // GRID * GRID]]
    est = [[[dense(4, 40), dense(200, 3), dense(9, 80)], [np.asarray([[0.0, 10.0], [1.0, 1.5]]) // GRID * GRID, dense(5, 9), dense(130, 5)]],
           [[none, dense(200, 30), none], [dense(65, 9), dense(64, 9), dense(63, 9)]]]
    want = R.intersection_counts_np(est, ref)
    assert want[0][0, 1, 2] == 200 + 5 and want[0][0, 1, 3] == 150 and 0 < want[0][0, 1, 0] < 150
    assert 0 < want[0][0, 2, 0] and want[1].sum() > 0
    assert_counts(intersection_counts_gpu(*to_gpu(est, ref)), want)


@pytest.mark.parametrize("T", [13, 313])
def test_lists_from_the_threshold_sweep(T):
    from bsed_amd.evaluation import EventReference, intersection_counts_gpu, sweep_events_gpu
    B, C, S = 4, 20, 5
    thresholds = thresholds_for(S)
    x = torch.from_numpy(probabilities(T + 1, B, T, C, thresholds)).cuda()
    events = sweep_events_gpu(x, thresholds, median_window=3, scale=SCALE, max_len_seconds=10.0)
    counts, _, seconds = events.host()
    assert events.total > 0
    # the reference: the events of the middle threshold, every third dropped, the others moved by a few frames
    rng = np.random.default_rng(T)
    at = np.concatenate([[0], np.cumsum(counts.ravel())])
    est = [[[seconds[at[(s * B + b) * C + c]:at[(s * B + b) * C + c + 1]] for c in range(C)] for b in range(B)] for s in range(S)]
    ref = []
    for b in range(B):
        row = []
        for c in range(C):
            a = est[S // 2][b][c]
            a = a[rng.random(len(a)) < 0.67] + rng.integers(-2, 3, (1, 2)) * SCALE
            a = a[a[:, 1] > a[:, 0]].clip(0, 10.0)
            row.append(a[np.lexsort((a[:, 1], a[:, 0]))])
        ref.append(row)
    rcounts = np.asarray([[len(ref[b][c]) for c in range(C)] for b in range(B)])
    reference = EventReference(rcounts, np.concatenate([a for r in ref for a in r]).reshape(-1, 2), list("abcd"), list(range(C)))
    want = R.intersection_counts_np(est, ref)
    assert want[0][:, :, 0].sum() > 0 and want[0][:, :, 1].sum() > 0
    assert_counts(intersection_counts_gpu(events, reference), want, T)


def test_unevaluated_clips_are_skipped_and_null_means_every_clip():
    from bsed_amd.evaluation import intersection_counts_gpu
    est, ref = R.soup(21, 3, 7, 5)
    evaluated = np.asarray([True, False, True, True, False, False, True])
    keep = np.nonzero(evaluated)[0]
    want = R.intersection_counts_np([[e[b] for b in keep] for e in est], [ref[b] for b in keep])
    events, reference = to_gpu(est, ref, evaluated)
    assert reference.device_evaluated().tolist() == evaluated.astype(int).tolist()
    assert_counts(intersection_counts_gpu(events, reference), want)
    assert_counts(intersection_counts_gpu(events, reference), R.intersection_counts_np(est, ref, evaluated=evaluated))
    # NULL = all on: the same as a mask of ones passed explicitly
    events, reference = to_gpu(est, ref)
    assert reference.device_evaluated() is None
    whole = intersection_counts_gpu(events, reference)
    assert_counts(whole, R.intersection_counts_np(est, ref))
    from bsed_amd import _lib as L
    S, B, C = 3, 7, 5
    ones = torch.ones(B, dtype=torch.uint8, device="cuda")
    acc = torch.zeros((S, C, 4), dtype=torch.int64, device="cuda")
    ct = torch.zeros((S, C, C), dtype=torch.int64, device="cuda")
    flags = torch.zeros(max(events.total, 1), dtype=torch.uint8, device="cuda")
    ref_off, ref_sec = reference.device()
    L.call("bsed_intersection_counts", L.ptr(events.offsets, torch.int32), L.ptr(events.seconds, torch.float64),
           L.ptr(ref_off, torch.int32), L.ptr(ref_sec, torch.float64), L.ptr(ones, torch.uint8), S, B, C, 0.5, 0.5, 0.3,
           L.ptr(flags, torch.uint8), L.ptr(acc, torch.int64), L.ptr(ct, torch.int64), L.stream())
    assert torch.equal(acc, whole[0]) and torch.equal(ct, whole[1])


def test_accumulation_over_batches_equals_one_batch_and_two_runs_give_the_same_bits():
    from bsed_amd._lib import BsedError
    from bsed_amd.evaluation import intersection_counts_gpu
    S, B, C = 6, 24, 20
    est, ref = R.soup(77, S, B, C)
    whole = intersection_counts_gpu(*to_gpu(est, ref))
    again = intersection_counts_gpu(*to_gpu(est, ref))
    assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1])
    assert_counts(whole, R.intersection_counts_np(est, ref))
    out = None
    for lo, hi in ((0, 7), (7, 8), (8, 24)):
        got = intersection_counts_gpu(*to_gpu([e[lo:hi] for e in est], ref[lo:hi]), out=out)
        assert out is None or (got[0] is out[0] and got[1] is out[1])
        out = got
    assert torch.equal(out[0], whole[0]) and torch.equal(out[1], whole[1])
    with pytest.raises(BsedError, match="out must be"):
        intersection_counts_gpu(*to_gpu(est, ref), out=(whole[0], whole[0]))
    with pytest.raises(BsedError, match=r"dtc must lie in \(0, 1\]"):
        intersection_counts_gpu(*to_gpu(est, ref), dtc=0.0)


def test_sentinels_behind_every_output_stay_intact():
    from bsed_amd import _lib as L
    S, B, C, PAD = 4, 6, 7, 64
    est, ref = R.soup(31, S, B, C)
    events, reference = to_gpu(est, ref)
    E = events.total
    assert E > 64
    ref_off, ref_sec = reference.device()
    acc = torch.full((S * C * 4 + PAD,), -7, dtype=torch.int64, device="cuda")
    ct = torch.full((S * C * C + PAD,), -7, dtype=torch.int64, device="cuda")
    flags = torch.full((E + PAD,), 0x5A, dtype=torch.uint8, device="cuda")
    acc[:S * C * 4] = 0
    ct[:S * C * C] = 0
    L.call("bsed_intersection_counts", L.ptr(events.offsets, torch.int32), L.ptr(events.seconds, torch.float64),
           L.ptr(ref_off, torch.int32), L.ptr(ref_sec, torch.float64), None, S, B, C, 0.5, 0.5, 0.3,
           L.ptr(flags, torch.uint8), L.ptr(acc, torch.int64), L.ptr(ct, torch.int64), L.stream())
    assert (acc[S * C * 4:] == -7).all() and (ct[S * C * C:] == -7).all() and (flags[E:] == 0x5A).all()
    assert (flags[:E] <= 1).all()
    want = R.intersection_counts_np(est, ref)
    assert np.array_equal(acc[:S * C * 4].reshape(S, C, 4).cpu().numpy(), want[0])
    assert np.array_equal(ct[:S * C * C].reshape(S, C, C).cpu().numpy(), want[1])
    # the flags are the DTC verdicts: as many zeros as false positives
    assert int((flags[:E] == 0).sum()) == want[0][:, :, 1].sum()


@pytest.fixture(scope="module")
def tiny_loader(tmp_path_factory):
    """the loader fixture of test_event_metrics_gpu's validate test: two batches of three clips with annotation files
    made from the model's own events at threshold 0.5 (moved about), clip4 empty in DESED's form, clip5 without a file"""
    from bsed_amd.evaluation import get_predictions
    from bsed_amd.labels import BIRD_LIST, ManyHotEncoder
    seed, B, T = 41, 6, 256
    crnn, pred = _seeded_models(seed)
    x = seeded.db_like_input(seed + 2, B, T)
    root = tmp_path_factory.mktemp("isect") / "d"
    (root / "wav").mkdir(parents=True); (root / "annotation").mkdir()
    loader = [(((torch.from_numpy(x[i:i + 3]), torch.from_numpy(x[i:i + 3])), None),
               [str(root / "wav" / f"clip{j}.npy") for j in range(i, i + 3)]) for i in (0, 3)]
    enc = ManyHotEncoder(BIRD_LIST, n_frames=T // 4)
    thresholds = [0.3, 0.5, 0.6, 0.7]
    kw = dict(pooling_time_ratio=4, thresholds=thresholds, predictor=pred, median_window=5)
    first, _, _ = get_predictions(crnn, loader, enc.decode_strong, **kw)
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
    preds, gt_df, dur_df = get_predictions(crnn, loader, enc.decode_strong, **kw)
    return dict(crnn=crnn, pred=pred, loader=loader, enc=enc, kw=kw, thresholds=thresholds, labels=BIRD_LIST,
                names=[f"clip{j}" for j in range(B)], preds=preds, gt_df=gt_df, dur_df=dur_df)


def test_validate_with_intersection_equals_get_predictions_followed_by_the_restatement(tiny_loader):
    from bsed_amd.evaluation import PsdsResult, validate
    t = tiny_loader
    est, ref, evaluated = R.frames_to_lists(t["preds"], t["gt_df"], t["labels"], t["names"])
    assert evaluated.tolist() == [True] * 5 + [False]
    want = R.intersection_counts_np(est, ref, evaluated=evaluated)
    assert want[0][:, :, 0].sum() > 0 and want[0][:, :, 1].sum() > 0
    plain = validate(t["crnn"], t["loader"], t["enc"].decode_strong, **t["kw"])
    res = validate(t["crnn"], t["loader"], t["enc"].decode_strong, intersection=True, **t["kw"])
    assert plain.intersection is None and isinstance(res.intersection, PsdsResult)
    # the collar-based side is untouched, bit for bit
    assert np.array_equal(res.counts, plain.counts) and res.best_index == plain.best_index
    for a, b in ((res.class_f1, plain.class_f1), (res.macro_f1, plain.macro_f1), (res.micro_f1, plain.micro_f1)):
        assert np.array_equal(a, b, equal_nan=True)
    got = res.intersection
    assert got.counts.dtype == np.int64 and np.array_equal(got.counts, want[0]) and np.array_equal(got.ct, want[1])
    cls, macro = R.intersection_f1_np(want[0])
    assert np.array_equal(got.class_f1, cls, equal_nan=True) and np.array_equal(got.macro_f1, macro, equal_nan=True)
    assert got.thresholds == t["thresholds"] and got.labels == t["labels"] and got.criteria == (0.5, 0.5, 0.3)
    assert got.total_duration == 50.0                               # five evaluated clips of 10 s
    dur = R.class_durations_np(ref, evaluated)
    assert np.allclose(got.ref_duration, dur, rtol=1e-12, atol=0)
    tpr, fpr, ctr = R.rates_np(want[0], want[1], got.ref_duration, 50.0)
    for alpha_ct, alpha_st in ((0, 0), (1, 0), (0, 1)):
        value = R.psds_np(tpr, R.efpr_np(fpr, ctr, alpha_ct), alpha_st, 100.0)
        assert abs(got.psds(alpha_ct, alpha_st, 100).value - value) <= 1e-12
    # other criteria through the tuple form
    strict = validate(t["crnn"], t["loader"], t["enc"].decode_strong, intersection=(0.7, 0.7, 0.1), **t["kw"]).intersection
    want7 = R.intersection_counts_np(est, ref, 0.7, 0.7, 0.1, evaluated=evaluated)
    assert np.array_equal(strict.counts, want7[0]) and np.array_equal(strict.ct, want7[1])


def test_the_dataframe_drop_ins_equal_the_restatement(tiny_loader):
    from bsed_amd.evaluation import compute_metrics, compute_psds_from_operating_points, event_f1, score_recording
    import event_metrics_reference as ER
    t = tiny_loader
    est, ref, evaluated = R.frames_to_lists(t["preds"], t["gt_df"], t["labels"], t["names"])
    want = R.intersection_counts_np(est, ref, evaluated=evaluated)
    res = compute_psds_from_operating_points(t["preds"], t["gt_df"], t["dur_df"], t["labels"])
    assert np.array_equal(res.counts, want[0]) and np.array_equal(res.ct, want[1]) and res.total_duration == 50.0
    tpr, fpr, ctr = R.rates_np(want[0], want[1], res.ref_duration, 50.0)
    assert np.allclose(res.ref_duration, R.class_durations_np(ref, evaluated), rtol=1e-12, atol=0)
    assert abs(res.psds(1, 0, 100).value - R.psds_np(tpr, R.efpr_np(fpr, ctr, 1), 0, 100.0)) <= 1e-12
    other = compute_psds_from_operating_points(t["preds"][:2], t["gt_df"], t["dur_df"], t["labels"], 0.6, 0.4, 0.2)
    want2 = R.intersection_counts_np(est[:2], ref, 0.6, 0.4, 0.2, evaluated=evaluated)
    assert np.array_equal(other.counts, want2[0]) and np.array_equal(other.ct, want2[1])
    ct_matrix, macro_event, macro_isect = compute_metrics(t["preds"][1], t["gt_df"], t["dur_df"], t["labels"])
    assert ct_matrix.shape == (20, 20) and np.array_equal(ct_matrix, want[1][1])
    assert macro_isect == R.intersection_f1_np(want[0])[1][1]
    assert macro_event == ER.f1_np(ER.event_counts_np(est[1:2], ref, evaluated=evaluated))[1][0]
    # one recording = one clip: the estimates of clip0 against its reference
    one = [df[df.filename == "clip0"] for df in t["preds"]]
    gt0 = t["gt_df"][t["gt_df"].filename == "clip0"]
    counts, isect = score_recording(one, gt0, t["labels"], intersection=True, duration=10.0)
    assert np.array_equal(counts, score_recording(one, gt0, t["labels"]))
    want0 = R.intersection_counts_np([[e[0]] for e in est], [ref[0]])
    assert np.array_equal(isect.counts, want0[0]) and np.array_equal(isect.ct, want0[1]) and isect.total_duration == 10.0
