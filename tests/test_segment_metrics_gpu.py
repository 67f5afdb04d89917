"""Segment-based counts on the GPU (csrc/segment_metrics.hip, ``bsed_amd.segment_metrics`` / ``validate(segment=...)`` /
``score_recording(segment=...)`` / ``compute_sed_eval_metrics``) against the event-roll restatement of
tests/segment_reference.py.  Both sides take one correctly rounded division per event end and count integers, so the
counts are compared with ==: there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import segment_reference as R
from test_intersection_gpu import tiny_loader, to_gpu  # noqa: F401  (the fixture is used by name)

pytestmark = pytest.mark.gpu


def assert_counts(got, want, what=None):
    class_acc, overall = got
    assert class_acc.dtype == torch.int64 and overall.dtype == torch.int64
    assert np.array_equal(class_acc.cpu().numpy(), want[0]), what
    assert np.array_equal(overall.cpu().numpy(), want[1]), what


def test_the_hand_worked_case_on_the_gpu():
    from bsed_amd.segment_metrics import SegmentResult, segment_counts_gpu
    got = segment_counts_gpu(*to_gpu([[R.HAND_EST]], [R.HAND_REF]))
    assert got[0].shape == (1, 3, 4) and got[1].shape == (1, 4)
    assert got[0][0].tolist() == R.HAND_CLASS and got[1][0].tolist() == R.HAND_OVERALL
    res = SegmentResult(*got, 1.0)
    assert res.f1[0] == res.precision[0] == res.recall[0] == 0.25 and res.error_rate[0] == 1.0
    # the edges of the rules, one event each: zero length on a boundary, [1, 2] is segment 1 only, a negative onset
    none = np.zeros((0, 2))
    edge_ref = [np.asarray([[2.0, 2.0]]), np.asarray([[-0.5, 0.5]]), none]
    edge_est = [np.asarray([[1.0, 2.0]]), none, np.asarray([[0.6, 1.0]])]
    for resolution, length in ((1.0, None), (0.2, None), (0.2, 1.0), (1.0, 3.0), (1.0, 10.0)):
        want = R.segment_counts_np([[edge_est]], [edge_ref], resolution, length)
        assert_counts(segment_counts_gpu(*to_gpu([[edge_est]], [edge_ref]), resolution, length), want, (resolution, length))
    # 0.6 / 0.2 < 3 in float64: class 2's estimate starts in segment 2 (false positives in segments 2, 3, 4)
    assert R.segment_counts_np([[edge_est]], [edge_ref], 0.2, 1.0)[0][0, 2].tolist() == [0, 3, 0, 2]
    for length in (3.0, 10.0):
        assert_counts(segment_counts_gpu(*to_gpu([[R.HAND_EST]], [R.HAND_REF]), 1.0, length),
                      R.segment_counts_np([[R.HAND_EST]], [R.HAND_REF], 1.0, length), length)


@pytest.mark.parametrize("C", [1, 20, 64])
def test_counts_equal_the_restatement_on_random_lists(C):
    from bsed_amd.segment_metrics import segment_counts_gpu
    S, B = 3, 5
    est, ref = R.soup(100 + C, S, B, C)
    every = np.concatenate([a for row in ref for a in row] + [a for e in est for row in e for a in row])
    assert (every[:, 0] == every[:, 1]).any() and (every[:, 0] < 0).any() and (every[:, 1] > 3.0).any()
    assert (every * 8 == np.rint(every * 8)).any() and (every * 8 != np.rint(every * 8)).any()
    assert any(len(a) == 0 for row in ref for a in row) and all(len(a) == 0 for a in ref[1])
    assert any(len(a) > 1 and (np.diff(a[:, 0]) < 0).any() for e in est for row in e for a in row)      # unsorted
    evaluated = np.asarray([True, True, True, False, True])
    for mask in (None, evaluated):
        events, reference = to_gpu(est, ref, mask)
        for resolution in (1.0, 0.2, 0.25):
            for length in (None, 10.0, 3.0):
                want = R.segment_counts_np(est, ref, resolution, length, evaluated=mask)
                assert_counts(segment_counts_gpu(events, reference, resolution, length), want, (C, resolution, length))
    # a hint of more than one tile column launches the kernel's wide instance: the same counts on the same short lists
    for resolution in (1.0, 0.25):
        want = R.segment_counts_np(est, ref, resolution, evaluated=evaluated)
        assert_counts(segment_counts_gpu(events, reference, resolution, expected_seconds=5000.0), want, ("wide", resolution))
    whole, part = R.segment_counts_np(est, ref), R.segment_counts_np(est, ref, evaluated=evaluated)
    assert whole[1][:, 3].sum() > part[1][:, 3].sum() > 0 and whole[0][:, :, :3].sum(1).min() > 0


def test_one_long_clip_at_every_grid_hint():
    from bsed_amd.segment_metrics import segment_counts_gpu
    S, B, C, span = 2, 1, 20, 40000.0
    rng = np.random.default_rng(9)

    def lists(n):                                       # mostly short events, a few that span several tiles
        out = []
        for _ in range(C):
            on = np.round(rng.uniform(0, span - 10.0, n) * 8) / 8
            length = np.where(rng.random(n) < 0.02, rng.uniform(500, 3000, n), rng.uniform(0, 12, n))
            out.append(np.stack([on, np.minimum(on + length, span)], 1))
        return out
    ref = [[a[np.lexsort((a[:, 1], a[:, 0]))] for a in lists(60)]]
    est = [[lists(90)], [lists(40)]]
    est[1][0][3] = np.zeros((0, 2))
    ref[0][0] = np.concatenate([ref[0][0], [[span - 0.5, span]]])    # the clip ends at 40 000 s, part-way into its last tile
    want = R.segment_counts_np(est, ref)
    assert want[1][0, 3] == 40000 and want[1][:, :3].min() > 0 and want[0][:, :, :3].min() >= 0
    events, reference = to_gpu(est, ref)
    assert events.total + len(reference.seconds) > 3000
    for hint in (1.0, 10.0, 1e6):                       # one tile column; the same; far more columns than tiles
        assert_counts(segment_counts_gpu(events, reference, expected_seconds=hint), want, hint)
    assert_counts(segment_counts_gpu(events, reference, 1.0, 20000.5), R.segment_counts_np(est, ref, 1.0, 20000.5), "cut")
    assert_counts(segment_counts_gpu(events, reference, 0.25, expected_seconds=span), R.segment_counts_np(est, ref, 0.25), 0.25)


def test_accumulation_repeatability_and_sentinels():
    from bsed_amd import _lib as L
    from bsed_amd.segment_metrics import segment_counts_gpu
    S, B, C, PAD = 4, 12, 7, 64
    est, ref = R.soup(77, S, B, C)
    whole, again = segment_counts_gpu(*to_gpu(est, ref)), segment_counts_gpu(*to_gpu(est, ref))
    assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1])
    assert_counts(whole, R.segment_counts_np(est, ref))
    out = None
    for lo, hi in ((0, 5), (5, 6), (6, 12)):
        got = segment_counts_gpu(*to_gpu([e[lo:hi] for e in est], ref[lo:hi]), out=out)
        assert out is None or (got[0] is out[0] and got[1] is out[1])
        out = got
    assert torch.equal(out[0], whole[0]) and torch.equal(out[1], whole[1])
    twice = segment_counts_gpu(*to_gpu(est, ref), out=(whole[0].clone(), whole[1].clone()))
    assert torch.equal(twice[0], 2 * whole[0]) and torch.equal(twice[1], 2 * whole[1])
    # nothing is written behind either accumulator
    events, reference = to_gpu(est, ref)
    ref_off, ref_sec = reference.device()
    class_acc = torch.full((S * C * 4 + PAD,), -7, dtype=torch.int64, device="cuda")
    overall = torch.full((S * 4 + PAD,), -7, dtype=torch.int64, device="cuda")
    class_acc[:S * C * 4] = 0
    overall[:S * 4] = 0
    L.call("bsed_segment_counts", L.ptr(events.offsets, torch.int32), L.ptr(events.seconds, torch.float64),
           L.ptr(ref_off, torch.int32), L.ptr(ref_sec, torch.float64), None, S, B, C, 1.0, 0.0, 10.0,
           L.ptr(class_acc, torch.int64), L.ptr(overall, torch.int64), L.stream())
    assert (class_acc[S * C * 4:] == -7).all() and (overall[S * 4:] == -7).all()
    assert torch.equal(class_acc[:S * C * 4].reshape(S, C, 4), whole[0]) and torch.equal(overall[:S * 4].reshape(S, 4), whole[1])


def test_refusals_leave_the_accumulators_unchanged():
    from bsed_amd._lib import BsedError
    from bsed_amd.segment_metrics import segment_counts_gpu
    est, ref = R.soup(5, 2, 3, 4)
    events, reference = to_gpu(est, ref)
    out = segment_counts_gpu(events, reference)
    before = (out[0].clone(), out[1].clone())
    with pytest.raises(BsedError, match="resolution must be a positive finite number"):
        segment_counts_gpu(events, reference, 0, out=out)
    other = to_gpu(*R.soup(6, 2, 3, 5))[1]                          # 3 x 5 against 3 x 4
    with pytest.raises(BsedError, match="3 clips x 4 classes, the reference 3 x 5"):
        segment_counts_gpu(events, other, out=out)
    with pytest.raises(BsedError, match="out must be"):
        segment_counts_gpu(events, reference, out=(out[0], out[0]))
    wide = to_gpu(*R.soup(7, 1, 1, 65, max_events=2))
    wide_out = (torch.zeros((1, 65, 4), dtype=torch.int64, device="cuda"), torch.zeros((1, 4), dtype=torch.int64, device="cuda"))
    with pytest.raises(BsedError, match="at most 64 classes, got 65"):
        segment_counts_gpu(*wide, out=wide_out)
    assert int(wide_out[0].abs().sum()) == 0 and int(wide_out[1].abs().sum()) == 0
    assert torch.equal(out[0], before[0]) and torch.equal(out[1], before[1])
    # no clip: the accumulators come back untouched
    from bsed_amd.evaluation import EventLists, EventReference
    nothing = segment_counts_gpu(EventLists.from_host(np.zeros((2, 0, 4), np.int64), np.zeros((0, 2))),
                                 EventReference(np.zeros((0, 4), np.int64), np.zeros((0, 2)), [], list("abcd")), out=out)
    assert nothing[0] is out[0] and torch.equal(out[0], before[0]) and torch.equal(out[1], before[1])


def test_validate_with_segment_equals_the_restatement_on_the_returned_frames(tiny_loader):
    from bsed_amd.evaluation import validate
    from bsed_amd.segment_metrics import SegmentResult
    t = tiny_loader
    plain = validate(t["crnn"], t["loader"], t["enc"].decode_strong, **t["kw"])
    res = validate(t["crnn"], t["loader"], t["enc"].decode_strong, segment=True, return_predictions=True, **t["kw"])
    assert plain.segment is None and isinstance(res.segment, SegmentResult) and res.intersection is None
    assert np.array_equal(res.counts, plain.counts) and res.best_index == plain.best_index
    assert np.array_equal(res.macro_f1, plain.macro_f1, equal_nan=True)
    est, ref, evaluated = R.frames_to_lists(res.predictions, res.groundtruth_df, t["labels"], t["names"])
    assert evaluated.tolist() == [True] * 5 + [False]
    want = R.segment_counts_np(est, ref, 1.0, evaluated=evaluated)
    assert want[0][:, :, 0].sum() > 0 and want[0][:, :, 1].sum() > 0 and want[0][:, :, 2].sum() > 0
    got = res.segment
    assert got.class_counts.dtype == np.int64 and np.array_equal(got.class_counts, want[0])
    assert np.array_equal(got.overall_counts, want[1])
    assert got.thresholds == t["thresholds"] and got.labels == t["labels"] and got.resolution == 1.0
    m = R.segment_metrics_np(*want)
    assert np.array_equal(got.f1, m["f1"], equal_nan=True) and np.array_equal(got.error_rate, m["error_rate"], equal_nan=True)
    assert np.array_equal(got.macro_f1, m["macro_f1"], equal_nan=True)
    assert got.results(1)["overall"]["f_measure"]["f_measure"] == m["f1"][1]
    # another resolution, together with the intersection counts of the same pass
    both = validate(t["crnn"], t["loader"], t["enc"].decode_strong, segment=0.25, intersection=True, **t["kw"])
    want4 = R.segment_counts_np(est, ref, 0.25, evaluated=evaluated)
    assert np.array_equal(both.segment.class_counts, want4[0]) and np.array_equal(both.segment.overall_counts, want4[1])
    assert both.intersection is not None and np.array_equal(both.counts, plain.counts)


def test_score_recording_and_the_dataframe_call_equal_the_restatement(tiny_loader):
    import event_metrics_reference as ER
    from bsed_amd.evaluation import PsdsResult, compute_metrics, score_recording
    from bsed_amd.segment_metrics import SegmentResult, compute_sed_eval_metrics
    t = tiny_loader
    est, ref, evaluated = R.frames_to_lists(t["preds"], t["gt_df"], t["labels"], t["names"])
    # one recording = one clip: the estimates of clip0 against its reference
    one = [df[df.filename == "clip0"] for df in t["preds"]]
    gt0 = t["gt_df"][t["gt_df"].filename == "clip0"]
    today = score_recording(one, gt0, t["labels"])
    counts, seg = score_recording(one, gt0, t["labels"], segment=0.5, duration=10.0)
    assert isinstance(today, np.ndarray) and np.array_equal(counts, today) and isinstance(seg, SegmentResult)
    want = R.segment_counts_np([[e[0]] for e in est], [ref[0]], 0.5, 10.0)
    assert np.array_equal(seg.class_counts, want[0]) and np.array_equal(seg.overall_counts, want[1])
    assert seg.overall_counts[:, 3].tolist() == [20] * len(one) and seg.resolution == 0.5 and seg.labels == t["labels"]
    counts, seg = score_recording(one, gt0, t["labels"], segment=True)            # no duration: up to the last event
    want = R.segment_counts_np([[e[0]] for e in est], [ref[0]], 1.0)
    assert np.array_equal(seg.class_counts, want[0]) and np.array_equal(seg.overall_counts, want[1])
    three = score_recording(one, gt0, t["labels"], intersection=True, segment=True, duration=10.0)
    assert len(three) == 3 and np.array_equal(three[0], today)
    assert isinstance(three[1], PsdsResult) and isinstance(three[2], SegmentResult)
    pair = score_recording(one, gt0, t["labels"], intersection=True, duration=10.0)
    assert len(pair) == 2 and np.array_equal(pair[1].counts, three[1].counts)
    # the reference's call on two frames: the files of the ground truth, the sorted union of the labels
    pred = t["preds"][1]
    event, segment = compute_sed_eval_metrics(pred, t["gt_df"])
    labels = sorted(set(t["gt_df"].event_label.dropna()) | set(pred.event_label.dropna()))
    names = list(dict.fromkeys(t["gt_df"].filename))
    assert names == t["names"][:5] and segment.labels == labels and 1 < len(labels) <= 20
    e2, r2, ev2 = R.frames_to_lists([pred], t["gt_df"], labels, names)
    want = R.segment_counts_np(e2, r2, 1.0, evaluated=ev2)
    assert np.array_equal(segment.class_counts, want[0]) and np.array_equal(segment.overall_counts, want[1])
    event_want = ER.event_counts_np(e2, r2, evaluated=ev2)
    assert np.array_equal(event["counts"], event_want) and event["macro"][0] == ER.f1_np(event_want)[1][0]
    # with the label list of compute_metrics: its macro event F1, to the bit
    event20, segment20 = compute_sed_eval_metrics(pred, t["gt_df"], t["labels"])
    assert float(event20["macro"][0]) == compute_metrics(pred, t["gt_df"], t["dur_df"], t["labels"])[1]
    want20 = R.segment_counts_np(est[1:2], ref, 1.0, evaluated=evaluated)
    assert np.array_equal(segment20.class_counts, want20[0]) and np.array_equal(segment20.overall_counts, want20[1])
    assert segment20.f1[0] == segment.f1[0] and segment20.error_rate[0] == segment.error_rate[0]
