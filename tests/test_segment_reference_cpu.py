"""The numpy restatement of the segment-based counts (tests/segment_reference.py) against hand-worked answers: the case
of the header's rules and every edge the rules name.  No GPU, milliseconds."""
import numpy as np

import segment_reference as R

NONE = np.zeros((0, 2))


def counts(ref, est, **kw):
    """one threshold, one clip: lists per class -> (class_acc (C,4), overall (4)) as lists"""
    class_acc, overall = R.segment_counts_np([[est]], [ref], **kw)
    return class_acc[0].tolist(), overall[0].tolist()


def test_the_hand_worked_case():
    # segment  0        1           2        3
    # ref      {0}      {0, 1}      {0}      {}
    # est      {}       {0, 2}      {2}      {2}
    # Sub      0        1           1        0     Del 1 0 0 0     Ins 0 0 0 1
    class_acc, overall = counts(R.HAND_REF, R.HAND_EST)
    assert overall == [2, 1, 1, 4] == R.HAND_OVERALL
    assert class_acc == [[1, 0, 2, 1], [0, 0, 1, 3], [0, 3, 0, 1]] == R.HAND_CLASS
    m = R.segment_metrics_np([class_acc], [overall])
    assert m["precision"][0] == m["recall"][0] == m["f1"][0] == 0.25 and m["error_rate"][0] == 1.0
    assert (m["substitution_rate"][0], m["deletion_rate"][0], m["insertion_rate"][0]) == (0.5, 0.25, 0.25)
    assert m["class_f1"][0].tolist() == [0.5, 0.0, 0.0] and m["macro_f1"][0] == 0.5 / 3
    assert m["class_er"][0, 0] == 2 / 3 and m["class_er"][0, 1] == 1.0 and np.isnan(m["class_er"][0, 2])
    assert m["sensitivity"][0] == 0.25 and m["specificity"][0] == 5 / 8 and m["accuracy"][0] == 6 / 12
    assert m["balanced_accuracy"][0] == (0.25 + 5 / 8) / 2


def test_segments_an_event_covers():
    assert R.covered(2.0, 2.0, 1.0) is None             # zero length on a boundary
    assert R.covered(1.0, 2.0, 1.0) == (1, 2)           # segment 1 only
    assert R.covered(1.0, 2.000001, 1.0) == (1, 3)
    assert R.covered(0.999999, 2.0, 1.0) == (0, 2)
    assert R.covered(-0.3, 0.5, 1.0) == (0, 1)          # a negative onset clamps to segment 0
    assert R.covered(-2.0, -1.0, 1.0) is None
    assert R.covered(1.5, 1.5, 1.0) == (1, 2)           # zero length inside a segment still marks it
    assert R.covered(3.0, 2.0, 1.0) is None
    # the division is the rule: 0.6 / 0.2 is below 3 in float64, so the event starts in segment 2
    assert 0.6 / 0.2 < 3.0
    assert R.covered(0.6, 1.0, 0.2) == (2, 5)
    assert R.covered(0.25, 0.75, 0.25) == (1, 3)


def test_zero_length_and_boundary_events_in_the_counts():
    class_acc, overall = counts([np.asarray([[2.0, 2.0]])], [np.asarray([[1.0, 2.0]])])
    assert overall == [0, 0, 1, 2] and class_acc == [[0, 1, 0, 1]]         # the reference is empty, two segments from its end
    class_acc, overall = counts([np.asarray([[-0.5, 0.5]])], [np.asarray([[0.0, 1.0]])])
    assert overall == [0, 0, 0, 1] and class_acc == [[1, 0, 0, 0]]


def test_evaluated_length_cuts_and_pads():
    class_acc, overall = counts(R.HAND_REF, R.HAND_EST, length_seconds=3)
    assert overall == [2, 1, 0, 3]                      # class 2's fourth segment, the one insertion, is cut off
    assert class_acc == [[1, 0, 2, 0], [0, 0, 1, 2], [0, 2, 0, 1]]
    class_acc, overall = counts(R.HAND_REF, R.HAND_EST, length_seconds=10)
    assert overall == [2, 1, 1, 10]                     # six all-negative segments more
    assert class_acc == [[1, 0, 2, 7], [0, 0, 1, 9], [0, 3, 0, 7]]
    assert R.n_segments([NONE], [NONE], 1.0) == 0 and R.n_segments([NONE], [NONE], 0.2, 1.0) == 5
    assert R.n_segments([np.asarray([[0.0, 2.5]])], [np.asarray([[1.0, 7.2]])], 1.0) == 8
    assert R.n_segments([np.asarray([[9.0, 9.0]])], [NONE], 1.0) == 9      # a zero-length event still ends the clip there


def test_resolution_overlaps_unsorted_lists_and_unevaluated_clips():
    ref = [np.asarray([[0.6, 1.0]])]
    est = [np.asarray([[0.8, 1.0], [0.0, 0.45], [0.3, 0.5]])]        # unsorted, overlapping
    class_acc, overall = counts(ref, est, resolution=0.2)
    # ref segments {2, 3, 4}; est {4} + {0, 1, 2} + {1, 2} = {0, 1, 2, 4}; five segments
    assert class_acc == [[2, 2, 1, 0]] and overall == [0, 1, 2, 5]
    est2, ref2 = R.soup(3, 2, 4, 3)
    assert all(len(a) == 0 for a in ref2[1]) and all(len(a) == 0 for a in est2[0][1])
    evaluated = np.asarray([True, False, True, True])
    keep = [0, 2, 3]
    a = R.segment_counts_np(est2, ref2, evaluated=evaluated)
    b = R.segment_counts_np([[e[i] for i in keep] for e in est2], [ref2[i] for i in keep])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    whole = R.segment_counts_np(est2, ref2)
    assert whole[1][:, 3].sum() == a[1][:, 3].sum()     # clip 1 is empty on both sides: no segment either way
    # per class the four counts add up to the number of segments, and Sub + Del = sum of Nfn, Sub + Ins = sum of Nfp
    assert (whole[0].sum(2) == whole[1][:, 3:4]).all()
    assert np.array_equal(whole[1][:, 0] + whole[1][:, 1], whole[0][:, :, 2].sum(1))
    assert np.array_equal(whole[1][:, 0] + whole[1][:, 2], whole[0][:, :, 1].sum(1))
