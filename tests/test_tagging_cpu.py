"""Clip-level tagging, host side: the ABI 7 entry points and their argument checks (all before any HIP call), the numpy
restatement of tests/tagging_reference.py against hand-worked counts, ``tag_f1`` / ``TaggingResult`` on hand-made counts,
and the pseudo-label TSV: formatting from given masks, the round trip through ``PseudoWeakDataset``, and the row format of
an excerpt of the file the reference ships."""
import os

import numpy as np
import pandas as pd
import pytest

import tagging_reference as R
from bsed_amd import _lib as L
from bsed_amd._lib import BsedError
from bsed_amd.evaluation import TaggingResult, TagThresholds, pseudo_label_frame, tag_f1
from bsed_amd.labels import BIRD_LIST, ManyHotEncoder


def test_abi7_entry_points_are_declared_and_refuse_bad_arguments_before_any_hip_call():
    lib = L.lib()
    assert lib.bsed_abi_version() >= 7
    for name in ("bsed_tag_counts", "bsed_tag_masks"):
        assert name in L.header_symbols()
    d = 0x1000                                          # non-null, never dereferenced on the host

    def refused(rc, word):
        msg = lib.bsed_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    # scores, T_scores, targets, T_targets, thresholds, per_class, S, B, C, counts, stream
    for k in (0, 2, 4, 9):
        args = [d, 0, d, 0, d, 0, 1, 1, 20, d, None]
        args[k] = None
        refused(lib.bsed_tag_counts(*args), "null")
    refused(lib.bsed_tag_counts(d, 0, d, 0, d, 0, 0, 1, 20, d, None), "bad shape")
    refused(lib.bsed_tag_counts(d, 0, d, 0, d, 0, 1, -1, 20, d, None), "bad shape")
    refused(lib.bsed_tag_counts(d, 0, d, 0, d, 0, 1, 1, 0, d, None), "bad shape")
    refused(lib.bsed_tag_counts(d, -1, d, 0, d, 0, 1, 1, 20, d, None), "bad shape")
    refused(lib.bsed_tag_counts(d, 0, d, -1, d, 0, 1, 1, 20, d, None), "bad shape")
    refused(lib.bsed_tag_counts(d, 0, d, 0, d, 2, 1, 1, 20, d, None), "per_class")
    refused(lib.bsed_tag_counts(d, 2 ** 30, d, 0, d, 0, 1, 1, 4, d, None), "too large")
    refused(lib.bsed_tag_counts(d, 0, d, 2 ** 30, d, 0, 1, 1, 4, d, None), "too large")
    refused(lib.bsed_tag_counts(d, 0, d, 0, d, 0, 2 ** 20, 1, 2 ** 10, d, None), "too large")
    # B == 0 is a no-op that returns 0, null tensors (what an empty batch has) included
    assert lib.bsed_tag_counts(None, 0, None, 0, d, 0, 1, 0, 20, d, None) == 0
    assert lib.bsed_tag_counts(None, 313, None, 313, d, 1, 50, 0, 20, d, None) == 0
    # scores, T_scores, class_thresholds, threshold, B, C, row_offset, N, masks, nonempty, stream
    refused(lib.bsed_tag_masks(d, 0, None, 0.5, 1, 65, 0, 1, d, d, None), "at most 64 classes")
    refused(lib.bsed_tag_masks(d, 0, None, 0.5, 1, 0, 0, 1, d, d, None), "bad shape")
    refused(lib.bsed_tag_masks(d, -1, None, 0.5, 1, 20, 0, 1, d, d, None), "bad shape")
    refused(lib.bsed_tag_masks(d, 2 ** 30, None, 0.5, 1, 20, 0, 1, d, d, None), "too large")
    refused(lib.bsed_tag_masks(d, 0, None, 0.5, 2, 20, 0, 1, d, d, None), "inside the buffer")
    refused(lib.bsed_tag_masks(d, 0, None, 0.5, 1, 20, 1, 1, d, d, None), "inside the buffer")
    refused(lib.bsed_tag_masks(d, 0, None, 0.5, 1, 20, -1, 1, d, d, None), "inside the buffer")
    refused(lib.bsed_tag_masks(d, 0, None, 0.5, 1, 20, 2 ** 62, 2 ** 62, d, d, None), "inside the buffer")
    for k in (0, 8, 9):
        args = [d, 0, None, 0.5, 1, 20, 0, 1, d, d, None]
        args[k] = None
        refused(lib.bsed_tag_masks(*args), "null")
    assert lib.bsed_tag_masks(None, 0, None, 0.5, 0, 20, 3, 3, d, d, None) == 0


def test_restatement_reproduces_the_hand_worked_counts():
    # the pieces by hand: strict compare (a score equal to the threshold is off), NaN is off
    est = R.binarization(R.HAND_SCORES, 0.5)
    assert est.tolist() == [[1, 0, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1]]
    tp, fp, fn, tn = R.intermediate_at_measures(R.HAND_TARGETS, est)
    assert np.stack([tp, fp, fn, tn], -1).tolist() == R.HAND_COUNTS
    got = R.counts_np([(R.HAND_SCORES, R.HAND_TARGETS)], [0.5, R.HAND_CLASS_THRESHOLDS])
    assert got.dtype == np.int64 and got.tolist() == [R.HAND_COUNTS, R.HAND_CLASS_COUNTS]
    # a row of -1 (encode_weak("empty")): fp where est == 0, tn where est == 1, as the reference's arithmetic counts it
    empty = ManyHotEncoder(BIRD_LIST[:3]).encode_weak("empty").astype(np.float32)[None]
    assert empty.tolist() == [[-1, -1, -1]]
    got = R.counts_np([(np.asarray([[0.9, 0.1, 0.5]], np.float32), empty)], [0.5])
    assert got[0].tolist() == [[0, 0, 0, 1], [0, 1, 0, 0], [0, 1, 0, 0]]
    # batches add up; every clip lands in exactly one of the four counts for targets in {-1, 0, 1}
    two = R.counts_np([(R.HAND_SCORES[:1], R.HAND_TARGETS[:1]), (R.HAND_SCORES[1:], R.HAND_TARGETS[1:])], [0.5])
    assert two.tolist() == [R.HAND_COUNTS] and (two.sum(-1) == 4).all()


def test_restatement_reduces_three_dimensional_scores_and_labels():
    # scores (B,T,C): max over time, NaN propagating as np.max does; labels (B,T,C): max over time, then > 0.5
    scores = np.asarray([[[0.1, 0.9], [0.6, 0.2]], [[0.4, np.nan], [0.5, 0.99]]], np.float32)    # max: .6 .9 / .5 nan
    labels = np.asarray([[[0.0, 0.5], [0.6, 0.4]], [[0.0, 0.0], [1.0, 0.7]]], np.float32)        # max: .6 .5 / 1 .7 -> 1 0 / 1 1
    got = R.counts_np([(scores, labels)], [0.5])
    # class 0: est 1 0 (0.5 is off), ref 1 1 -> tp, fn;  class 1: est 1 0 (nan), ref 0 1 -> fp, fn
    assert got[0].tolist() == [[1, 0, 1, 0], [0, 1, 1, 0]]
    # 2-D labels are used as given: 0.6 is neither 0 nor 1 and falls out of all four counts
    got = R.counts_np([(scores, np.asarray([[0.6, 0.0], [1.0, 1.0]], np.float32))], [0.5])
    assert got[0].tolist() == [[0, 0, 1, 0], [0, 1, 1, 0]]
    assert R.masks_np(scores).tolist() == [3, 0] and R.masks_np(scores, class_thresholds=[0.45, 0.95]).tolist() == [1, 1]


def test_f_measure_zero_denominator_and_values():
    counts = np.asarray([[[0, 0, 0, 7], [3, 1, 2, 0], [0, 4, 0, 1]]])
    f = tag_f1(counts)
    assert f.dtype == np.float64 and f.tolist() == [[0.0, 6 / 9, 0.0]]
    assert f[0].tolist() == R.f_measure_np(counts[0]).tolist()
    with pytest.raises(BsedError):
        tag_f1(np.zeros((2, 3, 3)))


def test_tagging_result_best_threshold_ties_and_class_thresholds():
    # three thresholds x two classes; F per class:  0.3: (2/3, 1/2)  0.5: (2/3, 1/2)  0.7: (1/2, 4/5)
    counts = np.asarray([[[1, 1, 0, 0], [1, 0, 2, 0]],
                         [[2, 2, 0, 0], [1, 2, 0, 0]],
                         [[1, 0, 2, 0], [2, 1, 0, 0]]])
    res = TaggingResult([0.3, 0.5, 0.7], counts, labels=["a", "b"])
    assert res.class_f1.tolist() == [[2 / 3, 0.5], [2 / 3, 0.5], [0.5, 0.8]]
    assert res.macro_f1.tolist() == [(2 / 3 + 0.5) / 2, (2 / 3 + 0.5) / 2, (0.5 + 0.8) / 2]
    assert res.best_index == 2 and res.best_threshold == 0.7 and res.best_macro_f1 == res.macro_f1[2]
    # class 0 ties between 0.3 and 0.5 -> the lowest; class 1 is best at 0.7: not the best macro threshold for class 0
    assert res.class_thresholds == [0.3, 0.7] and isinstance(res.class_thresholds, list)
    assert res.class_thresholds[0] != res.best_threshold
    # the tie rule looks at the threshold, not the row: the same rows in another order
    res = TaggingResult([0.7, 0.5, 0.3], counts[::-1], labels=["a", "b"])
    assert res.class_thresholds == [0.3, 0.7] and res.best_index == 0
    # a macro tie goes to the lowest threshold
    res = TaggingResult([0.6, 0.4], counts[[0, 1]])
    assert res.best_index == 1 and res.best_threshold == 0.4
    # per-class sweep rows: the threshold a class sees is its own column
    res = TaggingResult([[0.3, 0.9], [0.5, 0.8], [0.7, 0.1]], counts)
    assert res.class_thresholds == [0.3, 0.1] and res.best_threshold == [0.7, 0.1]
    with pytest.raises(BsedError):
        TaggingResult([0.5], counts)


def test_f_values_that_differ_beyond_float64_rounding_are_still_ordered():
    # F = 2^61 / (2^61 + 2) against 2^61 / (2^61 + 1): both round to 1.0 in float64, the second is larger
    big = 2 ** 60
    counts = np.asarray([[[big, 2, 0, 0]], [[big, 1, 0, 0]]], np.int64)
    res = TaggingResult([0.2, 0.4], counts)
    assert res.class_f1[0, 0] == res.class_f1[1, 0] == 1.0 and res.macro_f1[0] == res.macro_f1[1]
    assert res.best_index == 1 and res.class_thresholds == [0.4]        # rounded floats would tie and pick 0.2
    # and the other way round: the larger F at the lower threshold, still found
    res = TaggingResult([0.2, 0.4], counts[::-1])
    assert res.best_index == 0 and res.class_thresholds == [0.2]


def test_tag_thresholds_forms():
    t = TagThresholds([0.25, 0.5])
    assert (t.S, t.C, t.per_class, t.host) == (2, None, False, [0.25, 0.5])
    t = TagThresholds([[0.25, 0.5, 0.75]])
    assert (t.S, t.C, t.per_class, t.host) == (1, 3, True, [[0.25, 0.5, 0.75]])
    for bad in ([], 0.5, np.zeros((1, 2, 3))):
        with pytest.raises(BsedError):
            TagThresholds(bad)


def _mask(enc, text):
    return sum(1 << enc.labels.index(l) for l in text.split(",") if l)


def test_pseudo_label_tsv_label_order_dropped_rows_and_round_trip(tmp_path):
    from bsed_amd.data import PseudoWeakDataset
    enc = ManyHotEncoder(BIRD_LIST)
    root = tmp_path / "pool"
    (root / "wav").mkdir(parents=True)
    names = [f"clip{i}.npy" for i in range(6)]
    for n in names:
        np.save(root / "wav" / n, np.zeros((2, 2), np.float32))
    paths = [str(root / "wav" / n) for n in names]
    # bits given out of label order, an empty clip in the middle, the first and the last label, one class alone
    masks = np.asarray([_mask(enc, "BAWW,EATO,NOCA"), 0, _mask(enc, "BAWW"), _mask(enc, "EATO"), 0,
                        (1 << 20) - 1], np.uint64)
    df = pseudo_label_frame(masks, paths, enc.labels)
    assert list(df.columns) == ["filename", "event_labels"]
    assert df.filename.tolist() == [paths[0], paths[2], paths[3], paths[5]]             # loader order, empty rows dropped
    assert df.event_labels.tolist() == ["EATO,NOCA,BAWW", "BAWW", "EATO", ",".join(BIRD_LIST)]   # label-index order
    # what the reference's decoder gives for the same clips (src/audio_tagging_inference.py:304-311)
    for m, text in zip(masks[[0, 2, 3, 5]], df.event_labels):
        bits = [(int(m) >> c) & 1 for c in range(20)]
        assert text == ",".join(enc.decode_weak(bits))
    tsv = tmp_path / "pseudo.tsv"
    df.to_csv(tsv, index=False, sep="\t")
    assert open(tsv).read().splitlines()[:2] == ["filename\tevent_labels", f"{paths[0]}\tEATO,NOCA,BAWW"]
    ds = PseudoWeakDataset(str(root), enc.encode_weak, pseudo_label_tsv=str(tsv))
    assert len(ds) == 6
    for i in range(6):
        (_, target), path = ds[i]
        assert path == paths[i]
        assert sum(int(v) << c for c, v in enumerate(target)) == int(masks[i]) and set(target.tolist()) <= {0.0, 1.0}
    # int64 storage (what the device buffer is) reads as the same masks, bit 63 included
    top = np.asarray([-2 ** 63, 1], np.int64)
    df = pseudo_label_frame(top, ["a", "b"], [f"l{c}" for c in range(64)])
    assert df.event_labels.tolist() == ["l63", "l0"]
    with pytest.raises(BsedError):
        pseudo_label_frame(np.asarray([1 << 20], np.uint64), ["a"], enc.labels)         # a bit beyond the labels
    with pytest.raises(BsedError):
        pseudo_label_frame(masks, paths[:2], enc.labels)
    empty = pseudo_label_frame(np.zeros(0, np.uint64), [], enc.labels)
    assert list(empty.columns) == ["filename", "event_labels"] and len(empty) == 0


def test_written_rows_parse_like_the_excerpt_of_the_shipped_tsv(golden_dir, tmp_path):
    """tests/golden/pseudo_weak_excerpt.tsv: the header and the first 20 rows of the reference's
    src/unlabel_in_domain_pseudo_weak_resNet.tsv, a format fixture"""
    enc = ManyHotEncoder(BIRD_LIST)
    src = os.path.join(golden_dir, "pseudo_weak_excerpt.tsv")
    shipped = pd.read_csv(src, sep="\t")
    assert list(shipped.columns) == ["filename", "event_labels"] and len(shipped) == 20
    targets = np.stack([enc.encode_weak(shipped[shipped.filename == f]["event_labels"]) for f in shipped.filename])
    masks = np.asarray([sum(int(v) << c for c, v in enumerate(t)) for t in targets], np.uint64)
    assert (masks != 0).all()
    out = tmp_path / "again.tsv"
    pseudo_label_frame(masks, shipped.filename.tolist(), enc.labels).to_csv(out, index=False, sep="\t")
    again = pd.read_csv(out, sep="\t")
    assert again.equals(shipped)                                    # same columns, dtypes, rows
    assert open(out).read() == open(src).read()                     # and the same bytes
