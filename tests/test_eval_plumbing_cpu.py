"""The host plumbing every evaluation pass shares (evaluation._read_annotations / _eval_mode / _event_frame /
_event_table): no GPU, milliseconds."""
import numpy as np
import pandas as pd
import pytest
import torch

from bsed_amd._lib import BsedError
from bsed_amd.evaluation._common import _eval_mode, _event_frame, _read_annotations
from bsed_amd.evaluation.events import _event_table


def test_annotation_reader_on_a_tree_of_five_clips(tmp_path):
    ann = tmp_path / "annotation"
    other = tmp_path / "other"
    ann.mkdir(); other.mkdir()
    head = "onset\toffset\tevent_label\n"
    (ann / "two.txt").write_text(head + "1.0\t3.5\tEATO\n4.0\t4.5\tAMCR\n")
    (ann / "header.txt").write_text(head)
    (ann / "nan.txt").write_text(head + "\t\t\n")                   # DESED's form of a clip without events
    (ann / "twice.txt").write_text(head + "0.5\t0.75\tBAWW\n")
    (other / "twice.txt").write_text(head + "9.0\t9.5\tWOTH\n")     # the second occurrence of the name: never read
    names = ["two", "header", "nan", "missing", "twice", "twice"]
    folders = [str(ann)] * 5 + [str(other)]
    frames, found = _read_annotations(names, folders)
    assert found == 4 and len(frames) == 3                          # header.txt counts as found and gives no frame
    want = [pd.DataFrame({"onset": [1.0, 4.0], "offset": [3.5, 4.5], "event_label": ["EATO", "AMCR"], "filename": "two"}),
            pd.DataFrame({"onset": [np.nan], "offset": [np.nan], "event_label": [np.nan], "filename": "nan"}),
            pd.DataFrame({"onset": [0.5], "offset": [0.75], "event_label": ["BAWW"], "filename": "twice"})]
    for got, w in zip(frames, want):
        assert list(got.columns) == ["onset", "offset", "event_label", "filename"]
        pd.testing.assert_frame_equal(got, w, check_dtype=False)
    assert frames[0].onset.dtype == np.float64 and frames[0].offset.dtype == np.float64
    with pytest.raises(FileNotFoundError) as err:
        _read_annotations(names, folders, require_annotations=True)
    assert str(ann / "missing.txt") in str(err.value)
    # no file at all, and files without a row: get_predictions tells None from an empty frame by these two
    assert _read_annotations(["missing"], [str(ann)]) == ([], 0)
    assert _read_annotations(["header"], [str(ann)]) == ([], 1)


@pytest.mark.parametrize("with_predictor", [True, False])
def test_eval_mode_restores_both_flags_when_the_body_raises(with_predictor):
    for model_training in (True, False):
        model = torch.nn.Identity().train(model_training)
        predictor = torch.nn.Identity().train(not model_training) if with_predictor else None
        with pytest.raises(RuntimeError, match="inside the body"):
            with _eval_mode(model, predictor):
                assert not model.training and (predictor is None or not predictor.training)
                raise RuntimeError("inside the body")
        assert model.training is model_training
        assert predictor is None or predictor.training is (not model_training)
        with _eval_mode(model, predictor):                          # and on the way out of a body that does not raise
            assert not model.training
        assert model.training is model_training


def test_event_frame_columns_order_and_dtypes():
    labels = ["EATO", "WOTH", "BCCH"]
    got = _event_frame(labels, np.asarray([2, 0, 2], np.int32), np.asarray([[0.5, 1.0], [2.0, 2.25], [3.0, 9.5]]),
                       np.asarray(["a", "a", "b"], dtype=object))
    want = pd.DataFrame({"event_label": ["BCCH", "EATO", "BCCH"], "onset": [0.5, 2.0, 3.0], "offset": [1.0, 2.25, 9.5],
                         "filename": ["a", "a", "b"]})
    empty = _event_frame(labels, np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros(0, dtype=object))
    for df, n in ((got, 3), (empty, 0)):
        assert list(df.columns) == ["event_label", "onset", "offset", "filename"] and len(df) == n
        assert [str(t) for t in df.dtypes] == ["object", "float64", "float64", "object"]
        assert list(df.index) == list(range(n))
    assert got.equals(want) and (got.dtypes == want.dtypes).all()


def test_event_table_drops_nan_rows_flags_unknown_labels_and_keeps_the_order():
    labels = ["EATO", "WOTH"]
    df = pd.DataFrame({"onset": [5.0, np.nan, 1.0, 3.0, 2.0], "offset": [6.0, np.nan, 1.5, np.nan, 2.5],
                       "event_label": ["WOTH", np.nan, "EATO", "EATO", "XXXX"]})
    k, on, off, keep, bad = _event_table(df, labels, False)
    assert k.dtype == np.int64 and k.tolist() == [1, -1, 0, 0, -1]
    assert on.tolist()[0::2] == [5.0, 1.0, 2.0] and off.tolist()[0::2] == [6.0, 1.5, 2.5]       # the frame's order, untouched
    assert keep.tolist() == [True, False, True, False, False] and bad == 4      # a NaN row is dropped, not "unknown"
    k2, _, _, keep2, bad2 = _event_table(df, labels, True)
    assert bad2 is None and keep2.tolist() == keep.tolist() and k2.tolist() == k.tolist()
    # rows: an unknown label outside the rows that count neither raises nor is kept
    rows = np.asarray([True, True, False, True, False])
    _, _, _, keep3, bad3 = _event_table(df, labels, False, rows)
    assert bad3 is None and keep3.tolist() == [True, False, False, False, False]
    # the two callers raise their own message from the row
    from bsed_amd.evaluation import EventReference, recording_problem
    gt = df.assign(filename="clip")
    with pytest.raises(BsedError, match="'XXXX' of clip 'clip' is not in the label list"):
        EventReference.from_frame(gt, labels, ["clip"])
    with pytest.raises(BsedError, match="reference event label 'XXXX' is not in the label list"):
        recording_problem(df.iloc[:0], df, labels)
    ref = EventReference.from_frame(gt, labels, ["clip"], ignore_unknown=True)
    assert ref.counts.tolist() == [[1, 1]] and ref.seconds.tolist() == [[1.0, 1.5], [5.0, 6.0]]
