"""Segment-based scoring, host side: ``segment_metrics`` and ``SegmentResult.results()`` on hand-made counts (NaN cases
included) and against the plain-loop restatement of tests/segment_reference.py, the ABI 16 entry point -- declared,
exported, refusing every bad argument before any HIP call --, both import orders in fresh interpreters, and the
``segment=None`` keyword of the scoring passes.  No GPU."""
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import segment_reference as R
from bsed_amd import _lib as L
from bsed_amd._lib import BsedError


def same_or_nan(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_metrics_of_the_hand_worked_counts():
    from bsed_amd.segment_metrics import segment_metrics
    m = segment_metrics(np.asarray([R.HAND_CLASS]), np.asarray([R.HAND_OVERALL]))
    assert m["precision"][0] == m["recall"][0] == m["f1"][0] == 0.25 and m["error_rate"][0] == 1.0
    assert (m["substitution_rate"][0], m["deletion_rate"][0], m["insertion_rate"][0]) == (0.5, 0.25, 0.25)
    assert m["class_f1"][0].tolist() == [0.5, 0.0, 0.0] and m["macro_f1"][0] == 0.5 / 3
    assert m["class_precision"][0, 0] == 1.0 and m["class_recall"][0, 0] == 1 / 3
    # class 1 is never predicted (Nsys = 0): no precision; class 2 never occurs (Nref = 0): no recall and no error rate
    assert np.isnan(m["class_precision"][0, 1]) and m["class_recall"][0, 1] == 0.0 and m["class_er"][0, 1] == 1.0
    assert np.isnan(m["class_recall"][0, 2]) and np.isnan(m["class_er"][0, 2]) and m["class_precision"][0, 2] == 0.0
    assert np.isnan(m["class_deletion_rate"][0, 2]) and np.isnan(m["class_insertion_rate"][0, 2])
    assert m["macro_er"][0] == (2 / 3 + 1.0) / 2        # over the two classes that have one
    assert m["class_nref"][0].tolist() == [3, 1, 0] and m["class_nsys"][0].tolist() == [1, 0, 3]
    assert m["sensitivity"][0] == 0.25 and m["specificity"][0] == 5 / 8 and m["accuracy"][0] == 0.5
    assert m["balanced_accuracy"][0] == (0.25 + 5 / 8) / 2


def test_metrics_without_any_reference_and_without_any_segment():
    from bsed_amd.segment_metrics import segment_metrics
    # nothing occurs, class 0 is predicted in 2 of 5 segments
    m = segment_metrics(np.asarray([[[0, 2, 0, 3], [0, 0, 0, 5]]]), np.asarray([[0, 0, 2, 5]]))
    assert np.isnan(m["recall"][0]) and np.isnan(m["error_rate"][0]) and np.isnan(m["sensitivity"][0])
    assert np.isnan(m["substitution_rate"][0]) and np.isnan(m["balanced_accuracy"][0])
    assert m["precision"][0] == 0.0 and m["f1"][0] == 0.0 and m["specificity"][0] == 0.8 and m["accuracy"][0] == 0.8
    assert m["class_f1"][0, 0] == 0.0 and np.isnan(m["class_f1"][0, 1]) and m["macro_f1"][0] == 0.0
    assert np.isnan(m["class_er"]).all() and np.isnan(m["macro_er"][0])
    m = segment_metrics(np.zeros((2, 3, 4), np.int64), np.zeros((2, 4), np.int64))
    for key, value in m.items():
        if key not in ("class_nref", "class_nsys"):
            assert np.isnan(value).all(), key
    assert m["f1"].shape == (2,) and m["class_f1"].shape == (2, 3)
    with pytest.raises(BsedError, match=r"\(\.\.\., C, 4\)"):
        segment_metrics(np.zeros((2, 3, 3)), np.zeros((2, 4)))
    with pytest.raises(BsedError, match="do not belong together"):
        segment_metrics(np.zeros((2, 3, 4)), np.zeros((3, 4)))


def test_metrics_equal_the_restatement():
    from bsed_amd.segment_metrics import SegmentResult, segment_metrics
    for seed, S, B, C in ((0, 1, 1, 1), (1, 4, 3, 5), (2, 3, 6, 20)):
        est, ref = R.soup(seed, S, B, C)
        if C > 2:
            ref = [[a if c != 2 else np.zeros((0, 2)) for c, a in enumerate(row)] for row in ref]     # Nref = 0
            est = [[[a if c != 1 else np.zeros((0, 2)) for c, a in enumerate(row)] for row in e] for e in est]   # Nsys = 0
        class_acc, overall = R.segment_counts_np(est, ref)
        got, want = segment_metrics(class_acc, overall), R.segment_metrics_np(class_acc, overall)
        assert sorted(got) == sorted(want)
        for key in want:
            assert same_or_nan(got[key], want[key]), (seed, key)
        res = SegmentResult(class_acc, overall, 1.0)
        assert same_or_nan(res.macro_f1, want["macro_f1"]) and same_or_nan(res.error_rate, want["error_rate"])
        if C > 2:
            assert np.isnan(got["class_er"][:, 2]).all() and np.isnan(got["class_precision"][:, 1]).all()


def test_results_has_the_nested_layout():
    from bsed_amd.segment_metrics import SegmentResult
    res = SegmentResult(np.asarray([R.HAND_CLASS, [[0, 0, 0, 4]] * 3]), np.asarray([R.HAND_OVERALL, [0, 0, 0, 4]]), 1.0,
                        labels=["a", "b", "c"], thresholds=[0.5, 0.9])
    assert res.class_counts.dtype == np.int64 and res.overall_counts.dtype == np.int64 and res.resolution == 1.0
    r = res.results()
    assert list(r) == ["overall", "class_wise", "class_wise_average"]
    assert r["overall"]["f_measure"] == {"f_measure": 0.25, "precision": 0.25, "recall": 0.25}
    assert r["overall"]["error_rate"] == {"error_rate": 1.0, "substitution_rate": 0.5, "deletion_rate": 0.25,
                                          "insertion_rate": 0.25}
    assert r["overall"]["accuracy"] == {"accuracy": 0.5, "sensitivity": 0.25, "specificity": 5 / 8,
                                        "balanced_accuracy": (0.25 + 5 / 8) / 2}
    assert list(r["class_wise"]) == ["a", "b", "c"]
    assert r["class_wise"]["a"] == {"f_measure": {"f_measure": 0.5, "precision": 1.0, "recall": 1 / 3},
                                    "error_rate": {"error_rate": 2 / 3, "deletion_rate": 2 / 3, "insertion_rate": 0.0},
                                    "count": {"Nref": 3, "Nsys": 1}}
    assert r["class_wise"]["c"]["count"] == {"Nref": 0, "Nsys": 3} and math.isnan(r["class_wise"]["c"]["error_rate"]["error_rate"])
    assert r["class_wise_average"] == {"f_measure": {"f_measure": 0.5 / 3}, "error_rate": {"error_rate": (2 / 3 + 1.0) / 2}}
    quiet = res.results(1)                              # the second threshold: nothing occurs, nothing is predicted
    assert math.isnan(quiet["overall"]["f_measure"]["f_measure"]) and quiet["overall"]["accuracy"]["accuracy"] == 1.0
    assert math.isnan(quiet["class_wise_average"]["f_measure"]["f_measure"])
    assert list(SegmentResult(np.zeros((1, 2, 4)), np.zeros((1, 4)), 0.5).results()["class_wise"]) == [0, 1]
    with pytest.raises(BsedError, match="labels"):
        SegmentResult(np.zeros((1, 2, 4)), np.zeros((1, 4)), 1.0, labels=["a"])
    with pytest.raises(BsedError, match=r"\(S, C, 4\) and \(S, 4\)"):
        SegmentResult(np.zeros((1, 2, 4)), np.zeros((2, 4)), 1.0)


def test_abi16_entry_point_is_declared_exported_and_refuses_bad_arguments_before_any_hip_call():
    lib = L.lib()
    assert lib.bsed_abi_version() >= 16
    assert "bsed_segment_counts" in L.header_symbols() and hasattr(lib, "bsed_segment_counts")
    assert L.CONSTANTS["BSED_SEGMENT_MAX_CLASSES"] == 64
    header = open(L.HEADER_PATH).read()
    proto = re.search(r"int bsed_segment_counts\(([^)]*)\);", header)[1]
    assert [p.split()[-1].lstrip("*") for p in proto.split(",")] == [
        "est_offsets", "est_seconds", "ref_offsets", "ref_seconds", "evaluated", "S", "B", "C", "resolution",
        "length_seconds", "expected_seconds", "class_acc", "overall", "stream"]
    assert "parity with sed_eval not pinned" in header
    d = 0x1000                                          # non-null, never dereferenced on the host

    def refused(rc, word):
        msg = lib.bsed_last_error().decode()
        assert rc == -1 and msg.startswith("bsed_segment_counts:") and word in msg, (rc, msg)

    good = [d, d, d, d, None, 1, 1, 20, 1.0, 0.0, 10.0, d, d, None]
    for k in (0, 1, 2, 3, 11, 12):
        args = list(good)
        args[k] = None
        refused(lib.bsed_segment_counts(*args), "null")
    for k, v in ((5, 0), (6, 0), (7, 0), (5, -1), (6, -3), (7, -1)):
        args = list(good)
        args[k] = v
        refused(lib.bsed_segment_counts(*args), "bad shape")
    args = list(good)
    args[7] = 65
    refused(lib.bsed_segment_counts(*args), "at most 64 classes")
    for k, word, bad in ((8, "resolution", (0.0, -1.0, float("nan"), float("inf"))),
                         (9, "length_seconds", (-1.0, float("nan"), float("inf"))),
                         (10, "expected_seconds", (0.0, -2.0, float("nan"), float("inf")))):
        for v in bad:
            args = list(good)
            args[k] = v
            refused(lib.bsed_segment_counts(*args), word)
    args = list(good)
    args[5], args[6], args[7] = 2 ** 13, 2 ** 12, 64    # S * B * C = 2^31
    refused(lib.bsed_segment_counts(*args), "int32")
    args = list(good)
    args[8], args[9] = 1e-6, 1e5                        # 10^11 segments
    refused(lib.bsed_segment_counts(*args), "int32")


@pytest.mark.parametrize("first,second", [("bsed_amd.segment_metrics", "bsed_amd.evaluation"),
                                          ("bsed_amd.evaluation", "bsed_amd.segment_metrics")])
def test_both_import_orders_work_in_a_fresh_interpreter(first, second):
    code = (f"import {first}\nimport {second}\nimport bsed_amd.evaluation.validation as v, bsed_amd.segment_metrics as s\n"
            "assert v.SegmentResult is s.SegmentResult and v.segment_counts_gpu is s.segment_counts_gpu\n"
            "import bsed_amd.evaluation as ev\nassert len(ev.__all__) == 41 and 'SegmentResult' not in ev.__all__\nprint('ok')")
    root = os.path.dirname(os.path.dirname(os.path.abspath(L.HEADER_PATH)))          # the child starts in the repository
    done = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], cwd=root,
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr[-2000:]


def test_the_module_imports_only_the_library_numpy_and_torch_at_top_level():
    import ast
    import bsed_amd.segment_metrics as sm
    tree = ast.parse(open(sm.__file__).read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = sorted((n.module or "") + ":" + str(n.level) if isinstance(n, ast.ImportFrom) else n.names[0].name for n in top)
    assert names == [":1", "_lib:1", "numpy", "torch"], names
    inner = [n for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n not in top]
    assert inner and all((n.module or "").startswith("evaluation.") and n.level == 1 for n in inner)
    defined = {n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    assert not defined & {"_accumulator", "_host_counts", "_macro_in_class_order", "_frame_lists"}     # no second copy


def test_the_scoring_passes_carry_the_segment_keyword():
    from bsed_amd.evaluation import ValidationResult, score_recording, validate
    for fn in (validate, score_recording):
        p = inspect.signature(fn).parameters
        assert p["segment"].default is None and list(p)[-1] == "segment"
    p = inspect.signature(ValidationResult.__init__).parameters
    assert p["segment"].default is None and list(p)[-1] == "segment"
    res = ValidationResult([0.5], np.zeros((1, 2, 3), np.int64), ["a", "b"])
    assert res.segment is None and res.intersection is None and res.tagging is None


def test_the_segment_argument_and_the_wrapper_refuse_before_any_launch():
    from bsed_amd.segment_metrics import _resolution, segment_counts_gpu
    assert _resolution(None, "x") is None and _resolution(False, "x") is None
    assert _resolution(True, "x") == 1.0 and _resolution(0.5, "x") == 0.5 and _resolution(2, "x") == 2.0
    for bad in (0, -1.0, float("nan"), float("inf"), "fast", (1.0, 2.0)):
        with pytest.raises(BsedError, match="segment must be"):
            _resolution(bad, "validate")

    class Lists:                                        # the shape fields are all the wrapper reads before it refuses
        def __init__(self, S, B, C):
            self.S, self.B, self.C = S, B, C
    with pytest.raises(BsedError, match="2 clips x 3 classes, the reference 2 x 4"):
        segment_counts_gpu(Lists(1, 2, 3), Lists(1, 2, 4))
    with pytest.raises(BsedError, match="at most 64 classes, got 65"):
        segment_counts_gpu(Lists(1, 2, 65), Lists(1, 2, 65))
    for kw in (dict(resolution=0.0), dict(resolution=float("nan")), dict(length_seconds=0.0), dict(length_seconds=-3.0),
               dict(expected_seconds=float("inf"))):
        with pytest.raises(BsedError, match="must be a positive finite number"):
            segment_counts_gpu(Lists(1, 2, 3), Lists(1, 2, 3), **kw)
