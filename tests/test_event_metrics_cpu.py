"""Event-based validation metric, host side: the float64 restatement of tests/event_metrics_reference.py against
hand-worked counts, the pinned problem that separates first-fit from maximum matching, ``event_f1``, ``EventReference``
grouping, ``recording_problem`` and the argument checks of the ABI 6 entry points (all before any HIP call)."""
import numpy as np
import pandas as pd
import pytest

import event_metrics_reference as R
from bsed_amd import _lib as L
from bsed_amd._lib import BsedError
from bsed_amd.evaluation import MATCH_MAX_REF, EventReference, ValidationResult, event_f1, recording_problem

LABELS = ["EATO", "WOTH", "BCCH"]


@pytest.mark.parametrize("name,ref,est,ntp", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
def test_hand_worked_counts(name, ref, est, ntp):
    ref, est = np.asarray(ref, np.float64).reshape(-1, 2), np.asarray(est, np.float64).reshape(-1, 2)
    assert R.max_matching(R.hit_matrix(ref, est)) == ntp
    got = R.event_counts_np([[[est]]], [[ref]])
    assert got.tolist() == [[[ntp, len(est), len(ref)]]]


def test_hit_rule_by_hand():
    # the two rules spelled out for the long event: |1.0 - 1.1| = 0.1 <= 0.2; |11.0 - 12.5| = 1.5 <= max(0.2, 0.2 * 10) = 2
    h = R.hit_matrix([[1.0, 11.0]], [[1.1, 12.5], [1.1, 13.1], [1.3, 11.0]])
    assert h.tolist() == [[True, False, False]]
    # other collars: 0.05 s turns the 0.1 s onset error into a miss; percentage 1.0 makes the 2.1 s offset error a hit
    assert not R.hit_matrix([[1.0, 11.0]], [[1.1, 12.5]], t_collar=0.05).any()
    assert R.hit_matrix([[1.0, 11.0]], [[1.1, 13.1]], percentage_of_length=1.0).all()


def test_first_fit_is_not_enough_on_the_pinned_case():
    ref, est, greedy, best = R.FIRST_FIT_CASE
    h = R.hit_matrix(ref, est)
    assert h.tolist() == [[True, True], [True, False]]
    assert R.first_fit_ntp(h) == greedy == 1 and R.max_matching(h) == best == 2
    # such problems are not rare: a seeded search over small random problems finds many
    rng = np.random.default_rng(0)
    worse = 0
    for _ in range(3000):
        r = np.sort(rng.uniform(1, 2, (3, 1)), 0) + np.asarray([[0.0, 1.0]]) + rng.uniform(0, 0.3, (3, 2)) * [[0, 1]]
        e = np.sort(rng.uniform(1, 2, (3, 1)), 0) + np.asarray([[0.0, 1.0]]) + rng.uniform(0, 0.3, (3, 2)) * [[0, 1]]
        h = R.hit_matrix(r, e)
        assert R.first_fit_ntp(h) <= R.max_matching(h)
        worse += R.first_fit_ntp(h) < R.max_matching(h)
    assert worse > 10


def test_max_matching_against_brute_force():
    import itertools
    rng = np.random.default_rng(1)
    for _ in range(200):
        nr, ne = rng.integers(1, 5), rng.integers(1, 6)
        h = rng.random((nr, ne)) < 0.4
        best = 0
        for k in range(1, min(nr, ne) + 1):
            for rows in itertools.combinations(range(nr), k):
                if any(all(h[r, c] for r, c in zip(rows, cols)) for cols in itertools.permutations(range(ne), k)):
                    best = k
        assert R.max_matching(h) == best


def test_event_f1_with_empty_classes():
    #            Ntp Nsys Nref
    counts = [[[2, 4, 2],       # P = 0.5, R = 1: F = 2/3 = 2 * 2 / 6
               [0, 0, 0],       # neither predicted nor present: NaN, left out of the macro mean
               [0, 3, 0],       # predicted, never present: F = 0
               [0, 0, 5],       # present, never predicted: F = 0
               [1, 1, 1]],      # F = 1
              [[0, 0, 0]] * 5]  # nothing at all
    f = event_f1(np.asarray(counts))
    assert f["class_f1"].shape == (2, 5) and f["class_f1"].dtype == np.float64
    assert f["class_f1"][0, 0] == 4 / 6 and f["class_f1"][0, 2] == 0 and f["class_f1"][0, 3] == 0 and f["class_f1"][0, 4] == 1
    assert np.isnan(f["class_f1"][0, 1]) and np.isnan(f["class_f1"][1]).all()
    assert f["macro"][0] == (4 / 6 + 0 + 0 + 1) / 4 and np.isnan(f["macro"][1])
    assert f["micro"][0] == 2 * 3 / (8 + 8) and np.isnan(f["micro"][1])
    # 2 Ntp / (Nsys + Nref) is 2PR / (P + R) wherever both are defined
    p, r = 2 / 4, 2 / 2
    assert abs(f["class_f1"][0, 0] - 2 * p * r / (p + r)) < 1e-15
    cls, macro, micro = R.f1_np(np.asarray(counts))
    for a, b in ((f["class_f1"], cls), (f["macro"], macro), (f["micro"], micro)):
        assert np.array_equal(a, b, equal_nan=True)
    one = event_f1(np.asarray(counts[0]))               # (C,3) -> (C), scalars
    assert one["class_f1"].shape == (5,) and float(one["micro"]) == f["micro"][0] and float(one["macro"]) == f["macro"][0]
    with pytest.raises(BsedError):
        event_f1(np.zeros((3, 2)))


def test_validation_result_picks_the_lowest_threshold_on_ties():
    c = np.zeros((4, 1, 3), np.int64)
    c[0, 0] = (1, 4, 4); c[1, 0] = (2, 4, 4); c[2, 0] = (2, 4, 4); c[3, 0] = (0, 0, 0)
    res = ValidationResult([0.2, 0.7, 0.5, 0.9], c, ["EATO"])
    assert res.best_threshold == 0.5 and res.best_index == 2 and res.best_macro_f1 == 0.5
    assert np.isnan(res.macro_f1[3]) and res.class_f1.shape == (4, 1)
    assert ValidationResult([0.3, 0.6], np.zeros((2, 1, 3), np.int64), ["EATO"]).best_threshold == 0.3     # all NaN


def _gt(rows):
    return pd.DataFrame(rows, columns=["onset", "offset", "event_label", "filename"])


def test_event_reference_groups_sorts_and_drops_nan_rows():
    gt = _gt([(4.0, 4.5, "BCCH", "a"), (1.0, 3.5, "EATO", "a"), (0.5, 0.9, "EATO", "a"), (np.nan, np.nan, np.nan, "b"),
              (2.0, 3.0, "WOTH", "c"), (1.0, 1.2, "EATO", "other"), (1.0, np.nan, "EATO", "c")])
    ref = EventReference.from_frame(gt, LABELS, ["a", "b", "c", "d"])
    assert (ref.B, ref.C) == (4, 3)
    assert ref.counts.tolist() == [[2, 0, 1], [0, 0, 0], [0, 1, 0], [0, 0, 0]]
    assert ref.offsets.dtype == np.int32 and ref.offsets.tolist() == [0, 2, 2, 3, 3, 3, 3, 3, 4, 4, 4, 4, 4]
    assert ref.seconds.dtype == np.float64
    assert ref.seconds.tolist() == [[0.5, 0.9], [1.0, 3.5], [4.0, 4.5], [2.0, 3.0]]       # sorted by onset inside a group
    # "b" has only the NaN row of an empty clip: evaluated, no events.  "d" has no row at all: not evaluated
    assert ref.evaluated.tolist() == [True, True, True, False]
    empty = EventReference.from_frame(None, LABELS, ["a"])
    assert empty.counts.tolist() == [[0, 0, 0]] and empty.offsets.tolist() == [0, 0, 0, 0] and not empty.evaluated.any()
    ref.check_cap()


def test_event_reference_unknown_labels_duplicates_and_the_cap():
    gt = _gt([(1.0, 2.0, "EATO", "a"), (1.0, 2.0, "XXXX", "a"), (1.0, 2.0, "YYYY", "elsewhere")])
    with pytest.raises(BsedError, match="XXXX"):
        EventReference.from_frame(gt, LABELS, ["a"])
    ref = EventReference.from_frame(gt, LABELS, ["a"], ignore_unknown=True)
    assert ref.counts.tolist() == [[1, 0, 0]]
    with pytest.raises(BsedError, match="twice"):
        EventReference.from_frame(gt, LABELS, ["a", "a"])
    many = _gt([(0.1 * i, 0.1 * i + 0.05, "WOTH", "b") for i in range(MATCH_MAX_REF + 1)])
    big = EventReference.from_frame(many, LABELS, ["a", "b"])
    with pytest.raises(BsedError, match=r"'b'.*65.*'WOTH'"):
        big.check_cap()
    EventReference.from_frame(many.iloc[:MATCH_MAX_REF], LABELS, ["a", "b"]).check_cap()


def test_event_reference_from_annotation_dirs(tmp_path):
    folder = tmp_path / "annotation"
    folder.mkdir()
    (folder / "a.txt").write_text("onset\toffset\tevent_label\n2.0\t3.0\tWOTH\n0.5\t1.0\tWOTH\n")
    (folder / "b.txt").write_text("onset\toffset\tevent_label\n")                          # a header only: no row
    (folder / "c.txt").write_text("onset\toffset\tevent_label\n\t\t\n")                    # DESED's empty clip
    ref = EventReference.from_annotation_dirs(["a", "b", "c", "d"], [str(folder)] * 4, LABELS)
    assert ref.counts.sum(1).tolist() == [2, 0, 0, 0] and ref.seconds.tolist() == [[0.5, 1.0], [2.0, 3.0]]
    assert ref.evaluated.tolist() == [True, False, True, False]
    with pytest.raises(FileNotFoundError):
        EventReference.from_annotation_dirs(["d"], [str(folder)], LABELS, require_annotations=True)


def test_recording_problem_cuts_the_time_line_without_changing_the_counts():
    rng = np.random.default_rng(5)
    for trial in range(20):
        n_ref, n_est = int(rng.integers(0, 60)), int(rng.integers(0, 80))
        ron = rng.uniform(0, 120, n_ref)
        gt = _gt([(on, on + rng.uniform(0.1, 3), LABELS[rng.integers(0, 3)], "rec") for on in ron])
        pick = ron[rng.integers(0, n_ref, n_est)] if n_ref else rng.uniform(0, 120, n_est)
        dfs = []
        for s in range(2):
            eon = pick + rng.uniform(-0.4, 0.4, n_est)
            dfs.append(pd.DataFrame({"event_label": [LABELS[i] for i in rng.integers(0, 3, n_est)], "onset": eon,
                                     "offset": eon + rng.uniform(0.1, 3, n_est), "filename": "rec"}))
        counts, seconds, reference = recording_problem(dfs, gt, LABELS)
        S, Bp, C = counts.shape
        assert S == 2 and C == 3 and reference.counts.shape == (Bp, C) and counts.sum() == 2 * n_est == len(seconds)
        # the pieces, scored one by one and summed, against the whole recording scored as one clip
        eoff = np.concatenate([[0], np.cumsum(counts.ravel())])
        est = [[[seconds[eoff[(s * Bp + b) * C + c]:eoff[(s * Bp + b) * C + c + 1]] for c in range(C)] for b in range(Bp)]
               for s in range(S)]
        ref = [[reference.seconds[reference.offsets[b * C + c]:reference.offsets[b * C + c + 1]] for c in range(C)]
               for b in range(Bp)]
        whole_est, whole_ref, _ = R.frames_to_lists(dfs, gt, LABELS, ["rec"])
        assert np.array_equal(R.event_counts_np(est, ref), R.event_counts_np(whole_est, whole_ref)), trial
    with pytest.raises(BsedError, match="not in the label list"):
        recording_problem(dfs[0].assign(event_label="ZZZZ"), gt, LABELS)
    # 65 reference events 0.3 s apart form one run (gaps below 2 * 0.2 s): refused; 0.5 s apart they are 65 pieces
    dense = _gt([(0.3 * i, 0.3 * i + 0.1, "EATO", "rec") for i in range(MATCH_MAX_REF + 1)])
    with pytest.raises(BsedError, match="at most 64"):
        recording_problem(dfs[0], dense, LABELS)
    sparse = _gt([(0.5 * i, 0.5 * i + 0.1, "EATO", "rec") for i in range(MATCH_MAX_REF + 1)])
    assert recording_problem(dfs[0], sparse, LABELS)[2].counts.shape == (MATCH_MAX_REF + 1, 3)


def test_restated_sweep_matches_post_process_of_the_oracle():
    from oracle import labels_oracle as lo
    rng = np.random.default_rng(7)
    strong = rng.random((2, 40, 20)).astype(np.float32)
    scale = 4 / (32000 / 255)
    ev = R.sweep_events_np(strong, [0.5], [5] * 20, scale, 10.0)
    for b in range(2):
        want = lo.post_process(strong[b], threshold=0.5, median_window=5)
        got = [[lo.BIRD_LIST[c], float(r[0]), float(r[1])] for c in range(20) for r in ev[0][b][c][1]]
        assert got == want
    counts, frames, seconds = R.flatten(ev)
    assert counts.shape == (1, 2, 20) and counts.sum() == len(frames) == len(seconds)
    assert R.flatten(R.sweep_events_np(strong, [0.5], [0] * 20, scale, 10.0))[0].sum() == 0      # dropped classes


def test_abi6_entry_points_are_declared_and_refuse_bad_arguments_before_any_hip_call():
    lib = L.lib()
    assert lib.bsed_abi_version() >= 6
    for name in ("bsed_sweep_count", "bsed_sweep_write", "bsed_event_match"):
        assert name in L.header_symbols()
    assert L.CONSTANTS["BSED_MATCH_MAX_REF"] == MATCH_MAX_REF == 64
    d = 0x1000                                          # non-null, never dereferenced on the host

    def refused(rc, word):
        msg = lib.bsed_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    refused(lib.bsed_sweep_count(None, d, d, 1, 1, 313, 20, d, None), "null")
    refused(lib.bsed_sweep_count(d, None, d, 1, 1, 313, 20, d, None), "null")
    refused(lib.bsed_sweep_count(d, d, None, 1, 1, 313, 20, d, None), "null")
    refused(lib.bsed_sweep_count(d, d, d, 1, 1, 313, 20, None, None), "null")
    refused(lib.bsed_sweep_count(d, d, d, 0, 1, 313, 20, d, None), "bad shape")
    refused(lib.bsed_sweep_count(d, d, d, 1, 0, 313, 20, d, None), "bad shape")
    refused(lib.bsed_sweep_count(d, d, d, 1, 1, 0, 20, d, None), "bad shape")
    refused(lib.bsed_sweep_count(d, d, d, 1, 1, 313, -1, d, None), "bad shape")
    # 50 * 65536 * 20 * 157 = 1.03e10 > 2^31 - 1; and a product far beyond 64 bits
    refused(lib.bsed_sweep_count(d, d, d, 50, 65536, 313, 20, d, None), "2^31 - 1")
    refused(lib.bsed_sweep_count(d, d, d, 2 ** 21, 2 ** 31 - 1, 2 ** 20, 2 ** 9, d, None), "2^31 - 1")
    refused(lib.bsed_sweep_count(d, d, d, 1, 1, 2 ** 30, 4, d, None), "too large")
    for k in range(6):
        args = [d, d, d, d, 1, 1, 313, 20, 0.03, 10.0, d, d, None]
        args[k if k < 4 else k + 6] = None
        refused(lib.bsed_sweep_write(*args), "null")
    refused(lib.bsed_sweep_write(d, d, d, d, 1, 1, 313, 0, 0.03, 10.0, d, d, None), "bad shape")
    refused(lib.bsed_sweep_write(d, d, d, d, 50, 65536, 313, 20, 0.03, 10.0, d, d, None), "2^31 - 1")
    refused(lib.bsed_sweep_write(d, d, d, d, 1, 1, 313, 20, float("nan"), 10.0, d, d, None), "numbers")
    for k in (0, 1, 2, 3, 9):
        args = [d, d, d, d, 1, 1, 20, 0.2, 0.2, d, None]
        args[k] = None
        refused(lib.bsed_event_match(*args), "null")
    refused(lib.bsed_event_match(d, d, d, d, 0, 1, 20, 0.2, 0.2, d, None), "bad shape")
    refused(lib.bsed_event_match(d, d, d, d, 1, 1, 0, 0.2, 0.2, d, None), "bad shape")
    refused(lib.bsed_event_match(d, d, d, d, 2 ** 16, 2 ** 12, 2 ** 8, 0.2, 0.2, d, None), "int32")
    refused(lib.bsed_event_match(d, d, d, d, 1, 1, 20, -0.1, 0.2, d, None), "finite")
    refused(lib.bsed_event_match(d, d, d, d, 1, 1, 20, 0.2, float("inf"), d, None), "finite")
    refused(lib.bsed_event_match(d, d, d, d, 1, 1, 20, float("nan"), 0.2, d, None), "finite")
    refused(lib.bsed_event_match(d, d, d, d, 1, 65535 * 8 + 1, 20, 0.2, 0.2, d, None), "clips per call")
