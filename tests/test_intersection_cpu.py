"""Intersection-based scoring, host side: the plain-loop restatement of tests/intersection_reference.py against the
hand-worked cases (and the three mutants those cases are there to catch), the package's host arithmetic --
``intersection_f1``, ``psds_rates``, ``PsdsResult.efpr`` / ``.psds``, ``EventReference.class_durations`` -- against the
restatement, and the ABI 13 entry point: declared, exported, and refusing every bad argument before any HIP call."""
import re

import numpy as np
import pytest

import intersection_reference as R
from bsed_amd import _lib as L
from bsed_amd._lib import BsedError
from bsed_amd.evaluation import EventReference, PsdsResult, intersection_f1, psds_from_rates, psds_rates


@pytest.mark.parametrize("name,ref,est,counts,cts", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
def test_restatement_reproduces_the_hand_cases(name, ref, est, counts, cts):
    acc, ct = R.intersection_counts_np(*R.hand_lists(ref, est))
    want_acc, want_ct = R.hand_expected(counts, cts)
    assert acc.tolist() == want_acc.tolist() and ct.tolist() == want_ct.tolist()
    assert np.diagonal(ct, axis1=1, axis2=2).sum() == 0


@pytest.mark.parametrize("mutant", sorted(R.MUTANT_KILLERS))
def test_each_mutant_of_the_rules_changes_a_hand_case(mutant):
    changed = []
    for name, ref, est, counts, cts in R.HAND_CASES:
        got = R.intersection_counts_np(*R.hand_lists(ref, est), mutant=mutant)
        want = R.hand_expected(counts, cts)
        if got[0].tolist() != want[0].tolist() or got[1].tolist() != want[1].tolist():
            changed.append(name)
    assert any(n.startswith(R.MUTANT_KILLERS[mutant]) for n in changed), (mutant, changed)
    # the documented wrong answers: all detections covering gives case 7 a true positive, per-reference counting 2 in case 10
    if mutant == "gtc_all":
        _, ref, est, _, _ = R.HAND_CASES[6]
        assert R.intersection_counts_np(*R.hand_lists(ref, est), mutant=mutant)[0][0, 0].tolist() == [1, 1, 2, 1]
    if mutant == "ct_per_ref":
        _, ref, est, _, _ = R.HAND_CASES[9]
        assert R.intersection_counts_np(*R.hand_lists(ref, est), mutant=mutant)[1][0, R.B, R.A] == 2


def test_unevaluated_clips_are_skipped_whole_and_thresholds_move_the_ties():
    est, ref = R.soup(3, 2, 5, 3)
    evaluated = np.asarray([True, False, True, False, True])
    acc, ct = R.intersection_counts_np(est, ref, evaluated=evaluated)
    keep = [0, 2, 4]
    acc2, ct2 = R.intersection_counts_np([[e[b] for b in keep] for e in est], [ref[b] for b in keep])
    assert np.array_equal(acc, acc2) and np.array_equal(ct, ct2)
    full = R.intersection_counts_np(est, ref)[0]
    assert (full[:, :, 2:] >= acc[:, :, 2:]).all() and full[:, :, 2].sum() > acc[:, :, 2].sum()
    # case 2 sits exactly on dtc = 0.5: a slightly larger dtc turns the pass into a false positive
    _, r, e, _, _ = R.HAND_CASES[1]
    assert R.intersection_counts_np(*R.hand_lists(r, e), dtc=0.5000001)[0][0, 0].tolist() == [0, 1, 1, 1]


def random_counts(seed, S, C):
    rng = np.random.default_rng(seed)
    acc = np.zeros((S, C, 4), np.int64)
    acc[:, :, 3] = rng.integers(0, 40, (1, C))                     # Nref does not depend on the threshold
    acc[:, :, 0] = rng.integers(0, 41, (S, C)) % (acc[:, :, 3] + 1)
    acc[:, :, 1] = rng.integers(0, 60, (S, C))
    acc[:, :, 2] = acc[:, :, 1] + rng.integers(0, 40, (S, C))
    ct = rng.integers(0, 9, (S, C, C)) * (1 - np.eye(C, dtype=np.int64))
    return acc, ct


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_or_nan(a, b):
    """bit for bit, any NaN standing for any other NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and same_bits(np.nan_to_num(a), np.nan_to_num(b))


def test_intersection_f1_equals_the_restatement_bit_for_bit():
    for seed, S, C in ((0, 1, 1), (1, 5, 4), (2, 7, 20)):
        acc, _ = random_counts(seed, S, C)
        if C > 2:
            acc[:, 1, 3] = 0                                        # a class that never occurs: NaN, left out of the mean
            acc[:, 1, 0] = 0
        f = intersection_f1(acc)
        cls, macro = R.intersection_f1_np(acc)
        assert same_or_nan(f["class_f1"], cls) and same_or_nan(f["macro"], macro)
        if C > 2:
            assert np.isnan(f["class_f1"][:, 1]).all() and not np.isnan(f["macro"]).any()
    # psds_eval's rule, not event_f1's: predicted but never occurring is NaN here (0 there) and does not pull the mean down
    acc = np.asarray([[[3, 1, 4, 4], [0, 5, 5, 0]]])
    f = intersection_f1(acc)
    assert np.isnan(f["class_f1"][0, 1]) and f["macro"][0] == f["class_f1"][0, 0] == 6 / 8
    # all NaN
    f = intersection_f1(np.zeros((2, 3, 4), np.int64))
    assert np.isnan(f["class_f1"]).all() and np.isnan(f["macro"]).all() and f["macro"].shape == (2,)
    # the hand cases through the F rule: case 5 (passes DTC, covers too little) has F = 0 with no false positive
    assert intersection_f1(np.asarray([[[0, 0, 1, 1]]]))["class_f1"].tolist() == [[0.0]]
    with pytest.raises(BsedError, match=r"\(\.\.\., C, 4\)"):
        intersection_f1(np.zeros((2, 3, 3)))


def test_rates_equal_the_restatement_bit_for_bit():
    for seed, S, C in ((0, 1, 1), (1, 5, 4), (2, 7, 20)):
        acc, ct = random_counts(seed, S, C)
        rng = np.random.default_rng(seed)
        dur = rng.uniform(1.0, 500.0, C)
        if C > 2:
            dur[2] = 0.0
            acc[:, 2, 3] = 0
            acc[:, 2, 0] = 0
        total = float(rng.uniform(100.0, 90000.0))
        got = psds_rates(acc, ct, dur, total)
        tpr, fpr, ctr = R.rates_np(acc, ct, dur, total)
        assert same_or_nan(got["tpr"], tpr) and same_bits(got["fpr"], fpr) and same_or_nan(got["ctr"], ctr)
        if C > 2:
            assert np.isnan(got["ctr"][:, 2, :]).all() and np.isnan(got["tpr"][:, 2]).all()
            assert not np.isnan(got["ctr"][:, 0, :]).any()
        res = PsdsResult(acc, ct, dur, total)
        assert same_bits(res.efpr(0), fpr)
        for alpha_ct in (1.0, 0.3):
            assert np.allclose(res.efpr(alpha_ct), R.efpr_np(fpr, ctr, alpha_ct), rtol=1e-12, atol=0, equal_nan=True)
    with pytest.raises(BsedError, match="do not belong together"):
        psds_rates(np.zeros((2, 3, 4)), np.zeros((2, 3, 3)), np.zeros(2), 10.0)


def test_psds_by_hand_and_against_the_restatement():
    h = R.PSDS_HAND
    assert abs(R.psds_np(h["tpr"], h["efpr"], 0.0, h["max_efpr"]) - h["value_st0"]) <= 1e-12
    assert abs(R.psds_np(h["tpr"], h["efpr"], 1.0, h["max_efpr"]) - h["value_st1"]) <= 1e-12
    v0, axis, curve = psds_from_rates(h["tpr"], h["efpr"], 0.0, h["max_efpr"])
    v1, _, _ = psds_from_rates(h["tpr"], h["efpr"], 1.0, h["max_efpr"])
    assert abs(v0 - h["value_st0"]) <= 1e-12 and abs(v1 - h["value_st1"]) <= 1e-12
    assert axis.tolist() == [0.0, 5.0, 10.0, 50.0, 100.0]            # 100 inserted, 200 beyond max_efpr
    assert np.allclose(curve, [0.1, 0.35, 0.55, 0.65, 0.65], rtol=0, atol=1e-15)
    # max_efpr already on the axis; and below every point: the area of nothing
    assert abs(psds_from_rates(h["tpr"], h["efpr"], 0.0, 50.0)[0] - (0.5 + 1.75 + 22.0) / 50.0) <= 1e-12
    assert abs(psds_from_rates(h["tpr"][:, 1:], h["efpr"][:, 1:], 0.0, 4.0)[0]) == 0.0
    for seed, S, C in ((0, 1, 1), (1, 5, 4), (2, 50, 20)):
        acc, ct = random_counts(seed, S, C)
        rng = np.random.default_rng(seed + 10)
        dur = rng.uniform(1.0, 500.0, C)
        if C > 2:
            dur[2] = 0.0
            acc[:, 2, 3] = 0
            acc[:, 2, 0] = 0
        res = PsdsResult(acc, ct, dur, 36000.0)
        tpr, fpr, ctr = R.rates_np(acc, ct, dur, 36000.0)
        for alpha_ct, alpha_st, max_efpr in ((0, 0, 100), (1, 0, 100), (0, 1, 100), (0.5, 0.5, 3.0)):
            score = res.psds(alpha_ct, alpha_st, max_efpr)
            want = R.psds_np(tpr, R.efpr_np(fpr, ctr, alpha_ct), alpha_st, max_efpr)
            assert abs(score.value - want) <= 1e-12 * max(1.0, abs(want)), (seed, alpha_ct, alpha_st, max_efpr)
            assert score.efpr[-1] == max_efpr and len(score.efpr) == len(score.etpr) and np.all(np.diff(score.efpr) > 0)
        assert 0.0 <= res.psds().value <= 1.0
    # a class without reference events is left out; no class with reference events: NaN
    tpr = np.asarray([[0.5, np.nan], [1.0, np.nan]])
    efpr = np.asarray([[1.0, 2.0], [3.0, 50.0]])
    assert abs(psds_from_rates(tpr, efpr, 1.0, 100.0)[0] - (2 * 0.5 + 97 * 1.0) / 100.0) <= 1e-12
    assert abs(R.psds_np(tpr, efpr, 1.0, 100.0) - 0.98) <= 1e-12
    assert np.isnan(psds_from_rates(np.full((2, 2), np.nan), efpr, 0.0, 100.0)[0])
    assert np.isnan(R.psds_np(np.full((2, 2), np.nan), efpr, 0.0, 100.0))
    assert np.isnan(PsdsResult(np.zeros((3, 2, 4), np.int64), np.zeros((3, 2, 2), np.int64), np.zeros(2), 10.0).psds().value)
    with pytest.raises(BsedError, match="total duration"):
        PsdsResult(np.zeros((1, 2, 4), np.int64), np.zeros((1, 2, 2), np.int64), np.zeros(2), None).psds()


def test_class_durations_skip_unevaluated_clips():
    _, ref = R.soup(4, 1, 6, 5)
    counts = np.asarray([[len(ref[b][c]) for c in range(5)] for b in range(6)])
    flat = np.concatenate([ref[b][c] for b in range(6) for c in range(5)]).reshape(-1, 2)
    evaluated = np.asarray([True, True, False, True, False, True])
    reference = EventReference(counts, flat, [f"clip{b}" for b in range(6)], list("abcde"), evaluated)
    assert same_bits(reference.class_durations(), R.class_durations_np(ref, evaluated))
    reference.evaluated = np.ones(6, bool)
    assert same_bits(reference.class_durations(), R.class_durations_np(ref))
    assert reference.class_durations().sum() > R.class_durations_np(ref, evaluated).sum() > 0


def test_abi13_entry_point_is_declared_exported_and_refuses_bad_arguments_before_any_hip_call():
    lib = L.lib()
    assert lib.bsed_abi_version() >= 13
    assert "bsed_intersection_counts" in L.header_symbols() and hasattr(lib, "bsed_intersection_counts")
    header = open(L.HEADER_PATH).read()
    proto = re.search(r"int bsed_intersection_counts\(([^)]*)\);", header)[1]
    assert [p.split()[-1].lstrip("*") for p in proto.split(",")] == [
        "est_offsets", "est_seconds", "ref_offsets", "ref_seconds", "evaluated", "S", "B", "C", "dtc", "gtc", "cttc",
        "dtc_flags", "acc", "ct", "stream"]
    assert "parity with psds_eval not pinned" in header
    d = 0x1000                                          # non-null, never dereferenced on the host

    def refused(rc, word):
        msg = lib.bsed_last_error().decode()
        assert rc == -1 and msg.startswith("bsed_intersection_counts:") and word in msg, (rc, msg)

    good = [d, d, d, d, None, 1, 1, 20, 0.5, 0.5, 0.3, d, d, d, None]
    for k in (0, 1, 2, 3, 11, 12, 13):
        args = list(good)
        args[k] = None
        refused(lib.bsed_intersection_counts(*args), "null")
    for k, v in ((5, 0), (6, 0), (7, 0), (5, -1), (6, -3), (7, -1)):
        args = list(good)
        args[k] = v
        refused(lib.bsed_intersection_counts(*args), "bad shape")
    for k in (8, 9, 10):
        for v in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
            args = list(good)
            args[k] = v
            refused(lib.bsed_intersection_counts(*args), "(0, 1]")
    args = list(good)
    args[5], args[7] = 2, 2 ** 15                       # S * C * C = 2^31
    refused(lib.bsed_intersection_counts(*args), "int32")
    args[5], args[7] = 2 ** 20, 2 ** 10
    refused(lib.bsed_intersection_counts(*args), "int32")
    args = list(good)
    args[5], args[6], args[7] = 2 ** 10, 2 ** 14, 2 ** 7   # S * C * C fits, S * B * C = 2^31 offsets do not
    refused(lib.bsed_intersection_counts(*args), "int32")
