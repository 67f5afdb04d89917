"""Numpy restatement of the segment-based counts (include/bsed.h, ``bsed_segment_counts``) and of the host formulae of
``bsed_amd.segment_metrics``, built differently from the kernel: per (threshold, clip) two dense boolean event rolls
``(n_seg, C)`` are filled event by event -- as sed_eval's event roll is -- and every count is a sum along an axis of
them.  Float64 throughout; the one rule with arithmetic in it is the division ``time / resolution``, which Python and the
kernel both round correctly, so the counts are compared with ==."""
import math

import numpy as np

from intersection_reference import frames_to_lists  # noqa: F401  (frames -> est[s][b][c], ref[b][c], evaluated)


def _pairs(a):
    return [(float(r[0]), float(r[1])) for r in np.asarray(a, np.float64).reshape(-1, 2)]


def covered(onset, offset, resolution):
    """the half-open segment range of one event, or None when it is active nowhere"""
    lo, hi = max(0, math.floor(onset / resolution)), math.ceil(offset / resolution)
    return (lo, hi) if hi > lo else None


def n_segments(est_b, ref_b, resolution, length_seconds=None):
    """segments of one (threshold, clip): from the evaluated length, else where the last event of either side ends"""
    if length_seconds:
        return math.ceil(length_seconds / resolution)
    ends = [math.ceil(off / resolution) for side in (est_b, ref_b) for lst in side for _, off in _pairs(lst)]
    return max([0] + ends)


def event_roll(lists, n_seg, resolution):
    """lists[c]: (n,2) seconds -> (n_seg, C) bool"""
    roll = np.zeros((n_seg, len(lists)), bool)
    for c, lst in enumerate(lists):
        for on, off in _pairs(lst):
            span = covered(on, off, resolution)
            if span is not None:
                roll[span[0]:span[1], c] = True         # a slice past the end is cut by numpy: activity beyond the length
    return roll


def segment_counts_np(est, ref, resolution=1.0, length_seconds=None, evaluated=None):
    """est[s][b][c], ref[b][c]: (n,2) second arrays -> (class_acc (S,C,4) int64 of (Ntp, Nfp, Nfn, Ntn), overall (S,4)
    int64 of (Sub, Del, Ins, segments))"""
    S, B = len(est), len(ref)
    C = len(ref[0]) if B else 0
    class_acc, overall = np.zeros((S, C, 4), np.int64), np.zeros((S, 4), np.int64)
    for s in range(S):
        for b in range(B):
            if evaluated is not None and not evaluated[b]:
                continue
            n = n_segments(est[s][b], ref[b], resolution, length_seconds)
            sys_roll, ref_roll = event_roll(est[s][b], n, resolution), event_roll(ref[b], n, resolution)
            class_acc[s, :, 0] += (ref_roll & sys_roll).sum(0)
            class_acc[s, :, 1] += (sys_roll & ~ref_roll).sum(0)
            class_acc[s, :, 2] += (ref_roll & ~sys_roll).sum(0)
            class_acc[s, :, 3] += (~ref_roll & ~sys_roll).sum(0)
            nref, nsys, ntp = ref_roll.sum(1), sys_roll.sum(1), (ref_roll & sys_roll).sum(1)
            overall[s, 0] += (np.minimum(nref, nsys) - ntp).sum()
            overall[s, 1] += np.maximum(0, nref - nsys).sum()
            overall[s, 2] += np.maximum(0, nsys - nref).sum()
            overall[s, 3] += n
    return class_acc, overall


def _div(a, b):
    return a / b if b else float("nan")


def segment_metrics_np(class_acc, overall):
    """(S,C,4) and (S,4) counts -> dict of (S,C) / (S) float64 arrays with the keys of ``segment_metrics``, from plain
    Python loops over integers"""
    class_acc, overall = np.asarray(class_acc), np.asarray(overall)
    S, C, _ = class_acc.shape
    per_class = ("class_precision", "class_recall", "class_f1", "class_er", "class_deletion_rate", "class_insertion_rate",
                 "class_nref", "class_nsys")
    micro = ("precision", "recall", "f1", "error_rate", "substitution_rate", "deletion_rate", "insertion_rate",
             "sensitivity", "specificity", "accuracy", "balanced_accuracy", "macro_f1", "macro_er")
    out = {k: np.full((S, C), np.nan) for k in per_class}
    out.update({k: np.full(S, np.nan) for k in micro})
    for s in range(S):
        for c in range(C):
            tp, fp, fn, _ = (int(v) for v in class_acc[s, c])
            nref, nsys = tp + fn, tp + fp
            out["class_nref"][s, c], out["class_nsys"][s, c] = nref, nsys
            out["class_precision"][s, c], out["class_recall"][s, c] = _div(tp, nsys), _div(tp, nref)
            out["class_f1"][s, c] = _div(2 * tp, 2 * tp + fp + fn)
            out["class_er"][s, c] = _div(fn + fp, nref)
            out["class_deletion_rate"][s, c], out["class_insertion_rate"][s, c] = _div(fn, nref), _div(fp, nref)
        tp, fp, fn, tn = (int(v) for v in class_acc[s].sum(0))
        sub, dele, ins, _ = (int(v) for v in overall[s])
        nref = tp + fn
        out["precision"][s], out["recall"][s], out["f1"][s] = _div(tp, tp + fp), _div(tp, nref), _div(2 * tp, 2 * tp + fp + fn)
        out["error_rate"][s] = _div(sub + dele + ins, nref)
        out["substitution_rate"][s], out["deletion_rate"][s], out["insertion_rate"][s] = _div(sub, nref), _div(dele, nref), _div(ins, nref)
        out["sensitivity"][s], out["specificity"][s] = _div(tp, tp + fn), _div(tn, tn + fp)
        out["accuracy"][s] = _div(tp + tn, tp + tn + fp + fn)
        out["balanced_accuracy"][s] = (out["sensitivity"][s] + out["specificity"][s]) / 2
        for key, src in (("macro_f1", "class_f1"), ("macro_er", "class_er")):
            total, n = 0.0, 0
            for c in range(C):                          # in class order
                if not math.isnan(out[src][s, c]):
                    total, n = total + out[src][s, c], n + 1
            out[key][s] = _div(total, n)
    return out


# the hand-worked case of the header's rules: C = 3, resolution 1, no evaluated length
HAND_REF = [np.asarray([[0.5, 2.2]]), np.asarray([[1.0, 2.0]]), np.zeros((0, 2))]
HAND_EST = [np.asarray([[1.2, 1.8]]), np.zeros((0, 2)), np.asarray([[1.9, 3.1]])]
HAND_CLASS = [[1, 0, 2, 1], [0, 0, 1, 3], [0, 3, 0, 1]]
HAND_OVERALL = [2, 1, 1, 4]


def soup(seed, S, B, C, max_events=12, span=10.0):
    """random lists est[s][b][c], ref[b][c] with 0 .. max_events events each.  Times on a 1/8 s grid (so that ends land on
    segment edges of 1.0 and 0.25 often) mixed with off-grid ones; zero-length and overlapping events; estimated lists in
    no order, reference lists sorted; empty lists; clip 1 (when B > 1) empty on both sides; events beyond 3 s and up to
    ``span``"""
    rng = np.random.default_rng(seed)

    def one(sort):
        n = int(rng.integers(0, max_events + 1)) if rng.random() < 0.8 else 0
        on = rng.integers(0, int(span * 8), n) / 8.0
        length = rng.integers(0, 24, n) / 8.0                       # zero-length included
        off_grid = rng.random(n) < 0.4
        on = np.where(off_grid, on + rng.uniform(-0.06, 0.06, n), on)
        length = np.where(rng.random(n) < 0.4, length + rng.uniform(0, 0.1, n), length)
        a = np.stack([on, np.minimum(on + length, span)], 1).reshape(-1, 2)
        a[:, 0] = np.minimum(np.maximum(a[:, 0], -0.05), a[:, 1])   # a few negative onsets; onset <= offset
        return a[np.lexsort((a[:, 1], a[:, 0]))] if sort else a
    ref = [[one(True) for _ in range(C)] for _ in range(B)]
    est = [[[one(False) for _ in range(C)] for _ in range(B)] for _ in range(S)]
    # the edges are not left to chance: zero length on a boundary, a negative onset, [1, 2], a late event out of order
    fixed = np.asarray([[2.0, 2.0], [-0.05, 0.5], [1.0, 2.0]])
    ref[0][0] = np.concatenate([ref[0][0], fixed])
    ref[0][0] = ref[0][0][np.lexsort((ref[0][0][:, 1], ref[0][0][:, 0]))]
    est[0][0][0] = np.concatenate([[[min(9.0, span - 0.5), min(9.5, span)]], est[0][0][0], [[4.0, 4.0], [0.5, 0.77]]])
    if B > 1:
        ref[1] = [np.zeros((0, 2)) for _ in range(C)]
        for s in range(S):
            est[s][1] = [np.zeros((0, 2)) for _ in range(C)]
    return est, ref
