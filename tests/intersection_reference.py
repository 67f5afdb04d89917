"""Plain-loop float64 restatement of the intersection criteria (DTC / GTC / CTTC), the intersection F1, the rates and PSDS,
TEST INFRASTRUCTURE ONLY: Python floats and loops, no code shared with the package.  The rules are the ones
include/bsed.h states for ``bsed_intersection_counts``; the sums run left to right in the list order of the other side
with one division per pair, so the GPU counts must EQUAL these.  ``mutant`` switches one rule to a plausible wrong
reading: the hand cases below are chosen so that each of them changes a count."""
import math

import numpy as np


def _pairs(a):
    return [(float(r[0]), float(r[1])) for r in np.asarray(a, np.float64).reshape(-1, 2)]


def _ratio_sum(on, off, others):
    """sum over ``others`` (list order) of intersection / (off - on) for the pairs that intersect"""
    total = 0.0
    for o_on, o_off in others:
        it = min(off, o_off) - max(on, o_on)
        if it > 0:
            total += it / (off - on)
    return total


def intersection_counts_np(est, ref, dtc=0.5, gtc=0.5, cttc=0.3, evaluated=None, mutant=None):
    """est[s][b][c], ref[b][c]: (n,2) second arrays -> (acc (S,C,4) int64 of (Ntp, Nfp, Nsys, Nref), ct (S,C,C) int64
    indexed [reference class][estimated class]).  mutant: None, "gtc_all" (coverage summed over ALL detections), "strict"
    (> in place of >=) or "ct_per_ref" (a cross trigger counted per contributing reference event)."""
    S, B = len(est), len(ref)
    C = len(ref[0]) if B else 0
    acc, ct = np.zeros((S, C, 4), np.int64), np.zeros((S, C, C), np.int64)

    def reaches(value, bound):
        return value > bound if mutant == "strict" else value >= bound

    for s in range(S):
        for b in range(B):
            if evaluated is not None and not evaluated[b]:
                continue
            refs = [_pairs(ref[b][c]) for c in range(C)]
            for j in range(C):
                dets = _pairs(est[s][b][j])
                passed = []
                for on, off in dets:
                    ok = reaches(_ratio_sum(on, off, refs[j]), dtc)
                    passed.append(ok)
                    acc[s, j, 2] += 1
                    if ok:
                        continue
                    acc[s, j, 1] += 1
                    for k in range(C):
                        if k == j:
                            continue
                        if mutant == "ct_per_ref":
                            ct[s, k, j] += sum(1 for r in refs[k] if min(off, r[1]) - max(on, r[0]) > 0
                                               and reaches(_ratio_sum(on, off, refs[k]), cttc))
                        elif reaches(_ratio_sum(on, off, refs[k]), cttc):
                            ct[s, k, j] += 1
                for on, off in refs[j]:
                    covering = [d for d, ok in zip(dets, passed) if ok or mutant == "gtc_all"]
                    acc[s, j, 3] += 1
                    if reaches(_ratio_sum(on, off, covering), gtc):
                        acc[s, j, 0] += 1
    return acc, ct


def intersection_f1_np(acc):
    """(S,C,4) counts -> (class F (S,C), macro (S)): F = 2 Ntp / (2 Ntp + Nfp + (Nref - Ntp)), NaN where Nref == 0; macro:
    the mean over the non-NaN classes, summed in class order"""
    acc = np.asarray(acc)
    S, C, _ = acc.shape
    cls, macro = np.full((S, C), np.nan), np.full(S, np.nan)
    for s in range(S):
        vals = []
        for c in range(C):
            tp, fp, _, nref = (int(v) for v in acc[s, c])
            if nref:
                cls[s, c] = 2 * tp / (2 * tp + fp + (nref - tp))
                vals.append(cls[s, c])
        if vals:
            total = 0.0
            for v in vals:
                total += v
            macro[s] = total / len(vals)
    return cls, macro


def class_durations_np(ref, evaluated=None):
    """ref[b][c] -> (C) summed length of every class's reference events over the evaluated clips, clip by clip"""
    C = len(ref[0]) if len(ref) else 0
    out = [0.0] * C
    for b in range(len(ref)):
        if evaluated is not None and not evaluated[b]:
            continue
        for c in range(C):
            for on, off in _pairs(ref[b][c]):
                out[c] += off - on
    return np.asarray(out, np.float64)


def rates_np(acc, ct, ref_duration, total_duration):
    """-> (tpr (S,C), fpr (S,C), ctr (S,C,C)) per hour: Ntp / Nref (NaN for Nref == 0), Nfp / total_duration * 3600,
    ct[k][j] / ref_duration[k] * 3600 (NaN for ref_duration[k] == 0)"""
    acc, ct = np.asarray(acc), np.asarray(ct)
    S, C, _ = acc.shape
    tpr, fpr, ctr = np.full((S, C), np.nan), np.full((S, C), np.nan), np.full((S, C, C), np.nan)
    for s in range(S):
        for c in range(C):
            if acc[s, c, 3]:
                tpr[s, c] = int(acc[s, c, 0]) / int(acc[s, c, 3])
            fpr[s, c] = int(acc[s, c, 1]) / float(total_duration) * 3600
            for j in range(C):
                if float(ref_duration[c]) != 0:
                    ctr[s, c, j] = int(ct[s, c, j]) / float(ref_duration[c]) * 3600
    return tpr, fpr, ctr


def efpr_np(fpr, ctr, alpha_ct):
    """efpr[s,c] = fpr[s,c] + alpha_ct * (mean over k != c of the non-NaN ctr[s,k,c]); the term is left out when
    alpha_ct == 0 or when no such k has a rate"""
    S, C = fpr.shape
    out = np.array(fpr, np.float64)
    if alpha_ct == 0:
        return out
    for s in range(S):
        for c in range(C):
            vals = [ctr[s, k, c] for k in range(C) if k != c and not math.isnan(ctr[s, k, c])]
            if vals:
                out[s, c] = fpr[s, c] + alpha_ct * (math.fsum(vals) / len(vals))
    return out


def psds_np(tpr, efpr, alpha_st=0.0, max_efpr=100.0):
    """(S,C) tpr and efpr -> PSDS value: per class the points ordered by (efpr, tpr) with the running maximum of tpr, held
    to the left on the union of the finite efpr values (0 before a class's first point; a class without a tpr is NaN),
    nanmean - alpha_st * nanstd over classes, max_efpr inserted with the held value, area up to max_efpr / max_efpr"""
    S, C = tpr.shape
    xs = sorted({float(v) for v in np.asarray(efpr).ravel() if math.isfinite(v)})
    curves = []
    for c in range(C):
        if any(math.isnan(v) for v in tpr[:, c]):
            curves.append(None)
            continue
        pts = sorted((float(efpr[s, c]), float(tpr[s, c])) for s in range(S) if math.isfinite(efpr[s, c]))
        best, steps = 0.0, []
        for x, y in pts:
            best = max(best, y)
            steps.append((x, best))
        curves.append(steps)

    def at(x):
        vals = []
        for steps in curves:
            if steps is None:
                continue
            y = 0.0
            for px, py in steps:
                if px <= x:
                    y = py
            vals.append(y)
        if not vals:
            return math.nan
        mean = math.fsum(vals) / len(vals)
        std = math.sqrt(math.fsum((v - mean) ** 2 for v in vals) / len(vals))
        return mean - alpha_st * std

    axis = sorted(set(x for x in xs if x <= max_efpr) | {float(max_efpr)})
    ys = [at(x) for x in axis]
    area = 0.0
    for i in range(len(axis) - 1):
        area += (axis[i + 1] - axis[i]) * ys[i]
    return area / max_efpr


def frames_to_lists(dfs, gt_df, labels, names):
    """per-threshold prediction DataFrames + ground-truth DataFrame -> (est[s][b][c], ref[b][c], evaluated (B)): rows in
    frame order for the estimates, sorted by (onset, offset) for the reference, NaN reference rows dropped"""
    def lists(df, sort):
        out = [[np.zeros((0, 2)) for _ in labels] for _ in names]
        if df is None:
            return out
        for b, name in enumerate(names):
            for c, lab in enumerate(labels):
                sel = df[(df.filename == name) & (df.event_label == lab)]
                a = np.asarray(sel[["onset", "offset"]], np.float64).reshape(-1, 2)
                a = a[~np.isnan(a).any(1)]
                out[b][c] = a[np.lexsort((a[:, 1], a[:, 0]))] if sort else a
        return out
    evaluated = np.asarray([gt_df is not None and bool((gt_df.filename == n).any()) for n in names])
    return [lists(df, False) for df in dfs], lists(gt_df, True), evaluated


# Hand-worked problems of ONE clip with the classes A = 0 and B = 1, dtc = gtc = 0.5, cttc = 0.3:
# (name, reference {class: events}, estimate {class: events}, {class: (Ntp, Nfp, Nsys, Nref)}, {(k, j): ct[k][j]}).
A, B = 0, 1
HAND_CASES = [
    ("1 exact", {A: [[1, 2]]}, {A: [[1, 2]]}, {A: (1, 0, 1, 1)}, {}),
    ("2 precision exactly 0.5: the >= tie", {A: [[1, 2]]}, {A: [[1, 3]]}, {A: (1, 0, 1, 1)}, {}),
    ("3 precision 0.4", {A: [[1, 2]]}, {A: [[1, 3.5]]}, {A: (0, 1, 1, 1)}, {}),
    ("4 coverage 0.25 + 0.25 ties gtc", {A: [[0, 4]]}, {A: [[0, 1], [2, 3]]}, {A: (1, 0, 2, 1)}, {}),
    ("5 passes DTC, covers too little: neither TP nor FP", {A: [[0, 4]]}, {A: [[0, 1]]}, {A: (0, 0, 1, 1)}, {}),
    ("6 one detection over two references", {A: [[0, 1], [2, 3]]}, {A: [[0, 4]]}, {A: (2, 0, 1, 2)}, {}),
    ("7 a failing detection adds no coverage", {A: [[0, 4]]}, {A: [[0, 1], [1, 9]]}, {A: (0, 1, 2, 1)}, {}),
    ("8 cross trigger", {B: [[1, 2]]}, {A: [[1, 2]]}, {A: (0, 1, 1, 0), B: (0, 0, 0, 1)}, {(B, A): 1}),
    ("9 below cttc", {B: [[1, 1.25]]}, {A: [[1, 2]]}, {A: (0, 1, 1, 0), B: (0, 0, 0, 1)}, {}),
    ("10 cross trigger counted once, not twice", {B: [[1, 1.2], [1.5, 1.7]]}, {A: [[1, 2]]},
     {A: (0, 1, 1, 0), B: (0, 0, 0, 2)}, {(B, A): 1}),
    ("11 a DTC passer never cross-triggers", {A: [[1, 2]], B: [[1, 2]]}, {A: [[1, 2]]}, {A: (1, 0, 1, 1), B: (0, 0, 0, 1)}, {}),
    ("12 touching events do not intersect", {A: [[1, 2]]}, {A: [[2, 3]]}, {A: (0, 1, 1, 1)}, {}),
]
# which hand cases a mutant of the counting must change (checked on the restatement itself in the CPU tests)
MUTANT_KILLERS = {"gtc_all": "7 ", "strict": "2 ", "ct_per_ref": "10 "}


def hand_lists(ref, est, C=2):
    """the dicts of a hand case -> (est[0][0][c], ref[0][c]) nested lists"""
    def side(d):
        return [np.asarray(d.get(c, []), np.float64).reshape(-1, 2) for c in range(C)]
    return [[side(est)]], [side(ref)]


def hand_expected(counts, cts, C=2):
    acc, ct = np.zeros((1, C, 4), np.int64), np.zeros((1, C, C), np.int64)
    for c, v in counts.items():
        acc[0, c] = v
    for (k, j), v in cts.items():
        ct[0, k, j] = v
    return acc, ct


# PSDS by hand: C = 2, S = 3.  Class 0 has the points (0, .2), (10, .6), (50, .8), class 1 (5, .5), (10, .5), (200, 1).
# On the axis 0, 5, 10, 50, [100], 200 the curves are .2 .2 .6 .8 .8 .8 and 0 .5 .5 .5 .5 1; their mean .1 .35 .55 .65 .65;
# area to 100: 5 * .1 + 5 * .35 + 40 * .55 + 50 * .65 = 56.75 -> 0.5675.  Minus one standard deviation (|a - b| / 2):
# 0 .2 .5 .5 .5 -> 5 * 0 + 5 * .2 + 40 * .5 + 50 * .5 = 46 -> 0.46.
PSDS_HAND = dict(tpr=np.asarray([[.2, .5], [.6, .5], [.8, 1.0]]), efpr=np.asarray([[0.0, 5.0], [10.0, 10.0], [50.0, 200.0]]),
                 max_efpr=100.0, value_st0=0.5675, value_st1=0.46)


def soup(seed, S, B, C, max_ref=5, max_est=7, grid=0.031875, span=10.0):
    """random reference and estimated lists on the frame grid, clipped to ``span``: overlapping events, empty lists and
    all-empty clips; est[s][b][c], ref[b][c]"""
    rng = np.random.default_rng(seed)
    frames = int(span / grid) + 40                     # some events run past the end and are clipped

    def events(n, around=None):
        if around is not None and len(around) and n:
            base = np.rint(around[rng.integers(0, len(around), n), 0] / grid).astype(np.int64)
            on = np.clip(base + rng.integers(-20, 21, n), 0, frames - 2)
        else:
            on = rng.integers(0, frames - 1, n)
        length = np.where(rng.random(n) < 0.5, rng.integers(1, 30, n), rng.integers(1, 160, n))
        a = np.stack([on * grid, (on + length) * grid], 1).reshape(-1, 2).clip(0, span)
        return a[np.lexsort((a[:, 1], a[:, 0]))]

    empty_clip = rng.random(B) < 0.2
    ref = [[events(int(rng.integers(0, max_ref + 1))) if rng.random() < 0.6 and not empty_clip[b] else np.zeros((0, 2))
            for _ in range(C)] for b in range(B)]
    every = [np.concatenate(ref[b]).reshape(-1, 2) for b in range(B)]
    est = [[[events(int(rng.integers(0, max_est + 1)), every[b] if rng.random() < 0.8 else None)
             if rng.random() < 0.7 else np.zeros((0, 2)) for _ in range(C)] for b in range(B)] for _ in range(S)]
    return est, ref
