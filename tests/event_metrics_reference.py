"""Float64 numpy restatement of the validation path, TEST INFRASTRUCTURE ONLY: threshold -> scipy.ndimage.median_filter ->
contiguous regions (oracle.labels_oracle) -> seconds; the collar hit graph of sed_eval's event-based metric; Ntp as the
size of a maximum bipartite matching from scipy.sparse.csgraph -- an implementation that shares nothing with the GPU
matcher.  ``first_fit_ntp`` is the greedy matching the pinned case of the tests separates from the maximum."""
import numpy as np
import scipy.ndimage
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching

from oracle import labels_oracle as lo


def sweep_events_np(strong, thresholds, windows, scale, max_len):
    """strong (B,T,C) float32, thresholds (S), windows (C) ints (0 = no events) -> nested list ev[s][b][c] of
    ((E,2) int frames, (E,2) float64 seconds)"""
    strong = np.asarray(strong, np.float32)
    B, T, C = strong.shape
    out = []
    for thr in np.asarray(thresholds, np.float32):
        per_b = []
        for b in range(B):
            per_c = []
            for c in range(C):
                fr = np.zeros((0, 2), np.int64)
                if windows[c] > 0 and T > 0:
                    binar = (strong[b, :, c:c + 1] > thr).astype(np.float64)
                    filt = scipy.ndimage.median_filter(binar, (int(windows[c]), 1))
                    fr = np.asarray(lo.find_contiguous_regions(filt[:, 0]), np.int64).reshape(-1, 2)
                per_c.append((fr, np.clip(fr.astype(np.float64) * scale, 0, max_len)))
            per_b.append(per_c)
        out.append(per_b)
    return out


def flatten(ev):
    """ev[s][b][c] -> (counts (S,B,C), frames (E,2), seconds (E,2)) in the order threshold, clip, class, time"""
    counts = np.asarray([[[len(c[0]) for c in b] for b in s] for s in ev], np.int64)
    fr = [c[0] for s in ev for b in s for c in b]
    sec = [c[1] for s in ev for b in s for c in b]
    return (counts, np.concatenate(fr).reshape(-1, 2) if fr else np.zeros((0, 2), np.int64),
            np.concatenate(sec).reshape(-1, 2) if sec else np.zeros((0, 2)))


def hit_matrix(ref, est, t_collar=0.2, percentage_of_length=0.2):
    """ref (R,2), est (E,2) float64 [onset, offset] -> (R,E) bool, the two rules exactly as the kernel states them"""
    ref, est = np.asarray(ref, np.float64).reshape(-1, 2), np.asarray(est, np.float64).reshape(-1, 2)
    on = np.abs(ref[:, None, 0] - est[None, :, 0]) <= t_collar
    tol = np.maximum(t_collar, percentage_of_length * (ref[:, 1] - ref[:, 0]))
    off = np.abs(ref[:, None, 1] - est[None, :, 1]) <= tol[:, None]
    return on & off


def max_matching(hits):
    hits = np.asarray(hits, bool)
    if hits.size == 0 or not hits.any():
        return 0
    return int((maximum_bipartite_matching(csr_matrix(hits.astype(np.int8)), perm_type="column") >= 0).sum())


def first_fit_ntp(hits):
    """greedy: every estimated event, in list order, takes the first reference event it hits that is still free"""
    hits = np.asarray(hits, bool)
    free = np.ones(hits.shape[0], bool)
    n = 0
    for e in range(hits.shape[1]):
        cand = np.nonzero(hits[:, e] & free)[0]
        if len(cand):
            free[cand[0]] = False
            n += 1
    return n


def event_counts_np(est, ref, t_collar=0.2, percentage_of_length=0.2, evaluated=None, ntp=max_matching):
    """est[s][b][c] and ref[b][c]: (n,2) second arrays -> (S,C,3) int64 (Ntp, Nsys, Nref); clips with evaluated[b] False
    are left out, as the reference's event_based_evaluation_df leaves out files without a ground-truth row"""
    S, B, C = len(est), len(ref), len(ref[0]) if len(ref) else 0
    out = np.zeros((S, C, 3), np.int64)
    for s in range(S):
        for b in range(B):
            if evaluated is not None and not evaluated[b]:
                continue
            for c in range(C):
                e, r = np.asarray(est[s][b][c]).reshape(-1, 2), np.asarray(ref[b][c]).reshape(-1, 2)
                out[s, c] += (ntp(hit_matrix(r, e, t_collar, percentage_of_length)) if len(e) and len(r) else 0, len(e), len(r))
    return out


def f1_np(counts):
    """plain loops: per-class F = 2 Ntp / (Nsys + Nref) (NaN for 0 / 0), macro = mean over the non-NaN, micro from sums"""
    counts = np.asarray(counts)
    S, C, _ = counts.shape
    cls = np.full((S, C), np.nan)
    macro, micro = np.full(S, np.nan), np.full(S, np.nan)
    for s in range(S):
        vals = []
        for c in range(C):
            tp, ns, nr = (int(v) for v in counts[s, c])
            if ns + nr:
                cls[s, c] = 2 * tp / (ns + nr)
                vals.append(cls[s, c])
        if vals:
            macro[s] = sum(vals) / len(vals)
        tp, ns, nr = (int(v) for v in counts[s].sum(0))
        if ns + nr:
            micro[s] = 2 * tp / (ns + nr)
    return cls, macro, micro


def frames_to_lists(dfs, gt_df, labels, names):
    """per-threshold prediction DataFrames + ground-truth DataFrame -> (est[s][b][c], ref[b][c], evaluated (B)), rows in
    frame order for the estimates, sorted by onset for the reference, NaN reference rows dropped"""
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


# Hand-worked problems of one (clip, class), t_collar 0.2 and percentage_of_length 0.2: (name, reference, estimated, Ntp).
# The CPU tests check the restatement against these numbers, the GPU tests the kernel.
HAND_CASES = [
    ("exact hits", [[1.0, 2.0], [3.0, 4.5]], [[1.0, 2.0], [3.0, 4.5]], 2),
    # onsets 0.19 and 0.21 from the reference onset; the offsets are exact
    ("onset inside the collar", [[1.0, 2.0]], [[1.19, 2.0]], 1),
    ("onset outside the collar", [[1.0, 2.0]], [[1.21, 2.0]], 0),
    ("onset early inside the collar", [[1.0, 2.0]], [[0.81, 2.0]], 1),
    # a 10 s event: the offset may be 0.2 * 10 = 2 s off, far beyond the collar
    ("long event, offset inside 20 % of its length", [[1.0, 11.0]], [[1.1, 12.5]], 1),
    ("long event, offset outside 20 % of its length", [[1.0, 11.0]], [[1.1, 13.1]], 0),
    ("long event, early offset inside 20 % of its length", [[1.0, 11.0]], [[0.9, 9.5]], 1),
    # a 0.5 s event: 20 % of its length is 0.1 s, the collar of 0.2 s governs
    ("short event, offset inside the collar", [[1.0, 1.5]], [[1.0, 1.65]], 1),
    ("short event, offset outside the collar", [[1.0, 1.5]], [[1.0, 1.75]], 0),
    # two reference events that both hit the one estimate: one true positive, one miss
    ("two references, one estimate", [[1.0, 2.0], [1.1, 2.1]], [[1.05, 2.05]], 1),
    ("two estimates, one reference", [[1.0, 2.0]], [[0.95, 2.0], [1.05, 2.1]], 1),
    ("no estimate", [[1.0, 2.0]], [], 0),
    ("no reference", [], [[1.0, 2.0]], 0),
]

# Found by a seeded random search over two or three events a side (values rounded to 0.01, every compare at least 0.02
# from its bound) for problems where first-fit in event order is not maximum, then written out:
#   e0 = (1.78, 2.89) hits r0 = (1.75, 2.88) and r1 = (1.86, 3.01);  e1 = (1.92, 2.68) hits r0 only
#   (r1's onset is 0.06 away but its offset 0.33 > max(0.2, 0.2 * 1.15) = 0.23).
# First-fit gives e0 the first free reference it hits, r0, and e1 finds r0 taken: 1.  Maximum: e0 - r1, e1 - r0: 2.
FIRST_FIT_CASE = ([[1.75, 2.88], [1.86, 3.01]], [[1.78, 2.89], [1.92, 2.68]], 1, 2)
