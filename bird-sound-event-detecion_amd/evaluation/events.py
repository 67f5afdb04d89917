"""Event lists and the collar-based matcher: the event lists of ALL thresholds from one pair of launches
(``sweep_events_gpu``), the reference events of a batch (``EventReference``), Ntp / Nsys / Nref per (threshold, class)
counted on the GPU with sed_eval's optimal matching (``event_counts_gpu``), F1 from the integer counts on the host
(``event_f1``)."""
import numpy as np
import torch

from .. import _lib as L
from .._lib import BsedError
from ._common import (_accumulator, _count_then_write, _event_frame, _host_counts, _macro_in_class_order,
                      _read_annotations)

MATCH_MAX_REF = L.CONSTANTS["BSED_MATCH_MAX_REF"]


class EventLists:
    """Estimated events of S thresholds x B clips x C classes, held on the GPU: ``offsets`` (S*B*C + 1) int32, the
    exclusive prefix of the list lengths with the total last; ``seconds`` (max(E, 1), 2) float64 [onset, offset];
    ``frames`` (max(E, 1), 2) int32 or None.  Grouped by threshold, clip, class and ordered by time inside a group --
    the layout ``bsed_event_match`` reads.  ``sweep_events_gpu`` makes one per batch; ``from_host`` wraps any list."""

    def __init__(self, offsets, seconds, S, B, C, total, frames=None, thresholds=None):
        self.offsets, self.seconds, self.frame_pairs = offsets, seconds, frames
        self.S, self.B, self.C, self.total = int(S), int(B), int(C), int(total)
        self.thresholds = thresholds

    @classmethod
    def from_host(cls, counts, seconds, thresholds=None):
        """counts (S,B,C) list lengths + seconds (E,2) in the grouped order -> the lists on the current GPU"""
        counts = np.asarray(counts)
        seconds = np.ascontiguousarray(np.asarray(seconds, np.float64).reshape(-1, 2))
        if counts.ndim != 3 or counts.min(initial=0) < 0 or int(counts.sum()) != len(seconds):
            raise BsedError(f"EventLists.from_host: counts must be (S,B,C) list lengths that add up to the {len(seconds)} "
                            f"events given, got shape {counts.shape} with sum {int(counts.sum())}")
        if counts.sum() > 2 ** 31 - 1:
            raise BsedError("EventLists.from_host: more than 2^31 - 1 events")
        off = np.concatenate([[0], np.cumsum(counts.ravel())]).astype(np.int32)
        S, B, C = counts.shape
        sec = torch.from_numpy(seconds if len(seconds) else np.zeros((1, 2))).cuda()
        return cls(torch.from_numpy(off).cuda(), sec, S, B, C, len(seconds), thresholds=thresholds)

    def host(self):
        """(counts (S,B,C) int64, frames (E,2) int32 or None, seconds (E,2) float64) numpy arrays"""
        off = self.offsets.cpu().numpy().astype(np.int64)
        fr = None if self.frame_pairs is None else self.frame_pairs[:self.total].cpu().numpy()
        return np.diff(off).reshape(self.S, self.B, self.C), fr, self.seconds[:self.total].cpu().numpy()

    def frames(self, labels, names):
        """One DataFrame per threshold with the columns, dtypes and row order (clip, class, time) that ``get_predictions``
        gives for that threshold on the same batch: event_label / onset / offset / filename."""
        if len(labels) < self.C or len(names) != self.B:
            raise BsedError(f"EventLists.frames: need at least {self.C} labels and {self.B} names, got {len(labels)} and {len(names)}")
        counts, _, sec = self.host()
        group = np.repeat(np.arange(counts.size), counts.ravel())
        per_s = np.concatenate([[0], np.cumsum(counts.reshape(self.S, -1).sum(1))])
        nam, out = np.asarray(names, dtype=object), []
        for s in range(self.S):
            g = group[per_s[s]:per_s[s + 1]]
            out.append(_event_frame(labels, g % self.C, sec[per_s[s]:per_s[s + 1]], nam[(g // self.C) % self.B]))
        return out


def _sweep_thresholds(thresholds):
    if isinstance(thresholds, torch.Tensor):
        thr = thresholds.detach().to(device="cuda", dtype=torch.float32).reshape(-1).contiguous()
    else:
        thr = torch.tensor([float(t) for t in np.atleast_1d(np.asarray(thresholds, dtype=np.float64))],
                           dtype=torch.float32).cuda()
    if thr.numel() == 0:
        raise BsedError("sweep_events_gpu: at least one threshold is needed")
    return thr


def _sweep_windows(median_window, classwise_median_window, C):
    """the (C) int32 window list of the sweep kernel: one window for every class, or ``learned_post``'s list, where
    classes beyond the list get 0 = no events (what ``binarize_median_classwise_gpu`` does with them)"""
    if classwise_median_window is None:
        if isinstance(median_window, bool) or int(median_window) != median_window or median_window < 1:
            raise BsedError(f"sweep_events_gpu: median_window must be an integer of at least 1, got {median_window!r}")
        w = [int(median_window)] * C
    else:
        w = [int(v) for v in list(classwise_median_window)[:C]]
        if any(v < 1 for v in w):
            raise BsedError(f"sweep_events_gpu: class-wise median windows must be at least 1, got {w}")
        w += [0] * (C - len(w))
    return torch.tensor(w, dtype=torch.int32).cuda() if C else torch.zeros(0, dtype=torch.int32).cuda()


def _sweep(x, thr, win, scale, max_len_seconds):
    B, T, C = x.shape
    S = thr.numel()
    n = S * B * C
    if n == 0 or T == 0:                                # an empty batch decodes to empty lists
        return EventLists(torch.zeros(n + 1, device=x.device, dtype=torch.int32),
                          torch.zeros((1, 2), device=x.device, dtype=torch.float64), S, B, C, 0,
                          torch.zeros((1, 2), device=x.device, dtype=torch.int32), thr)
    offsets, E, (ev_frames, ev_seconds) = _count_then_write(
        n, x.device, ("frames", "seconds"),
        lambda counts: L.call("bsed_sweep_count", L.ptr(x), L.ptr(thr), L.ptr(win, torch.int32), S, B, T, C, counts, L.stream()),
        lambda offsets, *ev: L.call("bsed_sweep_write", L.ptr(x), L.ptr(thr), L.ptr(win, torch.int32), offsets, S, B, T, C,
                                    scale, max_len_seconds, *ev, L.stream()))
    return EventLists(offsets, ev_seconds, S, B, C, E, ev_frames, thr)


def sweep_events_gpu(pred_strong, thresholds, median_window=1, classwise_median_window=None, scale=4 / (32000 / 255),
                     max_len_seconds=10.0):
    """(B,T',C) GPU probabilities -> ``EventLists`` with the events of EVERY threshold: what ``binarize_median_gpu``
    (or ``binarize_median_classwise_gpu`` with ``classwise_median_window``) followed by ``decode_regions_gpu`` gives per
    threshold, bit for bit, from two HIP launches and one host sync (the total list length) whatever the number of
    thresholds.  ``scale``: seconds per output frame, ``pooling_time_ratio / (sr / hop_size)``."""
    x = pred_strong.contiguous()
    if x.dim() != 3:
        raise BsedError(f"sweep_events_gpu takes (B,T,C) probabilities, got shape {tuple(x.shape)}")
    return _sweep(x, _sweep_thresholds(thresholds), _sweep_windows(median_window, classwise_median_window, x.shape[2]),
                  float(scale), float(max_len_seconds))


def _event_table(df, labels, ignore_unknown, rows=None):
    """onset / offset / event_label columns of an event frame -> ``(class (n) int64, onset (n), offset (n), keep (n) bool,
    bad)`` in the frame's row order.  ``keep``: the rows (of ``rows``, a mask, when given) with a known label and neither
    onset nor offset NaN (how DESED-style files mark a clip without events); ``bad``: the first row of them whose label
    is not in ``labels``, for the caller's own error, or None -- always None with ``ignore_unknown``, which drops them."""
    on, off = np.asarray(df["onset"], np.float64), np.asarray(df["offset"], np.float64)
    valid = ~np.isnan(on) & ~np.isnan(off)
    if rows is not None:
        valid &= rows
    index = {l: i for i, l in enumerate(labels)}
    k = np.asarray([index.get(l, -1) for l in df["event_label"]], np.int64)
    bad = np.nonzero(valid & (k < 0))[0]
    return k, on, off, valid & (k >= 0), (int(bad[0]) if len(bad) and not ignore_unknown else None)


def _grouped_lists(df, labels, names, order, unknown, ignore_unknown=False, pieces=None):
    """The way from an event frame (onset / offset / event_label, and filename where ``names`` is given; may be None or
    empty) to grouped lists, for the reference and for estimated frames alike -> ``(counts (B,C), seconds (n,2) in the
    grouped order, evaluated (B) bool)``.  ``names``: the B clips in order; a row belongs to the clip of its file name,
    rows of other files are ignored, ``evaluated`` marks the clips that have a row at all.  ``names=None``:
    ``pieces(class (n), onset (n)) -> (group (n), B)`` places the kept rows instead (``recording_problem``, where a piece
    of a class's time line plays the clip) and every group counts as evaluated.  Rows with a NaN time are dropped; the
    first row whose label is not in ``labels`` raises ``BsedError(unknown(label, clip index or None))`` unless
    ``ignore_unknown`` drops such rows.  ``order``: ``"sorted"`` = by (clip, class, onset, offset), ``"stable"`` = by
    (clip, class) with the frame's order kept inside a group."""
    C, by_name = len(labels), names is not None
    k, on, off = np.zeros(0, np.int64), np.zeros(0), np.zeros(0)
    clip, evaluated = (np.zeros(0, np.int64), np.zeros(len(names), bool)) if by_name else (None, None)
    if df is not None and len(df):
        if by_name:
            index = {n: i for i, n in enumerate(names)}
            clip = np.asarray([index.get(f, -1) for f in df["filename"]], np.int64)
            evaluated[clip[clip >= 0]] = True
        k, on, off, keep, bad = _event_table(df, labels, ignore_unknown, clip >= 0 if by_name else None)
        if bad is not None:
            raise BsedError(unknown(df["event_label"].iloc[bad], clip[bad] if by_name else None))
        k, on, off = k[keep], on[keep], off[keep]
        clip = clip[keep] if by_name else None
    if not by_name:
        clip, B = pieces(k, on)
        evaluated = np.ones(B, bool)
    group = clip * C + k
    o = np.lexsort((off, on, group)) if order == "sorted" else np.argsort(group, kind="stable")
    counts = np.bincount(group, minlength=len(evaluated) * C).reshape(len(evaluated), C)
    return counts, np.stack([on[o], off[o]], 1), evaluated


class EventReference:
    """Reference events of B clips x C classes, grouped by clip and class and sorted by onset: ``offsets`` (B*C + 1) int32
    exclusive prefix, ``seconds`` (R,2) float64, ``counts`` (B,C), all numpy; ``device()`` uploads them once.
    ``evaluated`` (B) bool: clips that have a row in the ground truth.  As in the reference's
    ``event_based_evaluation_df`` (src/evaluation_measures.py:61-75), which walks the file names of the ground truth only,
    estimated events of the other clips are not scored."""

    def __init__(self, counts, seconds, names, labels, evaluated=None):
        self.counts = np.asarray(counts, np.int64)
        self.B, self.C = self.counts.shape
        self.seconds = np.ascontiguousarray(np.asarray(seconds, np.float64).reshape(-1, 2))
        self.offsets = np.concatenate([[0], np.cumsum(self.counts.ravel())]).astype(np.int32)
        self.names, self.labels = list(names), list(labels)
        self.evaluated = np.ones(self.B, bool) if evaluated is None else np.asarray(evaluated, bool)
        self._dev = None

    @classmethod
    def from_frame(cls, groundtruth_df, labels, names, ignore_unknown=False):
        """``groundtruth_df``: onset / offset / event_label / filename rows (``get_predictions``' second return value, or
        None); ``names``: the clips of the batch in order; rows of other files are ignored, so the ground truth of a
        whole set can be passed batch by batch.  Rows with a NaN onset or offset (how DESED-style files mark a clip
        without events) are dropped but keep their clip evaluated.  A label outside ``labels`` raises ``BsedError``
        unless ``ignore_unknown`` (then the row is dropped)."""
        names, labels = list(names), list(labels)
        if len(set(names)) != len(names):
            raise BsedError("EventReference: a clip name appears twice in the batch; scoring needs one event list per file")
        counts, seconds, evaluated = _grouped_lists(
            groundtruth_df, labels, names, "sorted", ignore_unknown=ignore_unknown,
            unknown=lambda label, b: f"EventReference: event label {label!r} of clip {names[b]!r} is not in the label list")
        return cls(counts, seconds, names, labels, evaluated)

    @classmethod
    def from_annotation_dirs(cls, names, folders, labels, ignore_unknown=False, require_annotations=False):
        """the reference of a batch from ``<folder>/<name>.txt`` (tab-separated onset / offset / event_label), the files
        ``get_predictions`` reads; a clip whose file is missing or has no row is not evaluated"""
        return _annotation_reference(names, folders, labels, ignore_unknown, require_annotations)[0]

    def check_cap(self, cap=MATCH_MAX_REF):
        """the matcher holds one reference event per lane of a wave: at most ``cap`` per (clip, class)"""
        if self.counts.size and self.counts.max() > cap:
            b, c = np.unravel_index(int(np.argmax(self.counts)), self.counts.shape)
            raise BsedError(f"event matching takes at most {cap} reference events per (clip, class): clip {self.names[b]!r} "
                            f"has {int(self.counts[b, c])} of class {self.labels[c]!r}")

    def device(self):
        if self._dev is None:
            sec = self.seconds if len(self.seconds) else np.zeros((1, 2))
            self._dev = (torch.from_numpy(self.offsets).cuda(), torch.from_numpy(sec).cuda())
        return self._dev

    def device_evaluated(self):
        """``evaluated`` as a (B) uint8 GPU tensor, or None when every clip is evaluated (the kernels' NULL)"""
        if self.evaluated.all():
            return None
        return torch.from_numpy(self.evaluated.astype(np.uint8)).cuda()

    def class_durations(self):
        """(C) float64: the summed length ``offset - onset`` of every class's reference events over the evaluated clips,
        added clip by clip in list order (``ref_duration`` of ``psds_rates``)"""
        out = np.zeros(self.C)
        group = np.repeat(np.arange(self.B * self.C), self.counts.ravel())
        keep = self.evaluated[group // self.C]
        lengths, cls = (self.seconds[:, 1] - self.seconds[:, 0])[keep], (group % self.C)[keep]
        for c in range(self.C):
            sel = lengths[cls == c]
            if len(sel):
                out[c] = np.cumsum(sel)[-1]             # cumsum adds left to right: the value is defined to the bit
        return out


def _annotation_reference(names, folders, labels, ignore_unknown=False, require_annotations=False):
    """the ``annotation/<name>.txt`` files of a batch -> ``(EventReference, the list of their non-empty frames)``"""
    import pandas as pd
    dfs, _ = _read_annotations(names, folders, require_annotations)
    frame = pd.concat(dfs, ignore_index=True) if dfs else None
    return EventReference.from_frame(frame, labels, names, ignore_unknown), dfs


def _frame_lists(dfs, labels, names, who):
    """prediction frames (one per operating point; event_label / onset / offset / filename) -> ``EventLists`` over
    ``names`` x ``labels``: rows grouped by (clip, class) in frame order; rows of other files are ignored, rows with a
    NaN time dropped, a label outside ``labels`` raises"""
    counts, secs = np.zeros((len(dfs), len(names), len(labels)), np.int64), [np.zeros((0, 2))]
    for s, df in enumerate(dfs):
        counts[s], sec, _ = _grouped_lists(
            df, labels, names, "stable", lambda label, _b: f"{who}: estimated event label {label!r} is not in the label list")
        secs.append(sec)
    return EventLists.from_host(counts, np.concatenate(secs))


def event_counts_gpu(events, reference, t_collar=0.2, percentage_of_length=0.2, out=None):
    """``EventLists`` x ``EventReference`` of the same batch -> (S,C,3) int64 GPU tensor of (Ntp, Nsys, Nref) summed over the
    clips, ADDED into ``out`` when given (the accumulator of a validation pass).  sed_eval's event-based counts with its
    optimal matching: a reference and an estimated event of one clip and class hit when the onsets lie within ``t_collar``
    and the offsets within ``max(t_collar, percentage_of_length * reference length)``; Ntp is the size of a maximum
    matching of the hit graph.  One HIP launch, no host sync.  At most ``MATCH_MAX_REF`` = 64 reference events per
    (clip, class): checked here, before the launch."""
    if (events.B, events.C) != (reference.B, reference.C):
        raise BsedError(f"event_counts_gpu: the events cover {events.B} clips x {events.C} classes, the reference "
                        f"{reference.B} x {reference.C}")
    reference.check_cap()
    S, B, C = events.S, events.B, events.C
    out = _accumulator(out, (S, C, 3), events.offsets.device, "event_counts_gpu")
    if S * B * C == 0:
        return out
    ref_off, ref_sec = reference.device()
    L.call("bsed_event_match", L.ptr(events.offsets, torch.int32), L.ptr(events.seconds, torch.float64),
           L.ptr(ref_off, torch.int32), L.ptr(ref_sec, torch.float64), S, B, C, float(t_collar), float(percentage_of_length),
           L.ptr(out, torch.int64), L.stream())
    if not reference.evaluated.all():                   # clips outside the ground truth: their events are not scored
        skip = torch.from_numpy(np.nonzero(~reference.evaluated)[0]).to(events.offsets.device)
        n = (events.offsets[1:] - events.offsets[:-1]).reshape(S, B, C)
        out[:, :, 1] -= n[:, skip, :].sum(1)
    return out


def event_f1(counts):
    """(..., C, 3) integer counts (Ntp, Nsys, Nref) -> dict of float64 numpy arrays: ``class_f1`` (..., C), ``macro`` and
    ``micro`` (...).  Per class F = 2 Ntp / (Nsys + Nref), which equals 2PR / (P + R) with P = Ntp / Nsys, R = Ntp / Nref
    wherever both are defined, and is 0 where only one is; F is NaN where Nsys + Nref == 0 (the class neither occurs nor
    is predicted).  ``macro`` is the mean over the classes whose F is not NaN, summed in class order (NaN if there is none); ``micro`` is F of
    the sums over classes, which equals sed_eval's overall matching because a hit requires equal labels.
    How sed_eval itself averages classes with Nsys = 0 or Nref = 0 could not be checked against the library, which is
    not installed where this project is developed; the integer counts are the primary result, so a caller can apply
    another rule."""
    c = _host_counts(counts, 3, "event_f1 takes (..., C, 3) counts").astype(np.float64)

    def f(ntp, den):
        return np.divide(2.0 * ntp, den, out=np.full(den.shape, np.nan), where=den > 0)

    class_f1 = f(c[..., 0], c[..., 1] + c[..., 2])
    tot = c.sum(-2)
    return {"class_f1": class_f1, "macro": _macro_in_class_order(class_f1), "micro": f(tot[..., 0], tot[..., 1] + tot[..., 2])}
