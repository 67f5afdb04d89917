"""The segment-based scorer: sed_eval's ``SegmentBasedMetrics`` -- the second metric of the reference's
``compute_sed_eval_metrics`` (src/evaluation_measures.py:87-120, :318-325) -- counted on the GPU from the event lists of
``bsed_amd.evaluation`` (``segment_counts_gpu``; rules as stated in include/bsed.h, parity with sed_eval not pinned), F1,
error rate and accuracy from the integer counts on the host (``segment_metrics``, ``SegmentResult``), and the reference's
call on DataFrames (``compute_sed_eval_metrics``).  It lives beside the ``evaluation`` package, whose ``validate`` and
``score_recording`` call it on request; what it needs from the package is imported inside the functions that use it."""
import numpy as np
import torch

from . import _lib as L
from ._lib import BsedError

SEGMENT_MAX_CLASSES = L.CONSTANTS["BSED_SEGMENT_MAX_CLASSES"]


def _resolution(segment, who):
    """``segment`` argument of a scoring pass -> the time resolution in seconds as a float (True = 1.0, the reference's
    value), or None for None and False: not asked for"""
    if segment is None or segment is False:
        return None
    if segment is True:
        return 1.0
    try:
        resolution = float(segment)
    except (TypeError, ValueError):
        resolution = float("nan")
    if not (np.isfinite(resolution) and resolution > 0):
        raise BsedError(f"{who}: segment must be None, True or a positive time resolution in seconds, got {segment!r}")
    return resolution


def segment_counts_gpu(events, reference, resolution=1.0, length_seconds=None, out=None, expected_seconds=10.0):
    """``EventLists`` x ``EventReference`` of the same batch -> ``(class_acc, overall)`` GPU tensors: ``class_acc`` (S,C,4)
    int64 of (Ntp, Nfp, Nfn, Ntn) segments per class and ``overall`` (S,4) int64 of (Sub, Del, Ins, number of segments),
    summed over the evaluated clips and ADDED into ``out = (class_acc, overall)`` when given (the accumulators of a
    validation pass).  sed_eval's segment-based counts as include/bsed.h states them (``bsed_segment_counts``; parity with
    sed_eval not pinned): an event is active in the segments ``[max(0, floor(onset / resolution)), ceil(offset /
    resolution))``; a clip has ``ceil(length_seconds / resolution)`` segments or, with ``length_seconds=None`` (how the
    reference calls sed_eval), as many as its last event of either side reaches; per segment the classes active in the
    reference and in the estimate are compared.  One HIP launch, no host sync; no cap on the length of a list or of a
    clip, at most ``SEGMENT_MAX_CLASSES`` = 64 classes.  ``expected_seconds``: the length of a typical clip when
    ``length_seconds`` is None -- it sizes the launch (a 12 h recording wants its length here) and never changes a
    count."""
    from .evaluation._common import _accumulator
    who = "segment_counts_gpu"
    if (events.B, events.C) != (reference.B, reference.C):
        raise BsedError(f"{who}: the events cover {events.B} clips x {events.C} classes, the reference "
                        f"{reference.B} x {reference.C}")
    S, B, C = events.S, events.B, events.C
    if C > SEGMENT_MAX_CLASSES:
        raise BsedError(f"{who}: at most {SEGMENT_MAX_CLASSES} classes, got {C}")
    for name, v, optional in (("resolution", resolution, False), ("length_seconds", length_seconds, True),
                              ("expected_seconds", expected_seconds, False)):
        if not (optional and v is None) and not (np.isfinite(float(v)) and float(v) > 0):
            raise BsedError(f"{who}: {name} must be a positive finite number" + (" or None" if optional else "") + f", got {v!r}")
    dev = events.offsets.device
    pair = f"an (({S}, {C}, 4), ({S}, 4)) pair of tensors"
    if out is None:
        out = (None, None)
    elif len(out) != 2:
        raise BsedError(f"{who}: out must be {pair}")
    out = (_accumulator(out[0], (S, C, 4), dev, who, pair), _accumulator(out[1], (S, 4), dev, who, pair))
    if S * B * C == 0:
        return out
    if events.total > events.seconds.shape[0] or events.offsets.numel() != S * B * C + 1:
        raise BsedError(f"{who}: the event lists hold {events.seconds.shape[0]} rows and "
                        f"{events.offsets.numel()} offsets for {events.total} events in {S * B * C} groups")
    ref_off, ref_sec = reference.device()
    length = 0.0 if length_seconds is None else float(length_seconds)
    L.call("bsed_segment_counts", L.ptr(events.offsets, torch.int32), L.ptr(events.seconds, torch.float64),
           L.ptr(ref_off, torch.int32), L.ptr(ref_sec, torch.float64), L.ptr(reference.device_evaluated(), torch.uint8),
           S, B, C, float(resolution), length, length if length_seconds is not None else float(expected_seconds),
           L.ptr(out[0], torch.int64), L.ptr(out[1], torch.int64), L.stream())
    return out


def _ratio(num, den):
    return np.divide(num, den, out=np.full(np.shape(den), np.nan), where=np.asarray(den) > 0)


def segment_metrics(class_counts, overall_counts):
    """(..., C, 4) counts (Ntp, Nfp, Nfn, Ntn) and (..., 4) counts (Sub, Del, Ins, segments) -> dict of float64 numpy
    arrays.  Per class (..., C), with Nref = Ntp + Nfn and Nsys = Ntp + Nfp: ``class_precision`` = Ntp / Nsys,
    ``class_recall`` = Ntp / Nref, ``class_f1`` = 2 Ntp / (2 Ntp + Nfp + Nfn), ``class_er`` = (Nfn + Nfp) / Nref with its
    parts ``class_deletion_rate`` = Nfn / Nref and ``class_insertion_rate`` = Nfp / Nref, ``class_nref``, ``class_nsys``.
    Micro (...), from the sums over classes: ``precision``, ``recall``, ``f1``; ``error_rate`` = (Sub + Del + Ins) / sum
    Nref with ``substitution_rate``, ``deletion_rate``, ``insertion_rate``; ``sensitivity`` = Ntp / (Ntp + Nfn),
    ``specificity`` = Ntn / (Ntn + Nfp), ``accuracy`` = (Ntp + Ntn) / all, ``balanced_accuracy`` = their mean.
    ``macro_f1`` / ``macro_er``: the mean of ``class_f1`` / ``class_er`` over the classes where the value is defined,
    summed in class order.  NaN wherever a denominator is 0.
    How sed_eval itself averages classes with Nsys = 0 or Nref = 0 could not be checked against the library, which is
    not installed where this project is developed; the integer counts are the primary result, so a caller can apply
    another rule."""
    from .evaluation._common import _host_counts, _macro_in_class_order
    c = _host_counts(class_counts, 4, "segment_metrics takes (..., C, 4) class counts").astype(np.float64)
    o = np.asarray(overall_counts.detach().cpu().numpy() if isinstance(overall_counts, torch.Tensor) else overall_counts)
    if o.shape != c.shape[:-2] + (4,):
        raise BsedError(f"segment_metrics: class counts {c.shape} and overall counts {o.shape} do not belong together")
    o = o.astype(np.float64)
    tp, fp, fn, tn = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    nref, nsys = tp + fn, tp + fp
    out = {"class_precision": _ratio(tp, nsys), "class_recall": _ratio(tp, nref),
           "class_f1": _ratio(2.0 * tp, 2.0 * tp + fp + fn), "class_er": _ratio(fn + fp, nref),
           "class_deletion_rate": _ratio(fn, nref), "class_insertion_rate": _ratio(fp, nref),
           "class_nref": nref, "class_nsys": nsys}
    TP, FP, FN, TN = tp.sum(-1), fp.sum(-1), fn.sum(-1), tn.sum(-1)
    NREF = TP + FN
    out.update({"precision": _ratio(TP, TP + FP), "recall": _ratio(TP, NREF), "f1": _ratio(2.0 * TP, 2.0 * TP + FP + FN),
                "error_rate": _ratio(o[..., 0] + o[..., 1] + o[..., 2], NREF), "substitution_rate": _ratio(o[..., 0], NREF),
                "deletion_rate": _ratio(o[..., 1], NREF), "insertion_rate": _ratio(o[..., 2], NREF),
                "sensitivity": _ratio(TP, NREF), "specificity": _ratio(TN, TN + FP),
                "accuracy": _ratio(TP + TN, TP + TN + FP + FN)})
    out["balanced_accuracy"] = (out["sensitivity"] + out["specificity"]) / 2.0
    out["macro_f1"] = _macro_in_class_order(out["class_f1"])
    out["macro_er"] = _macro_in_class_order(out["class_er"])
    return out


class SegmentResult:
    """The segment-based result of S operating points (thresholds): ``class_counts`` (S,C,4) int64 numpy (Ntp, Nfp, Nfn,
    Ntn), ``overall_counts`` (S,4) int64 (Sub, Del, Ins, segments), ``resolution``, ``labels``, ``thresholds``, and every
    field of ``segment_metrics`` as an attribute (``f1``, ``error_rate``, ``class_f1``, ``macro_f1``, ...), one row per
    threshold.  ``results(i)`` is threshold ``i`` in the layout of sed_eval's ``results()``, key names as this project
    states them (parity with sed_eval not pinned)."""

    def __init__(self, class_counts, overall_counts, resolution, labels=None, thresholds=None):
        from .evaluation._common import _host_counts
        self.class_counts = _host_counts(class_counts, 4, "SegmentResult takes (S, C, 4) class counts").astype(np.int64)
        o = overall_counts.detach().cpu().numpy() if isinstance(overall_counts, torch.Tensor) else np.asarray(overall_counts)
        self.overall_counts = o.astype(np.int64)
        if self.class_counts.ndim != 3 or self.overall_counts.shape != (self.class_counts.shape[0], 4):
            raise BsedError(f"SegmentResult: class counts {self.class_counts.shape} and overall counts "
                            f"{self.overall_counts.shape} are not (S, C, 4) and (S, 4)")
        self.resolution = float(resolution)
        self.labels = None if labels is None else list(labels)
        self.thresholds = None if thresholds is None else list(thresholds)
        if self.labels is not None and len(self.labels) != self.class_counts.shape[1]:
            raise BsedError(f"SegmentResult: {len(self.labels)} labels for {self.class_counts.shape[1]} classes")
        self.metrics = segment_metrics(self.class_counts, self.overall_counts)
        for name, value in self.metrics.items():
            setattr(self, name, value)

    def results(self, i=0):
        """threshold ``i`` as a nested dict of Python floats / ints: ``overall`` (``f_measure``, ``error_rate``,
        ``accuracy``), ``class_wise`` (one entry per label, or per class index without labels: ``f_measure``,
        ``error_rate``, ``count``) and ``class_wise_average`` (``f_measure``, ``error_rate``)"""
        m = {k: v[i] for k, v in self.metrics.items()}
        labels = self.labels if self.labels is not None else list(range(self.class_counts.shape[1]))
        class_wise = {}
        for c, label in enumerate(labels):
            class_wise[label] = {
                "f_measure": {"f_measure": float(m["class_f1"][c]), "precision": float(m["class_precision"][c]),
                              "recall": float(m["class_recall"][c])},
                "error_rate": {"error_rate": float(m["class_er"][c]), "deletion_rate": float(m["class_deletion_rate"][c]),
                               "insertion_rate": float(m["class_insertion_rate"][c])},
                "count": {"Nref": int(m["class_nref"][c]), "Nsys": int(m["class_nsys"][c])}}
        return {
            "overall": {
                "f_measure": {"f_measure": float(m["f1"]), "precision": float(m["precision"]), "recall": float(m["recall"])},
                "error_rate": {"error_rate": float(m["error_rate"]), "substitution_rate": float(m["substitution_rate"]),
                               "deletion_rate": float(m["deletion_rate"]), "insertion_rate": float(m["insertion_rate"])},
                "accuracy": {"accuracy": float(m["accuracy"]), "sensitivity": float(m["sensitivity"]),
                             "specificity": float(m["specificity"]), "balanced_accuracy": float(m["balanced_accuracy"])}},
            "class_wise": class_wise,
            "class_wise_average": {"f_measure": {"f_measure": float(m["macro_f1"])},
                                   "error_rate": {"error_rate": float(m["macro_er"])}}}

    def __repr__(self):
        return (f"SegmentResult(resolution={self.resolution}, f1={np.array2string(self.f1, precision=5)}, "
                f"error_rate={np.array2string(self.error_rate, precision=5)})")


def compute_sed_eval_metrics(predictions, groundtruth, labels=None):
    """The reference's call (src/evaluation_measures.py:318-325) on DataFrames without sed_eval -> ``(event, segment)``:
    ``event`` is ``event_f1``'s dict (``class_f1``, ``macro``, ``micro``) of the collar-based metric at t_collar 0.2 s and
    20 % of the length, with its (1,C,3) int64 ``counts`` (Ntp, Nsys, Nref); ``segment`` is the ``SegmentResult`` at
    resolution 1.0 with no evaluated length.  The evaluated files are the file names of the ground truth (:61, :99);
    ``labels`` defaults to the sorted union of both frames' labels (:63-66, :101-104, which take them in set order)."""
    from .evaluation.events import EventReference, _frame_lists, event_counts_gpu, event_f1
    if labels is None:
        found = set(groundtruth["event_label"].dropna().unique()) | set(predictions["event_label"].dropna().unique())
        labels = sorted(found)
    labels = list(labels)
    names = list(dict.fromkeys(groundtruth["filename"]))
    reference = EventReference.from_frame(groundtruth, labels, names)
    events = _frame_lists([predictions], labels, names, "compute_sed_eval_metrics")
    counts = event_counts_gpu(events, reference, 0.2, 0.2).cpu().numpy()
    event = dict(event_f1(counts), counts=counts)
    return event, SegmentResult(*segment_counts_gpu(events, reference, 1.0), 1.0, labels)
